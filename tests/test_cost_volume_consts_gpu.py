"""GPU: the forward cost volume with its constants resident in LDS (rtk_cost_volume_split_shared / rtk_cost_volume_split_term) against
the same kernel reading them from global memory on every tile (rtk_cost_volume_split_gconst), bit for bit.

The shapes are the smallest that reach each path of the kernel:
  (B = 8, N = 24), 8 workgroups   the flat XCD grid, every workgroup walks three tiles: the image outlives the weight stream's wraps;
                   0 workgroups   the default grid (one workgroup per tile here);
  (B = 3, N = 20)                 the 2-D grid; the last group of a sample has two empty waves;
  (B = 16, N = 17), 128 asked     a group of ONE point (a half-valid wave), and more workgroups asked for than an XCD has tiles (the
                                  launcher gives a tile at most one workgroup; a workgroup without a tile would fill and leave).
Every case runs twice in a row, each time into a sentinel-filled output of pitch 264 with four rows to spare: nothing but the result is
written, and the second launch gives the first one's bits."""
import pytest
import torch

from ratrack_amd import _lib
from ratrack_amd import fused as F
from ratrack_amd import pointnet2_utils as PU
from ratrack_amd import synth
from ratrack_amd.track4d import Args, Track4D

pytestmark = pytest.mark.gpu
DEV = "cuda"
PITCH, SPARE, SENTINEL = 264, 4, 7.0
CASES = [(8, 24, 8), (8, 24, 0), (3, 20, 0), (16, 17, 128)]


@pytest.fixture(scope="module")
def eng():
    net = Track4D(Args()).to(DEV).eval()
    synth.fill_state_dict(net.state_dict())
    net.invalidate_fused()
    e = F.FusedBackbone(net)
    assert e.cv_split
    return e


def _operands(B, N):
    gen = torch.Generator().manual_seed(131 * B + N)
    x1 = torch.randn(B, N, 3, generator=gen).to(DEV)
    x2 = (x1.cpu() + 0.05 * torch.randn(B, N, 3, generator=gen)).to(DEV)
    p1 = torch.randn(B * N, 256, generator=gen).to(DEV)
    p2 = torch.randn(B * N, 256, generator=gen).to(DEV)
    s = torch.randn(B, 256, generator=gen).to(DEV)
    knn = PU.knn_point(16, x2, x1).contiguous()
    assert knn.dtype == torch.int64 and knn.shape == (B, N, 16)
    return x1, x2, knn, p1, p2, s


def _launch(eng, name, B, N, x1, x2, knn, p1, p2, term, wgs):
    out = torch.full((B * N + SPARE, PITCH), SENTINEL, device=DEV)
    head = (B, N, N, x1.data_ptr(), x2.data_ptr(), knn.data_ptr(), p1.data_ptr(), p2.data_ptr())
    tail = (eng.cv_wd.data_ptr(), eng.cv_images.data_ptr(), eng.cv_scales.data_ptr(), eng.cv_bias23[0].data_ptr(),
            eng.cv_bias23[1].data_ptr(), eng.wn1.arr, out.data_ptr(), PITCH, wgs, F._stream())
    _lib.call(name, *head, *(() if term is None else (term.data_ptr(),)), *tail)
    return out


def _check_written(out, rows, what):
    assert torch.all(out[:, 256:] == SENTINEL), what + ": columns beyond the result written"
    assert torch.all(out[rows:] == SENTINEL), what + ": rows beyond the result written"
    assert torch.isfinite(out[:rows, :256]).all() and float(out[:rows, :256].abs().max()) > 0, what


@pytest.mark.parametrize("B,N,wgs", CASES)
def test_lds_constants_give_the_bits_of_global_constants(eng, B, N, wgs):
    x1, x2, knn, p1, p2, s = _operands(B, N)
    p1s = p1 + s.repeat_interleave(N, 0)
    with torch.no_grad():
        ref = _launch(eng, "rtk_cost_volume_split_gconst", B, N, x1, x2, knn, p1, p2, None, wgs)
        ref_s = _launch(eng, "rtk_cost_volume_split_gconst", B, N, x1, x2, knn, p1s, p2, None, wgs)
        got = [_launch(eng, "rtk_cost_volume_split_shared", B, N, x1, x2, knn, p1, p2, None, wgs) for _ in range(2)]
        got_s = [_launch(eng, "rtk_cost_volume_split_term", B, N, x1, x2, knn, p1, p2, s, wgs) for _ in range(2)]
        torch.cuda.synchronize()
    rows = B * N
    for what, o in [("gconst", ref), ("gconst, p1 + s", ref_s), ("shared, run 1", got[0]), ("shared, run 2", got[1]),
                    ("term, run 1", got_s[0]), ("term, run 2", got_s[1])]:
        _check_written(o, rows, "B=%d N=%d wgs=%d %s" % (B, N, wgs, what))
    assert not torch.equal(ref, ref_s)      # (the term changes the result: the two comparisons below are two)
    for k in range(2):
        assert torch.equal(got[k], ref), "shared, run %d" % (k + 1)
        assert torch.equal(got_s[k], ref_s), "term, run %d" % (k + 1)
