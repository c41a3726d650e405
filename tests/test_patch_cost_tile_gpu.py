"""GPU: rtk_patch_cost on the 32-position tile (csrc/fused_patch.hip) against the float64 restatement of its contract
(tests/_stage_f64.py::patch_cost_f64, with the bound of test_stage_f64_gpu.py: error relative to scale <= 2e-6 and <= 3 x the error
of the same restatement in torch fp32 + 2e-7) and, bit for bit, against the kernel with one wave per point it replaced on the hot path
(rtk_patch_cost_wave16).  The shapes are the smallest at which the tile can go wrong: the minimum the entry point takes, a half-empty
last tile on the 2-D grid, the XCD-aware flat grid, feature pitches that are no multiple of a cache line, and a launch whose
workgroups each loop over several tiles.  Clouds hold every point twice: neighbours repeat and the first direction is 0.

The tile's k-slots and its hidden-layer fma chain follow the wave16 kernel's accumulation order, so the two
are expected to agree bit for bit and every case compares with torch.equal; each case prints the largest difference before it
asserts."""
import pytest
import torch

from ratrack_amd import _lib
from ratrack_amd import fused as F
from ratrack_amd import pointnet2_utils as PU

from _stage_f64 import patch_cost_f64

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -5.0          # what the output buffer holds before a launch
POISON = 1e30        # feature columns >= 256: large and finite (a NaN could vanish in a ReLU)
PT_WGS_TARGET = 1024 # fused_patch.hip
PT_PPW = 8           # points per workgroup iteration (four waves x two points)


@pytest.fixture(scope="module")
def eng():
    from ratrack_amd.track4d import Args, Track4D
    from _util import reference_state_dict
    net = Track4D(Args()).to(DEV).eval()
    net.load_state_dict(reference_state_dict(DEV), strict=True)
    e = F.FusedBackbone(net)
    e.sd = {k: v.detach() for k, v in net.state_dict().items()}
    return e


def _wn2(eng):
    sd = lambda k: eng.sd[k].double()
    return [(sd("fc_layer.weightnet2.mlp_convs.%d.weight" % i).reshape(-1, 3 if i == 0 else 8),
             sd("fc_layer.weightnet2.mlp_convs.%d.bias" % i)) for i in range(3)]


def _operands(B, N, feat_pitch, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x1 = torch.randn(B, N, 3, generator=g, device=DEV)
    x1[:, N // 2:] = x1[:, :N - N // 2].clone()                          # every point twice
    knn = PU.knn_point(16, x1, x1)
    feat = torch.full((B * N, feat_pitch), POISON, device=DEV)
    feat[:, :256] = torch.randn(B * N, 256, generator=g, device=DEV)
    return x1, knn, feat


def _launch(eng, name, B, N, x1, knn, feat, out_pitch):
    out = torch.full((B * N + 4, out_pitch), SENT, device=DEV)
    _lib.call(name, B, N, x1.data_ptr(), knn.data_ptr(), feat.data_ptr(), feat.shape[1], eng.wn2.arr, out.data_ptr(), out_pitch, 0,
              F._stream())
    torch.cuda.synchronize()
    assert (out[B * N:] == SENT).all() and (out[:, 256:] == SENT).all(), name      # nothing beyond the (B N, 256) result
    return out[:B * N, :256]


def _scale_err(got, r64):
    return float((got.double() - r64).abs().max() / r64.abs().max().clamp_min(1e-300))


def _grid(B, N):
    """(workgroups per sample, tiles per sample) by the launcher's rule."""
    groups = (N + PT_PPW - 1) // PT_PPW
    gx = groups
    while gx * B > PT_WGS_TARGET and gx > 1:
        gx = (gx + 1) // 2
    return gx, groups


# B, N, feature pitch, output pitch
SHAPES = [(1, 16, 256, 256),      # the minimum the entry point accepts
          (3, 17, 256, 272),      # a half-empty last tile, the 2-D grid (B % 8 != 0)
          (8, 33, 256, 256),      # the XCD-aware flat grid
          (2, 64, 260, 264),      # rows that start 16 bytes into a line
          (2, 64, 264, 260)]


@pytest.mark.parametrize("B,N,feat_pitch,out_pitch", SHAPES)
def test_tile_matches_float64_and_the_wave16_kernel(eng, B, N, feat_pitch, out_pitch):
    x1, knn, feat = _operands(B, N, feat_pitch, seed=B * 31 + N + feat_pitch)
    first = x1[torch.arange(B, device=DEV)[:, None], knn[:, :, 0].long()]
    assert float((first - x1).abs().max()) == 0.0                        # the first direction is 0
    wn2 = _wn2(eng)
    ref = lambda dt: patch_cost_f64(x1.to(dt), knn, feat[:, :256].to(dt).reshape(B, N, 256),
                                    [(w.to(dt), b.to(dt)) for w, b in wn2]).reshape(B * N, 256)
    r64, r32 = ref(torch.float64), ref(torch.float32)
    got = _launch(eng, "rtk_patch_cost", B, N, x1, knn, feat, out_pitch)
    old = _launch(eng, "rtk_patch_cost_wave16", B, N, x1, knn, feat, out_pitch)
    e, e_old, e32 = _scale_err(got, r64), _scale_err(old, r64), _scale_err(r32, r64)
    print("\npatch cost tile B %d N %d pitch %d: tile %.2e  wave16 %.2e  torch fp32 %.2e  |tile - wave16| max %.3e"
          % (B, N, feat_pitch, e, e_old, e32, float((got - old).abs().max())))
    assert e <= 2e-6 and e <= 3 * e32 + 2e-7, (e, e32)
    assert torch.equal(got, old)


def test_every_workgroup_loops_over_tiles_and_the_last_is_partial(eng):
    """B 128, N 229: 29 groups of eight points per sample, halved to 8 workgroups per sample by the launcher -- each takes 3 or 4
    tiles, the last group holds five points (two full waves, half a wave, an empty one).  Reference: the wave16 kernel."""
    B, N = 128, 229
    gx, groups = _grid(B, N)
    assert (gx, groups) == (8, 29) and groups // gx >= 3 and N % PT_PPW == 5
    x1, knn, feat = _operands(B, N, 256, seed=77)
    got = _launch(eng, "rtk_patch_cost", B, N, x1, knn, feat, 256)
    old = _launch(eng, "rtk_patch_cost_wave16", B, N, x1, knn, feat, 256)
    print("\npatch cost tile B %d N %d: |tile - wave16| max %.3e" % (B, N, float((got - old).abs().max())))
    assert torch.equal(got, old)


def test_non_finite_feature_row(eng):
    """+inf and a NaN in one gathered feature row: non-finite exactly where the float64 restatement is, and where the wave16 kernel is;
    the finite outputs are the wave16 kernel's bits."""
    B, N = 2, 64
    x1, knn, feat = _operands(B, N, 256, seed=9)
    r = int(knn[1, 5, 3]) + N
    feat[r, 7], feat[r, 100] = float("inf"), float("nan")
    ref = patch_cost_f64(x1.double(), knn, feat.double().view(B, N, 256), _wn2(eng)).reshape(B * N, 256)
    got = _launch(eng, "rtk_patch_cost", B, N, x1, knn, feat, 256)
    old = _launch(eng, "rtk_patch_cost_wave16", B, N, x1, knn, feat, 256)
    bad_g, bad_r, bad_o = ~torch.isfinite(got), ~torch.isfinite(ref), ~torch.isfinite(old)
    print("\npatch cost tile non-finite: reference %d, tile %d, wave16 %d" % (int(bad_r.sum()), int(bad_g.sum()), int(bad_o.sum())))
    assert bad_r.any()
    assert torch.equal(bad_g, bad_r) and torch.equal(bad_g, bad_o)
    assert torch.equal(got[~bad_g], old[~bad_g])
