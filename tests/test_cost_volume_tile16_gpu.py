"""GPU: the forward cost volume on the 16-position tile (rtk_cost_volume_split16_shared / _term: cost_volume_split_kernel16, two waves
per SIMD) against the float64 restatement of the operator's contract (tests/_stage_f64.py::cost_volume_f64), with exactly the bound of
tests/test_stage_f64_gpu.py::_check: rel-to-scale error <= 2e-6 and <= 3 x the error of the same restatement in torch fp32 + 2e-7.
The bits differ from the 32-position kernel's (a matrix instruction sums 32 products instead of 16), so nothing here compares the two
bit for bit; the packer's two fragment orders hold the same pieces under the same scale, and that is pinned.

Shapes: the cases of tests/_cost_volume_cases.py as they are --

| id | B, n1, n2 | what it enters |
|---|---|---|
| b5_n1_from_16 | 5, 1, 16 | one query: seven of the workgroup's eight waves idle (clamped to point 0, nothing stored) |
| b3_n77 | 3, 77, 77 | 2-D grid, a partial last group of eight |
| b2_n50_from_131, b2_n131_from_50 | | n1 != n2 |
| b64_n37_looping | 64, 37, 37 | flat XCD grid, 40 tiles on 32 workgroups per XCD: several tiles per workgroup, the stream's wrap |
| b3_n77_padded | 3, 77, 77 | duplicate rows: hot row 0 |

-- and B = 8, N = 24 on 8 workgroups (one per XCD for its three tiles).  Every shape runs both forms: _shared, and _term with a
per-sample term that the reference adds to p1 in fp32 (the kernel's own first sum, rounded once)."""
import pytest
import torch

from ratrack_amd import _lib
from ratrack_amd import fused as F
from ratrack_amd import pointnet2_utils as PU

from _cost_volume_cases import Case, case_by_name, parameters
from _stage_f64 import cost_volume_f64

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -5.0
PITCH = 264
NAMES = ["b5_n1_from_16", "b3_n77", "b2_n50_from_131", "b2_n131_from_50", "b64_n37_looping", "b3_n77_padded"]


@pytest.fixture(scope="module")
def eng():
    from ratrack_amd.track4d import Args, Track4D
    from _util import reference_state_dict
    net = Track4D(Args()).to(DEV).eval()
    net.load_state_dict(reference_state_dict(DEV), strict=True)
    return F.FusedBackbone(net)


def _scale_err(got, r64):
    return float((got.double() - r64).abs().max() / r64.abs().max().clamp_min(1e-300))


def _check(what, got, r64, r32, bound=2e-6):
    e, e32 = _scale_err(got, r64), _scale_err(r32, r64)
    print("\n%s: kernel %.2e  torch fp32 %.2e" % (what, e, e32))
    assert e <= bound and e <= 3 * e32 + 2e-7, (what, e, e32)


def _knn(case):
    x1, x2 = case.xyz1.to(DEV), case.xyz2.to(DEV)
    if case.live is None:
        return PU.knn_point(16, x2, x1).contiguous()
    nv = torch.tensor(case.live, dtype=torch.int32, device=DEV)
    idx = torch.empty(case.B, case.n1, 16, dtype=torch.int64, device=DEV)
    _lib.call("rtk_knn_point_masked", case.B, case.n1, case.n2, 16, x1.data_ptr(), x2.data_ptr(), idx.data_ptr(), nv.data_ptr(), F._stream())
    return idx


def _launch(eng, B, n1, n2, x1, x2, knn, p1, p2, term=None, workgroups=0):
    """rtk_cost_volume_split16_shared (term None) / _term on the engine's images -> the (B n1 + 4, PITCH) buffer, SENT where unwritten."""
    out = torch.full((B * n1 + 4, PITCH), SENT, device=DEV)
    head = (B, n1, n2, x1.data_ptr(), x2.data_ptr(), knn.data_ptr(), p1.data_ptr(), p2.data_ptr())
    tail = (eng.cv_wd.data_ptr(), eng.cv_images16.data_ptr(), eng.cv_scales.data_ptr(), eng.cv_bias23[0].data_ptr(), eng.cv_bias23[1].data_ptr(),
            eng.wn1.arr, out.data_ptr(), PITCH, workgroups, F._stream())
    if term is None:
        _lib.call("rtk_cost_volume_split16_shared", *head, *tail)
    else:
        _lib.call("rtk_cost_volume_split16_term", *head, term.data_ptr(), *tail)
    torch.cuda.synchronize()
    return out


def _reference(dtype, B, n1, n2, x1, x2, knn, p1, p2, par):
    c = lambda t: t.to(device=DEV, dtype=dtype)
    wd, w2, b2, w3, b3, wa, ba, wb, bb, wc, bc = [c(t) for t in par]
    return cost_volume_f64(c(x1), c(x2), knn, c(p1).view(B, n1, 256), c(p2).view(B, n2, 256), wd, [(w2, b2), (w3, b3)],
                           [(wa, ba), (wb, bb), (wc, bc)]).reshape(B * n1, 256)


def _both_forms(eng, what, B, n1, n2, x1, x2, knn, p1, p2, workgroups, seed):
    par = parameters("cpu", torch.float32)
    term = torch.randn(B, 256, generator=torch.Generator().manual_seed(seed)).to(DEV)
    p1t = (p1.view(B, n1, 256) + term[:, None, :]).reshape(B * n1, 256).contiguous()      # fp32: the kernel's own first sum
    for form, t, p1ref in (("shared", None, p1), ("term", term, p1t)):
        r64 = _reference(torch.float64, B, n1, n2, x1, x2, knn, p1ref, p2, par)
        r32 = _reference(torch.float32, B, n1, n2, x1, x2, knn, p1ref, p2, par)
        out = _launch(eng, B, n1, n2, x1, x2, knn, p1, p2, term=t, workgroups=workgroups)
        assert (out[B * n1:] == SENT).all() and (out[:, 256:] == SENT).all(), form
        _check("cost volume tile16 %s %s" % (form, what), out[:B * n1, :256], r64, r32)
        again = _launch(eng, B, n1, n2, x1, x2, knn, p1, p2, term=t, workgroups=workgroups)
        assert torch.equal(out, again), "%s %s: two launches, different bits" % (form, what)


@pytest.mark.parametrize("name", NAMES)
def test_tile16_matches_float64(eng, name):
    case = case_by_name(name)
    knn = _knn(case)
    x1, x2, p1, p2 = (t.to(DEV) for t in (case.xyz1, case.xyz2, case.p1, case.p2))
    _both_forms(eng, name, case.B, case.n1, case.n2, x1, x2, knn, p1, p2, 0, seed=len(name))


def test_tile16_fewer_workgroups_than_tiles(eng):
    """B = 8, N = 24: three tiles per XCD on ONE workgroup per XCD (workgroups = 8) -- and on all of them (0), the same bits."""
    case = Case("b8_n24", 8, 24, 24, 11)
    knn = _knn(case)
    x1, x2, p1, p2 = (t.to(DEV) for t in (case.xyz1, case.xyz2, case.p1, case.p2))
    _both_forms(eng, "b8_n24 on 8 workgroups", 8, 24, 24, x1, x2, knn, p1, p2, 8, seed=12)
    one = _launch(eng, 8, 24, 24, x1, x2, knn, p1, p2, workgroups=8)
    assert torch.equal(one, _launch(eng, 8, 24, 24, x1, x2, knn, p1, p2, workgroups=0))


def test_tile16_non_finite_inputs(eng):
    """One +inf and one NaN in one gathered p2 row: non-finite exactly where the reference is
    (tests/test_stage_f64_gpu.py::test_cost_volume_non_finite_inputs asks the same of the 32-position entries)."""
    case = Case("b2_n64", 2, 64, 64, 3)
    knn = _knn(case)
    x1, x2, p1, p2 = (t.to(DEV) for t in (case.xyz1, case.xyz2, case.p1, case.p2))
    r = int(knn[1, 5, 3]) + 64
    p2[r, 7], p2[r, 100] = float("inf"), float("nan")
    par = parameters("cpu", torch.float32)
    ref = _reference(torch.float64, 2, 64, 64, x1, x2, knn, p1, p2, par)
    for term in (None, torch.zeros(2, 256, device=DEV)):
        got = _launch(eng, 2, 64, 64, x1, x2, knn, p1, p2, term=term)[:128, :256]
        bad_g, bad_r = ~torch.isfinite(got), ~torch.isfinite(ref)
        print("\ncost volume tile16: reference non-finite %d, kernel non-finite %d" % (int(bad_r.sum()), int(bad_g.sum())))
        assert bad_r.any()
        assert torch.equal(bad_g, bad_r)


def test_pack_split_layer16_is_its_host_restatement(eng):
    """rtk_pack_split_layer16 against fused.pack_layer_split16, bit for bit, plain and transposed; the scale is rtk_pack_split_layer's."""
    g = torch.Generator(device=DEV).manual_seed(5)
    w = torch.randn(256, 256, generator=g, device=DEV) * torch.logspace(-3, 1, 256, device=DEV)[:, None]
    for transposed, wm in ((0, w), (1, w.t().contiguous())):      # transposed: the layer is wm^T
        img = torch.empty(2 * 256 * 256, dtype=torch.int16, device=DEV)
        inv, inv32 = torch.empty(1, device=DEV), torch.empty(1, device=DEV)
        _lib.call("rtk_pack_split_layer16", 256, 256, wm.data_ptr(), transposed, img.data_ptr(), inv.data_ptr(), F._stream())
        _lib.call("rtk_pack_split_layer", 256, 256, wm.data_ptr(), transposed, torch.empty_like(img).data_ptr(), inv32.data_ptr(), F._stream())
        torch.cuda.synchronize()
        himg, hinv = F.pack_layer_split16(wm.t().contiguous() if transposed else wm)
        assert torch.equal(img, himg.to(DEV)) and float(inv) == hinv == float(inv32)
    assert torch.equal(eng.cv_images16.view(2, -1)[0].sort().values, eng.cv_images.view(2, -1)[0].sort().values)      # the same pieces, reordered


def test_backbone_cost_volume_takes_the_switch(eng, monkeypatch):
    """FusedBackbone._cost_volume on a backbone's own operands (p1 / p2 from the encoder's tap, the per-sample term) with CV_TILE16 off and
    on: two different kernels (the bits differ), both within the bound of the float64 restatement."""
    B, N = 8, 64
    g = torch.Generator(device=DEV).manual_seed(21)
    pc1 = torch.randn(B, 3, N, generator=g, device=DEV) * 5
    pc2 = pc1 + 0.2 * torch.randn(B, 3, N, generator=g, device=DEV)
    f1, f2 = torch.randn(B, 2, N, generator=g, device=DEV), torch.randn(B, 2, N, generator=g, device=DEV)
    monkeypatch.setattr(F, "CV_TILE16", False)
    eng.backbone(pc1, pc2, f1, f2, None)
    torch.cuda.synchronize()
    Bc, Nc, x1, x2, knn, p1, p2, cor1, st = eng._last_cv
    p1ref = p1 if st is None else (p1.view(B, N, 256) + st[:, None, :]).reshape(B * N, 256)
    par = parameters("cpu", torch.float32)
    r64 = _reference(torch.float64, B, N, N, x1, x2, knn, p1ref, p2, par)
    r32 = _reference(torch.float32, B, N, N, x1, x2, knn, p1ref, p2, par)
    got = {}
    for on in (False, True):
        monkeypatch.setattr(F, "CV_TILE16", on)
        cor1.fill_(SENT)
        eng._cost_volume(*eng._last_cv)
        torch.cuda.synchronize()
        got[on] = cor1.clone()
        _check("backbone cost volume CV_TILE16 = %s" % on, got[on], r64, r32)
    assert not torch.equal(got[False], got[True])
