"""CPU: the float64 restatement of the per-point chains (tests/_pointwise_f64.py) against the module classes in float64 on the CPU,
with the oracle's three-NN tables -- the ground the GPU tests (tests/test_pointwise_f64_gpu.py) measure the kernels on."""
import pytest
import torch

from oracle import pointnet2_ref as R
from ratrack_amd import fused as F
from ratrack_amd import pointnet2_utils as PU
from ratrack_amd.pointnet2_modules import PointnetFPModule

from _pointwise_f64 import ACT_NONE, ACT_RELU, ACT_SIGMOID, pair_f64, pointwise_f64, tap_f64


def _randomise_bn(module, gen):
    for m in module.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            c = m.num_features
            m.weight.data = 0.5 + torch.rand(c, generator=gen, dtype=torch.float64)
            m.bias.data = 0.2 * torch.randn(c, generator=gen, dtype=torch.float64)
            m.running_mean = 0.3 * torch.randn(c, generator=gen, dtype=torch.float64)
            m.running_var = 0.5 + torch.rand(c, generator=gen, dtype=torch.float64)


def _oracle_interp(monkeypatch):
    """three_nn from the oracle (fp32 coordinates, as the kernels' tables), the distances and the interpolation in float64."""
    def three_nn(unknown, known):
        d2, idx = R.three_nn(unknown.float().contiguous(), known.float().contiguous())
        return torch.sqrt(d2.double()), idx

    def three_interpolate(feats, idx, weight):          # (B, C, m), (B, n, 3), (B, n, 3) -> (B, C, n)
        g = torch.stack([f[:, i.long()] for f, i in zip(feats, idx)])      # (B, C, n, 3)
        return (g * weight[:, None]).sum(-1)
    monkeypatch.setattr(PU, "three_nn", three_nn)
    monkeypatch.setattr(PU, "three_interpolate", three_interpolate)


@pytest.mark.parametrize("cint,cskip", [(128, 0), (128, 32), (64, 64), (20, 6)])
@pytest.mark.parametrize("dups", [False, True])
def test_fp_module_matches_the_restatement(cint, cskip, dups, monkeypatch):
    """PointnetFPModule (three_nn, inverse-distance weights, three_interpolate, cat skip, Conv + BatchNorm with randomised
    statistics + ReLU) against pointwise_f64 on the fold_bn weights.  Unknown points on known points (one zero distance: weight 1)
    and, with dups, known rows >= u that are copies of known row 0 with unknown points on top of them: the table names the copies,
    the module reads them, the restatement reads row 0 through nuniq while their rows hold 1e30.  (20, 6): segments that are no
    multiple of 16 channels."""
    _oracle_interp(monkeypatch)
    gen = torch.Generator().manual_seed(cint + 3 * cskip + dups)
    B, n, m = 2, 50, 24
    mod = PointnetFPModule(mlp=[cint + cskip, 128]).double().eval()
    _randomise_bn(mod, gen)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    known, unknown = rn(B, m, 3).float().double() * 4, rn(B, n, 3).float().double() * 4
    kf = rn(B, m, cint)
    unknown[:, :5] = known[:, 3:8]
    nu = None
    if dups:
        u = torch.tensor([m - 7, m - 2], dtype=torch.int32)
        for s in range(B):
            known[s, int(u[s]):] = known[s, 0]
            kf[s, int(u[s]):] = kf[s, 0]
        unknown[:, 10:14] = known[:, :1]
        nu = u
    skip = rn(B, n, cskip) if cskip else None
    with torch.no_grad():
        ref = mod(unknown, known, skip.permute(0, 2, 1).contiguous() if cskip else None, kf.permute(0, 2, 1).contiguous())   # (B, 128, n)
    sd = mod.state_dict()
    w, b = F.fold_bn(sd["mlp.layer0.conv.weight"], "mlp.layer0.bn.bn", sd)
    d2, idx = R.three_nn(unknown.float().contiguous(), known.float().contiguous())
    assert (d2[:, :5, 0] == 0).all()
    kf_r = kf.clone()
    if dups:
        assert all(bool((idx[s, 10:14] >= int(nu[s])).any()) for s in range(B)), "the table must name duplicate rows"
        for s in range(B):
            kf_r[s, int(nu[s]):] = 1e30
    # the layer's input columns in the kernel's layout: every segment padded to 16 channels
    wi = torch.zeros(128, F.ceil16(cint) + F.ceil16(cskip), dtype=torch.float64)
    wi[:, :cint] = w[:, :cint]
    wi[:, F.ceil16(cint):F.ceil16(cint) + cskip] = w[:, cint:]
    got, cm = pointwise_f64(n, [(skip, False)] if cskip else [], [(wi, b, ACT_RELU)], interp=(kf_r, idx, d2.double(), nu), colmax=True)
    assert (ref > 0).any()
    torch.testing.assert_close(got, ref.permute(0, 2, 1), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(cm, torch.max(ref, -1)[0], rtol=1e-12, atol=1e-12)     # models/track4d.py:89-92


def test_broadcast_source_is_a_sample_bias():
    """A four-layer head on [local 128 || per-sample 128 broadcast over the sample's points] against the same head with the
    broadcast columns of layer 0 moved into sample_bias -- the identity the engine relies on (the global halves of the cost volume's,
    the decoder's and the flow head's first layers are rtk_global_terms jobs)."""
    gen = torch.Generator().manual_seed(2)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    B, n = 3, 21
    loc, glob = rn(B, n, 128), rn(B, 128)
    dims = [(128, 256), (64, 128), (32, 64), (3, 32)]
    layers = [(rn(co, ci) / ci ** 0.5, rn(co) * 0.1, ACT_RELU if i < 3 else ACT_NONE) for i, (co, ci) in enumerate(dims)]
    full = pointwise_f64(n, [(loc, False), (glob, True)], layers)
    w0, b0, a0 = layers[0]
    moved = pointwise_f64(n, [(loc, False)], [(w0[:, :128], torch.zeros(128, dtype=torch.float64), a0)] + layers[1:],
                          sample_bias=glob @ w0[:, 128:].T + b0)
    direct = torch.cat([loc, glob[:, None, :].expand(B, n, 128)], 2)
    for i, (w, b, _) in enumerate(layers):
        direct = direct @ w.T + b
        direct = torch.relu(direct) if i < 3 else direct
    assert full.shape == (B, n, 3)
    torch.testing.assert_close(full, direct, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(moved, full, rtol=1e-12, atol=1e-12)


def test_column_maximum_output_layouts_and_live_rows():
    """colmax == torch.max(features, -1) over the live rows, its padding channels act(0); rows at or past row_nuniq, channels at
    or past out_channels and rows after the last keep what the buffer held, point-major and channel-major."""
    gen = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    B, n = 2, 9
    x = rn(B, n, 40)
    layers = [(rn(24, 48), rn(24), ACT_RELU), (rn(5, 32), rn(5), ACT_SIGMOID)]
    y = torch.sigmoid(torch.relu(x @ layers[0][0][:, :40].T + layers[0][1]) @ layers[1][0][:, :24].T + layers[1][1])
    nu = torch.tensor([4, 9], dtype=torch.int32)
    res, cm = pointwise_f64(n, [(x, False)], layers, row_nuniq=nu, colmax=True)
    torch.testing.assert_close(res, y, rtol=1e-12, atol=1e-12)
    assert cm.shape == (B, 16)
    torch.testing.assert_close(cm[0, :5], torch.max(y[0, :4].T, -1)[0], rtol=1e-12, atol=0)
    torch.testing.assert_close(cm[1, :5], torch.max(y[1].T, -1)[0], rtol=1e-12, atol=0)
    assert (cm[:, 5:] == 0.5).all()
    out = torch.full((B * n + 3, 8), -5.0, dtype=torch.float64)
    got = pointwise_f64(n, [(x, False)], layers, out_channels=3, out=out, row_nuniq=nu)
    want = out.clone()
    want[0:4, :3] = y[0, :4, :3]
    want[n:2 * n, :3] = y[1, :, :3]
    assert torch.equal(got, want)
    out_cm = torch.full((B, 3, n), -5.0, dtype=torch.float64)
    got = pointwise_f64(n, [(x, False)], layers, out_channels=3, out=out_cm, channel_major=True, row_nuniq=nu)
    want = out_cm.clone()
    want[0, :, :4] = y[0, :4, :3].T
    want[1] = y[1, :, :3].T
    assert torch.equal(got, want)


def test_tap_and_pair_are_their_standalone_launches():
    gen = torch.Generator().manual_seed(6)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    B, n, m = 4, 7, 5
    interp = (rn(B, m, 128), torch.randint(0, m, (B, n, 3), generator=gen), rn(B, n, 3).abs(), None)
    layer = (rn(128, 128) / 11, rn(128) * 0.1, ACT_RELU)
    proj = [(rn(256, 128) / 11, rn(256) * 0.1, ACT_NONE) for _ in range(2)]
    out, cm, po = tap_f64(n, interp, layer, proj, 3)
    assert torch.equal(cm, out.amax(1)) and po.shape == (B, n, 256)
    assert torch.equal(po[:3], out[:3] @ proj[0][0].T + proj[0][1]) and torch.equal(po[3:], out[3:] @ proj[1][0].T + proj[1][1])
    srcs = [(rn(B, n, 2), False), (rn(B, n, 128), False), (rn(B, n, 256), False)]
    la = (rn(32, 400) * 0.05, rn(32) * 0.1, ACT_NONE)
    lb = [(rn(co, ci) / ci ** 0.5, rn(co) * 0.1, a) for (co, ci), a in zip([(128, 256), (64, 128), (32, 64), (1, 32)],
                                                                          [ACT_RELU] * 3 + [ACT_SIGMOID])]
    sb = rn(B, 32)
    a, b = pair_f64(n, srcs, sb, la, lb, 1)
    xin = torch.cat([torch.nn.functional.pad(srcs[0][0], (0, 14)), srcs[1][0], srcs[2][0]], 2)
    torch.testing.assert_close(a, xin @ la[0].T + la[1] + sb[:, None, :], rtol=1e-12, atol=1e-12)
    assert b.shape == (B, 1, n) and torch.equal(b, pointwise_f64(n, srcs[-1:], lb, out_channels=1).permute(0, 2, 1))
