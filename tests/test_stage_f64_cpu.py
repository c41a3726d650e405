"""CPU: the float64 restatements of tests/_stage_f64.py against the module classes (the reference's formulation: grouped tensors,
concatenated inputs, un-folded BatchNorm) in float64 on the CPU, with the oracle's index ops -- the ground the GPU tests
(tests/test_stage_f64_gpu.py) measure the grouped stage kernels on."""
import pytest
import torch

from oracle import pointnet2_ref as R
from ratrack_amd import fused as F
from ratrack_amd import model_utils as MU
from ratrack_amd import pointnet2_utils as PU
from ratrack_amd.pointnet2_modules import PointnetSAModuleMSG

from _cost_volume_cases import CASES as CV_CASES, LOOPING as CV_LOOPING, band_share, case_by_name, parameters, tiles_per_workgroup
from _stage_f64 import MARGIN, _gather, clear_of_zero, cost_volume_f64, decode_sign_masks, margin, patch_cost_f64, sa_scale_f64, weight_net


def _group_f64(features, idx):
    """grouping_operation in any dtype: (B, C, N), (B, S, ns) -> (B, C, S, ns)."""
    return torch.stack([f[:, i.long()] for f, i in zip(features, idx)])


def _oracle_ops(monkeypatch):
    monkeypatch.setattr(PU, "ball_query", lambda r, ns, xyz, new_xyz: R.ball_query(r, ns, xyz.float(), new_xyz.float()))
    monkeypatch.setattr(PU, "grouping_operation", _group_f64)
    monkeypatch.setattr(MU, "knn_point", lambda k, xyz, new_xyz: R.knn_point(k, xyz.float().contiguous(), new_xyz.float().contiguous()))


def _randomise_bn(module, gen):
    for m in module.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            c = m.num_features
            m.weight.data = 0.5 + torch.rand(c, generator=gen, dtype=torch.float64)
            m.bias.data = 0.2 * torch.randn(c, generator=gen, dtype=torch.float64)
            m.running_mean = 0.3 * torch.randn(c, generator=gen, dtype=torch.float64)
            m.running_var = 0.5 + torch.rand(c, generator=gen, dtype=torch.float64)


# (radius, nsample, mlp after the 3 + Cf input channels, Cf): the six MSG scales of a PNHead (model_utils.py:176-178)
SA_SCALES = [(2.0, 4, [16, 16, 32], 5), (4.0, 8, [16, 16, 32], 5), (4.0, 8, [32, 32], 32), (8.0, 16, [32, 64], 32),
             (8.0, 16, [64, 64], 64), (16.0, 32, [64, 64], 64)]


@pytest.mark.parametrize("radius,ns,mlp,cf", SA_SCALES)
@pytest.mark.parametrize("dups", [False, True])
def test_sa_scale_restatement_matches_the_module(radius, ns, mlp, cf, dups, monkeypatch):
    """One scale of PointnetSAModuleMSG (grouped [xyz - centroid || features] -> SharedMLP with BatchNorm -> max_pool2d) against
    sa_scale_f64 on the fold_bn weights and the per-point projection q = Wf.features.  dups: the source rows >= u are copies of
    row 0 (a level after furthest-point sampling exhausted its cloud) -- the module reads them, the restatement aliases them to row
    0 through src_nuniq while their q rows hold garbage."""
    _oracle_ops(monkeypatch)
    monkeypatch.setattr(PointnetSAModuleMSG, "project_first", False)
    gen = torch.Generator().manual_seed(ns * 100 + mlp[-1] + dups)
    B, n, S = 2, 96, 40
    mod = PointnetSAModuleMSG(npoint=S, radii=[radius], nsamples=[ns], mlps=[[3 + cf] + mlp]).double().eval()
    _randomise_bn(mod, gen)
    xyz = torch.rand(B, n, 3, generator=gen, dtype=torch.float64) * radius * 3
    feats = torch.randn(B, cf, n, generator=gen, dtype=torch.float64)
    u = None
    if dups:
        u = torch.tensor([n - 17, n], dtype=torch.int32)
        feats[0, :, n - 17:] = feats[0, :, :1]
    new_xyz = xyz[:, :S].clone()
    new_xyz[1, 3] = 1e3                                                       # an empty ball: its idx row stays zero
    with torch.no_grad():
        _, ref = mod(xyz, feats, new_xyz)                                     # (B, cout, S)
    sd = mod.state_dict()
    ws = []
    while "mlps.0.layer%d.conv.weight" % len(ws) in sd:
        i = len(ws)
        ws.append(F.fold_bn(sd["mlps.0.layer%d.conv.weight" % i], "mlps.0.layer%d.bn.bn" % i, sd))
    w1, b1 = ws[0]
    q = feats.permute(0, 2, 1) @ w1[:, 3:].T
    if dups:
        q[0, n - 17:] = 1e30                                                  # never read: aliased to row 0
    idx = R.ball_query(radius, ns, xyz.float(), new_xyz.float())
    assert (idx[1, 3] == 0).all()
    got = sa_scale_f64(xyz, new_xyz, idx, q, w1[:, :3], b1, ws[1:], src_nuniq=u)
    assert (ref > 0).any()
    torch.testing.assert_close(got, ref.permute(0, 2, 1), rtol=1e-12, atol=1e-12)


def test_sa_scale_restatement_writes_only_live_rows_at_the_offset():
    gen = torch.Generator().manual_seed(4)
    B, n, S, ns = 2, 20, 6, 4
    xyz, new_xyz = torch.rand(B, n, 3, generator=gen, dtype=torch.float64), torch.rand(B, S, 3, generator=gen, dtype=torch.float64)
    idx = torch.randint(0, n, (B, S, ns), generator=gen, dtype=torch.int32)
    q = torch.randn(B, n, 16, generator=gen, dtype=torch.float64)
    wx, b1 = torch.randn(16, 3, generator=gen, dtype=torch.float64), torch.randn(16, generator=gen, dtype=torch.float64)
    layers = [(torch.randn(32, 16, generator=gen, dtype=torch.float64), torch.randn(32, generator=gen, dtype=torch.float64))]
    y = sa_scale_f64(xyz, new_xyz, idx, q, wx, b1, layers)
    out = torch.full((B * S, 40), -5.0, dtype=torch.float64)
    got = sa_scale_f64(xyz, new_xyz, idx, q, wx, b1, layers, out=out, out_offset=8, dst_nuniq=torch.tensor([4, 6]))
    want = out.clone()
    want[0:4, 8:40] = y[0, :4]
    want[S:2 * S, 8:40] = y[1]
    assert torch.equal(got, want)


@pytest.mark.parametrize("B,N", [(2, 40), (1, 17)])
def test_cost_volume_and_patch_cost_restatements_match_the_module(B, N, monkeypatch):
    """FeatureCorrelator in the reference's formulation (the 2 D + 3 channel concatenation [f1 || f2[idx] || direction], three
    convs with LeakyReLU, WeightNet 1, weighted sum; then kNN in frame 1, WeightNet 2, weighted sum) against cost_volume_f64
    (conv 0 split by input segment, its bias in p1) followed by patch_cost_f64.  Frame 2 holds every point twice (repeated
    neighbours) and frame 1's point 0 (a neighbour at distance zero)."""
    _oracle_ops(monkeypatch)
    gen = torch.Generator().manual_seed(B * 100 + N)
    D, C = 24, 64
    mod = MU.FeatureCorrelator(16, in_channel=2 * D + 3, mlp=[C, C, C]).double().eval()
    mod.project_first = False
    for p in mod.parameters():
        p.data = torch.randn(p.shape, generator=gen, dtype=torch.float64) / max(p.shape[1] if p.dim() > 1 else 1, 1) ** 0.5
    pc1 = torch.randn(B, 3, N, generator=gen, dtype=torch.float64)
    pc2 = torch.randn(B, 3, N, generator=gen, dtype=torch.float64)
    pc2[:, :, N // 2:] = pc2[:, :, :N - N // 2]
    pc2[:, :, 1] = pc1[:, :, 0]
    f1, f2 = torch.randn(B, D, N, generator=gen, dtype=torch.float64), torch.randn(B, D, N, generator=gen, dtype=torch.float64)
    with torch.no_grad():
        ref = mod(pc1, pc2, f1, f2).permute(0, 2, 1)                         # (B, N, C)
    x1, x2 = pc1.permute(0, 2, 1).contiguous(), pc2.permute(0, 2, 1).contiguous()
    k12 = R.knn_point(16, x2.float(), x1.float())
    k11 = R.knn_point(16, x1.float(), x1.float())
    assert (k12[:, 0, 0] == 1).all()
    conv = lambda m: (m.weight[:, :, 0, 0].detach(), m.bias.detach())
    w0, b0 = conv(mod.mlp_convs[0])
    p1 = f1.permute(0, 2, 1) @ w0[:, :D].T + b0
    p2 = f2.permute(0, 2, 1) @ w0[:, D:2 * D].T
    wn1 = [conv(m) for m in mod.weightnet1.mlp_convs]
    wn2 = [conv(m) for m in mod.weightnet2.mlp_convs]
    cv = cost_volume_f64(x1, x2, k12, p1, p2, w0[:, 2 * D:], [conv(mod.mlp_convs[1]), conv(mod.mlp_convs[2])], wn1)
    got = patch_cost_f64(x1, k11, cv, wn2)
    assert ref.abs().max() > 0
    torch.testing.assert_close(got, ref, rtol=1e-12, atol=1e-12 * float(ref.abs().max()))


# ---- what tests/test_cost_volume_bwd_gpu.py stands on ---------------------------------------------------------------------------
def _cv_small(dtype, seed=8):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).to(dtype)
    B, n1, n2 = 2, 9, 21
    knn = torch.randint(0, n2, (B, n1, 16), generator=gen)
    layers = [(r(256, 256) * 0.06, r(256) * 0.1), (r(256, 256) * 0.06, r(256) * 0.1)]
    wn = [(r(8, 3), r(8)), (r(8, 8) * 0.4, r(8)), (r(256, 8) * 0.4, r(256))]
    return r(B, n1, 3), r(B, n2, 3), knn, r(B, n1, 256), r(B, n2, 256), r(256, 3) * 0.3, layers, wn


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_cost_volume_restatement_with_given_decisions(dtype):
    """decisions=None is the function as it was (restated here), bit for bit; so is decisions = [z > 0] of its own activations, whose
    product with the slope is leaky_relu's; and a flipped decision takes the other slope."""
    xyz1, xyz2, knn, p1, p2, wd, layers, wn = args = _cv_small(dtype)
    lk = lambda t: torch.nn.functional.leaky_relu(t, 0.1)
    d = _gather(xyz2, knn) - xyz1[:, :, None, :]
    x = lk(p1[:, :, None, :] + _gather(p2, knn) + d @ wd.T)
    for W, b in layers:
        x = lk(x @ W.T + b)
    old = (weight_net(d, wn) * x).sum(2)
    assert torch.equal(cost_volume_f64(*args), old)
    out, acts = cost_volume_f64(*args, with_acts=True)
    assert torch.equal(out, old) and torch.equal(acts[2], x) and all(a.shape == (2, 9, 16, 256) for a in acts)
    dec = [a > 0 for a in acts]
    assert all(0.2 < float(m.double().mean()) < 0.8 for m in dec)
    out2, acts2 = cost_volume_f64(*args, decisions=dec, with_acts=True)
    assert torch.equal(out2, old) and all(torch.equal(a, b) for a, b in zip(acts, acts2))
    flipped = [dec[0], dec[1], ~dec[2]]
    _, acts3 = cost_volume_f64(*args, decisions=flipped, with_acts=True)
    neg = ~dec[2]
    torch.testing.assert_close(acts3[2][neg], acts[2][neg] * 10, rtol=1e-6, atol=0)
    torch.testing.assert_close(acts3[2][dec[2]], acts[2][dec[2]] * 0.1, rtol=1e-6, atol=0)


def test_sign_mask_decoder_inverts_a_literal_encoder():
    """Bit 4v + r of word (position, g) <-> channel 16v + 4g + r, bit 63 included (the words are signed)."""
    gen = torch.Generator().manual_seed(1)
    M = 37
    want = torch.rand(M, 256, generator=gen) < 0.5
    want[0], want[1] = True, False
    want[2] = False
    want[2, 16 * 15 + 4 * 2 + 3] = True                                       # bit 63 of word 2 alone
    words = torch.zeros(M, 4, dtype=torch.int64)
    for m in range(M):
        for g in range(4):
            w = 0
            for v in range(16):
                for r in range(4):
                    if want[m, 16 * v + 4 * g + r]:
                        w |= 1 << (4 * v + r)
            words[m, g] = w - (1 << 64) if w >= 1 << 63 else w
    assert int(words[2, 2]) == -(1 << 63) and int(words[0, 0]) == -1
    assert torch.equal(decode_sign_masks(words), want)


def test_margin_helpers_on_one_cloud_and_two():
    """margin / clear_of_zero take the directions xyz2[knn] - xyz1: one cloud given twice is the patch cost's case."""
    gen = torch.Generator().manual_seed(3)
    x1, x2 = torch.randn(2, 20, 3, generator=gen, dtype=torch.float64), torch.randn(2, 30, 3, generator=gen, dtype=torch.float64)
    knn = torch.randint(0, 30, (2, 20, 16), generator=gen)
    wn = [(torch.randn(8, 3, generator=gen, dtype=torch.float64), torch.randn(8, generator=gen, dtype=torch.float64)),
          (torch.randn(8, 8, generator=gen, dtype=torch.float64), torch.randn(8, generator=gen, dtype=torch.float64)),
          (torch.randn(256, 8, generator=gen, dtype=torch.float64), torch.randn(256, generator=gen, dtype=torch.float64))]
    d = _gather(x2, knn) - x1[:, :, None, :]
    z = [d @ wn[0][0].T + wn[0][1]]
    z.append(torch.relu(z[0]) @ wn[1][0].T + wn[1][1])
    z.append(torch.relu(z[1]) @ wn[2][0].T + wn[2][1])
    assert margin(x1, x2, knn, wn) == min(float(t.abs().min() / t.abs().max()) for t in z)
    keep, mixed = clear_of_zero(x1, x2, knn, wn)
    near = [t.abs() < MARGIN * t.abs().max() for t in z]
    want = ~(near[0].any(3).any(2) | near[1].any(3).any(2))[:, :, None] & ~near[2].any(2)
    assert keep.shape == (2, 20, 256) and torch.equal(keep, want) and 0 < mixed <= 272


@pytest.mark.parametrize("name", [c[0] for c in CV_CASES])
def test_cost_volume_backward_cases_meet_their_conditions(name):
    """What tests/test_cost_volume_bwd_gpu.py requires of a case's inputs and the float64 reference alone decides, on the host's
    neighbour table: at least half of the cotangent clear of a WeightNet decision, at least 136 of the 272 WeightNet channels changing
    sign between positions, at most 1e-3 of the leaky-ReLU pre-activations within the forward's bound of zero, and for the looping
    shapes more than one tile per workgroup with the last query of some sample keeping part of its cotangent."""
    case = case_by_name(name)
    knn = case.knn_host()
    assert knn.shape == (case.B, case.n1, 16) and int(knn.max()) < case.n2
    if case.live is not None:
        assert all(int(knn[b].max()) < v for b, v in enumerate(case.live))
    par = parameters("cpu", torch.float64)
    keep, mixed = case.keep_mask(knn, par)
    kept = float(keep.double().mean())
    _, acts, _ = case.reference(knn, par, torch.float64, "cpu", grads=False)
    share = band_share(acts)
    print("\n%s: kept %.3f, mixed %d, band share %.1e" % (name, kept, mixed, share))
    assert kept >= 0.5 and mixed >= 136 and share <= 1e-3, (kept, mixed, share)
    if name in CV_LOOPING:
        for kernel, (tiles, wgs) in tiles_per_workgroup(case.B, case.n1).items():
            assert tiles > wgs, (kernel, tiles, wgs)
        assert case.n1 % 8 != 0 and case.n1 % 4 != 0
        assert keep.view(case.B, case.n1, 256)[:, -1].any(1).any()
