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

from _stage_f64 import cost_volume_f64, patch_cost_f64, sa_scale_f64


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
