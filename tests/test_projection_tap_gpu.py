"""GPU: the cost volume's first-layer projections computed by the encoder's last layer (rtk_pointwise_mlp_tap), the per-sample term
they leave out (the paired rtk_global_terms job) and the cost volume that adds it (rtk_cost_volume_split_term).

Each launch is checked bit for bit against the sequence it replaces: the standalone fp1 launch followed by rtk_pointwise_mlp with the
p1_loc / p2_loc chains, two rtk_global_terms jobs added in torch, and the cost volume fed p1 + term.  The whole backbone is checked
against the float64 oracle: pc1_features / pc2_features are bit-identical to the standalone sequence, and every other output may move
by where one rounding of layer 1's sum sits -- at most 2x the parent tree's distance from float64 plus one fp32 ulp of the tensor's
largest element.

Shapes: the bench's synthetic batch (B = 64, N = 256), B = 3 (not a multiple of 8: the 2-D grids), B = 1 at N = 1024, and the three
real View-of-Delft frames as one padded batch with n_valid."""
import os

import numpy as np
import pytest
import torch

from oracle import track4d_ref as R
from ratrack_amd import fused as F
from ratrack_amd import pointnet2_utils as PU
from ratrack_amd import synth, vod_gt, vod_io
from ratrack_amd.track4d import Args, Track4D

from _util import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ["flow", "h", "cls", "cor", "pc1_features", "pc2_features", "prop"]
SHAPES = ["b64_n256", "b3_n243", "b1_n1024", "real3"]

# Distance max|out - float64| of the parent tree's backbone (the standalone launch sequence) on the inputs of _inputs(), per shape and
# output, measured with commit 9549c1c on an MI355X on 2026-10-16 (backbone_outputs() and oracle_distances() run on that tree's package).
PARENT_DIST = {
    "b64_n256": {"flow": 2.6642e-08, "h": 1.4238e-07, "cls": 6.6458e-07, "cor": 4.9442e-04,
                 "pc1_features": 1.4479e-07, "pc2_features": 1.4907e-07, "prop": 6.6196e-07},
    "b3_n243": {"flow": 2.1274e-08, "h": 7.5281e-08, "cls": 1.1698e-07, "cor": 2.6450e-04,
                "pc1_features": 8.9141e-08, "pc2_features": 1.0602e-07, "prop": 2.5729e-07},
    "b1_n1024": {"flow": 2.2495e-08, "h": 5.2158e-08, "cls": 1.1250e-07, "cor": 6.2227e-05,
                 "pc1_features": 1.1899e-07, "pc2_features": 9.5000e-08, "prop": 1.0686e-07},
    "real3": {"flow": 2.5371e-08, "h": 3.8356e-07, "cls": 1.2616e-06, "cor": 7.1592e-04,
              "pc1_features": 1.4112e-07, "pc2_features": 1.4112e-07, "prop": 1.2930e-06},
}



def _net():
    net = Track4D(Args()).to(DEV).eval()
    synth.fill_state_dict(net.state_dict())      # the bench's weights
    net.invalidate_fused()
    return net


def _inputs(shape):
    """-> pc1, pc2, feature1, feature2 (on the device), n_valid (2, B) or None, the unpadded pairs (real3) or None, h0 (5, B, 128)."""
    if shape == "real3":
        ex = os.path.join(GOLDEN, "vod_example")
        scans = [vod_io.load_radar_bin(os.path.join(ex, "radar_%s.bin" % f)) for f in ("00549", "01047", "01201")]
        pairs = [vod_io.frame_pair_tensors(scans[i], scans[(i + 1) % 3], device=DEV) for i in range(3)]
        pc1, pc2, f1, f2, nv = vod_gt.pad_frame_pairs(pairs, device=DEV)
    else:
        B, N = {"b64_n256": (64, 256), "b3_n243": (3, 243), "b1_n1024": (1, 1024)}[shape]
        d = synth.make_frame_pairs(B, N, case_id=1000)          # bench.py's first resident batch at its default shape
        pc1, pc2, f1, f2 = (torch.from_numpy(d[k]).to(DEV) for k in ("pc1", "pc2", "feature1", "feature2"))
        nv, pairs = None, None
    B = pc1.shape[0]
    h0 = torch.randn(5, B, 128, generator=torch.Generator().manual_seed(17)) * 0.1
    return pc1.contiguous(), pc2.contiguous(), f1.contiguous(), f2.contiguous(), nv, pairs, h0.to(DEV)


def _encoder_operands(eng, pc1, pc2, f1, f2, nv):
    """The encoder's inputs as FusedBackbone.backbone makes them: (geometry, q1)."""
    B, _, N = pc1.shape
    xyz = torch.empty(2 * B, N, 3, device=DEV)
    raw = torch.empty(2 * B * N, 4, device=DEV)
    q1 = torch.empty(2 * B * N, 32, device=DEV)
    nvf = nv.to(torch.int32).reshape(2 * B).contiguous() if nv is not None else None
    geo = F.Geometry(xyz, eng.npoint, knn_frames=B, n_valid=nvf, prepare=(pc1, pc2, f1, f2, raw), q1=(eng.enc_q1_w, q1))
    geo.wait("front")
    if not geo.q1_done:
        F.pointwise(2 * B * N, N, [(raw, 2, False)], eng.enc_q1, q1)
    return geo, q1


@pytest.mark.parametrize("shape", SHAPES)
def test_tap_launch_is_the_standalone_sequence(shape):
    """loc and gmax of the tap launch == the standalone fp1 launch; P12 == rtk_pointwise_mlp with the p1_loc chain (frame 1) / the
    p2_loc chain (frame 2) on loc, without sample bias.  All bit for bit."""
    net = _net()
    eng = F.FusedBackbone(net)
    pc1, pc2, f1, f2, nv, _, _ = _inputs(shape)
    B, _, N = pc1.shape
    with torch.no_grad():
        geo, q1 = _encoder_operands(eng, pc1, pc2, f1, f2, nv)
        loc0 = torch.full((2 * B * N, 128), float("nan"), device=DEV)
        gmax0 = torch.zeros(2 * B, 128, device=DEV)
        F.run_pnhead(eng.enc, geo, q1, out=loc0, gmax=gmax0)
        loc1 = torch.full((2 * B * N, 128), float("nan"), device=DEV)
        gmax1 = torch.zeros(2 * B, 128, device=DEV)
        p12 = torch.full((2 * B * N, 256), float("nan"), device=DEV)
        F.run_pnhead(eng.enc, geo, q1, out=loc1, gmax=gmax1, tap=((eng.p1_loc, eng.p2_loc), B, p12))
        ref1 = F.pointwise(B * N, N, [(loc0[:B * N], 128, False)], eng.p1_loc, torch.empty(B * N, 256, device=DEV))
        ref2 = F.pointwise(B * N, N, [(loc0[B * N:], 128, False)], eng.p2_loc, torch.empty(B * N, 256, device=DEV))
        torch.cuda.synchronize()
    assert torch.isfinite(loc0).all() and float(loc0.abs().max()) > 0
    assert torch.equal(loc1, loc0)
    assert torch.equal(gmax1, gmax0)
    assert torch.equal(p12[:B * N], ref1), "frame 1 (p1_loc)"
    assert torch.equal(p12[B * N:], ref2), "frame 2 (p2_loc)"


@pytest.mark.parametrize("shape", SHAPES)
def test_global_terms_pair_is_the_sum_of_the_two_jobs(shape):
    """s = rtk_global_terms' paired job == sb1 + sb2 from the two separate jobs (a torch fp32 add), with the decoder's job and the
    broadcast in the same launch as in the backbone."""
    net = _net()
    eng = F.FusedBackbone(net)
    pc1, _, _, _, _, _, _ = _inputs(shape)
    B, _, N = pc1.shape
    g = torch.rand(2 * B, 128, generator=torch.Generator().manual_seed(B + N)).to(DEV) * 3.0      # max-pooled ReLU outputs: >= 0
    new = lambda r, c: torch.full((r, c), float("nan"), device=DEV)
    sb1, sb2, sbq, s, sbq2 = new(B, 256), new(B, 256), new(B, 32), new(B, 256), new(B, 32)
    bc, bc2 = new(2 * B * N, 256), new(2 * B * N, 256)
    with torch.no_grad():
        F.global_terms(g, [(eng.p1_glob_wt, eng.p1_glob_b, sb1, 0), (eng.p2_glob_wt, None, sb2, B), (eng.dec_q1_glob_wt, None, sbq, 0)],
                       bcast=bc[:, 128:], n=N)
        F.global_terms(g, [(eng.p1_glob_wt, eng.p1_glob_b, s, 0, eng.p2_glob_wt, B), (eng.dec_q1_glob_wt, None, sbq2, 0)],
                       bcast=bc2[:, 128:], n=N)
        torch.cuda.synchronize()
    assert torch.isfinite(sb1).all() and torch.isfinite(sb2).all()
    assert torch.equal(s, sb1 + sb2)
    assert torch.equal(sbq2, sbq)
    assert torch.equal(bc2[:, 128:], bc[:, 128:])


def _cv_operands(shape):
    pc1, pc2, _, _, _, _, _ = _inputs(shape)
    B, _, N = pc1.shape
    x1 = pc1.permute(0, 2, 1).contiguous()
    x2 = pc2.permute(0, 2, 1).contiguous()
    gen = torch.Generator().manual_seed(7 * B + N)
    p1 = torch.randn(B * N, 256, generator=gen).to(DEV)
    p2 = torch.randn(B * N, 256, generator=gen).to(DEV)
    s = torch.randn(B, 256, generator=gen).to(DEV)
    k1 = PU.knn_point(16, x2, x1)
    return B, N, x1, x2, k1, p1, p2, s


@pytest.mark.parametrize("grid", ["full", "shared", "sliced"])
@pytest.mark.parametrize("shape", SHAPES)
def test_cost_volume_term_is_the_folded_p1(shape, grid, monkeypatch):
    """rtk_cost_volume_split_term(p1, p2, s) == the existing entry point fed p1 + s[b] (a torch fp32 add) and p2, bit for bit: the
    full grid, a share of the CUs (cv_shared) and batches cut into slices (CV_SPLIT_MAX_ROWS lowered); nothing written beyond."""
    net = _net()
    eng = F.FusedBackbone(net)
    B, N, x1, x2, k1, p1, p2, s = _cv_operands(shape)
    eng.cv_shared = grid == "shared"
    if grid == "sliced":
        monkeypatch.setattr(F, "CV_SPLIT_MAX_ROWS", max(N, (B // 3) * N + 7))      # 21 + 21 + 21 + 1, 1 + 1 + 1, ... samples
    p1s = p1 + s.repeat_interleave(N, 0)
    with torch.no_grad():
        ref = torch.full((B * N + 4, 256), 7.0, device=DEV)
        eng._cost_volume(B, N, x1, x2, k1, p1s, p2, ref)
        got = torch.full((B * N + 4, 256), 7.0, device=DEV)
        eng._cost_volume(B, N, x1, x2, k1, p1, p2, got, sample_term=s)
        torch.cuda.synchronize()
    assert torch.all(got[B * N:] == 7.0)
    assert torch.isfinite(ref[:B * N]).all()
    assert torch.equal(got[:B * N], ref[:B * N])


def backbone_outputs(shape, engine_hook=None):
    """FusedBackbone.backbone on _inputs(shape), as float32 host tensors.  engine_hook(eng) may change the engine before the run."""
    net = _net()
    eng = F.FusedBackbone(net)
    if engine_hook is not None:
        engine_hook(eng)
    pc1, pc2, f1, f2, nv, _, h0 = _inputs(shape)
    with torch.no_grad():
        out = eng.backbone(pc1, pc2, f1, f2, h0, n_valid=nv)
        return [o.float().cpu() for o in out]


def oracle_distances(shape, out):
    """{name: (max|out - float64 oracle|, one fp32 ulp of max|oracle|)} for the backbone outputs `out` on _inputs(shape); padded
    batches: every pair through the oracle on its own, unpadded, against its valid columns."""
    net = _net()
    pc1, pc2, f1, f2, nv, pairs, h0 = _inputs(shape)
    sd = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in net.state_dict().items()}
    torch.set_num_threads(min(16, torch.get_num_threads()))
    d = lambda t: t.detach().cpu().double()
    if pairs is None:
        ref = R.backbone(sd, d(pc1), d(pc2), d(f1), d(f2), d(h0), training=False)
        pieces = [[(o.double(), r) for o, r in zip(out, ref)]]
    else:
        pieces = []
        for b, p in enumerate(pairs):
            ref = R.backbone(sd, *[d(t) for t in p], d(h0[:, b:b + 1]), training=False)
            row = []
            for nm, o, r in zip(NAMES, out, ref):
                if nm == "h":
                    row.append((o[:, b].double(), r[:, 0]))
                else:
                    row.append((o[b, ..., :r.shape[-1]].double(), r[0]))      # the valid columns: n_valid of the cloud
            pieces.append(row)
    dist = {}
    for i, nm in enumerate(NAMES):
        e = max(float((a - r).abs().max()) for a, r in (pc[i] for pc in pieces))
        top = max(float(r.abs().max()) for _, r in (pc[i] for pc in pieces))
        dist[nm] = (e, float(np.spacing(np.float32(top))))
    return dist


@pytest.mark.parametrize("shape", SHAPES)
def test_backbone_against_float64(shape):
    """pc1_features / pc2_features bit-identical to the standalone launch sequence (proj_tap off); every other output no further from
    the float64 oracle than 2x the parent tree's distance (PARENT_DIST) + one fp32 ulp of the tensor's largest element."""
    out = backbone_outputs(shape)
    std = backbone_outputs(shape, engine_hook=lambda e: setattr(e, "proj_tap", False))
    dist = oracle_distances(shape, out)
    for nm in NAMES:
        e, ulp = dist[nm]
        print("%s %-13s distance from float64 %.3e (parent %.3e, ulp %.1e)" % (shape, nm, e, PARENT_DIST[shape][nm], ulp))
    assert torch.equal(out[4], std[4]) and torch.equal(out[5], std[5])
    for nm in NAMES:
        if nm in ("pc1_features", "pc2_features"):
            continue
        e, ulp = dist[nm]
        assert e <= 2.0 * PARENT_DIST[shape][nm] + ulp, (shape, nm, e, PARENT_DIST[shape][nm], ulp)
