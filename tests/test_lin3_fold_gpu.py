"""GPU: linear3 composed into fp3 (fused.FOLD_LIN3: fp3 interpolates sa3's 128 channels on the image [W_i W3 | W_s], no linear3
launch) and, with it, the decoder front in one launch (FusedBackbone.pair_readers).

fp3 alone: the composed launch and the two-launch sequence (linear3, then fp3 on its output), each against a float64 restatement of
the sequence on the host; the composed launch may be at most 2x as far from it as the sequence, plus one fp32 ulp of the tensor's
largest element -- both distances come from the same run.  (The margin of 2 is the project's rule for a moved rounding,
tests/test_projection_tap_gpu.py.)

Whole backbone: every output's distance from the float64 oracle at most 2x the parent tree's (PARENT_DIST) plus one ulp; pair_readers
alone moves no bit.  linear3 sits in the encoder, whose features reach all seven outputs: there is no output the fold cannot reach."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import track4d_ref as R
from ratrack_amd import fused as F
from ratrack_amd import synth, vod_gt, vod_io
from ratrack_amd.track4d import Args, Track4D

from _util import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ["flow", "h", "cls", "cor", "pc1_features", "pc2_features", "prop"]
SHAPES = ["b3_n243", "b8_n256", "real3"]

# Distance max|out - float64| of the parent tree's backbone (linear3 and the two readers of cor as launches of their own) on the inputs of
# _inputs(), per shape and output, measured with commit 68576de on an MI355X on 2026-10-18 (backbone_outputs() and oracle_distances() of
# this file run on that tree's package).
PARENT_DIST = {
    "b3_n243": {"flow": 2.1274e-08, "h": 1.0903e-07, "cls": 1.1698e-07, "cor": 2.6450e-04,
                "pc1_features": 8.9141e-08, "pc2_features": 1.0602e-07, "prop": 2.5729e-07},
    "b8_n256": {"flow": 2.5507e-08, "h": 9.4100e-08, "cls": 3.0722e-07, "cor": 2.6917e-04,
                "pc1_features": 9.9363e-08, "pc2_features": 1.1761e-07, "prop": 3.5608e-07},
    "real3": {"flow": 2.3002e-08, "h": 3.0187e-07, "cls": 1.2616e-06, "cor": 4.3832e-04,
              "pc1_features": 1.4112e-07, "pc2_features": 1.4112e-07, "prop": 1.4095e-06},
}


def _net():
    net = Track4D(Args()).to(DEV).eval()
    synth.fill_state_dict(net.state_dict())      # the bench's weights
    net.invalidate_fused()
    return net


def _inputs(shape):
    """As tests/test_projection_tap_gpu._inputs: pc1, pc2, feature1, feature2 (on the device), n_valid (2, B) or None, the unpadded pairs
    (real3) or None, h0 (5, B, 128).  bB_nN: synth.make_frame_pairs(B, N, case_id=1000), the bench's first resident batch."""
    if shape == "real3":
        ex = os.path.join(GOLDEN, "vod_example")
        scans = [vod_io.load_radar_bin(os.path.join(ex, "radar_%s.bin" % f)) for f in ("00549", "01047", "01201")]
        pairs = [vod_io.frame_pair_tensors(scans[i], scans[(i + 1) % 3], device=DEV) for i in range(3)]
        pc1, pc2, f1, f2, nv = vod_gt.pad_frame_pairs(pairs, device=DEV)
    else:
        B, N = (int(x) for x in re.fullmatch(r"b(\d+)_n(\d+)", shape).groups())
        d = synth.make_frame_pairs(B, N, case_id=1000)
        pc1, pc2, f1, f2 = (torch.from_numpy(d[k]).to(DEV) for k in ("pc1", "pc2", "feature1", "feature2"))
        nv, pairs = None, None
    B = pc1.shape[0]
    h0 = torch.randn(5, B, 128, generator=torch.Generator().manual_seed(17)) * 0.1
    return pc1.contiguous(), pc2.contiguous(), f1.contiguous(), f2.contiguous(), nv, pairs, h0.to(DEV)


def backbone_outputs(shape, fold=True, pair=True):
    """FusedBackbone.backbone on _inputs(shape) as float32 host tensors, with the two flags as given."""
    net = _net()
    eng = F.FusedBackbone(net)
    eng.pair_readers = pair
    saved = getattr(F, "FOLD_LIN3", None)
    F.FOLD_LIN3 = fold
    try:
        pc1, pc2, f1, f2, nv, _, h0 = _inputs(shape)
        with torch.no_grad():
            out = eng.backbone(pc1, pc2, f1, f2, h0, n_valid=nv)
            return [o.float().cpu() for o in out]
    finally:
        F.FOLD_LIN3 = saved


def oracle_distances(shape, out):
    """{name: (max|out - float64 oracle|, one fp32 ulp of max|oracle|)}, as tests/test_projection_tap_gpu.oracle_distances."""
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


# ---- fp3 alone --------------------------------------------------------------------------------------------------------------------

def _fp3_f64(sd, prefix, sa3, t2, idx, d2, nu3, S):
    """The sequence in float64 on the host: l3 = W3 sa3 + b3, three-NN inverse-distance interpolation of l3 (known rows beyond the
    sample's unique count read as its row 0), relu(W [interp | t2[:, :64]] + b) with BatchNorm folded."""
    w, b = F.fold_bn(sd[prefix + "fp3.mlp.layer0.conv.weight"], prefix + "fp3.mlp.layer0.bn.bn", sd)
    w, b = w.cpu(), b.cpu()
    wl, bl = sd[prefix + "linear3.weight"].double().cpu(), sd[prefix + "linear3.bias"].double().cpu()
    samples = sa3.shape[0] // S
    l3 = (sa3.double().cpu() @ wl.t() + bl).view(samples, S, 64)
    idx = idx.cpu().long().view(samples, S, 3)
    idx = torch.where(idx < nu3.cpu().long().view(samples, 1, 1), idx, torch.zeros_like(idx))
    r = 1.0 / (d2.double().cpu().view(samples, S, 3).sqrt() + 1e-8)
    wgt = r / r.sum(-1, keepdim=True)
    known = torch.gather(l3.unsqueeze(1).expand(-1, S, -1, -1), 2, idx.unsqueeze(-1).expand(-1, -1, -1, 64))      # (samples, S, 3, 64)
    interp = (known * wgt.unsqueeze(-1)).sum(2).view(samples * S, 64)
    x = torch.cat([interp, t2[:, :64].double().cpu()], 1)
    return torch.relu(x @ w.t() + b)


@pytest.mark.parametrize("head", ["pn_head.", "fd_layer.mse."])
def test_fp3_composed_against_the_sequence_in_float64(head):
    net = _net()
    eng = F.FusedBackbone(net)
    W = eng.enc if head == "pn_head." else eng.dec
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    d = synth.make_frame_pairs(3, 243, case_id=1000)
    xyz = torch.from_numpy(np.concatenate([d["pc1"], d["pc2"]], 0)).to(DEV).permute(0, 2, 1).contiguous()      # (6, 243, 3)
    S_, S = xyz.shape[0], eng.npoint
    g = torch.Generator().manual_seed(5)
    sa3 = torch.rand(S_ * S, 128, generator=g).to(DEV) * 2.0          # max-pooled ReLU outputs: >= 0
    t2 = torch.randn(S_ * S, 192, generator=g).to(DEV)
    with torch.no_grad():
        geo = F.Geometry(xyz, S)
        nu = geo.nuniq
        d2, idx, m = geo.nn["fp3"]
        tab = (m, idx.reshape(-1, 3), d2.reshape(-1, 3), nu[2])
        l3 = F.pointwise(S_ * S, S, [(sa3, 128, False)], W.lin3, torch.empty(S_ * S, 64, device=DEV), row_nuniq=nu[2])
        seq = F.pointwise(S_ * S, S, [(t2[:, 0:64], 64, False)], W.fp["fp3"], torch.zeros(S_ * S, 128, device=DEV), row_nuniq=nu[1],
                          interp=(l3, 64) + tab)
        com = F.pointwise(S_ * S, S, [(t2[:, 0:64], 64, False)], W.fp3c, torch.zeros(S_ * S, 128, device=DEV), row_nuniq=nu[1],
                          interp=(sa3, 128) + tab)
        torch.cuda.synchronize()
    assert int(nu[2].min()) < S and int(nu[1].min()) < S              # aliased known rows occur; rows beyond nuniq are not written
    ref = _fp3_f64(sd, head, sa3, t2, idx, d2, nu[2], S)
    live = (torch.arange(S).view(1, S) < nu[1].cpu().view(S_, 1)).reshape(-1)
    e_seq = float((seq.cpu().double() - ref)[live].abs().max())
    e_com = float((com.cpu().double() - ref)[live].abs().max())
    ulp = float(np.spacing(np.float32(ref[live].abs().max())))
    print("%s fp3: sequence %.3e, composed %.3e from float64 (ulp %.1e)" % (head, e_seq, e_com, ulp))
    assert float(ref[live].abs().max()) > 0 and e_seq < 1e-3 * float(ref[live].abs().max())
    assert e_com <= 2.0 * e_seq + ulp


# ---- whole backbone ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_backbone_against_float64(shape):
    out = backbone_outputs(shape)
    dist = oracle_distances(shape, out)
    for nm in NAMES:
        e, ulp = dist[nm]
        print("%s %-13s distance from float64 %.3e (parent %.3e, ulp %.1e)" % (shape, nm, e, PARENT_DIST[shape][nm], ulp))
    for nm in NAMES:
        e, ulp = dist[nm]
        assert e <= 2.0 * PARENT_DIST[shape][nm] + ulp, (shape, nm, e, PARENT_DIST[shape][nm], ulp)


@pytest.mark.parametrize("shape", SHAPES)
def test_pair_readers_moves_no_bit(shape):
    """With the fold off, the backbone with the decoder front in one launch is the backbone with the two standalone launches, in
    every output."""
    std = backbone_outputs(shape, fold=False, pair=False)
    got = backbone_outputs(shape, fold=False, pair=True)
    for nm, a, b in zip(NAMES, got, std):
        assert torch.isfinite(b).all(), nm
        assert torch.equal(a, b), nm
