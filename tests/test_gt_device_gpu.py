"""GPU: ground truth and scoring on the device (ratrack_amd/gt_device.py, csrc/gt_eval.hip) against the host path it stands in
for -- vod_gt.filter_object_points / gt_scene_flow and metrics.eval_scene_flow / eval_motion_seg run per stream on the stream's
valid slice -- and against the reference's own values (tests/golden/train_gt_real.npz, eval_*.npz)."""
import os
import warnings

import numpy as np
import pytest
import torch

import _gt_util as U
from _util import EVAL_CASES, GOLDEN, load_case, reference_state_dict
from ratrack_amd import gt_device as G
from ratrack_amd import metrics as M
from ratrack_amd import synth, tracker as T, vod_gt, vod_io
from ratrack_amd.track4d import Args, Track4D

pytestmark = pytest.mark.gpu
DEV = "cuda"
U24 = 2.0 ** -24


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check_stream_against_host(gt, bb, b, h, n1, N):
    """Membership, ids and counts of stream b equal the host path's, exactly; padding columns take part in nothing."""
    cls = gt.gt_cls[b].cpu().numpy()
    obj = gt.obj_id[b].cpu().numpy()
    idx = gt.box_index[b].cpu().numpy()
    assert cls.dtype == np.bool_
    assert np.array_equal(cls[:n1], h["cls"]), b
    assert np.array_equal(obj[:n1], h["obj_id"]), b
    assert not cls[n1:].any() and (obj[n1:] == -1).all() and (idx[n1:] == -1).all(), b
    ids1, ids2 = bb.host["box_id"][0, b], bb.host["box_id"][1, b]
    assert np.array_equal(obj[:n1], np.where(idx[:n1] >= 0, ids1[np.maximum(idx[:n1], 0)], -1)), b
    c1, c2 = gt.counts1[b].cpu().numpy(), gt.counts2[b].cpu().numpy()
    assert c1.tolist() == [h["counts1"].get(int(i), 0) if i >= 0 else 0 for i in ids1], b
    assert c2.tolist() == [h["counts2"].get(int(i), 0) if i >= 0 else 0 for i in ids2], b
    warp, comp = gt.gt_warp[b].cpu().numpy(), gt.pc1_comp[b].cpu().numpy()
    assert np.array_equal(warp[:, n1:], comp[:, n1:]), b
    return cls, obj, idx, warp, comp


# ---- ground truth ----------------------------------------------------------------------------------------------------------
def test_real_frames_match_the_reference_fixture_and_the_host_path():
    per_stream, pairs, egos = U.real_streams()
    pc1, pc2, f1, f2, nv = vod_gt.pad_frame_pairs(pairs, device=DEV)
    assert tuple(pc1.shape) == (3, 3, 352) and nv.tolist() == [[352, 322, 242], [242, 352, 322]]
    bb = G.pack_boxes(per_stream, 16, DEV)
    gt = G.ground_truth(pc1, pc2, bb, n_valid=nv)
    gt.check()
    g = np.load(os.path.join(GOLDEN, "train_gt_real.npz"), allow_pickle=False)
    p1, p2 = pc1.cpu().numpy(), pc2.cpu().numpy()
    for b in range(3):
        n1, n2 = int(nv[0, b]), int(nv[1, b])
        h = U.host_ground_truth(per_stream[b], p1[b], p2[b], n1, n2, egos[b])
        cls, obj, idx, warp, comp = _check_stream_against_host(gt, bb, b, h, n1, 352)
        assert 0 < cls.sum() < n1
        if b < 2:      # the reference's own GT code on these files
            pre = "p%d_" % b
            assert np.array_equal(cls[:n1], g[pre + "gt_cls"])
            e_warp = float(np.abs(warp[:, :n1] - g[pre + "gt"][0]).max())
            e_comp = float(np.abs(comp[:, :n1] - g[pre + "pc1_comp"][0]).max())
            print("stream %d: max |gt_warp - fixture| %.3e, max |pc1_comp - fixture| %.3e" % (b, e_warp, e_comp))
            assert e_warp <= 2e-5 and e_comp <= 2e-5
        assert float(np.abs(warp[:, :n1] - h["gt"]).max()) <= 2e-5 and float(np.abs(comp[:, :n1] - h["comp"]).max()) <= 2e-5


def test_synthetic_batch_b64_n256_k32_equals_the_host_functions_per_stream():
    """Membership, ids and counts exact.  gt_warp of a point that moves with its box: within 4 * 2^-24 * sum_j |T_rj p_j| of the
    float64 application of the same fp32 matrix (three products and three sums, each rounded once to fp32; the fourth product is by
    1).  pc1_comp: the float32 of a float64 sum of four terms -- within 2^-24 |v| (the cast) + 2^-50 sum |terms| (two float64
    evaluation orders) of the host's float64 value.  Every other point: gt_warp is pc1_comp, bit for bit."""
    B, N, K = 64, 256, 32
    d = U.synthetic_batch(B, N, K)
    assert U.face_margin(d["per_stream"], d["pc1"], d["pc2"], d["n_valid"]) >= 1e-9      # no membership decision depends on rounding
    bb = G.pack_boxes(d["per_stream"], K, DEV)
    gt = G.ground_truth(_dev(d["pc1"]), _dev(d["pc2"]), bb, n_valid=_dev(d["n_valid"]))
    gt.check()
    moved_points = fallback_points = overlap_points = 0
    worst_w = worst_c = 0.0
    for b in range(B):
        n1, n2 = (int(v) for v in d["n_valid"][:, b])
        item = d["per_stream"][b]
        h = U.host_ground_truth(item, d["pc1"][b], d["pc2"][b], n1, n2, d["ego"][b] if item is not None else None)
        cls, obj, idx, warp, comp = _check_stream_against_host(gt, bb, b, h, n1, N)
        p = d["pc1"][b].astype(np.float64)
        # pc1_comp of every column (padding included) against the float64 host formula
        hom = np.vstack([p, np.ones((1, N))])
        E = np.linalg.inv(d["ego"][b].T).T[:3] if item is not None else np.eye(4)[:3]
        v64 = E @ hom
        bound_c = U24 * np.abs(v64) + 2.0 ** -50 * (np.abs(E) @ np.abs(hom))
        err_c = np.abs(comp.astype(np.float64) - v64)
        assert (err_c <= bound_c).all(), (b, float((err_c / bound_c).max()))
        worst_c = max(worst_c, float((err_c / bound_c).max()))
        assert (np.abs(h["comp64"] - v64[:, :n1]) <= 2.0 ** -50 * (np.abs(E) @ np.abs(hom))[:, :n1]).all(), b      # the host's own float64
        moves = np.zeros(N, dtype=bool)
        if item is not None and item[0]:
            moves[:n1] = cls[:n1] & np.isin(obj[:n1], list(h["moving_ids"]))
            pts = p.T
            inside = np.stack([np.isin(np.arange(N), vod_gt.points_in_box(bx, pts)) for bx in h["boxes1"].values()])
            many = inside[:, :n1].sum(0) > 1
            overlap_points += int(many.sum())
            last = (inside.shape[0] - 1 - np.argmax(inside[::-1], axis=0))[:n1]
            assert np.array_equal(idx[:n1][many], last[many]), b                                   # the LAST box wins
        assert np.array_equal(warp[:, ~moves], comp[:, ~moves]), b
        fallback_points += int((cls & ~moves).sum())
        for q in np.nonzero(moves)[0]:
            T32 = bb.host["motion"][b, idx[q]].reshape(3, 4).astype(np.float64)
            terms = T32 * hom[:, q]
            bound = 4 * U24 * np.abs(terms).sum(1)
            err = np.abs(warp[:, q].astype(np.float64) - terms.sum(1))
            assert (err <= bound).all(), (b, q, err, bound)
            worst_w = max(worst_w, float((err / bound).max()))
            assert (np.abs(warp[:, q].astype(np.float64) - h["gt"][:, q].astype(np.float64)) <= 2 * bound).all(), (b, q)   # host fp32 matmul
            moved_points += 1
    print("moved %d, labelled but not moved %d, in several boxes %d; worst error / bound: gt_warp %.3f, pc1_comp %.3f"
          % (moved_points, fallback_points, overlap_points, worst_w, worst_c))
    assert moved_points >= 200 and fallback_points >= 50 and overlap_points >= 10


def test_points_on_a_face_are_inside():
    """An axis-aligned box (ry = -pi/2: R = Rz(0)) with faces at x in {-1, 3}, y in {1, 3}, z in {1, 2}: all exactly representable,
    and so is the float64 difference of every test point from the centre."""
    lab = U._label(5, 1.0, 2.0, 1.5, 4.0, 2.0, 1.0, -np.pi / 2)
    box = vod_gt.box_in_radar_frame(lab, U.IDENTITY_TF)
    assert np.array_equal(box.R, np.eye(3)) and box.extent.tolist() == [4.0, 2.0, 1.0]
    up = lambda v: float(np.nextafter(np.float32(v), np.float32(np.inf)))
    dn = lambda v: float(np.nextafter(np.float32(v), np.float32(-np.inf)))
    pts = np.array([[3, 2, 1.5], [-1, 2, 1.5], [1, 1, 1.5], [1, 3, 1.5], [1, 2, 1], [1, 2, 2], [3, 3, 2], [-1, 1, 1],      # on faces, corners
                    [up(3), 2, 1.5], [dn(-1), 2, 1.5], [1, dn(1), 1.5], [1, up(3), 1.5], [1, 2, dn(1)], [1, 2, up(2)],      # one ulp outside
                    [dn(3), 2, 1.5], [1, 2, 1.5]], dtype=np.float32)                                                         # inside
    expect = [True] * 8 + [False] * 6 + [True] * 2
    assert vod_gt.points_in_box(box, pts).tolist() == [i for i, e in enumerate(expect) if e]
    pc = _dev(pts.T[None])
    bb = G.pack_boxes([({5: lab}, U.IDENTITY_TF, {5: lab}, U.IDENTITY_TF)], 2, DEV)
    gt = G.ground_truth(pc, pc, bb)
    gt.check()
    assert gt.gt_cls[0].cpu().tolist() == expect
    assert gt.counts1[0].cpu().tolist() == [10, 0] and gt.counts2[0].cpu().tolist() == [10, 0]
    assert gt.obj_id[0].cpu().tolist() == [5 if e else -1 for e in expect]
    # the partner is the same box: T = identity, labelled points stay where they are; no ego matrix: pc1_comp is pc1
    assert torch.equal(gt.gt_warp, pc) and torch.equal(gt.pc1_comp, pc)


def test_non_contiguous_views_give_the_bits_of_contiguous_copies():
    d = U.synthetic_batch(8, 256, 32, seed=77)
    bb = G.pack_boxes(d["per_stream"], 32, DEV)
    nv = _dev(d["n_valid"])
    pc1, pc2 = _dev(d["pc1"]), _dev(d["pc2"])
    a = G.ground_truth(pc1, pc2, bb, n_valid=nv)
    wide1 = torch.zeros(8, 256, 5, device=DEV)
    wide1[:, :, 1:4] = pc1.permute(0, 2, 1)
    v1 = wide1[:, :, 1:4].permute(0, 2, 1)                       # (B,3,N) view of a point-major buffer with a pitch of 5
    v2 = pc2.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    assert not v1.is_contiguous() and not v2.is_contiguous()
    b = G.ground_truth(v1, v2, bb, n_valid=nv)
    for name in ("gt_cls", "box_index", "obj_id", "gt_warp", "pc1_comp", "counts1", "counts2", "flags"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    g = torch.Generator().manual_seed(3)
    warp = a.gt_warp + 0.05 * torch.randn(8, 3, 256, generator=g).to(DEV)
    cls = torch.rand(8, 256, generator=g).to(DEV)
    mask = 1.0 - a.gt_cls.float()
    m0 = G.frame_metrics(pc1, warp, a.gt_warp, mask, cls, a.gt_cls, n_valid=nv)
    vw = warp.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    vg = a.gt_warp.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    vc = torch.stack([cls, cls], dim=2)[:, :, 1].unsqueeze(1)    # (B,1,N), point stride 2
    assert not vc.is_contiguous()
    m1 = G.frame_metrics(v1, vw, vg, mask, vc, a.gt_cls, n_valid=nv[0])
    assert torch.equal(m0.sums, m1.sums) and torch.equal(m0.values.view(torch.int64), m1.values.view(torch.int64))


def test_flags_and_check_name_the_stream():
    d = U.synthetic_batch(4, 256, 8, seed=5)
    bb = G.pack_boxes(d["per_stream"], 8, DEV)
    pc1, pc2 = _dev(d["pc1"]), _dev(d["pc2"])
    good = G.ground_truth(pc1, pc2, bb, n_valid=_dev(d["n_valid"]))
    good.check()
    assert good.flags.cpu().tolist() == [0, 0, 0, 0]
    nv = _dev(d["n_valid"]).clone()
    nv[1, 2] = 257
    bad = G.ground_truth(pc1, pc2, bb, n_valid=nv)
    assert bad.flags.cpu().tolist() == [0, 0, 2, 0]
    with pytest.raises(RuntimeError, match="stream 2 has an n_valid"):
        bad.check()
    for name in ("gt_cls", "obj_id", "gt_warp", "counts1"):                     # the other streams are what they were
        assert torch.equal(getattr(bad, name)[:2], getattr(good, name)[:2]) and torch.equal(getattr(bad, name)[3], getattr(good, name)[3])
    saved = bb.count.clone()
    bb.count[0, 1] = 11                                                          # more boxes than slots: clamped and flagged
    over = G.ground_truth(pc1, pc2, bb, n_valid=_dev(d["n_valid"]))
    assert over.flags.cpu().tolist() == [0, 1, 0, 0]
    with pytest.raises(RuntimeError, match="stream 1 has a box count"):
        over.check()
    bb.count.copy_(saved)
    with pytest.raises(ValueError):
        G.ground_truth(pc1, pc2, bb, n_valid=torch.tensor([1, 2, 3, 4]))


# ---- metrics ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EVAL_CASES)
def test_metrics_match_the_reference_values(name):
    case = load_case(name)
    pc1, flow, gt = _dev(case["in_pc1"]), _dev(case["flow"]), _dev(case["in_gt_warp"])
    gt_cls = _dev(case["in_gt_cls"])
    mask = (~gt_cls).float()
    fm = G.frame_metrics(pc1, pc1 + flow, gt, mask, _dev(case["cls"]), gt_cls)
    got = fm.stream(0)
    assert fm.keys == G.KEYS and list(got) == list(G.KEYS)
    for keys, vals in ((case["metric_sf_keys"], case["metric_sf_vals"]), (case["metric_seg_keys"], case["metric_seg_vals"])):
        for k, v in zip(keys, vals):
            print("%s %-10s device %.12g reference %.12g" % (name, k, got[str(k)], v))
            assert abs(got[str(k)] - v) <= 1e-6 * max(1.0, abs(v)), (name, k, got[str(k)], v)


def _host_metrics(pc1, warp, gt, mask, cls, gt_cls, b, n, threshold=0.5):
    """metrics.eval_scene_flow / eval_motion_seg on stream b's valid slice alone, inputs cast to float64, its own mask row."""
    s = lambda t: t[b:b + 1, :, :n].double()
    with np.errstate(invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")                            # the mean of an empty slice (no static point) warns and is NaN
        sf = M.eval_scene_flow(s(pc1), s(warp), s(gt), mask[b:b + 1, :n].double())
    pre = (cls[b:b + 1, :n] > threshold).double()
    g = gt_cls[b:b + 1, :n].double()
    seg = M.eval_motion_seg(pre, g)
    counts = [int(((pre == 1) & (g == 1)).sum()), int(((pre == 0) & (g == 0)).sum()), int(((pre == 1) & (g == 0)).sum()),
              int(((pre == 0) & (g == 1)).sum())]
    return {**sf, **seg}, counts


def _random_frame(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    pc1 = torch.cat([40 * torch.rand(B, 2, N, generator=g) - 20, 4 * torch.rand(B, 1, N, generator=g) - 2], dim=1)
    gt = pc1 + 0.3 * torch.randn(B, 3, N, generator=g)
    scale = torch.rand(B, 1, N, generator=g) ** 3                 # errors from tiny to large: both sides of the sas / ras thresholds
    warp = gt + 0.4 * scale * torch.randn(B, 3, N, generator=g)
    gt_cls = torch.rand(B, N, generator=g) < 0.3
    cls = torch.rand(B, N, generator=g)
    mask = 1.0 - gt_cls.float()
    mask[torch.rand(B, N, generator=g) < 0.05] = 0.5              # neither static nor moving
    return pc1, warp, gt, mask, cls, gt_cls


def _assert_values(got, ref, what):
    for k in G.KEYS:
        a, r = got[k], float(ref[k])
        if np.isnan(r):
            assert np.isnan(a), (what, k, a)
        else:
            assert abs(a - r) <= 1e-10 * max(1.0, abs(r)), (what, k, a, r)


def test_padded_batch_equals_the_float64_host_call_per_stream():
    B, N = 6, 2048
    pc1, warp, gt, mask, cls, gt_cls = _random_frame(B, N, 11)
    n_valid = [2048, 1500, 777, 2048, 64, 1]
    mask[2] = 0.0                                                  # a stream with no static point: stat_rne is NaN on both sides
    mask[3, :100] = 1.0
    active = [1, 1, 1, 1, 0, 1]
    for t in (pc1, warp, gt, mask, cls):                           # padding columns must not matter: make them conspicuous
        for b, n in enumerate(n_valid):
            t[b, ..., n:] = 1e3
    fm = G.frame_metrics(pc1.to(DEV), warp.to(DEV), gt.to(DEV), mask.to(DEV), cls.to(DEV), gt_cls.to(DEV),
                         n_valid=torch.tensor(n_valid, dtype=torch.int32), active=active)
    vals, sums = fm.values.cpu().numpy(), fm.sums.cpu().numpy()
    worst = 0.0
    for b, n in enumerate(n_valid):
        if not active[b]:
            assert (vals[b] == 0).all() and (sums[b] == 0).all()
            continue
        ref, counts = _host_metrics(pc1, warp, gt, mask, cls, gt_cls, b, n)
        _assert_values(fm.stream(b), ref, "stream %d" % b)
        worst = max([worst] + [abs(fm.stream(b)[k] - ref[k]) / max(1.0, abs(ref[k])) for k in G.KEYS if not np.isnan(ref[k])])
        assert sums[b, 9:13].tolist() == [float(c) for c in counts], b
        assert sums[b, 0] == n and sums[b, 4] == float((mask[b, :n] == 0).sum()) and sums[b, 6] == float((mask[b, :n] == 1).sum())
    print("worst |device - host float64| / max(1, |v|) = %.3e" % worst)
    assert np.isnan(vals[2, 3]) and np.isnan(vals[2, 1]) and not np.isnan(vals[3, 3])
    # run to run: the same bits
    again = G.frame_metrics(pc1.to(DEV), warp.to(DEV), gt.to(DEV), mask.to(DEV), cls.to(DEV), gt_cls.to(DEV),
                            n_valid=torch.tensor(n_valid, dtype=torch.int32), active=active)
    assert torch.equal(again.sums, fm.sums)


def test_accumulator_equals_the_host_loop_over_frames_with_a_changing_active_mask():
    B, N, frames = 4, 300, 4
    acc = G.MetricAccumulator(B, device=DEV)
    host_sum = np.zeros((B, len(G.KEYS)))
    host_counts = np.zeros((B, 4))
    host_points = np.zeros(B)
    host_frames = np.zeros(B, dtype=np.int64)
    schedule = [[1, 1, 1, 1], [1, 0, 1, 1], [0, 0, 1, 1], [1, 0, 1, 0]]
    n_valid = [300, 211, 300, 150]
    for f in range(frames):
        pc1, warp, gt, mask, cls, gt_cls = _random_frame(B, N, 100 + f)
        mask[3] = 1.0 - gt_cls[3].float()
        active = schedule[f]
        fm = G.frame_metrics(pc1.to(DEV), warp.to(DEV), gt.to(DEV), mask.to(DEV), cls.to(DEV), gt_cls.to(DEV),
                             n_valid=torch.tensor(n_valid, dtype=torch.int32), active=active if f % 2 else None)
        acc.update(fm, active=None if f % 2 else active)          # the mask comes with the frame, or with the update
        for b in range(B):
            if not active[b]:
                continue
            ref, counts = _host_metrics(pc1, warp, gt, mask, cls, gt_cls, b, n_valid[b])
            host_sum[b] += [ref[k] for k in G.KEYS]
            host_counts[b] += counts
            host_points[b] += n_valid[b]
            host_frames[b] += 1
    r = acc.result()
    assert r["frames"].tolist() == host_frames.tolist() == [3, 1, 4, 3]
    for i, k in enumerate(G.KEYS):
        for b in range(B):
            ref = host_sum[b, i] / host_frames[b]
            assert abs(r["per_stream"][k][b] - ref) <= 1e-10 * max(1.0, abs(ref)), (k, b)
        ref = host_sum[:, i].sum() / host_frames.sum()
        assert abs(r["overall"][k] - ref) <= 1e-10 * max(1.0, abs(ref)), k
    assert np.array_equal(r["sums"][:, 9:13], host_counts) and np.array_equal(r["sums"][:, 0], host_points)
    tp, tn, fp, fn = host_counts.sum(0) + 1e-20
    assert abs(r["pooled"]["acc"] - (tp + tn) / (tp + tn + fp + fn)) <= 1e-12 and abs(r["pooled"]["sen"] - tp / (tp + fn)) <= 1e-12


# ---- no host round trip --------------------------------------------------------------------------------------------------------
def _ref_net(train=False):
    sd = reference_state_dict(DEV)
    if not train:
        sd["fd_layer.cp.linear.bias"] = sd["fd_layer.cp.linear.bias"] + 0.09      # moving points in every frame (tests/test_tracker_gpu.py)
    net = Track4D(Args()).to(DEV)
    net.load_state_dict(sd, strict=True)
    return net.train() if train else net.eval()


def test_track_label_score_accumulate_without_host_synchronisation():
    """As tests/test_tracker_gpu.py does for the association stage: the backbone runs first, then everything after it -- the tracker's
    four launches, ground_truth, frame_metrics, MetricAccumulator.update -- under torch's sync debug mode "error"."""
    net = _ref_net()
    B = 4
    trk = T.BatchedTracker(net, streams=B)
    t = {k: torch.from_numpy(v) for k, v in synth.make_frame_pairs(B, 256, case_id=50).items()}
    pairs = [(t["pc1"][i:i + 1], t["pc2"][i:i + 1], t["feature1"][i:i + 1], t["feature2"][i:i + 1]) for i in range(B)]
    d = U.synthetic_batch(B, 256, 8, seed=9)
    # boxes around the clouds' own points, so that some are labelled
    per_stream = []
    for b in range(B):
        p = t["pc1"][b].numpy()
        labels = {k: U._label(k, p[0, 10 * k], p[1, 10 * k], p[2, 10 * k], 6.0, 4.0, 3.0, 0.3 * k) for k in range(6)}
        per_stream.append((labels, U.IDENTITY_TF, labels, U.IDENTITY_TF, d["ego"][b]))
    bb = G.pack_boxes(per_stream, 8, DEV)
    acc = G.MetricAccumulator(B, device=DEV)
    for step in range(2):
        pc1, pc2, f1, f2, nv = vod_gt.pad_frame_pairs(pairs, device=DEV)
        reset = torch.zeros(B, dtype=torch.uint8, device=DEV)
        active = torch.ones(B, dtype=torch.uint8, device=DEV)
        with torch.no_grad():
            flow, h, cls, _, _, _, prop = net._fused_engine().backbone(pc1, pc2, f1, f2, trk.h, n_valid=nv)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = trk.associate(pc1, f1, flow, cls, prop, nv, reset, active)
            gt = G.ground_truth(pc1, pc2, bb, n_valid=nv)
            fm = G.frame_metrics(pc1, pc1 + out.flow, gt.gt_warp, 1.0 - gt.gt_cls.float(), out.cls, gt.gt_cls, n_valid=nv, active=active)
            acc.update(fm)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        trk.h = h
        out.check()
        gt.check()
    r = acc.result()
    assert r["frames"].tolist() == [2] * B and int(gt.gt_cls.sum()) > 0
    assert all(np.isfinite(r["overall"][k]) for k in G.KEYS)


def test_train_step_on_device_ground_truth_equals_the_step_on_host_ground_truth():
    from ratrack_amd.train import Trainer
    per_stream, pairs, egos = U.real_streams()
    pc1, pc2, f1, f2, nv = vod_gt.pad_frame_pairs(pairs, device=DEV)
    N = pc1.shape[2]
    gt = G.ground_truth(pc1, pc2, G.pack_boxes(per_stream, 16, DEV), n_valid=nv)
    gt.check()
    assert gt.gt_cls.dtype == torch.bool
    host_warp, host_cls = torch.zeros(3, 3, N), torch.zeros(3, N, dtype=torch.bool)
    p1, p2 = pc1.cpu().numpy(), pc2.cpu().numpy()
    for b in range(3):
        n1, n2 = int(nv[0, b]), int(nv[1, b])
        h = U.host_ground_truth(per_stream[b], p1[b], p2[b], n1, n2, egos[b])
        host_warp[b, :, :n1] = torch.from_numpy(h["gt"])
        host_warp[b, :, n1:] = torch.from_numpy(h["comp"][:, :1])              # padding: the compensated copy of point 0
        host_cls[b, :n1] = torch.from_numpy(h["cls"])
    tr = Trainer(_ref_net(train=True), lr=0.0, graph=False, deterministic=True)   # lr 0: both steps start from the same weights
    items_h, _ = tr.step(pc1, pc2, f1, f2, host_warp.to(DEV), host_cls.to(DEV), n_valid=nv)
    items_h = {k: float(v) for k, v in items_h.items()}
    items_d, _ = tr.step(pc1, pc2, f1, f2, gt.gt_warp, gt.gt_cls, n_valid=nv)
    items_d = {k: float(v) for k, v in items_d.items()}
    print("loss items, host GT:  ", items_h)
    print("loss items, device GT:", items_d)
    assert set(items_h) == set(items_d) and items_h["Loss"] > 0
    for k in items_h:
        assert abs(items_h[k] - items_d[k]) <= 1e-6, (k, items_h[k], items_d[k])
