"""GPU: ground-truth objects, their matching to detections and the running tracking score on the device
(ratrack_amd/track_score.py, csrc/track_score.hip) against the host path they stand in for, run per stream on the valid slice:
vod_gt.filter_object_points, vod_gt.map_gt_objects, the target list of loss.affinity_loss and the counter loop of
tests/_track_score_util.py.  Integers must be equal, `iou` bit-equal (the same float64 division), iou_sum / mean_iou within 1e-12."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _gt_util as U
import _track_score_util as S
from _util import reference_state_dict
from ratrack_amd import gt_device as G
from ratrack_amd import loss as L
from ratrack_amd import synth, tracker as T, track_score as TS, vod_gt
from ratrack_amd.track4d import Args, Track4D

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(obj, names):
    return {k: getattr(obj, k).cpu().numpy() for k in names}


GOBJ = ("slot", "label_id", "count", "size", "members", "centre", "flags")
MATCH = ("pred_gt_slot", "pred_gt_id", "gt_pred", "iou", "aff_target", "aff_defined")


def _columns(words, N):
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:N]
    return np.nonzero(bits)[0]


def _rows(a):
    return sorted(map(tuple, np.asarray(a).view(np.uint32).tolist()))


def check_gt_objects(g, b, r, item, pc_b, N):
    """Stream b of the downloaded GtObjects `g` against elements 7..9 of the host tuple `r`."""
    labels = list(r[7].keys())
    cnt = int(g["count"][b])
    assert cnt == len(labels), (b, cnt, labels)
    assert g["label_id"][b, :cnt].tolist() == labels and (g["label_id"][b, cnt:] == -1).all(), b
    slot_of = {k: i for i, k in enumerate(item[0].keys())} if item is not None else {}
    assert g["slot"][b, :cnt].tolist() == [slot_of[k] for k in labels] and (g["slot"][b, cnt:] == -1).all(), b
    assert (g["size"][b, cnt:] == 0).all() and (g["members"][b, cnt:] == 0).all() and (g["centre"][b, cnt:] == 0).all(), b
    for j, k in enumerate(labels):
        cols = _columns(g["members"][b, j], N)
        host_pts = r[7][k][0].numpy().T
        assert int(g["size"][b, j]) == len(cols) == len(host_pts), (b, k)
        assert _rows(pc_b[:, cols].T) == _rows(host_pts), (b, k)                 # the same point set, bit for bit
        idx = r[8][k].numpy()
        if len(idx) == len(host_pts) and np.array_equal(pc_b[:, idx].T.view(np.uint32), host_pts.view(np.uint32)):
            assert cols.tolist() == idx.tolist(), (b, k)                         # nothing merged in: the box's own columns
        # fp32 mean of n points on the host against the float64 one: (n + 1) roundings of at most the largest coordinate
        c = r[9][k][0].double().numpy()
        tol = (len(idx) + 1) * 2.0 ** -24 * float(np.abs(pc_b[:, idx]).max())
        assert np.abs(g["centre"][b, j] - c).max() <= tol, (b, k, g["centre"][b, j], c)


def check_match(m, g, b, h, Kobj):
    """Stream b of the downloaded MatchResult `m` against the host row `h` (tests/_track_score_util.host_sequence)."""
    P, labels = len(h["gt_id"]), h["labels"]
    cnt = len(labels)
    assert m["pred_gt_id"][b, :P].tolist() == h["gt_id"] and (m["pred_gt_id"][b, P:] == -1).all(), (b, m["pred_gt_id"][b], h["gt_id"])
    slot_of = dict(zip(labels, g["slot"][b, :cnt].tolist()))
    assert m["pred_gt_slot"][b, :P].tolist() == [slot_of.get(k, -1) for k in h["gt_id"]] and (m["pred_gt_slot"][b, P:] == -1).all(), b
    pred_of = {k: i for i, k in enumerate(h["gt_id"]) if k >= 0}
    assert m["gt_pred"][b, :cnt].tolist() == [pred_of.get(k, -1) for k in labels] and (m["gt_pred"][b, cnt:] == -1).all(), b
    assert np.array_equal(m["iou"][b, :P].view(np.int64), np.array(h["iou"], dtype=np.float64).view(np.int64)), (b, m["iou"][b, :P], h["iou"])
    assert (m["iou"][b, P:] == 0).all(), b
    full = np.zeros((Kobj, Kobj), dtype=np.float32)
    if h["target"] is not None:
        full[:h["target"].shape[0], :h["target"].shape[1]] = h["target"]
    assert int(m["aff_defined"][b]) == int(h["target"] is not None), b
    assert np.array_equal(m["aff_target"][b], full), b


def check_result(res, scorers):
    for b, s in enumerate(scorers):
        fin = s.final()
        for k in S.COUNTERS:
            assert int(res["per_stream"][k][b]) == fin[k], (b, k, int(res["per_stream"][k][b]), fin[k])
        assert abs(res["per_stream"]["iou_sum"][b] - s.iou_sum) <= 1e-12 * max(abs(s.iou_sum), 1e-300), b
        if fin["tp"]:
            ref = s.iou_sum / fin["tp"]
            assert abs(res["per_stream"]["mean_iou"][b] - ref) <= 1e-12 * ref, b
    tot = {k: sum(s.final()[k] for s in scorers) for k in S.COUNTERS}
    for k in S.COUNTERS:
        assert res["overall"][k] == tot[k], k
    assert abs(res["overall"]["mota"] - (1 - (tot["fn"] + tot["fp"] + tot["idsw"]) / tot["gt"])) <= 1e-15
    assert abs(res["overall"]["recall"] - tot["tp"] / tot["gt"]) <= 1e-15 and abs(res["overall"]["mt_fraction"] - tot["mt"] / tot["tracks"]) <= 1e-15
    ref = sum(s.iou_sum for s in scorers)
    assert abs(res["overall"]["iou_sum"] - ref) <= 1e-12 * ref


# ---- 1: the shipped frames -------------------------------------------------------------------------------------------------------
def test_shipped_frames_give_the_host_paths_combined_objects():
    per_stream, pairs, egos = U.real_streams()
    pc1, pc2, f1, f2, nv = vod_gt.pad_frame_pairs(pairs, device=DEV)
    N = pc1.shape[2]
    bb = G.pack_boxes(per_stream, 16, DEV)
    gobj = TS.gt_objects(pc1, bb, TS.pack_box_types(per_stream, 16, DEV), n_valid=nv, min_obj_points=2)
    gobj.check()
    g, p1 = _host(gobj, GOBJ), pc1.cpu().numpy()
    riders = merged = 0
    for b in range(3):
        n1 = int(nv[0, b])
        r = S.host_gt_objects(per_stream[b], p1[b], n1)
        check_gt_objects(g, b, r, per_stream[b], p1[b], N)
        riders += sum(1 for k in r[4] if per_stream[b][0][k].type == "rider")
        merged += len(r[2]) - len(r[7])
    print("shipped frames: %d rider objects, %d objects merged away or below the minimum size" % (riders, merged))
    assert int(g["count"].sum()) > 0


# ---- 2 + 3: the seeded sequence ----------------------------------------------------------------------------------------------------
def _run_sequence(seq, scorer, strided=False):
    """-> per frame (GtObjects host copy, MatchResult host copy); one upload per frame, the downloads after the last launch."""
    B, N, K = seq["B"], seq["N"], seq["K"]
    kept = []
    for fr in seq["frames"]:
        pc1 = _dev(fr["pc1"])
        if strided:
            pc1 = pc1.permute(0, 2, 1).contiguous().permute(0, 2, 1)
        bb = G.pack_boxes(fr["per_stream"], K, DEV)
        nv = _dev(fr["n_valid"])
        gobj = TS.gt_objects(pc1, bb, TS.pack_box_types(fr["per_stream"], K, DEV), n_valid=nv, min_obj_points=S.MIN_PTS)
        m = scorer.update_raw(pc1, _dev(fr["obj"]), _dev(fr["num"]), _dev(fr["ids"]), gobj, nv, _dev(fr["reset"]), _dev(fr["active"]))
        kept.append((gobj, m))
    return [(_host(g, GOBJ), _host(m, MATCH)) for g, m in kept]


def test_seeded_sequence_matches_and_scores_as_the_host_path():
    seq = S.synthetic_sequence()
    B, N, K = seq["B"], seq["N"], seq["K"]
    assert B == 64 and N == 256 and K == 32 and len(seq["frames"]) >= 12
    # the input conditions under which the host's fp32 decisions and the kernel's float64 ones coincide, before any comparison
    cond = S.input_conditions(seq)
    print("input conditions:", cond)
    assert cond["rider_gap"] >= 1e-3 and cond["point_gap"] >= 1e-3 and cond["face_margin"] >= 1e-6 and cond["negative_zero"] == 0, cond
    ref, scorers, census = S.host_sequence()
    print("census:", census)
    assert all(v > 0 for v in census.values()), census
    scorer = TS.TrackScorer(streams=B, max_objects=K, max_boxes=K, max_gt_tracks=64)
    dev = _run_sequence(seq, scorer)
    for f, (fr, (g, m)) in enumerate(zip(seq["frames"], dev)):
        assert (g["flags"] == 0).all()
        for b in range(B):
            n = int(fr["n_valid"][b])
            if b in ref[f]:
                check_gt_objects(g, b, ref[f][b]["r"], fr["per_stream"][b], fr["pc1"][b], N)
                check_match(m, g, b, ref[f][b], K)
            else:                                                               # inactive: reports nothing
                assert (m["pred_gt_id"][b] == -1).all() and (m["pred_gt_slot"][b] == -1).all() and (m["gt_pred"][b] == -1).all()
                assert (m["iou"][b] == 0).all() and (m["aff_target"][b] == 0).all() and m["aff_defined"][b] == 0
    res = scorer.result()
    check_result(res, scorers)
    print("overall:", res["overall"])
    # the same bits on a second run
    again = _run_sequence(seq, TS.TrackScorer(streams=B, max_objects=K, max_boxes=K, max_gt_tracks=64))
    for (g0, m0), (g1, m1) in zip(dev, again):
        assert all(np.array_equal(g0[k], g1[k]) for k in GOBJ) and all(np.array_equal(m0[k], m1[k]) for k in MATCH)


# ---- 4: strided views ----------------------------------------------------------------------------------------------------------------
def test_strided_views_give_the_bits_of_contiguous_copies():
    seq = S.synthetic_sequence(8, 128, 8, 3)
    mk = lambda: TS.TrackScorer(streams=8, max_objects=8, max_boxes=8, max_gt_tracks=16)
    s0, s1 = mk(), mk()
    a, b = _run_sequence(seq, s0), _run_sequence(seq, s1, strided=True)
    for (g0, m0), (g1, m1) in zip(a, b):
        assert all(np.array_equal(g0[k], g1[k]) for k in GOBJ) and all(np.array_equal(m0[k], m1[k]) for k in MATCH)
    assert torch.equal(s0.counters, s1.counters) and torch.equal(s0.iou_sum, s1.iou_sum) and int(s0.counters[:, 3].sum()) > 0


# ---- 5: flags --------------------------------------------------------------------------------------------------------------------
def _small_run(T=16, bad_nv=None, bad_count=None):
    seq = S.synthetic_sequence(8, 128, 8, 3)
    scorer = TS.TrackScorer(streams=8, max_objects=8, max_boxes=8, max_gt_tracks=T)
    last = None
    for fr in seq["frames"]:
        pc1, nv = _dev(fr["pc1"]), _dev(fr["n_valid"])
        bb = G.pack_boxes(fr["per_stream"], 8, DEV)
        if bad_nv is not None:
            nv[bad_nv] = 128 + 7
        if bad_count is not None:
            bb.count[0, bad_count] = 9
        gobj = TS.gt_objects(pc1, bb, TS.pack_box_types(fr["per_stream"], 8, DEV), n_valid=nv, min_obj_points=S.MIN_PTS)
        m = scorer.update_raw(pc1, _dev(fr["obj"]), _dev(fr["num"]), _dev(fr["ids"]), gobj, nv, _dev(fr["reset"]), _dev(fr["active"]))
        last = (gobj, m)
    return scorer, last


def test_flags_name_the_stream_and_leave_the_others_intact():
    clean, (gobj0, m0) = _small_run()
    clean.check()
    gobj0.check()
    base = clean.result()["per_stream"]
    others = lambda bad: [b for b in range(8) if b != bad]
    # stream 0 keeps four label ids in a clip: a table of three overflows there and nowhere else
    small, _ = _small_run(T=3)
    with pytest.raises(RuntimeError, match="stream 0 saw more than max_gt_tracks=3"):
        small.check()
    with pytest.raises(RuntimeError, match="stream 0 saw more than max_gt_tracks=3"):
        small.result()
    res = small.result(check=False)
    assert res["flags"].tolist() == [TS.FLAG_TRACKS] + [0] * 7
    for k in S.COUNTERS:
        assert res["per_stream"][k][1:].tolist() == base[k][1:].tolist(), k
    for k in ("frames", "gt", "pred", "tp", "fp", "fn"):       # the frame counts of the flagged stream do not go through the table
        assert res["per_stream"][k][0] == base[k][0], k
    assert res["per_stream"]["tracks"][0] == 3
    # an n_valid beyond N (clamped: the padding columns are read, nothing past the row)
    bad, (gobj, m) = _small_run(bad_nv=2)
    with pytest.raises(RuntimeError, match="stream 2 has an n_valid"):
        gobj.check()
    with pytest.raises(RuntimeError, match="stream 2 has an n_valid"):
        bad.result()
    res = bad.result(check=False)
    for k in S.COUNTERS:
        assert res["per_stream"][k][others(2)].tolist() == base[k][others(2)].tolist(), k
    for k in GOBJ[:-1]:
        assert torch.equal(getattr(gobj, k)[others(2)], getattr(gobj0, k)[others(2)]), k
    # a box count beyond the slots (clamped)
    bad, (gobj, m) = _small_run(bad_count=1)
    with pytest.raises(RuntimeError, match="stream 1 has a box count"):
        gobj.check()
    assert gobj.flags.tolist() == [0, TS.FLAG_BOXES] + [0] * 6
    for k in GOBJ[:-1]:
        assert torch.equal(getattr(gobj, k)[others(1)], getattr(gobj0, k)[others(1)]), k
    for k in MATCH:
        assert torch.equal(getattr(m, k)[others(1)], getattr(m0, k)[others(1)]), k


# ---- 6 + 7: behind the tracker, without a host round trip ----------------------------------------------------------------------------
def _ref_net():
    sd = reference_state_dict(DEV)
    sd["fd_layer.cp.linear.bias"] = sd["fd_layer.cp.linear.bias"] + 0.09      # moving points in every frame (tests/test_tracker_gpu.py)
    net = Track4D(Args()).to(DEV)
    net.load_state_dict(sd, strict=True)
    return net.eval()


@pytest.fixture(scope="module")
def tracked():
    """BatchedTracker.associate -> ground_truth -> gt_objects -> scorer.update over three frames, everything after the backbone under
    torch's sync debug mode "error" (as test_track_label_score_accumulate_without_host_synchronisation does); then the host path of
    every stream and frame, fed with out.objects(b)."""
    net = _ref_net()
    B, K = 4, 8
    trk = T.BatchedTracker(net, streams=B)
    t = {k: torch.from_numpy(v) for k, v in synth.make_frame_pairs(B, 256, case_id=50).items()}
    pairs = [(t["pc1"][i:i + 1], t["pc2"][i:i + 1], t["feature1"][i:i + 1], t["feature2"][i:i + 1]) for i in range(B)]
    per_stream = []
    for b in range(B):
        p = t["pc1"][b].numpy()
        mk = lambda k: vod_gt.Label("rider" if k == 2 else "Car", k, 0, 0, 0, 0, 0, 0, 3.0, 4.0, 6.0, float(p[0, 10 * k]), float(p[1, 10 * k]),
                                    float(p[2, 10 * k]), 0.3 * k)
        labels = {k: mk(k) for k in range(6)}
        per_stream.append((labels, U.IDENTITY_TF, labels, U.IDENTITY_TF))
    bb = G.pack_boxes(per_stream, K, DEV)
    types = TS.pack_box_types(per_stream, K, DEV)
    scorer = TS.TrackScorer(streams=B, max_objects=trk.K, max_boxes=K, max_gt_tracks=32)
    steps = []
    for step in range(3):
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
            gobj = TS.gt_objects(pc1, bb, types, n_valid=nv, min_obj_points=net.min_obj_points)
            m = scorer.update(out, gobj, reset=reset, active=active)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        trk.h = h
        steps.append((pc1, nv, out, gt, gobj, m))
    for _, _, out, gt, gobj, _ in steps:
        out.check()
        gt.check()
        gobj.check()
    host, scorers = [], [S.HostScorer() for _ in range(B)]
    for pc1, nv, out, gt, gobj, m in steps:
        p1, row = pc1.cpu().numpy(), {}
        for b in range(B):
            r = S.host_gt_objects(per_stream[b], p1[b], int(nv[0, b]), min_pts=net.min_obj_points)
            objects, _ = out.objects(b)
            objects = {k: v.cpu() for k, v in objects.items()}
            mapping, gt_id, iou = S.host_match(r, objects)
            target, _ = scorers[b].frame(list(r[7].keys()), list(objects.keys()), gt_id, iou, mapping, False)
            row[b] = dict(r=r, labels=list(r[7].keys()), mapping=mapping, gt_id=gt_id, iou=iou, target=target)
        host.append(row)
    return dict(B=B, per_stream=per_stream, steps=steps, host=host, scorers=scorers, scorer=scorer, Kobj=trk.K)


def test_track_match_score_without_host_synchronisation_equals_the_host_path(tracked):
    d = tracked
    objects = matches = 0
    for (pc1, nv, out, gt, gobj, m), row in zip(d["steps"], d["host"]):
        g, mm, p1 = _host(gobj, GOBJ), _host(m, MATCH), pc1.cpu().numpy()
        for b in range(d["B"]):
            check_gt_objects(g, b, row[b]["r"], d["per_stream"][b], p1[b], pc1.shape[2])
            check_match(mm, g, b, row[b], d["Kobj"])
            objects += len(row[b]["gt_id"])
            matches += sum(1 for k in row[b]["gt_id"] if k >= 0)
    res = d["scorer"].result()
    check_result(res, d["scorers"])
    print("the run contained %d detected objects, %d of them matched; overall %s" % (objects, matches, res["overall"]))
    assert objects > 0 and res["overall"]["pred"] == objects and res["overall"]["frames"] == 3 * d["B"]


def test_affinity_target_gives_the_host_tracking_loss(tracked):
    d = tracked
    defined = 0
    for f in range(1, len(d["steps"])):
        out, m = d["steps"][f][2], d["steps"][f][5]
        prev_map = d["host"][f - 1]
        for b in range(d["B"]):
            mp, mc = prev_map[b]["mapping"], d["host"][f][b]["mapping"]
            on = int(m.aff_defined[b])
            assert on == int(len(mp) > 0 and len(mc) > 0), (f, b)
            if not on:
                continue
            defined += 1
            rows, cols = int(out.num_prev[b]), int(out.num_objects[b])
            assert rows == len(mp) and cols == len(mc)
            ours = F.binary_cross_entropy(out.aff[b, :rows, :cols].reshape(-1), m.aff_target[b, :rows, :cols].reshape(-1))
            theirs = L.affinity_loss(mp, mc, out.aff_mat(b).reshape(-1))
            assert torch.equal(ours, theirs), (f, b, float(ours), float(theirs))
    print("tracking loss compared on %d stream-frames" % defined)
    assert defined > 0


# ---- 8: the ten variants of the one scoring launch -------------------------------------------------------------------------------------
STATE = ("counters", "iou_sum", "table_key", "table_last", "table_seen", "table_matched", "table_used", "prev_gt_id", "prev_count", "prev_gt",
         "flags")
LOG = ("log_cursor", "log_frame", "log_label", "log_track", "log_best", "log_conf", "log_iou")


def _tail_frames():
    """Three frames of B = 2 streams at sizes that are no multiple of anything: N = 33 columns with n_valid = (33, 20), Kobj = 7
    detection slots, K = 5 box slots.  Four 2 m cars per stream, their points (multiples of 1/64) shuffled among clutter; detections:
    one exact, one with a point exchanged for clutter, one split in two, one that appears from the second frame on, one of clutter
    alone; a track id that changes; a reset of stream 0 on the second frame; stream 1 inactive in the third."""
    B, N, Kobj, K, q = 2, 33, 7, 5, 1.0 / 64
    rng = np.random.default_rng(20250921)
    sizes, n_valid = ((5, 4, 4, 3), (4, 4, 3, 2)), (33, 20)
    local = [[rng.integers(-40, 41, (k, 3)).astype(np.float64) * q for k in sizes[b]] for b in range(B)]
    clutter = [(rng.integers(-64, 65, (N, 3)) + np.array([-3000, 0, 0])).astype(np.float64) * q for b in range(B)]
    frames = []
    for f in range(3):
        pc1 = np.zeros((B, 3, N), dtype=np.float32)
        obj, num, ids = np.full((B, N), -1, dtype=np.int32), np.zeros(B, dtype=np.int32), np.full((B, Kobj), -1, dtype=np.int32)
        det_box, det_valid, per_stream = np.zeros((B, Kobj, 8)), np.zeros((B, Kobj), dtype=np.int32), []
        for b in range(B):
            centres = [np.array([6.0 * j + 0.25 * f, 2.0 * b, 0.0]) for j in range(4)]
            labels = {20 + j: vod_gt.Label("Car", 20 + j, 0, 0, 0, 0, 0, 0, 2.0, 2.0, 2.0, *(float(v) for v in c), -(0.2 * j + np.pi / 2))
                      for j, c in enumerate(centres)}
            per_stream.append((labels, U.IDENTITY_TF, labels, U.IDENTITY_TF))
            pts = np.concatenate([c + l for c, l in zip(centres, local[b])] + [clutter[b]])[:n_valid[b]]
            perm = rng.permutation(len(pts))
            where = np.empty(len(pts), dtype=np.int64)
            where[perm] = np.arange(len(pts))
            pc1[b, :, :len(pts)] = pts[perm].T.astype(np.float32)
            pc1[b, :, len(pts):] = pc1[b, :, :1]
            start = np.cumsum((0,) + sizes[b])
            own = [[int(where[i]) for i in range(start[j], start[j + 1])] for j in range(4)]
            spare = [int(where[i]) for i in range(start[4], len(pts))]
            preds = [(30 + 100 * (f == 1 and b == 1), own[0]), (31, own[1][:-1] + spare[:1]), (32, own[2][:1]), (532, own[2][1:])]
            if f > 0:
                preds.append((33, own[3]))
            preds.append((900 + f, spare[1:4]))
            if f == 1:
                preds.reverse()
            for i, (tid, cols) in enumerate(preds):
                obj[b, cols], ids[b, i] = i, tid
                c = pc1[b][:, cols].astype(np.float64).mean(axis=1)
                det_box[b, i], det_valid[b, i] = (c[0], c[1], c[2], 2.0, 1.5, 2.0, 0.1 * i, 0.0), 3
            num[b] = len(preds)
        frames.append(dict(per_stream=per_stream, pc1=pc1, obj=obj, num=num, ids=ids, det_box=det_box, det_valid=det_valid,
                           conf=rng.random((B, Kobj)).astype(np.float32), n_valid=np.array(n_valid, dtype=np.int32),
                           reset=np.array([f == 1, 0], dtype=np.uint8), active=np.array([1, f != 2], dtype=np.uint8)))
    return frames, B, N, Kobj, K


def _bytes(t):
    return t.cpu().numpy().tobytes()


def test_all_ten_variants_of_the_scoring_launch_agree_outside_the_pair_log():
    """The same frames through the ten instantiations the one launcher chooses among: whatever a variant adds, everything but the pair
    log is the plain launch's bit for bit, and the main log is the same in the eight variants that keep one.  The memory variants get
    the detections themselves as the table (table_ids = object_ids, table_count = num_objects), so nothing coasts."""
    frames, B, N, Kobj, K = _tail_frames()
    log, pairs = dict(sweep_frames=4, sweep_records=32), dict(sweep_frames=4, sweep_records=32, sweep_pairs=64)
    variants = dict(plain={}, logged=log, pairs=pairs, centre=dict(pairs, similarity="centre"), box=dict(pairs, similarity="box"))
    variants.update({k + "_memory": dict(v, track_memory=True) for k, v in list(variants.items())})
    variants["box_memory"]["similarity"] = "box_bev"                    # (the same instantiation: the mode is an argument)
    assert len(variants) == 10
    scorers = {k: TS.TrackScorer(streams=B, max_objects=Kobj, max_boxes=K, max_gt_tracks=8, **kw) for k, kw in variants.items()}
    matches = {k: [] for k in variants}
    for fr in frames:
        pc1, nv = _dev(fr["pc1"]), _dev(fr["n_valid"])
        gobj = TS.gt_objects(pc1, G.pack_boxes(fr["per_stream"], K, DEV), TS.pack_box_types(fr["per_stream"], K, DEV), n_valid=nv,
                             min_obj_points=S.MIN_PTS)
        args = [_dev(fr[k]) for k in ("obj", "num", "ids")]
        kw = dict(reset=_dev(fr["reset"]), active=_dev(fr["active"]), object_conf=_dev(fr["conf"]), table_ids=args[2], table_count=args[1],
                  det_boxes=_dev(fr["det_box"]), det_box_valid=_dev(fr["det_valid"]))
        for k, s in scorers.items():
            matches[k].append(s.update_raw(pc1, *args, gobj, nv, **kw))
    plain = scorers["plain"]
    res = plain.result()["overall"]
    assert not plain.flags.any() and res["frames"] == 5 and res["tp"] > 0 and res["fp"] > 0 and res["fn"] > 0 and res["idsw"] > 0, res
    assert sum(int(m.aff_defined.sum()) for m in matches["plain"]) > 0 and int(matches["plain"][2].pred_gt_id[1].max()) == -1
    for k, s in scorers.items():
        for f, (m, m0) in enumerate(zip(matches[k], matches["plain"])):
            for name in MATCH:
                assert _bytes(getattr(m, name)) == _bytes(getattr(m0, name)), (k, f, name)
        for name in STATE:
            assert _bytes(getattr(s, name)) == _bytes(getattr(plain, name)), (k, name)
        # each scorer really ran its own variant: the record of the table, the logs, the similarity
        assert s.track_memory == k.endswith("_memory") and s.logging == (not k.startswith("plain"))
        if s.track_memory:
            assert s.row_track[0].tolist() == frames[2]["ids"][0].tolist() and s.row_track[1].tolist() == frames[1]["ids"][1].tolist(), k
            assert not s.labelled_coasted.any(), k
        if s.logging:
            for name in LOG:
                assert _bytes(getattr(s, name)) == _bytes(getattr(scorers["logged"], name)), (k, name)
            assert s.log_cursor[:, 0].tolist() == [3, 2] and s.log_cursor[:, 1].tolist() == [int(sum(fr["num"][0] for fr in frames)),
                                                                                            int(sum(fr["num"][1] for fr in frames[:2]))], k
        if s.pairs:
            assert s.pair_cursor.min() > 0 and s.pair_frame[0, :3, 1].sum() == s.pair_cursor[0], k
            assert (s.pair_sim[:, 0] > 0).all() if s.has_sim else not hasattr(s, "pair_sim"), k
    # the pair logs differ where they should: the point IoU, the centre distance and the two box IoUs are four different similarities
    assert _bytes(scorers["centre"].pair_sim) != _bytes(scorers["box"].pair_sim) != _bytes(scorers["box_memory"].pair_sim)
    assert _bytes(scorers["centre"].pair_sim) == _bytes(scorers["centre_memory"].pair_sim)
    assert _bytes(scorers["pairs"].pair_key) == _bytes(scorers["pairs_memory"].pair_key)
