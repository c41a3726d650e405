"""GPU: the pair log (csrc/track_score.hip `rtk_track_score_pairs`, `TrackScorer(sweep_pairs=...)`) and the replay under the
per-frame optimal matching (csrc/track_optimal.hip `rtk_score_replay_optimal`, `TrackScorer.sweep(matching="optimal")`,
`clear_optimal`) against the host statement of tests/_track_optimal_util.py.  The device delivers integers and fixed-order float64
sums, so everything is compared with == / bit for bit."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _gt_util as U
import _track_optimal_util as O
import _track_score_util as S
import _track_sweep_util as W
from _util import reference_state_dict
from ratrack_amd import gt_device as G
from ratrack_amd import synth, tracker as T, track_score as TS, vod_gt
from ratrack_amd.abi import stream as _stream
from ratrack_amd.track4d import Args, Track4D

pytestmark = pytest.mark.gpu
DEV = "cuda"
STATE = ("counters", "iou_sum", "table_key", "table_last", "table_seen", "table_matched", "table_used", "prev_gt_id", "prev_count", "prev_gt",
         "flags")
LOG = ("log_cursor", "log_frame", "log_label", "log_track", "log_best", "log_conf", "log_iou")
PAIRS = ("pair_cursor", "pair_frame", "pair_key", "pair_common", "log_size", "log_label_size")
OUT = ("pred_gt_slot", "pred_gt_id", "gt_pred", "iou", "aff_target", "aff_defined")
CI = {k: i for i, k in enumerate(O.COUNTERS)}
SEED = 1                                   # tests/test_track_optimal_cpu.py checks what this seed's logs hold


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _equal_tensors(a, b, names):
    for k in names:
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8) if x.dtype.is_floating_point else x,
                                                   y.view(torch.uint8) if y.dtype.is_floating_point else y), k


def _holds(sc, arrays, names):
    for k in names:
        dev, host = getattr(sc, k).cpu().numpy(), arrays[k]
        assert dev.shape == host.shape and np.array_equal(dev.view(np.uint8), host.view(np.uint8)), (k, np.argwhere(dev != host)[:6])


def _download(sc):
    return O.entries_from_logs(*(getattr(sc, k).cpu().numpy() for k in LOG), *(getattr(sc, k).cpu().numpy() for k in PAIRS[1:]))


# ---- 1: logging the pairs changes nothing else -----------------------------------------------------------------------------------------
F_SMALL, R_SMALL = 16, 128


def _small_scorer(pairs):
    kw = dict(sweep_pairs=pairs) if pairs else {}
    return TS.TrackScorer(streams=3, max_objects=8, max_boxes=5, max_gt_tracks=16, sweep_frames=F_SMALL, sweep_records=R_SMALL, **kw)


def _feed_small(seq, scorers):
    K = seq["K"]
    for fr in seq["frames"]:
        pc1, nv = _dev(fr["pc1"]), _dev(fr["n_valid"])
        gobj = TS.gt_objects(pc1, G.pack_boxes(fr["per_stream"], K, DEV), TS.pack_box_types(fr["per_stream"], K, DEV), n_valid=nv,
                             min_obj_points=S.MIN_PTS)
        outs = [sc.update_raw(pc1, _dev(fr["obj"]), _dev(fr["num"]), _dev(fr["ids"]), gobj, nv, _dev(fr["reset"]), _dev(fr["active"]),
                              object_conf=_dev(fr["conf"])) for sc in scorers]
        for o in outs[1:]:
            _equal_tensors(outs[0], o, OUT)


@pytest.fixture(scope="module")
def small():
    seq = O.small_sequence()
    logs = O.small_sequence_log(seq)
    with_pairs, plain = _small_scorer(256), _small_scorer(None)
    _feed_small(seq, (with_pairs, plain))
    return dict(seq=seq, logs=logs, scorer=with_pairs, plain=plain)


def test_logging_the_pairs_changes_nothing_else_and_the_pair_log_is_the_hosts(small):
    sc, plain, logs = small["scorer"], small["plain"], small["logs"]
    _equal_tensors(sc, plain, STATE + LOG)
    sc.check()
    host = O.pack(logs, F_SMALL, R_SMALL, 256)
    _holds(sc, host, PAIRS + ("log_cursor", "log_frame", "log_label", "log_track", "log_best", "log_conf"))
    assert _download(sc) == [[dict(e, dets=[(d[0], d[1], d[2], float(d[3])) for d in e["dets"]]) for e in lb] for lb in logs]
    assert int(sc.pair_cursor.sum()) == sum(len(e["pairs"]) for lb in logs for e in lb) > 150
    assert not hasattr(plain, "pair_key")


def test_the_pair_log_running_out_drops_the_frame_from_both_logs(small):
    seq, logs, plain = small["seq"], small["logs"], small["plain"]
    Q = 18
    kept = [O.fitting(lb, F_SMALL, R_SMALL, Q) for lb in logs]
    # a stream drops a frame and logs a later, smaller one
    later = [any(e in kb for e in lb[lb.index(next(x for x in lb if x not in kb)):]) for lb, kb in zip(logs, kept) if len(kb) < len(lb)]
    assert all(len(kb) < len(lb) for lb, kb in zip(logs, kept)) and any(later), [len(kb) for kb in kept]
    sc = _small_scorer(Q)
    _feed_small(seq, (sc,))
    _holds(sc, O.pack(kept, F_SMALL, R_SMALL, Q), PAIRS + ("log_cursor", "log_frame", "log_label", "log_track", "log_best", "log_conf"))
    assert sc.flags.cpu().tolist() == [TS.FLAG_LOG] * 3
    with pytest.raises(RuntimeError, match="or its pair log of sweep_pairs=18 pairs"):
        sc.check()
    # the score itself saw every frame
    _equal_tensors(sc, plain, [k for k in STATE if k != "flags"])


def test_logging_the_pairs_behind_a_tracker_with_track_memory():
    sd = reference_state_dict(DEV)
    sd["fd_layer.cp.linear.bias"] = sd["fd_layer.cp.linear.bias"] + 0.09      # moving points in every frame (tests/test_tracker_gpu.py)
    net = Track4D(Args()).to(DEV)
    net.load_state_dict(sd, strict=True)
    net = net.eval()
    B, K, steps = 4, 8, 6
    trk = T.BatchedTracker(net, streams=B, max_age=2)
    t = {k: torch.from_numpy(v) for k, v in synth.make_frame_pairs(B, 128, case_id=50).items()}
    pairs = [(t["pc1"][i:i + 1], t["pc2"][i:i + 1], t["feature1"][i:i + 1], t["feature2"][i:i + 1]) for i in range(B)]
    per_stream = []
    for b in range(B):
        p = t["pc1"][b].numpy()
        mk = lambda k: vod_gt.Label("rider" if k == 2 else "Car", k, 0, 0, 0, 0, 0, 0, 3.0, 4.0, 6.0, float(p[0, 10 * k]), float(p[1, 10 * k]),
                                    float(p[2, 10 * k]), 0.3 * k)
        labels = {k: mk(k) for k in range(6)}
        per_stream.append((labels, U.IDENTITY_TF, labels, U.IDENTITY_TF))
    bb, types = G.pack_boxes(per_stream, K, DEV), TS.pack_box_types(per_stream, K, DEV)
    mk_scorer = lambda **kw: TS.TrackScorer(streams=B, max_objects=trk.K, max_boxes=K, max_gt_tracks=32, sweep_frames=8, sweep_records=8 * trk.K,
                                            track_memory=True, **kw)
    sc, plain = mk_scorer(sweep_pairs=4096), mk_scorer()
    host = [[] for _ in range(B)]
    for step in range(steps):
        pc1, pc2, f1, f2, nv = vod_gt.pad_frame_pairs(pairs, device=DEV)
        reset = torch.tensor([step == 0, step in (0, 3), step == 0, step == 0], dtype=torch.uint8, device=DEV)
        active = torch.ones(B, dtype=torch.uint8, device=DEV)
        with torch.no_grad():
            flow, h, cls, _, _, _, prop = net._fused_engine().backbone(pc1, pc2, f1, f2, trk.h, n_valid=nv)
        out = trk.associate(pc1, f1, flow, cls, prop, nv, reset, active)
        gobj = TS.gt_objects(pc1, bb, types, n_valid=nv, min_obj_points=net.min_obj_points)
        a, b2 = sc.update(out, gobj, reset=reset, active=active), plain.update(out, gobj, reset=reset, active=active)
        _equal_tensors(a, b2, OUT)
        trk.h = h
        # the host's pairs, from the detections' point sets and the kept objects' (gt_objects' members: that launch is pinned elsewhere)
        pc, obj, num, ids, conf = (x.cpu().numpy() for x in (out.pc1, out.obj, out.num_objects, out.object_ids, out.object_conf))
        members, count, label_id = gobj.members.cpu().numpy().view(np.uint32), gobj.count.cpu().numpy(), gobj.label_id.cpu().numpy()
        for b in range(B):
            n = int(nv.reshape(-1, B)[0, b]) if nv is not None else pc.shape[2]
            kept = {}
            for j in range(int(count[b])):
                cols = [p for p in range(n) if (int(members[b, j, p >> 5]) >> (p & 31)) & 1]
                kept[int(label_id[b, j])] = torch.from_numpy(np.ascontiguousarray(pc[b][:, cols])).unsqueeze(0)
            objects = S.objects_dict(pc[b], obj[b, :n], ids[b], int(num[b]))
            host[b].append(O.host_entry([None] * 7 + [kept], objects, conf[b, :len(objects)], bool(reset[b])))
    sc.check()
    _equal_tensors(sc, plain, STATE + LOG + ("row_track", "labelled_coasted"))
    got = _download(sc)
    strip = lambda lb: [dict(reset=e["reset"], labels=e["labels"], tracks=[d[0] for d in e["dets"]], sizes=e["sizes"],
                             label_sizes=e["label_sizes"], pairs=e["pairs"]) for e in lb]
    assert [strip(lb) for lb in got] == [strip(lb) for lb in host]
    assert sum(len(e["pairs"]) for lb in got for e in lb) > 0
    # and the optimal replay of that log is the host's
    res = sc.clear_optimal(0.25)
    cn, iq, qs = O.host_replays(got, [[[0.0] * len(e["dets"]) for e in lb] for lb in got], [-math.inf], 0.25)
    assert np.array_equal(np.stack([res["per_stream"][k] for k in O.COUNTERS], axis=1), cn[0])
    assert np.array_equal(res["per_stream"]["iou_q"], iq[0]) and np.array_equal(_bits(res["per_stream"]["iou_sum"]), _bits(qs[0]))


# ---- 2: fabricated logs with known answers ---------------------------------------------------------------------------------------------
F, R, Q = 64, 4096, 8192


def _fabricated(logs, max_gt_tracks=1024):
    """A scorer whose log and pair-log tensors hold `logs`, written as rtk_track_score_pairs packs them."""
    sc = TS.TrackScorer(streams=len(logs), max_objects=8, max_boxes=8, max_gt_tracks=max_gt_tracks, sweep_frames=F, sweep_records=R, sweep_pairs=Q)
    for k, a in O.pack(logs, F, R, Q).items():
        getattr(sc, k).copy_(_dev(a))
    return sc


def _plain_scores(logs):
    return [[[0.0] * len(e["dets"]) for e in lb] for lb in logs]


def _check_point(sc, logs, min_iou, threshold=None, streams=None, check=True):
    """clear_optimal against host statement (a): the 12 counters and iou_q ==, iou_sum bit for bit, per stream."""
    res = sc.clear_optimal(min_iou, threshold=threshold, check=check)
    scores = _plain_scores(logs) if threshold is None else [W.track_scores(lb)[0] for lb in logs]
    cn, iq, qs = O.host_replays(logs, scores, [-math.inf if threshold is None else threshold], min_iou)
    dev = np.stack([res["per_stream"][k] for k in O.COUNTERS], axis=1)
    pick = list(range(len(logs))) if streams is None else streams
    assert np.array_equal(dev[pick], cn[0][pick]), (dev, cn[0])
    assert np.array_equal(res["per_stream"]["iou_q"][pick], iq[0][pick])
    assert np.array_equal(_bits(res["per_stream"]["iou_sum"])[pick], _bits(qs[0])[pick])
    return res


def _two_on_one_frame(reset=True, confs=(0.5, 0.5)):
    # d0 has IoU 0.6 with A and 0.5 with B, d1 has 0.55 with A only
    return O.make_frame([1, 2], [20, 10], [(10, confs[0], 20), (11, confs[1], 11)], [(0, 0, 15), (0, 1, 10), (1, 0, 11)], reset)


def _one(tid, on=True, reset=False):
    return O.frame_from_ious([7], [(tid, 0.5)], {(0, 0): 16} if on else {}, reset)


def test_fabricated_logs_with_known_answers():
    rng = np.random.default_rng(4)
    dense = O.make_frame(range(32), [40] * 32, [(100 + i, 0.5, 40) for i in range(32)],
                         [(i, j, int(rng.integers(1, 41))) for i in range(32) for j in range(32)], True)
    logs = [
        [_two_on_one_frame()],                                                                  # 0: greedy 1, optimal 2
        [_two_on_one_frame(confs=(0.125, 0.875))],                                             # 1: the threshold removes d0 and frees A
        [_one(1, reset=True), _one(1), _one(2), _one(2)],                                  # 2: an id switch
        [_one(1, reset=True), _one(1, on=False), _one(1)],                                 # 3: a fragmentation
        [_one(1, reset=True), _one(1, on=False), _one(1, on=False)],                       # 4: the same gap without a re-match
        [_one(1, reset=True), _one(1, on=False), _one(1, reset=True)],                     # 5: a reset closes the clip
        [O.make_frame([7, 8], [9, 9], [], [], True), O.make_frame([], [], [(1, 0.5, 9), (2, 0.5, 9)], []), _one(1)],      # 6: empty sides
        [dense],                                                                           # 7: 32 x 32, every pair present
    ]
    sc = _fabricated(logs)
    col = lambda res, k: res["per_stream"][k].tolist()
    res = _check_point(sc, logs, 0.3)
    assert not res["flags"].any()
    assert O.greedy_tp(logs[0][0]) == 1 and col(res, "tp")[0] == 2 and col(res, "fp")[0] == 0 and col(res, "fn")[0] == 0
    assert res["per_stream"]["iou_sum"][0] == 0.55 + 0.5 and res["per_stream"]["iou_q"][0] == int(0.55 * 65536) + int(0.5 * 65536)
    assert col(res, "idsw")[2:6] == [1, 0, 0, 0] and col(res, "frag")[2:6] == [0, 1, 0, 0] and col(res, "tracks")[2:6] == [1, 1, 1, 2]
    assert col(res, "tp")[2:6] == [4, 2, 1, 2] and col(res, "mt")[2:6] == [1, 0, 0, 1] and col(res, "pt")[2:6] == [0, 1, 1, 1]
    assert (col(res, "frames")[6], col(res, "gt")[6], col(res, "pred")[6], col(res, "tp")[6], col(res, "fp")[6], col(res, "fn")[6]) == (3, 3, 3, 1, 2, 2)
    assert col(res, "pred")[7] == 32 and 0 < col(res, "tp")[7] <= 32
    assert res["overall"]["tp"] == sum(col(res, "tp")) and res["overall"]["motp"] == res["overall"]["iou_sum"] / res["overall"]["tp"]
    # the dense frame with all of its 1024 pairs, against the independent solver
    low = _check_point(sc, logs, 0.01)
    _, edges, _ = O.frame_edges(dense, [0.0] * 32, -math.inf, 0.01)
    wb, _ = O.independent_solve(32, 32, edges)
    assert len(edges) == 1024 and (col(low, "tp")[7], int(low["per_stream"]["iou_q"][7])) == (32, wb & (O.ONE - 1)) and wb >> 23 == 32
    # an IoU exactly at min_iou stays; just above it the pair is refused and d0 goes back to A
    assert col(_check_point(sc, logs, 0.5), "tp")[0] == 2
    res = _check_point(sc, logs, 0.55)
    assert col(res, "tp")[0] == 1 and res["per_stream"]["iou_sum"][0] == 0.6 and col(res, "fp")[0] == 1
    assert col(_check_point(sc, logs, 0.61), "tp")[:2] == [0, 0]
    # a detection removed by the threshold frees its object: d0 (score 0.125) goes, d1 takes A
    res = _check_point(sc, logs, 0.3, threshold=0.5)
    assert (col(res, "pred")[1], col(res, "tp")[1]) == (1, 1) and res["per_stream"]["iou_sum"][1] == 0.55 and res["threshold"] == 0.5
    # a score equal to the threshold stays
    assert col(_check_point(sc, logs, 0.3, threshold=0.875), "pred")[1] == 1 and col(_check_point(sc, logs, 0.3, threshold=0.125), "pred")[1] == 2
    # the same bits on a second call, and nothing of the scorer is written
    again = sc.clear_optimal(0.3, threshold=0.5)
    assert all(np.array_equal(np.asarray(res["per_stream"][k]).view(np.int64), np.asarray(again["per_stream"][k]).view(np.int64))
               for k in O.COUNTERS + ("iou_q", "iou_sum"))
    assert int(sc.flags.sum()) == 0


def test_a_frame_with_too_many_candidates_flags_its_stream_alone():
    # 64 detections x 33 objects, every pair present: 2112 candidates in one frame
    bad = [O.make_frame(range(33), [40] * 33, [(100 + i, 0.5, 40) for i in range(64)], [(i, j, 20) for i in range(64) for j in range(33)], True)]
    assert len(bad[0]["pairs"]) > TS.PAIR_EDGES
    logs = [[_two_on_one_frame(), _one(1)], bad, [_one(1, reset=True), _one(1, on=False), _one(1)]]
    sc = _fabricated(logs)
    with pytest.raises(RuntimeError, match="stream 1 has a frame with more than %d candidate" % TS.PAIR_EDGES):
        sc.clear_optimal(0.3)
    res = sc.clear_optimal(0.3, check=False)
    assert res["flags"].tolist() == [0, TS.FLAG_OPTIMAL, 0] and int(sc.flags.sum()) == 0
    _check_point(sc, logs, 0.3, streams=[0, 2], check=False)
    # at a min_iou that refuses every pair of the frame (20 / 60) nothing overflows
    assert not _check_point(sc, logs, 0.34)["flags"].any()
    # one object fewer fits exactly: 2048 candidates, no flag, 32 matches
    fits = [[O.make_frame(range(32), [40] * 32, [(100 + i, 0.5, 40) for i in range(64)], [(i, j, 20) for i in range(64) for j in range(32)], True)]]
    res = _check_point(_fabricated(fits), fits, 0.3)
    assert not res["flags"].any() and res["per_stream"]["tp"].tolist() == [32]


# ---- 3: random logs ---------------------------------------------------------------------------------------------------------------------
def test_random_logs_equal_the_host_statement_and_the_independent_solver():
    logs = O.random_logs(SEED)
    B = len(logs)
    assert B == 4 and all(len(lb) == 40 for lb in logs)
    sc = _fabricated(logs)
    scores = [W.track_scores(lb)[0] for lb in logs]
    pool = sorted(s for sb in scores for f in sb for s in f)
    taus = [-math.inf] + [pool[len(pool) * k // 5] for k in range(1, 5)]
    min_iou = 0.2
    # the device's own track scores, then the replay at the five thresholds with the mask of index 0
    dev = sc.counters.device
    lg, pr = sc._log_block(), sc._pair_block()
    score = torch.zeros(B, R, dtype=torch.float64, device=dev)
    flags = torch.zeros(B, dtype=torch.int32, device=dev)
    TS._lib.call("rtk_score_track_means", B, ctypes.addressof(lg), score.data_ptr(), flags.data_ptr(), _stream())
    mask = torch.zeros(B, R, dtype=torch.uint8, device=dev)
    c, iq, q = sc._replay_optimal(ctypes.addressof(lg), ctypes.addressof(pr), score, _dev(np.array(taus)), None, len(taus), min_iou, mask, flags,
                                  _stream())
    c, iq, q, mask = c.cpu().numpy(), iq.cpu().numpy(), q.cpu().numpy(), mask.cpu().numpy()
    assert not flags.cpu().numpy().any()
    # (a): all 12 counters, iou_q, iou_sum
    cn, hq, hs = O.host_replays(logs, scores, taus, min_iou)
    assert np.array_equal(c, cn), np.argwhere(c != cn)[:8]
    assert np.array_equal(iq, hq) and np.array_equal(_bits(q), _bits(hs))
    assert cn[0, :, CI["idsw"]].sum() > 0 and cn[0, :, CI["frag"]].sum() > 0 and cn[0, :, CI["tp"]].sum() > cn[4, :, CI["tp"]].sum() > 0
    # (b) frame by frame: tp and iou_q of every frame, summed per stream; the matched rows wherever the optimum is unique
    uniq = total = 0
    for x, tau in enumerate(taus):
        for b in range(B):
            tp = iouq = r0 = 0
            first = O.replay(logs[b], scores[b], tau, min_iou)
            for f, (e, s) in enumerate(zip(logs[b], scores[b])):
                P, Gk = len(e["dets"]), len(e["labels"])
                _, edges, _ = O.frame_edges(e, s, tau, min_iou)
                wb, _ = O.independent_solve(P, Gk, edges)
                tp, iouq = tp + (wb >> 23), iouq + (wb & (O.ONE - 1))
                if x == 0:
                    rows = np.nonzero(mask[b, r0:r0 + P])[0].tolist()
                    assert rows == first[3][f], (b, f, rows, first[3][f])
                    if edges:
                        total += 1
                        only, match = O.unique_optimum(P, Gk, edges)
                        if only:
                            uniq += 1
                            assert rows == sorted(match) and {j: i for i, j in match.items()} == {j: i for j, i in enumerate(first[4][f]) if i >= 0}
                r0 += P
            assert (tp, iouq) == (int(c[x, b, CI["tp"]]), int(iq[x, b])), (x, b)
    assert total > 100 and 2 * uniq >= total, (uniq, total)
    assert mask.sum() == cn[0, :, CI["tp"]].sum()


# ---- 4: the sweep -----------------------------------------------------------------------------------------------------------------------
def _same_sweep(a, b, extra=()):
    for k in ("counters", "thresholds", "tp", "fp", "fn", "idsw", "gt", "pred", "tracks", "mt", "pt", "ml", "flags") + tuple(extra):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    for k in ("iou_sums", "mota", "smota", "motp", "moda", "recall", "precision"):
        assert np.array_equal(_bits(getattr(a, k)), _bits(getattr(b, k))), k
    assert (a.reached, a.levels, a.amota, a.samota, a.amotp, a.best, a.unfiltered) == (b.reached, b.levels, b.amota, b.samota, b.amotp, b.best,
                                                                                       b.unfiltered)


def test_the_sweep_under_the_optimal_matching_equals_the_host_statement(small):
    sc, plain, logs = small["scorer"], small["plain"], small["logs"]
    host = O.host_sweep(logs, 0.3)
    sw = sc.sweep(matching="optimal", min_iou=0.3)
    assert sw.matching == "optimal" and sw.min_iou == 0.3 and sw.reached == host["reached"] > 10 and not sw.flags.any()
    assert np.array_equal(_bits(sw.thresholds), _bits(host["thresholds"]))
    want = TS.optimal_sweep_values(host["counters"], host["iou_q"], host["iou_sums"], host["thresholds"], host["reached"], 40)
    for k in ("counters", "frag", "iou_q", "frag_streams", "iou_q_streams", "tp", "fp", "fn", "idsw", "gt", "pred", "tracks", "mt", "pt", "ml"):
        assert np.array_equal(getattr(sw, k), want[k]), k
    for k in ("iou_sums", "mota", "smota", "motp", "moda", "recall", "precision"):
        assert np.array_equal(_bits(getattr(sw, k)), _bits(want[k])), k
    assert (sw.amota, sw.samota, sw.amotp, sw.best, sw.unfiltered) == (want["amota"], want["samota"], want["amotp"], want["best"], want["unfiltered"])
    assert sw.best is not None and "frag" in sw.best and sw.motp[sw.best["level"]] == sw.iou_sum[sw.best["level"]] / sw.tp[sw.best["level"]]
    # the one operating point at the best threshold is that level of the sweep
    op = sc.clear_optimal(0.3, threshold=sw.best["threshold"])
    k = sw.best["level"]
    assert all(op["overall"][n] == int(getattr(sw, n)[k]) for n in ("tp", "fp", "fn", "idsw", "frag", "iou_q", "gt", "pred"))
    assert op["overall"]["mota"] == sw.best["mota"] and op["overall"]["motp"] == sw.best["motp"]
    # the same bits on a second run
    _same_sweep(sw, sc.sweep(matching="optimal", min_iou=0.3), extra=("frag", "iou_q", "frag_streams", "iou_q_streams"))
    # the default sweep afterwards on the same scorer is that of a scorer that never had a pair log
    g1, g0 = sc.sweep(), plain.sweep()
    assert g1.matching == "greedy" and g1.frag is None and g1.iou_q is None
    _same_sweep(g1, g0)
    _same_sweep(g1, sc.sweep())
    _equal_tensors(sc, plain, STATE + LOG)
