"""GPU: HOTA over the scorer's log (ratrack_amd/track_score.py `TrackScorer.hota`, csrc/track_hota.hip `rtk_score_hota`) against the
host statement of tests/_track_hota_util.py.  The device delivers integers and fixed-order float64 sums and the host does the same
arithmetic on them, so everything is compared with == / bit for bit: every counter and every sum at every level and stream, every
ratio, HOTA and its parts."""
import math

import numpy as np
import pytest
import torch

import _gt_util as U
import _track_hota_util as H
import _track_score_util as S
import _track_sweep_util as W
from _util import reference_state_dict
from ratrack_amd import gt_device as G
from ratrack_amd import synth, tracker as T, track_score as TS, vod_gt
from ratrack_amd.track4d import Args, Track4D

pytestmark = pytest.mark.gpu
DEV = "cuda"
STATE = ("counters", "iou_sum", "table_key", "table_last", "table_seen", "table_matched", "table_used", "prev_gt_id", "prev_count", "prev_gt",
         "flags")
LOG = ("log_cursor", "log_frame", "log_label", "log_track", "log_best", "log_conf", "log_iou")
PER_LEVEL = ("tp", "fn", "fp", "gt", "pred", "pairs", "deta", "detre", "detpr", "assa", "assre", "asspr", "loca", "hota_alpha")
MEANS = ("hota", "deta_mean", "assa_mean", "detre_mean", "detpr_mean", "assre_mean", "asspr_mean", "loca_mean")
CI = {k: i for i, k in enumerate(H.COUNTERS)}
SI = {k: i for i, k in enumerate(H.SUMS)}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def _check(ho, host, streams=None):
    """A HotaResult against `host_hota`'s dict: counters ==, the four sums bit for bit, every value ==.  streams: only these (the
    values are then recomputed for them on both sides)."""
    c, q = np.asarray(ho.counters), np.asarray(ho.sums)
    hc, hq = host["counters"], host["sums"]
    if streams is not None:
        c, q, hc, hq = c[:, streams], q[:, streams], hc[:, streams], hq[:, streams]
        dev, host = TS.hota_values(c, q), H.values(hc, hq)
    else:
        dev = ho.__dict__
    assert np.array_equal(c, hc), np.argwhere(c != hc)[:8]
    assert np.array_equal(_bits(q), _bits(hq)), np.argwhere(_bits(q) != _bits(hq))[:8]
    for k in PER_LEVEL:
        assert len(dev[k]) == len(host[k]) and all(_same(float(x), float(y)) for x, y in zip(dev[k], host[k])), (k, dev[k], host[k])
    for k in MEANS:
        assert dev[k] == host[k], (k, dev[k], host[k])


def _same_result(a, b):
    assert np.array_equal(a.counters, b.counters) and np.array_equal(_bits(a.sums), _bits(b.sums)) and np.array_equal(a.flags, b.flags)
    assert all(getattr(a, k) == getattr(b, k) for k in MEANS)
    assert all(np.array_equal(_bits(getattr(a, k)), _bits(getattr(b, k))) for k in PER_LEVEL)


# ---- 1 and 2: the planned sequence ---------------------------------------------------------------------------------------------------
def _scorer(seq):
    return TS.TrackScorer(streams=seq["B"], max_objects=seq["K"], max_boxes=seq["K"], max_gt_tracks=64, sweep_frames=16, sweep_records=128)


def _feed(seq, confs, scorers, frames):
    K = seq["K"]
    for f, (fr, conf) in enumerate(zip(seq["frames"], confs)):
        if f not in frames:
            continue
        pc1, nv = _dev(fr["pc1"]), _dev(fr["n_valid"])
        gobj = TS.gt_objects(pc1, G.pack_boxes(fr["per_stream"], K, DEV), TS.pack_box_types(fr["per_stream"], K, DEV), n_valid=nv,
                             min_obj_points=S.MIN_PTS)
        for sc in scorers:
            sc.update_raw(pc1, _dev(fr["obj"]), _dev(fr["num"]), _dev(fr["ids"]), gobj, nv, _dev(fr["reset"]), _dev(fr["active"]),
                          object_conf=_dev(conf))


@pytest.fixture(scope="module")
def planned():
    """The planned sequence through two logging scorers, one of which evaluates HOTA after six frames."""
    seq, confs, logs, sw = W.planned()
    assert (seq["B"], seq["N"], seq["K"], len(seq["frames"])) == (16, 256, 32, 12)
    scorer, plain = _scorer(seq), _scorer(seq)
    _feed(seq, confs, (scorer, plain), range(0, 6))
    mid = scorer.hota()                                     # reads only: scoring goes on
    _feed(seq, confs, (scorer, plain), range(6, 12))
    return dict(seq=seq, logs=logs, sw=sw, scorer=scorer, plain=plain, mid=mid)


def test_hota_of_the_planned_sequence_equals_the_host_statement(planned):
    scorer, plain, logs = planned["scorer"], planned["plain"], planned["logs"]
    for k in STATE + LOG:
        assert torch.equal(getattr(scorer, k), getattr(plain, k)), k
    scorer.check()
    host = H.host_hota(logs)
    ho = scorer.hota()
    print("HOTA %.6f DetA %.6f AssA %.6f LocA %.6f; tp %s; pairs %s" % (ho.hota, ho.deta_mean, ho.assa_mean, ho.loca_mean, ho.tp.tolist(),
                                                                       ho.pairs.tolist()))
    _check(ho, host)
    assert ho.alphas == 19 and ho.alpha.tolist() == H.alpha_levels(19) and ho.threshold is None and not ho.flags.any()
    assert ho.tp[0] == 273 and ho.tp[-1] == 81 and ho.pairs[0] == 66 and abs(ho.hota - 0.41369681694671) < 1e-13
    assert sum(host["freed"]) > 100                         # the matches a "replay, then drop" evaluation would not find
    # every stream on its own
    for b in range(len(logs)):
        _check(ho, host, streams=[b])
    # gt is the scorer's at every level; the run after six frames saw half of the log
    gt = scorer.counters[:, TS.COUNTERS.index("gt")].cpu().numpy()
    assert all(np.array_equal(ho.counters[a, :, CI["gt"]], gt) for a in range(19))
    mid = planned["mid"]
    seen = [sum(int(fr["active"][b]) for fr in planned["seq"]["frames"][:6]) for b in range(len(logs))]
    _check(mid, H.host_hota([lb[:n] for lb, n in zip(logs, seen)]))
    assert 0 < mid.counters[0, :, CI["frames"]].sum() < ho.counters[0, :, CI["frames"]].sum()
    # the same bits on a second call, and the state and the log it read are untouched
    _same_result(ho, scorer.hota())
    for k in STATE + LOG:
        assert torch.equal(getattr(scorer, k), getattr(plain, k)), k
    # another number of levels
    h9 = scorer.hota(alphas=9)
    _check(h9, H.host_hota(logs, A=9))
    assert h9.alpha.tolist() == [a / 10 for a in range(1, 10)] and h9.counters.shape == (9, 16, 6)


def test_hota_at_a_threshold_equals_the_filtered_host_statement(planned):
    scorer, logs, sw = planned["scorer"], planned["logs"], planned["sw"]
    best = scorer.sweep().best
    assert best["level"] == sw["best"] == 9 and best["threshold"] == 0.55234375
    host = H.host_hota(logs, sw["scores"], best["threshold"])
    ho = scorer.hota(threshold=best["threshold"])
    _check(ho, host)
    assert ho.threshold == best["threshold"] and ho.tp[0] == 118 and ho.tp[-1] == 19 and ho.pred[0] < 617 and ho.gt[0] == 363
    _same_result(ho, scorer.hota(threshold=torch.tensor(best["threshold"], dtype=torch.float64, device=DEV)))       # a 0-dim tensor
    # a score equal to the threshold stays; -inf removes nothing
    plain = scorer.hota()
    low = scorer.hota(threshold=float("-inf"))
    assert low.threshold == float("-inf")
    _same_result(plain, low)
    assert not np.array_equal(plain.counters, ho.counters)


# ---- 3: fabricated logs --------------------------------------------------------------------------------------------------------------
F, R = 64, 4096


def _det(tid, best=-1, iou=0.0, conf=0.0):
    return (int(tid), np.float32(conf), int(best), float(iou))


def _frame(labels, dets, reset=False):
    return dict(reset=bool(reset), labels=[int(v) for v in labels], dets=list(dets))


def _fabricated(logs, max_gt_tracks=1024):
    """A scorer whose log_* tensors hold `logs` (per stream a list of frames), written as rtk_track_score_logged packs them."""
    B = len(logs)
    sc = TS.TrackScorer(streams=B, max_objects=8, max_boxes=8, max_gt_tracks=max_gt_tracks, sweep_frames=F, sweep_records=R)
    cursor, frame = np.zeros((B, 4), np.int32), np.zeros((B, F, 4), np.int32)
    label, track, best = np.zeros((B, R), np.int32), np.zeros((B, R), np.int32), np.zeros((B, R), np.int32)
    conf, iou = np.zeros((B, R), np.float32), np.zeros((B, R), np.float64)
    for b, lb in enumerate(logs):
        r = l = 0
        assert len(lb) <= F
        for f, e in enumerate(lb):
            P, Gk = len(e["dets"]), len(e["labels"])
            assert P <= TS.MAX_OBJECTS and Gk <= TS.MAX_BOXES and r + P <= R and l + Gk <= R
            frame[b, f] = (r, l, P + 65536 * int(e["reset"]), Gk)
            label[b, l:l + Gk] = e["labels"]
            for i, d in enumerate(e["dets"]):
                track[b, r + i], conf[b, r + i], best[b, r + i], iou[b, r + i] = d
            r, l = r + P, l + Gk
        cursor[b, :3] = (len(lb), r, l)
    for name, a in (("cursor", cursor), ("frame", frame), ("label", label), ("track", track), ("best", best), ("conf", conf), ("iou", iou)):
        getattr(sc, "log_" + name).copy_(_dev(a))
    return sc


def _one_label(ids, absent=(), reset_at=()):
    """Label 7 with IoU 0.9 under track id ids[f] in every frame not in `absent` (there: no label and no detection)."""
    return [_frame([], [], f == 0) if f in absent else _frame([7], [_det(tid, 7, 0.9)], f == 0 or f in reset_at) for f, tid in enumerate(ids)]


def test_fabricated_logs_levels_identities_and_clips():
    third = 3.0 / 5.0
    logs = [
        # (a) two detections share one best label, IoU 0.3 then 0.7; (b) an IoU that is a level
        [_frame([5, 6], [_det(1, 5, 0.3), _det(2, 5, 0.7), _det(3, 6, third)], True)],
        # (c) one label for ten frames whose track id changes after five
        _one_label([1] * 5 + [2] * 5),
        # (d) seen in frames 0-3, absent in 4-5, back in 6-9: under the same id, and under a fresh one
        _one_label([4] * 10, absent=(4, 5)),
        _one_label([4] * 6 + [9] * 4, absent=(4, 5)),
        # (e) a reset in mid-log: the same (label, track) on both sides
        _one_label([3] * 8, reset_at=(4,)),
    ]
    sc = _fabricated(logs)
    ho = sc.hota()
    _check(ho, H.host_hota(logs))
    per = lambda b: TS.hota_values(ho.counters[:, b:b + 1], ho.sums[:, b:b + 1])
    c, q = ho.counters, ho.sums
    # (a): label 5 goes to the first detection up to 0.30, to the second from 0.35 to 0.70, to none above
    assert c[:, 0, CI["tp"]].tolist() == [2] * 12 + [1] * 2 + [0] * 5           # label 6's match ends after 0.60, see (b)
    assert (c[:, 0, CI["pred"]] == 3).all() and (c[:, 0, CI["gt"]] == 2).all()
    for a in range(19):                                                           # loc adds in detection order, from 0
        loc = 0.3 + third if a <= 5 else 0.7 + third if a <= 11 else 0.0 + 0.7 if a <= 13 else 0.0
        assert q[a, 0, SI["loc"]] == loc, (a, q[a, 0, SI["loc"]], loc)
    # the pair is (5, track 1) then (5, track 2): ct = 1 each, cg = 1
    assert q[5, 0, SI["ass"]] == 2.0 and q[6, 0, SI["ass"]] == 2.0 and q[12, 0, SI["ass"]] == 1.0 and q[14, 0, SI["ass"]] == 0.0
    # (b): 3/5 >= 12/20 and not >= 13/20
    assert ho.alpha[11] == third and c[11, 0, CI["tp"]] == 2 and c[12, 0, CI["tp"]] == 1 and c[12, 0, CI["pairs"]] == 1
    # (c): DetA 1 and AssA 0.5 exactly (two pairs of 5 matches: 25 / (10 + 5 - 5) each, over 10)
    v = per(1)
    assert v["deta"][0] == 1.0 and v["assa"][0] == 0.5 and v["pairs"][0] == 2 and v["assre"][0] == 0.5 and v["asspr"][0] == 1.0
    assert v["hota_alpha"][0] == math.sqrt(0.5) and v["loca"][0] == sum([0.9] * 10) / 10
    # (d): the re-acquisition -- same id AssA 1, fresh id AssA 0.5; CLEAR-MOT sees one idsw
    same, fresh = per(2), per(3)
    assert same["assa"][0] == 1.0 and fresh["assa"][0] == 0.5 and same["deta"][0] == fresh["deta"][0] == 1.0
    assert same["tp"][0] == fresh["tp"][0] == 8 and same["pairs"][0] == 1 and fresh["pairs"][0] == 2
    assert c[0, 2, CI["frames"]] == 10 and c[0, 2, CI["clips"]] == 1
    sw = sc.sweep(levels=1, check=False)
    u = sw.counters[0]
    col = lambda k: TS.COUNTERS.index(k)
    assert u[2, col("idsw")] == 0 and u[3, col("idsw")] == 1
    assert all(u[2, col(k)] == u[3, col(k)] for k in ("gt", "pred", "tp", "fp", "fn"))
    mota = lambda b: 1.0 - (u[b, col("fp")] + u[b, col("fn")] + u[b, col("idsw")]) / u[b, col("gt")]
    assert mota(2) == 1.0 and mota(3) == 1.0 - 1 / 8
    # (e): two clips, two pairs, each whole: AssA 1
    v = per(4)
    assert c[0, 4, CI["clips"]] == 2 and v["pairs"][0] == 2 and v["assa"][0] == 1.0 and v["tp"][0] == 8
    # IoU 0.9 is below the last level only
    assert (c[17, 1:, CI["tp"]] > 0).all() and (c[18, 1:, CI["tp"]] == 0).all()


def _overflow(bad, flagged=2, max_gt_tracks=1024):
    small = [_one_label([1] * 5 + [2] * 5), _frame_list_two(), [], _one_label([3] * 8, reset_at=(4,))]
    logs = small[:flagged] + [bad] + small[flagged + 1:]
    sc = _fabricated(logs, max_gt_tracks=max_gt_tracks)
    with pytest.raises(RuntimeError, match="TrackScorer.hota: stream %d has a clip with more than max_gt_tracks=%d label ids, %d track ids or %d"
                                           % (flagged, max_gt_tracks, TS.SWEEP_TRACKS, TS.HOTA_PAIRS)):
        sc.hota()
    ho = sc.hota(check=False)
    assert ho.flags.tolist() == [TS.FLAG_HOTA if b == flagged else 0 for b in range(4)], ho.flags
    assert int(sc.flags.sum()) == 0                         # the scorer's own sticky flags are not written
    others = [b for b in range(4) if b != flagged]
    _check(ho, H.host_hota(logs), streams=others)
    return ho


def _frame_list_two():
    return [_frame([1, 2], [_det(10 + f % 2, 1, 0.5), _det(20, 2, 0.8), _det(30 + f)], f == 0) for f in range(6)]


def test_a_clip_with_too_many_pairs_flags_its_stream_alone():
    # 17 labels matched by fresh track ids on every one of 64 frames: 1088 pairs (and 1088 track ids, which fit)
    bad = [_frame(range(17), [_det(100 + 17 * f + g, g, 0.9) for g in range(17)], f == 0) for f in range(F)]
    assert 17 * F > TS.HOTA_PAIRS and 17 * F <= TS.SWEEP_TRACKS
    _overflow(bad)
    # one frame fewer than the limit needs: no flag, the host's numbers
    fits = [bad[:TS.HOTA_PAIRS // 17], [], [], []]
    sc = _fabricated(fits)
    ho = sc.hota()
    _check(ho, H.host_hota(fits))
    assert ho.pairs[0] == ho.tp[0] == 17 * (TS.HOTA_PAIRS // 17) and not ho.flags.any()


def test_a_clip_with_too_many_track_ids_or_labels_flags_its_stream_alone():
    # 33 unmatched detections with fresh track ids on every one of 64 frames: 2112 track ids, no pair at all
    bad = [_frame([1], [_det(1000 + 33 * f + i) for i in range(33)], f == 0) for f in range(F)]
    assert 33 * F > TS.SWEEP_TRACKS
    _overflow(bad, flagged=1)
    # with a threshold the track scores refuse the same stream
    logs = [[], bad, [], []]
    sc = _fabricated(logs)
    with pytest.raises(RuntimeError, match="stream 1 has more than %d track ids in one clip" % TS.SWEEP_TRACKS):
        sc.hota(threshold=0.0)
    # a reset in the middle halves the clip: it fits
    halved = [dict(e, reset=(f in (0, F // 2))) for f, e in enumerate(bad)]
    sc = _fabricated([[], halved, [], []])
    ho = sc.hota()
    _check(ho, H.host_hota([[], halved, [], []]))
    assert ho.pred[0] == 33 * F and ho.tp[0] == 0 and ho.deta[0] == 0.0 and np.isnan(ho.assa[0])
    # more label ids in a clip than max_gt_tracks
    bad = [_frame([f], [_det(1, f, 0.9)], f == 0) for f in range(5)]
    _overflow(bad, flagged=0, max_gt_tracks=4)


def test_an_empty_log_and_a_stream_without_frames():
    sc = _fabricated([[], [], [], []])
    ho = sc.hota()
    assert not ho.counters.any() and not ho.sums.any() and not ho.flags.any() and ho.hota == 0.0 and ho.deta_mean == 0.0
    assert all(np.isnan(getattr(ho, k)).all() for k in ("deta", "assa", "loca", "hota_alpha"))
    _check(ho, H.host_hota([[], [], [], []]))
    assert np.isnan(sc.hota(threshold=0.5).deta).all()
    logs = [_one_label([1] * 3), [], _one_label([2] * 4), []]
    ho = _fabricated(logs).hota()
    _check(ho, H.host_hota(logs))
    assert not ho.counters[:, 1].any() and not ho.counters[:, 3].any() and ho.tp[0] == 7 and ho.counters[0, :, CI["clips"]].tolist() == [1, 0, 1, 0]


# ---- 4: behind the tracker -----------------------------------------------------------------------------------------------------------
def test_hota_behind_a_tracker_with_track_memory():
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
    scorer = TS.TrackScorer(streams=B, max_objects=trk.K, max_boxes=K, max_gt_tracks=32, sweep_frames=8, sweep_records=8 * trk.K)
    for step in range(steps):
        pc1, pc2, f1, f2, nv = vod_gt.pad_frame_pairs(pairs, device=DEV)
        reset = torch.tensor([step == 0, step in (0, 3), step == 0, step == 0], dtype=torch.uint8, device=DEV)
        active = torch.ones(B, dtype=torch.uint8, device=DEV)
        with torch.no_grad():
            flow, h, cls, _, _, _, prop = net._fused_engine().backbone(pc1, pc2, f1, f2, trk.h, n_valid=nv)
        out = trk.associate(pc1, f1, flow, cls, prop, nv, reset, active)
        gobj = TS.gt_objects(pc1, bb, types, n_valid=nv, min_obj_points=net.min_obj_points)
        scorer.update(out, gobj, reset=reset, active=active)
        trk.h = h
    scorer.check()
    logs = H.entries_from_log(*(getattr(scorer, k).cpu().numpy() for k in LOG))
    assert [len(lb) for lb in logs] == [steps] * B and sum(e["reset"] for e in logs[1]) == 2
    host = H.host_hota(logs)
    ho = scorer.hota()
    print("behind the tracker: HOTA %.6f DetA %.6f AssA %.6f LocA %.6f, tp %s" % (ho.hota, ho.deta_mean, ho.assa_mean, ho.loca_mean, ho.tp.tolist()))
    _check(ho, host)
    assert ho.tp[0] > 0 and ho.counters[0, :, CI["clips"]].tolist() == [1, 2, 1, 1]
    res = scorer.result()
    for k in ("frames", "gt", "pred"):
        assert np.array_equal(ho.counters[0, :, CI[k]], res["per_stream"][k]), k
    sw = scorer.sweep()
    if sw.best is not None:
        scores = [W.track_scores(lb)[0] for lb in logs]
        _check(scorer.hota(threshold=sw.best["threshold"]), H.host_hota(logs, scores, sw.best["threshold"]))


# ---- 5: what the score now sees of track memory ---------------------------------------------------------------------------------------
def test_assa_sees_how_much_of_a_life_the_gap_costs():
    """The constructed case of tests/test_track_motion_gpu.py (three objects at 1.2 m per frame, one hidden for two of six frames):
    held still the returning object gets a fresh id, moved it keeps its own.  CLEAR-MOT counts one idsw of 18; AssA says the object
    spent its life under two ids."""
    import test_track_motion_gpu as M

    def scored(motion):
        trk = T.BatchedTracker(M.affinity_net(8.0, 4.0), streams=1, max_objects=8, max_age=2, motion=motion)
        scorer = TS.TrackScorer(streams=1, max_objects=8, max_boxes=8, max_gt_tracks=16, sweep_frames=8, sweep_records=64)
        for t, frame in enumerate(M.fast_scenario(2)):
            first = torch.tensor([t == 0], dtype=torch.uint8, device=DEV)
            out = M.associate(trk, frame, reset=first)
            c = M.fast_centres(t).tolist()
            labels = {k: vod_gt.Label("Car", k, 0, 0, 0, 0, 0, 0, 3.0, 4.0, 6.0, c[k][0], c[k][1], c[k][2], 0.0) for k in range(3)}
            per_stream = [(labels, U.IDENTITY_TF, labels, U.IDENTITY_TF)]
            nv = torch.tensor([frame[0]["n_valid"]], dtype=torch.int32, device=DEV)
            gobj = TS.gt_objects(out.pc1, G.pack_boxes(per_stream, 8, DEV), TS.pack_box_types(per_stream, 8, DEV), n_valid=nv, min_obj_points=2)
            scorer.update(out, gobj, reset=first)
        trk.check()
        ho = scorer.hota()
        _check(ho, H.host_hota(H.entries_from_log(*(getattr(scorer, k).cpu().numpy() for k in LOG))))
        return ho, scorer.result()["overall"]

    (held, hr), (moving, mr) = scored(None), scored("flow")
    print("held still: AssA %.6f HOTA %.6f; moved: AssA %.6f HOTA %.6f; AssA per level %s against %s"
          % (held.assa_mean, held.hota, moving.assa_mean, moving.hota, held.assa.tolist(), moving.assa.tolist()))
    assert int(hr["idsw"]) == 1 and int(mr["idsw"]) == 0 and int(hr["gt"]) == 18
    assert held.tp.tolist() == moving.tp.tolist() and held.tp[0] == 16 and np.array_equal(_bits(held.deta), _bits(moving.deta))
    assert held.pairs[0] == 4 and moving.pairs[0] == 3
    # the hidden object has 6 frames of life and 4 matches: under one id 16 / (6 + 4 - 4), under two ids 4 / (6 + 2 - 2) twice
    assert moving.sums[0, 0, SI["ass"]] == 16.0 / 6.0 + 6.0 + 6.0 and moving.assa[0] == (16.0 / 6.0 + 6.0 + 6.0) / 16.0
    assert held.sums[0, 0, SI["ass"]] == 4.0 / 6.0 + 6.0 + 6.0 + 4.0 / 6.0
    assert held.assa_mean < moving.assa_mean and held.hota < moving.hota
    assert mr["mota"] - hr["mota"] == pytest.approx(1 / 18)
