"""GPU: the identity metrics over the scorer's log (ratrack_amd/track_score.py `TrackScorer.identity`, csrc/track_identity.hip
`rtk_score_identity`, csrc/lds_assignment.h) against the host statement of tests/_track_identity_util.py.  The device delivers
integers and the host does the same arithmetic on them, so everything is compared with ==: every counter at every level and stream,
and every ratio.  The fabricated, random and dense clips are those on which a greedy pairing falls short of the optimum
(tests/test_track_identity_cpu.py asserts that of the generators)."""
import math

import numpy as np
import pytest
import torch

import _gt_util as U
import _track_hota_util as H
import _track_identity_util as I
import _track_memory_util as MEM
import _track_motion_util as MU
import _track_score_util as S
import _track_sweep_util as W
from ratrack_amd import gt_device as G
from ratrack_amd import tracker as T, track_score as TS, vod_gt
from ratrack_amd.track4d import Args, Track4D

pytestmark = pytest.mark.gpu
DEV = "cuda"
STATE = ("counters", "iou_sum", "table_key", "table_last", "table_seen", "table_matched", "table_used", "prev_gt_id", "prev_count", "prev_gt",
         "flags")
LOG = ("log_cursor", "log_frame", "log_label", "log_track", "log_best", "log_conf", "log_iou")
INTS = ("idtp", "idfn", "idfp", "gt", "pred", "pairs")
RATIOS = ("idf1", "idr", "idp")
CI = {k: i for i, k in enumerate(I.COUNTERS)}
HOTA_LEVELS = tuple(H.alpha_levels(19))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def _check(idn, host, streams=None):
    """An IdentityResult against `host_identity`'s dict: counters ==, every value ==.  streams: only these (the values are then
    recomputed for them on both sides)."""
    c, hc = np.asarray(idn.counters), host["counters"]
    if streams is not None:
        c, hc = c[:, streams], hc[:, streams]
        dev, host = TS.identity_values(c, idn.alpha), I.values(hc)
    else:
        dev = idn.__dict__
    assert np.array_equal(c, hc), np.argwhere(c != hc)[:8]
    for k in INTS + RATIOS:
        assert len(dev[k]) == len(host[k]) and all(_same(float(x), float(y)) for x, y in zip(dev[k], host[k])), (k, dev[k], host[k])


def _same_result(a, b):
    assert np.array_equal(a.counters, b.counters) and np.array_equal(a.flags, b.flags) and a.alpha.tolist() == b.alpha.tolist()
    for k in INTS + RATIOS:
        assert all(_same(float(x), float(y)) for x, y in zip(getattr(a, k), getattr(b, k))), k


# ---- 1: the planned sequence ---------------------------------------------------------------------------------------------------------
def _scorer(seq):
    return TS.TrackScorer(streams=seq["B"], max_objects=seq["K"], max_boxes=seq["K"], max_gt_tracks=64, sweep_frames=16, sweep_records=128)


def _feed(seq, confs, scorers):
    K = seq["K"]
    for fr, conf in zip(seq["frames"], confs):
        pc1, nv = _dev(fr["pc1"]), _dev(fr["n_valid"])
        gobj = TS.gt_objects(pc1, G.pack_boxes(fr["per_stream"], K, DEV), TS.pack_box_types(fr["per_stream"], K, DEV), n_valid=nv,
                             min_obj_points=S.MIN_PTS)
        for sc in scorers:
            sc.update_raw(pc1, _dev(fr["obj"]), _dev(fr["num"]), _dev(fr["ids"]), gobj, nv, _dev(fr["reset"]), _dev(fr["active"]),
                          object_conf=_dev(conf))


@pytest.fixture(scope="module")
def planned():
    """The planned sequence through two logging scorers; only the first is ever asked for the identity metrics."""
    seq, confs, logs, sw = W.planned()
    assert (seq["B"], seq["N"], seq["K"], len(seq["frames"])) == (16, 256, 32, 12)
    scorer, twin = _scorer(seq), _scorer(seq)
    _feed(seq, confs, (scorer, twin))
    return dict(seq=seq, logs=logs, sw=sw, scorer=scorer, twin=twin)


def test_identity_of_the_planned_sequence_equals_the_host_statement(planned):
    scorer, twin, logs = planned["scorer"], planned["twin"], planned["logs"]
    scorer.check()
    one = scorer.identity()
    _check(one, I.host_identity(logs))
    print("IDF1 %.6f IDR %.6f IDP %.6f; idtp %d of gt %d, pred %d" % (one.idf1[0], one.idr[0], one.idp[0], one.idtp[0], one.gt[0], one.pred[0]))
    assert one.alpha.tolist() == [0.5] and one.threshold is None and not one.flags.any() and one.counters.shape == (1, 16, 6)
    assert (one.gt[0], one.pred[0], one.idtp[0]) == (363, 617, 229) and one.idf1[0] == 458 / 980
    _same_result(one, scorer.identity(alphas=0.5))                             # a float is one level
    host = I.host_identity(logs, alphas=HOTA_LEVELS)
    idn = scorer.identity(alphas=HOTA_LEVELS)
    _check(idn, host)
    assert idn.alpha.tolist() == list(HOTA_LEVELS) and idn.idtp[0] == 262 and np.array_equal(idn.counters[9], one.counters[0])
    assert all(x >= y for x, y in zip(idn.idtp, idn.idtp[1:])) and len(set(idn.idtp.tolist())) > 8
    for b in range(len(logs)):                                                  # every stream on its own
        _check(idn, host, streams=[b])
    # gt and frames are the scorer's at every level
    for k in ("gt", "frames"):
        mine = scorer.counters[:, TS.COUNTERS.index(k)].cpu().numpy()
        assert all(np.array_equal(idn.counters[a, :, CI[k]], mine) for a in range(19)), k
    # the same numbers on a second call, and the state and the log it read are untouched
    _same_result(idn, scorer.identity(alphas=HOTA_LEVELS))
    for k in STATE + LOG:
        assert torch.equal(getattr(scorer, k), getattr(twin, k)), k


def test_identity_at_a_threshold_equals_the_filtered_host_statement(planned):
    scorer, logs, sw = planned["scorer"], planned["logs"], planned["sw"]
    best = scorer.sweep().best
    assert best["level"] == sw["best"] == 9 and best["threshold"] == 0.55234375
    levels = (0.5, 0.05, 0.8)
    idn = scorer.identity(alphas=levels, threshold=best["threshold"])
    _check(idn, I.host_identity(logs, sw["scores"], best["threshold"], alphas=levels))
    assert idn.threshold == best["threshold"] and (idn.gt[0], idn.pred[0], idn.idtp[0], idn.idtp[1]) == (363, 149, 54, 118)
    _same_result(idn, scorer.identity(alphas=levels, threshold=torch.tensor(best["threshold"], dtype=torch.float64, device=DEV)))      # 0-dim
    plain, low = scorer.identity(alphas=levels), scorer.identity(alphas=levels, threshold=float("-inf"))
    assert low.threshold == float("-inf")
    _same_result(plain, low)
    assert not np.array_equal(plain.counters, idn.counters)
    for k in STATE + LOG:
        assert torch.equal(getattr(scorer, k), getattr(planned["twin"], k)), k


# ---- 2: fabricated logs ----------------------------------------------------------------------------------------------------------------
_det = I._det


def _frame(labels, dets, reset=False):
    return dict(reset=bool(reset), labels=[int(v) for v in labels], dets=list(dets))


def _fabricated(logs, max_gt_tracks=1024, F=64, R=4096):
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


A_, B_ = 11, 12


def test_fabricated_logs_with_hand_numbers():
    third = 3.0 / 5.0
    logs = [
        # (a) greedy loses: track 1 on A for five frames, then track 2 on A and track 1 on B for four
        [_frame([A_, B_], [_det(1, A_, 0.9)], f == 0) for f in range(5)] + [_frame([A_, B_], [_det(2, A_, 0.9), _det(1, B_, 0.9)]) for _ in range(4)],
        # (b) two detections of one frame share a best label: both pairs are counted, idtp takes one of them
        [_frame([5, 6], [_det(1, 5, 0.7), _det(2, 5, 0.8)], f == 0) for f in range(3)],
        # (c) an IoU of exactly 3/5
        [_frame([5], [_det(1, 5, third)], True)],
        # (d) a best label that is not among the frame's labels (and one that is, in the next frame)
        [_frame([5], [_det(1, 9, 0.9)], True), _frame([5, 9], [_det(1, 9, 0.9)])],
        # (e) a reset in mid-log: track 1 serves A before and B after, both in full
        [_frame([A_, B_], [_det(1, A_, 0.9)], f == 0) for f in range(4)] + [_frame([A_, B_], [_det(1, B_, 0.9)], f == 0) for f in range(4)],
        [_frame([A_, B_], [_det(1, A_, 0.9)], f == 0) for f in range(4)] + [_frame([A_, B_], [_det(1, B_, 0.9)]) for f in range(4)],
        # (f) HOTA's (c) and (d): an id that changes after 5 of 10 frames; the re-acquisition under the same id and under a fresh one
        _one_label([1] * 5 + [2] * 5),
        _one_label([4] * 10, absent=(4, 5)),
        _one_label([4] * 6 + [9] * 4, absent=(4, 5)),
    ]
    levels = (0.5, 0.6, 0.65, 0.75)
    sc = _fabricated(logs)
    idn = sc.identity(alphas=levels)
    host = I.host_identity(logs, alphas=levels)
    _check(idn, host)
    c = idn.counters
    col = lambda a, b, *ks: tuple(int(c[a, b, CI[k]]) for k in ks)
    per = lambda b: TS.identity_values(c[:, b:b + 1], levels)
    # (a): n[A,1] = 5, n[A,2] = 4, n[B,1] = 4: the optimum is 4 + 4, heaviest-pair-first would stop at 5
    assert col(0, 0, "gt", "pred", "idtp", "pairs", "clips", "frames") == (18, 13, 8, 3, 1, 9)
    assert host["clips"][0][0] == (8, 5, 3) and per(0)["idf1"][0] == 16 / 31
    # (b): pairs (5,1) and (5,2) with 3 frames each; label 5 can take one track
    assert col(0, 1, "gt", "pred", "idtp", "pairs") == (6, 6, 3, 2)
    assert col(3, 1, "idtp", "pairs") == (3, 1)                                   # at 0.75 only the second detection is a candidate
    # (c): 3/5 >= 0.6 and not >= 0.65
    assert col(1, 2, "idtp", "pairs") == (1, 1) and col(2, 2, "idtp", "pairs") == (0, 0) and col(2, 2, "gt", "pred") == (1, 1)
    # (d): label 9 is kept in the second frame only
    assert col(0, 3, "gt", "pred", "idtp", "pairs") == (3, 2, 1, 1)
    # (e): two clips are assigned separately, 4 + 4; as one clip the track can serve one label only
    assert col(0, 4, "clips", "idtp", "pairs") == (2, 8, 2) and col(0, 5, "clips", "idtp", "pairs") == (1, 4, 2)
    # (f): one label under two ids of five frames each: idtp 5 of gt 10, pred 10
    v = per(6)
    assert (v["idtp"][0], v["gt"][0], v["pred"][0]) == (5, 10, 10) and v["idf1"][0] == 2 * 5 / 20 == I.values(host["counters"][:, 6:7])["idf1"][0]
    same, fresh = per(7), per(8)
    assert same["idtp"][0] == 8 and fresh["idtp"][0] == 4 and same["gt"][0] == fresh["gt"][0] == 8 and same["idf1"][0] == 1.0 and fresh["idf1"][0] == 0.5
    # IoU 0.9 is a candidate at every one of these levels
    assert all(col(3, b, "idtp") == col(0, b, "idtp") for b in (0, 4, 5, 6, 7, 8))
    assert not idn.flags.any()


# ---- 3: random clips ---------------------------------------------------------------------------------------------------------------
def test_random_clips_equal_the_host_statement():
    rng = np.random.default_rng(2024)
    logs = [[e for k in range(3) for e in I.random_clip(rng, *I.RANDOM_SHAPES[(b + k) % 3], ious=(0.3, 0.6, 0.9))] for b in range(8)]
    levels = (0.3, 0.5, 0.7)
    sc = _fabricated(logs, F=128, R=1024)
    host = I.host_identity(logs, alphas=levels)
    idn = sc.identity(alphas=levels)
    _check(idn, host)
    clips = host["clips"][0]
    short = sum(greedy < best for best, greedy, _ in clips)
    print("random clips: heaviest-pair-first below the optimum in %d of %d; idtp %s" % (short, len(clips), idn.idtp.tolist()))
    assert len(clips) == 24 and short >= 6 and idn.idtp[0] > idn.idtp[1] > idn.idtp[2] > 0
    assert (idn.counters[0, :, CI["clips"]] == 3).all()
    scores = [W.track_scores(lb)[0] for lb in logs]
    tau = float(np.median([s for sb in scores for f in sb for s in f]))
    filt = sc.identity(alphas=levels, threshold=tau)
    _check(filt, I.host_identity(logs, scores, tau, alphas=levels))
    assert 0 < filt.pred[0] < idn.pred[0] and 0 < filt.idtp[0] < idn.idtp[0]


# ---- 4: the dense clip -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sticky", [False, True])
def test_the_dense_clip_is_solved_at_the_limit(sticky):
    logs = [I.dense_clip(sticky=sticky)]
    host = I.host_identity(logs)
    (best, greedy, pairs), = host["clips"][0]
    assert greedy < best                                    # the case cannot pass by accident
    sc = _fabricated(logs, F=256, R=8192)
    idn = sc.identity()
    print("dense clip, sticky %s: %d pairs, idtp %d (heaviest-pair-first %d), IDF1 %.6f" % (sticky, idn.pairs[0], idn.idtp[0], greedy, idn.idf1[0]))
    _check(idn, host)
    assert not idn.flags.any() and idn.idtp[0] == best and idn.pairs[0] == pairs and idn.gt[0] == idn.pred[0] == 32 * 256
    assert pairs == 1024 if not sticky else 900 < pairs <= 1024


# ---- 5: overflow -------------------------------------------------------------------------------------------------------------------
def _frame_list_two():
    return [_frame([1, 2], [_det(10 + f % 2, 1, 0.5), _det(20, 2, 0.8), _det(30 + f)], f == 0) for f in range(6)]


def _overflow(bad, flagged=2, max_gt_tracks=1024):
    small = [_one_label([1] * 5 + [2] * 5), _frame_list_two(), [], _one_label([3] * 8, reset_at=(4,))]
    logs = small[:flagged] + [bad] + small[flagged + 1:]
    sc = _fabricated(logs, max_gt_tracks=max_gt_tracks)
    with pytest.raises(RuntimeError, match="TrackScorer.identity: stream %d has a clip with more than max_gt_tracks=%d label ids, %d track ids or %d"
                                           % (flagged, max_gt_tracks, TS.SWEEP_TRACKS, TS.IDENTITY_PAIRS)):
        sc.identity()
    idn = sc.identity(check=False)
    assert idn.flags.tolist() == [TS.FLAG_IDENTITY if b == flagged else 0 for b in range(4)], idn.flags
    assert int(sc.flags.sum()) == 0                         # the scorer's own sticky flags are not written
    others = [b for b in range(4) if b != flagged]
    small[flagged] = []
    _check(idn, I.host_identity(small), streams=others)
    return idn


def test_a_clip_with_too_many_pairs_flags_its_stream_alone():
    # 17 labels matched by fresh track ids on every one of 64 frames: 1088 pairs (and 1088 track ids, which fit)
    bad = [_frame(range(17), [_det(100 + 17 * f + g, g, 0.9) for g in range(17)], f == 0) for f in range(64)]
    assert 17 * 64 > TS.IDENTITY_PAIRS and 17 * 64 <= TS.SWEEP_TRACKS
    _overflow(bad)
    # one frame fewer than the limit needs: no flag, the host's numbers -- every label keeps one of its 60 tracks
    fits = [bad[:TS.IDENTITY_PAIRS // 17], [], [], []]
    idn = _fabricated(fits).identity()
    _check(idn, I.host_identity(fits))
    assert idn.pairs[0] == 17 * (TS.IDENTITY_PAIRS // 17) == 1020 and idn.idtp[0] == 17 and not idn.flags.any()


def test_a_clip_with_too_many_track_ids_or_labels_flags_its_stream_alone():
    # 33 unmatched detections with fresh track ids on every one of 64 frames: 2112 track ids, no pair at all
    bad = [_frame([1], [_det(1000 + 33 * f + i) for i in range(33)], f == 0) for f in range(64)]
    assert 33 * 64 > TS.SWEEP_TRACKS
    _overflow(bad, flagged=1)
    # more label ids in a clip than max_gt_tracks
    bad = [_frame([f], [_det(1, f, 0.9)], f == 0) for f in range(5)]
    _overflow(bad, flagged=0, max_gt_tracks=4)
    # exactly max_gt_tracks label ids fit
    fits = [bad[:4], [], [], []]
    idn = _fabricated(fits, max_gt_tracks=4).identity()
    _check(idn, I.host_identity(fits))
    assert idn.idtp[0] == 1 and idn.pairs[0] == 4 and not idn.flags.any()


# ---- 6: empty logs -----------------------------------------------------------------------------------------------------------------
def test_an_empty_log_and_a_stream_without_frames():
    sc = _fabricated([[], [], [], []])
    idn = sc.identity(alphas=(0.5, 0.9))
    assert not idn.counters.any() and not idn.flags.any() and idn.counters.shape == (2, 4, 6)
    assert all(np.isnan(getattr(idn, k)).all() for k in RATIOS) and idn.idtp.tolist() == [0, 0]
    _check(idn, I.host_identity([[], [], [], []], alphas=(0.5, 0.9)))
    assert np.isnan(sc.identity(threshold=0.5).idf1).all()
    logs = [_one_label([1] * 3), [], _one_label([2] * 4), []]
    idn = _fabricated(logs).identity()
    _check(idn, I.host_identity(logs))
    assert not idn.counters[:, 1].any() and not idn.counters[:, 3].any() and idn.idtp[0] == 7 and idn.counters[0, :, CI["clips"]].tolist() == [1, 0, 1, 0]
    assert idn.idf1[0] == 1.0


# ---- 7: behind the tracker ---------------------------------------------------------------------------------------------------------
SPEED = 1.2


def _affinity_net(c, s):
    """A Track4D whose Affinity is distance_affinity(c, s) (tests/test_track_motion_gpu.py)."""
    net = Track4D(Args()).to(DEV).eval()
    net.affinity.load_state_dict(MEM.distance_affinity(c, s).state_dict())
    net.invalidate_fused()
    return net


def _fast_centres(t):
    return MEM.lattice(3) + torch.tensor([SPEED * t, 0.0, 0.0])


def _fast_scenario(g):
    """Three objects moving 1.2 m per frame along x, their flow (1.2, 0, 0); object 0 is hidden in frames 2 .. 2 + g - 1."""
    out = []
    for t in range(2 + g + 2):
        visible = [not 2 <= t < 2 + g, True, True]
        out.append([MU.flow_stream(_fast_centres(t), visible, 32, [[SPEED, 0.0, 0.0]] * 3, points=3, seed=100 + t)])
    return out


def test_idf1_sees_how_much_of_a_life_the_gap_costs():
    """The constructed case of tests/test_track_hota_gpu.py::test_assa_sees_how_much_of_a_life_the_gap_costs: held still the returning
    object gets a fresh id, moved it keeps its own.  The hidden object's four matches fall under two ids of two each, or under one."""
    def scored(motion):
        trk = T.BatchedTracker(_affinity_net(8.0, 4.0), streams=1, max_objects=8, max_age=2, motion=motion)
        scorer = TS.TrackScorer(streams=1, max_objects=8, max_boxes=8, max_gt_tracks=16, sweep_frames=8, sweep_records=64)
        for t, frame in enumerate(_fast_scenario(2)):
            first = torch.tensor([t == 0], dtype=torch.uint8, device=DEV)
            pc1, f1, flow, cls, prop, nv = MEM.batch(frame, DEV)
            out = trk.associate(pc1, f1, flow, cls, prop, nv, first, torch.ones(1, dtype=torch.uint8, device=DEV))
            c = _fast_centres(t).tolist()
            labels = {k: vod_gt.Label("Car", k, 0, 0, 0, 0, 0, 0, 3.0, 4.0, 6.0, c[k][0], c[k][1], c[k][2], 0.0) for k in range(3)}
            per_stream = [(labels, U.IDENTITY_TF, labels, U.IDENTITY_TF)]
            nv1 = torch.tensor([frame[0]["n_valid"]], dtype=torch.int32, device=DEV)
            gobj = TS.gt_objects(out.pc1, G.pack_boxes(per_stream, 8, DEV), TS.pack_box_types(per_stream, 8, DEV), n_valid=nv1, min_obj_points=2)
            scorer.update(out, gobj, reset=first)
        trk.check()
        idn = scorer.identity()
        _check(idn, I.host_identity(H.entries_from_log(*(getattr(scorer, k).cpu().numpy() for k in LOG))))
        return idn, scorer.hota()

    (held, hh), (moving, mh) = scored(None), scored("flow")
    print("held still: IDF1 %.6f AssA %.6f; moved: IDF1 %.6f AssA %.6f" % (held.idf1[0], hh.assa_mean, moving.idf1[0], mh.assa_mean))
    assert (held.gt[0], held.pred[0], held.idtp[0], held.pairs[0]) == (18, 16, 14, 4)
    assert (moving.gt[0], moving.pred[0], moving.idtp[0], moving.pairs[0]) == (18, 16, 16, 3)
    assert held.idf1[0] == 28 / 34 and moving.idf1[0] == 32 / 34 and held.idf1[0] < moving.idf1[0]
    assert hh.assa_mean < mh.assa_mean
