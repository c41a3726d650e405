"""GPU: HOTA under the optimal matching (csrc/track_hota_optimal.hip `rtk_score_alignment`, `rtk_score_hota_optimal`,
`TrackScorer.hota(matching="optimal")`) and the identity metrics over every pair (csrc/track_identity_pairs.hip
`rtk_score_identity_pairs`, `TrackScorer.identity(pairs="all")`) against the host statement of tests/_track_hota_optimal_util.py.  The
device delivers integers and fixed-order float64 sums, so everything is compared with == / bit for bit, no case left out.  The logs are
written through `pack` (fabricated) or `update_raw` (the small sequence of tests/_track_optimal_util.py)."""
import math

import numpy as np
import pytest
import torch

import _track_hota_optimal_util as HO
import _track_hota_util as H
import _track_identity_util as I
import _track_optimal_util as O
import _track_score_util as S
import _track_sweep_util as W
from ratrack_amd import gt_device as G
from ratrack_amd import track_score as TS

pytestmark = pytest.mark.gpu
DEV = "cuda"
F, R, Q = 16, 512, 4096
LOG = ("log_cursor", "log_frame", "log_label", "log_track", "log_best", "log_conf", "log_iou")
PAIRS = ("pair_frame", "pair_key", "pair_common", "log_size", "log_label_size")
TP, LOC = HO.COUNTERS.index("tp"), HO.SUMS.index("loc")
LEVELS = (0.3, 0.5, 0.6, 0.7)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _fabricated(logs, max_gt_tracks=64):
    """A scorer whose log and pair-log tensors hold `logs`, written as rtk_track_score_pairs packs them."""
    sc = TS.TrackScorer(streams=len(logs), max_objects=8, max_boxes=8, max_gt_tracks=max_gt_tracks, sweep_frames=F, sweep_records=R, sweep_pairs=Q)
    for k, a in O.pack(logs, F, R, Q).items():
        getattr(sc, k).copy_(_dev(a))
    return sc


def _scores(logs, threshold):
    return (None, -math.inf) if threshold is None else ([W.track_scores(lb)[0] for lb in logs], threshold)


def _check_hota(sc, logs, A=19, threshold=None, streams=None, check=True):
    """hota(matching="optimal") against the host statement: the 6 counters ==, the 4 sums bit for bit, per stream and level."""
    res = sc.hota(alphas=A, threshold=threshold, matching="optimal", check=check)
    scores, tau = _scores(logs, threshold)
    host = HO.host_hota_optimal(logs, scores, tau, A)
    pick = list(range(len(logs))) if streams is None else streams
    assert res.matching == "optimal" and res.counters.shape == host["counters"].shape and res.threshold == threshold
    assert np.array_equal(res.counters[:, pick], host["counters"][:, pick]), (res.counters[:, pick], host["counters"][:, pick])
    assert np.array_equal(_bits(res.sums)[:, pick], _bits(host["sums"])[:, pick]), (res.sums[:, pick], host["sums"][:, pick])
    if streams is None:          # the ratios are hota_values of what was just compared
        want = TS.hota_values(host["counters"], host["sums"])
        assert all(np.array_equal(_bits(getattr(res, k)), _bits(want[k])) for k in ("hota_alpha", "deta", "assa", "loca", "hota", "assa_mean"))
    return res, host


def _check_identity(sc, logs, alphas=LEVELS, threshold=None):
    res = sc.identity(alphas=alphas, threshold=threshold, pairs="all")
    scores, tau = _scores(logs, threshold)
    host = HO.host_identity_all(logs, scores, tau, alphas)
    assert res.pair_mode == "all" and np.array_equal(res.counters, host["counters"]), (res.counters, host["counters"])
    assert res.idtp.tolist() == host["idtp"] and np.array_equal(_bits(res.idf1), _bits(host["idf1"]))
    return res, host


# ---- 1: the constructed cases ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def constructed():
    cases = HO.constructed_logs()
    logs = list(cases.values())
    return dict(names=list(cases), logs=logs, scorer=_fabricated(logs))


def test_constructed_cases_equal_the_host_statement(constructed):
    sc, logs, at = constructed["scorer"], constructed["logs"], constructed["names"].index
    res, host = _check_hota(sc, logs)
    assert not res.flags.any()
    # the alignment case: track 1 keeps object 5 in frame 2; its IoU 3/5 counts at alpha = 12/20 and not at 13/20, where the frame
    # has no true positive at all -- the greedy rule finds one there, through the intruder
    b = at("alignment")
    assert host["trace"][b][2]["cp"] == [0] and res.counters[11, b, TP] == 4 and res.counters[12, b, TP] == 0
    greedy = sc.hota()
    assert greedy.matching == "greedy" and greedy.counters[12, b, TP] == 1
    one = lambda r: TS.hota_values(r.counters[:, b:b + 1], r.sums[:, b:b + 1])["hota"]
    assert one(res) != one(greedy)
    # a reset in the middle: the one-frame clip after it takes the intruder (A does not leak across clips)
    assert host["trace"][at("leak")][4]["cp"] == [1] and res.counters[12, at("leak"), TP] == 1
    # the clamp: the pair with IoU 3 is a true positive at every level and adds 3 to loc; the tie: object 0 (IoU 1), not object 1 (IoU 3)
    assert res.counters[18, at("clamp"), TP] == 2 and res.sums[18, at("clamp"), LOC] == 6.0
    assert host["trace"][at("tie")][0]["cp"] == [0, -1] and res.sums[0, at("tie"), LOC] == 1.0
    assert res.counters[0, at("empty_sides")].tolist() == [3, 1, 3, 3, 1, 1] and not res.counters[:, at("empty")].any()
    # one level only
    _check_hota(sc, logs, A=1)
    # a threshold that removes track 10 of the threshold case: another pair's A changes with it
    b = at("threshold")
    thr, _ = _check_hota(sc, logs, threshold=0.5)
    assert thr.counters[0, b, HO.COUNTERS.index("pred")] == 3 and res.counters[0, b, HO.COUNTERS.index("pred")] == 5
    assert not np.array_equal(_bits(thr.sums[:, b]), _bits(res.sums[:, b]))
    # the same bits on a second call, and nothing of the scorer is written
    again = sc.hota(matching="optimal")
    assert np.array_equal(again.counters, res.counters) and np.array_equal(_bits(again.sums), _bits(res.sums)) and int(sc.flags.sum()) == 0


def test_identity_over_every_pair_on_the_constructed_cases(constructed):
    sc, logs, at = constructed["scorer"], constructed["logs"], constructed["names"].index
    res, _ = _check_identity(sc, logs)
    best = sc.identity(alphas=LEVELS)
    b, idtp = at("identity"), I.COUNTERS.index("idtp")
    assert best.pair_mode == "best" and res.counters[1, b, idtp] == 3 and best.counters[1, b, idtp] == 2
    assert res.counters[2, b, idtp] == 3 and res.counters[3, b, idtp] == 0          # 3/5 counts at 0.6, nothing at 0.7
    _check_identity(sc, logs, alphas=(0.5,), threshold=0.5)
    assert not res.flags.any() and int(sc.flags.sum()) == 0


def test_the_defaults_are_the_calls_they_were(constructed):
    sc, logs = constructed["scorer"], constructed["logs"]
    for threshold in (None, 0.5):
        scores, tau = _scores(logs, threshold)
        ho, host = sc.hota(threshold=threshold), H.host_hota(logs, scores, tau)
        assert np.array_equal(ho.counters, host["counters"]) and np.array_equal(_bits(ho.sums), _bits(host["sums"])) and ho.hota == host["hota"]
        idn, ihost = sc.identity(alphas=LEVELS, threshold=threshold), I.host_identity(logs, scores, tau, LEVELS)
        assert np.array_equal(idn.counters, ihost["counters"]) and idn.idtp.tolist() == ihost["idtp"]


# ---- 2: random logs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,streams", [(1, 4), (2, 2), (3, 3)])
def test_random_logs_equal_the_host_statement(seed, streams):
    logs = O.random_logs(seed, streams=streams, frames=12, max_dets=12, max_objs=8)
    sc = _fabricated(logs)
    pool = sorted(s for lb in logs for f in W.track_scores(lb)[0] for s in f)
    res, host = _check_hota(sc, logs)
    assert res.counters[0, :, TP].sum() > res.counters[14, :, TP].sum() > 0 and not res.flags.any()
    assert sum(len(t) for t in host["trace"]) == 12 * streams
    _check_hota(sc, logs, A=1)
    _check_hota(sc, logs, threshold=pool[len(pool) // 2])
    _check_identity(sc, logs)
    _check_identity(sc, logs, alphas=(0.5,), threshold=pool[len(pool) // 2])


# ---- 3: the overflows ---------------------------------------------------------------------------------------------------------------------
def _one(tid, reset=False):
    return O.frame_from_ious([7], [(tid, 0.5)], {(0, 0): 16}, reset)


def test_a_frame_with_too_many_valid_pairs_flags_its_stream_alone():
    bad = HO.edge_overflow_frame()
    assert len(bad["pairs"]) == TS.PAIR_EDGES + 1 and len({(j, d[0]) for j in range(32) for d in bad["dets"]}) <= TS.ALIGN_PAIRS
    logs = [HO.alignment_case(), [bad], [_one(1, True), _one(2)]]
    sc = _fabricated(logs)
    with pytest.raises(RuntimeError, match="stream 1 has a frame with more than %d candidate" % TS.PAIR_EDGES):
        sc.hota(matching="optimal")
    res, _ = _check_hota(sc, logs, streams=[0, 2], check=False)
    assert res.flags.tolist() == [0, TS.FLAG_OPTIMAL, 0] and int(sc.flags.sum()) == 0
    # one pair fewer fits exactly
    fits = [[dict(bad, pairs=bad["pairs"][:-1])]]
    assert not _check_hota(_fabricated(fits), fits)[0].flags.any()


def test_a_clip_with_too_many_potential_pairs_flags_its_stream_alone():
    bad = HO.pair_overflow_frame()
    assert TS.ALIGN_PAIRS < len(bad["pairs"]) <= TS.PAIR_EDGES
    logs = [[_one(1, True), _one(2)], [bad], HO.alignment_case()]
    sc = _fabricated(logs)
    with pytest.raises(RuntimeError, match="TrackScorer.hota: stream 1 has a clip with more than"):
        sc.hota(matching="optimal")
    res, _ = _check_hota(sc, logs, streams=[0, 2], check=False)
    assert res.flags.tolist() == [0, TS.FLAG_HOTA, 0] and int(sc.flags.sum()) == 0
    # 64 x 16 = 1024 potential pairs fit exactly
    fits = [[O.make_frame(range(16), [40] * 16, [(100 + i, 0.5, 40) for i in range(64)], [(i, j, 20) for i in range(64) for j in range(16)], True)]]
    assert not _check_hota(_fabricated(fits), fits)[0].flags.any()


# ---- 4: a log written by the scoring launch ---------------------------------------------------------------------------------------------
def test_a_log_written_by_update_raw_with_an_inactive_stream():
    seq = O.small_sequence()
    for fr in seq["frames"]:
        fr["active"][1] = 0                       # stream 1 never logs; stream 2 also skips frame 4
    sc = TS.TrackScorer(streams=3, max_objects=8, max_boxes=5, max_gt_tracks=16, sweep_frames=16, sweep_records=128, sweep_pairs=256)
    K = seq["K"]
    for fr in seq["frames"]:
        pc1, nv = _dev(fr["pc1"]), _dev(fr["n_valid"])
        gobj = TS.gt_objects(pc1, G.pack_boxes(fr["per_stream"], K, DEV), TS.pack_box_types(fr["per_stream"], K, DEV), n_valid=nv,
                             min_obj_points=S.MIN_PTS)
        sc.update_raw(pc1, _dev(fr["obj"]), _dev(fr["num"]), _dev(fr["ids"]), gobj, nv, _dev(fr["reset"]), _dev(fr["active"]),
                      object_conf=_dev(fr["conf"]))
    sc.check()
    logs = O.entries_from_logs(*(getattr(sc, k).cpu().numpy() for k in LOG + PAIRS))
    assert [len(lb) for lb in logs] == [12, 0, 11] and sum(len(e["pairs"]) for lb in logs for e in lb) > 60
    res, _ = _check_hota(sc, logs)
    assert res.counters[0, :, TP].tolist()[1] == 0 and res.counters[0, 0, TP] > 0
    _check_hota(sc, logs, threshold=0.5)
    _check_identity(sc, logs)


# ---- 5: the error paths ---------------------------------------------------------------------------------------------------------------------
def test_error_paths(constructed):
    sc = constructed["scorer"]
    plain = TS.TrackScorer(streams=2, max_objects=8, max_boxes=8, sweep_frames=4, sweep_records=32)
    with pytest.raises(RuntimeError, match="TrackScorer.hota: the optimal matching needs the pair log \\(give sweep_pairs\\)"):
        plain.hota(matching="optimal")
    with pytest.raises(RuntimeError, match="TrackScorer.identity: the optimal matching needs the pair log \\(give sweep_pairs\\)"):
        plain.identity(pairs="all")
    with pytest.raises(ValueError, match="matching='best'"):
        sc.hota(matching="best")
    with pytest.raises(ValueError, match="pairs='optimal'"):
        sc.identity(pairs="optimal")
