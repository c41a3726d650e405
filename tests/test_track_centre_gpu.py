"""GPU: TrackEval's centre-distance similarity on the pair log (csrc/track_score.hip `rtk_track_score_pairs_centre`,
the replays' `_sim` entry points, `TrackScorer(similarity="centre")`) against the host statement of tests/_track_centre_util.py.  The producer's
integers, decisions and -- bit for bit -- similarities; everything but the pair log equal to the "iou" scorer's; the four replays on
constructed and on produced logs against the existing host statements with their two similarity functions substituted.  The ground-truth
objects are built by hand where that is simpler (`GtObjects` is a plain holder of tensors)."""
import math

import numpy as np
import pytest
import torch

import _track_centre_util as C
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
STATE = ("counters", "iou_sum", "table_key", "table_last", "table_seen", "table_matched", "table_used", "prev_gt_id", "prev_count", "prev_gt",
         "flags")
LOG = ("log_cursor", "log_frame", "log_label", "log_track", "log_best", "log_conf", "log_iou")
SIZES = ("log_size", "log_label_size")
PAIRS = ("pair_cursor", "pair_frame", "pair_key", "pair_common", "pair_sim")
OUT = ("pred_gt_slot", "pred_gt_id", "gt_pred", "iou", "aff_target", "aff_defined")
LEVELS = (0.25, 0.5, 0.6, 0.75)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _equal_tensors(a, b, names):
    for k in names:
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8) if x.dtype.is_floating_point else x,
                                                   y.view(torch.uint8) if y.dtype.is_floating_point else y), k


def _gobj(fr, K, N):
    return TS.GtObjects(slot=_dev(fr["slot"]), label_id=_dev(fr["label_id"]), count=_dev(fr["count"]), size=_dev(fr["size"]),
                        members=_dev(fr["members"].view(np.int32)), centre=_dev(fr["centre"]), flags=torch.zeros(len(fr["count"]), dtype=torch.int32,
                                                                                                                device=DEV),
                        n_valid=_dev(fr["n_valid"]), max_boxes=K, points=N)


def _feed(frames, scorers, K, N, tables=None):
    """Every frame through every scorer; the MatchResults of one frame are equal bit for bit."""
    for f, fr in enumerate(frames):
        gobj = _gobj(fr, K, N)
        kw = {} if tables is None else dict(table_ids=_dev(tables[f][0]), table_count=_dev(tables[f][1]))
        outs = [sc.update_raw(_dev(fr["pc1"]), _dev(fr["obj"]), _dev(fr["num"]), _dev(fr["ids"]), gobj, _dev(fr["n_valid"]), _dev(fr["reset"]),
                              _dev(fr["active"]), object_conf=_dev(fr["conf"]), **kw) for sc in scorers]
        for o in outs[1:]:
            _equal_tensors(outs[0], o, OUT)


def _holds_pair_log(sc, host):
    """The scorer's pair log is the host statement's: the integers ==, pair_sim bit for bit."""
    for k in PAIRS:
        dev = getattr(sc, k).cpu().numpy()
        assert dev.shape == host[k].shape and np.array_equal(dev.view(np.uint8), host[k].view(np.uint8)), (k, np.argwhere(dev != host[k])[:6])


# ---- 1, 3: the producer on hand-built frames; everything else is rtk_track_score_pairs ----------------------------------------------------
F1, R1, Q1 = 8, 256, 1024


@pytest.mark.parametrize("N,seed", [(96, 7), (320, 8)])
def test_the_pair_log_is_the_host_statements_and_everything_else_is_the_iou_scorers(N, seed):
    B, Kobj, K = 4, 16, 8
    frames = C.scenario(seed, B=B, N=N, Kobj=Kobj, K=K)
    mk = lambda **kw: TS.TrackScorer(streams=B, max_objects=Kobj, max_boxes=K, max_gt_tracks=32, sweep_frames=F1, sweep_records=R1, sweep_pairs=Q1, **kw)
    iou, centre, again = mk(), mk(similarity="centre"), mk(similarity="centre", zero_distance=2.0)
    _feed(frames, (iou, centre, again), K, N)
    centre.check()
    host = C.host_pair_log(frames, B, F1, R1, Q1)
    _holds_pair_log(centre, host)
    # what the cases are there for: pairs without a common point and with one; a detection without a live column; P = 0, G = 0, an inactive
    # stream (one frame fewer), a reset in the middle
    commons = [c for b in range(B) for ps, _ in host["entries"][b] for _, _, c in ps]
    assert min(commons) == 0 < max(commons) and int(host["pair_cursor"].sum()) > 50
    assert host["frames"].tolist() == [3, 3, 2, 3] and centre.log_cursor[:, 0].cpu().tolist() == [3, 3, 2, 3]
    assert all(i != 1 for ps, _ in host["entries"][2] for i, _, _ in ps)
    assert host["pair_frame"][0, 1, 1] == 0 and host["pair_frame"][1, 1, 1] == 0
    assert (centre.log_frame[3, 1, 2].item() >> 16) & 1 == 1
    # everything but the pair log: counters, iou_sum, the track table, the main log, the sizes, flags -- the "iou" scorer's bits
    _equal_tensors(centre, iou, STATE + LOG + SIZES)
    assert not torch.equal(centre.pair_key, iou.pair_key) and int(centre.flags.sum()) == 0
    # the same bits on a second run
    _equal_tensors(centre, again, STATE + LOG + SIZES + PAIRS)


# ---- 2: the boundaries ------------------------------------------------------------------------------------------------------------------
def _boundary_frame():
    """One stream, zero_distance 2.  Detection 0: columns 0, 1 at (0,0,0), (2,0,0): centre (1,0,0).  Detection 1: column 2 at (1,2,0).
    Objects: 0 at the centre (s = 1); 1 at (1,1,0), distance 1 from both detections (s = 0.5); 2 at (1,0,2), distance 2 from detection 0
    (s = 0: not logged); 3 at (1.5,0,0) without a common point (s = 0.75 with detection 0: logged, common 0); 4 a long object that owns
    detection 0's columns, its position (9,0,0) far away (common 2: not logged)."""
    N, K, Kobj = 64, 8, 4
    pc1 = np.zeros((1, 3, N), np.float32)
    pc1[0, :, 3:] = (np.arange(3 * (N - 3), dtype=np.float32).reshape(3, -1) + 40.0)
    pc1[0, :, 0], pc1[0, :, 1], pc1[0, :, 2] = (0, 0, 0), (2, 0, 0), (1, 2, 0)
    obj = np.full((1, N), -1, np.int32)
    obj[0, :2], obj[0, 2] = 0, 1
    members = np.zeros((1, K, 2), np.uint32)
    for j, cols in enumerate(([0, 1], [2, 10], [11, 12], [13, 14], [0, 1, 20, 21, 22, 23])):
        for p in cols:
            members[0, j, p >> 5] |= np.uint32(1 << (p & 31))
    centre = np.zeros((1, K, 3), np.float64)
    centre[0, :5] = [(1, 0, 0), (1, 1, 0), (1, 0, 2), (1.5, 0, 0), (9, 0, 0)]
    fr = dict(pc1=pc1, obj=obj, num=np.array([2], np.int32), ids=np.array([[7, 8, -1, -1]], np.int32), conf=np.full((1, Kobj), 0.5, np.float32),
              n_valid=np.array([N], np.int32), count=np.array([5], np.int32), members=members, centre=centre,
              slot=np.array([[0, 1, 2, 3, 4, -1, -1, -1]], np.int32), label_id=np.array([[10, 11, 12, 13, 14, -1, -1, -1]], np.int32),
              size=np.array([[2, 2, 2, 2, 6, 0, 0, 0]], np.int32), active=np.ones(1, np.uint8), reset=np.ones(1, np.uint8))
    return fr, N, K, Kobj


def test_the_boundaries_of_the_similarity_and_of_the_levels(monkeypatch):
    fr, N, K, Kobj = _boundary_frame()
    sc = TS.TrackScorer(streams=1, max_objects=Kobj, max_boxes=K, max_gt_tracks=16, sweep_frames=4, sweep_records=32, sweep_pairs=32,
                        similarity="centre")
    _feed([fr], (sc,), K, N)
    sc.check()
    n = int(sc.pair_cursor[0])
    got = [(int(k) >> 8, int(k) & 255, int(c), float(s)) for k, c, s in zip(sc.pair_key[0, :n].cpu(), sc.pair_common[0, :n].cpu(), sc.pair_sim[0, :n].cpu())]
    # d = 0: s = 1; d = 1: s = 0.5; a pair without a common point is logged; d = 2 (objects 2 and, for detection 1, 0) is not, and
    # neither is the long object 4, common points or not
    assert got == [(0, 0, 2, 1.0), (0, 1, 0, 0.5), (0, 3, 0, 0.75), (1, 1, 1, 0.5)]
    _holds_pair_log(sc, C.host_pair_log([fr], 1, 4, 32, 32))
    # s = 0.5 stays at min_iou = 0.5 (detection 0 takes object 0, detection 1 object 1) and at alpha = 0.5; just above, it does not
    at, above = sc.clear_optimal(0.5), sc.clear_optimal(math.nextafter(0.5, 1.0))
    assert at["overall"]["tp"] == 2 and at["overall"]["iou_sum"] == 1.5 and above["overall"]["tp"] == 1 and at["similarity"] == "centre"
    idn = sc.identity(alphas=(0.5, math.nextafter(0.5, 1.0), 0.75, 1.0), pairs="all")
    assert idn.counters[:, 0, I.COUNTERS.index("pairs")].tolist() == [4, 2, 2, 1] and idn.zero_distance == 2.0
    ho = sc.hota(alphas=19, matching="optimal")
    assert ho.counters[9, 0, HO.COUNTERS.index("tp")] == 2 and ho.counters[10, 0, HO.COUNTERS.index("tp")] == 1          # alpha = 10/20, 11/20
    assert TS.similarity_distance(at["overall"]["motp"], sc.zero_distance) == 0.5                                        # metres


# ---- 4: track memory ----------------------------------------------------------------------------------------------------------------------
def test_the_centre_log_behind_a_tracker_with_track_memory():
    B, N, Kobj, K = 4, 96, 16, 8
    frames = C.scenario(11, B=B, N=N, Kobj=Kobj, K=K, frames=4)
    rng = np.random.default_rng(11)
    tables = []
    for fr in frames:                      # the tracker's new table: this frame's detections, then up to 3 coasted rows
        ids, count = fr["ids"].copy(), fr["num"].copy()
        for b in range(B):
            extra = int(rng.integers(0, 4))
            ids[b, count[b]:count[b] + extra] = 100 + rng.choice(16, extra, replace=False)          # ids earlier frames used
            count[b] += extra
        tables.append((ids, count))
    mk = lambda **kw: TS.TrackScorer(streams=B, max_objects=Kobj, max_boxes=K, max_gt_tracks=32, sweep_frames=F1, sweep_records=R1, sweep_pairs=Q1,
                                     track_memory=True, **kw)
    iou, centre, again = mk(), mk(similarity="centre"), mk(similarity="centre")
    _feed(frames, (iou, centre, again), K, N, tables)
    centre.check()
    _holds_pair_log(centre, C.host_pair_log(frames, B, F1, R1, Q1))
    _equal_tensors(centre, iou, STATE + LOG + SIZES + ("row_track", "labelled_coasted"))
    _equal_tensors(centre, again, STATE + LOG + SIZES + PAIRS + ("row_track", "labelled_coasted"))
    assert int(centre.pair_cursor.sum()) > 60 and (centre.prev_count.cpu().numpy() == tables[-1][1]).all()


# ---- 5: the overflows ---------------------------------------------------------------------------------------------------------------------
def test_a_frame_whose_pairs_do_not_fit_is_in_neither_log():
    B, N, Kobj, K = 4, 96, 16, 8
    frames = C.scenario(7, B=B, N=N, Kobj=Kobj, K=K)
    full = C.host_pair_log(frames, B, F1, R1, Q1)
    Q = int(full["pair_frame"][3, 0, 1]) + 1          # stream 3's first frame fits, with one pair to spare
    host = C.host_pair_log(frames, B, F1, R1, Q)
    assert host["dropped"].any()
    sc = TS.TrackScorer(streams=B, max_objects=Kobj, max_boxes=K, max_gt_tracks=32, sweep_frames=F1, sweep_records=R1, sweep_pairs=Q, similarity="centre")
    _feed(frames, (sc,), K, N)
    _holds_pair_log(sc, host)
    assert sc.log_cursor[:, 0].cpu().tolist() == host["frames"].tolist() and host["frames"].sum() < full["frames"].sum()
    assert sc.flags.cpu().tolist() == [TS.FLAG_LOG if d else 0 for d in host["dropped"]]
    with pytest.raises(RuntimeError, match="or its pair log of sweep_pairs=%d pairs" % Q):
        sc.check()
    # the score itself saw every frame
    plain = TS.TrackScorer(streams=B, max_objects=Kobj, max_boxes=K, max_gt_tracks=32, sweep_frames=F1, sweep_records=R1, sweep_pairs=Q1)
    _feed(frames, (plain,), K, N)
    _equal_tensors(sc, plain, [k for k in STATE if k != "flags"])


def test_a_frame_with_too_many_valid_pairs_flags_its_stream_alone():
    B, N, Kobj, K = 2, 128, 64, 40
    pc1 = (np.arange(B * 3 * N, dtype=np.float32).reshape(B, 3, N) % 17) / np.float32(64.0)          # everything within a quarter metre
    obj = np.full((B, N), -1, np.int32)
    obj[0, :] = np.arange(N) % 64                     # stream 0: 64 detections of two columns each
    obj[1, :4] = [0, 0, 1, 1]                         # stream 1: two detections
    W = (N + 31) // 32
    members = np.zeros((B, K, W), np.uint32)
    for j in range(K):
        members[:, j, j >> 5] |= np.uint32(1 << (j & 31))
        members[:, j, (j + 64) >> 5] |= np.uint32(1 << ((j + 64) & 31))
    fr = dict(pc1=pc1, obj=obj, num=np.array([64, 2], np.int32), ids=np.tile(np.arange(64, dtype=np.int32) % 16 + 100, (B, 1)),          # 16 track ids x 40 labels: the clip's pairs fit the alignment pass
              conf=np.full((B, Kobj), 0.5, np.float32), n_valid=np.array([N, N], np.int32), count=np.array([K, 3], np.int32), members=members,
              centre=np.full((B, K, 3), 0.125, np.float64), slot=np.tile(np.arange(K, dtype=np.int32), (B, 1)),
              label_id=np.tile(np.arange(K, dtype=np.int32) + 10, (B, 1)), size=np.full((B, K), 2, np.int32), active=np.ones(B, np.uint8),
              reset=np.ones(B, np.uint8))
    sc = TS.TrackScorer(streams=B, max_objects=Kobj, max_boxes=K, max_gt_tracks=64, sweep_frames=2, sweep_records=128, sweep_pairs=4096,
                        similarity="centre")
    _feed([fr], (sc,), K, N)
    sc.check()
    assert sc.pair_cursor.cpu().tolist() == [64 * K, 2 * 3] and 64 * K > TS.PAIR_EDGES
    _holds_pair_log(sc, C.host_pair_log([fr], B, 2, 128, 4096))
    with pytest.raises(RuntimeError, match="stream 0 has a frame with more than %d candidate" % TS.PAIR_EDGES):
        sc.clear_optimal(0.25)
    assert sc.clear_optimal(0.25, check=False)["flags"].tolist() == [TS.FLAG_OPTIMAL, 0]
    ho = sc.hota(matching="optimal", check=False)
    assert ho.flags.tolist() == [TS.FLAG_OPTIMAL, 0] and ho.counters[0, 1, HO.COUNTERS.index("tp")] == 2
    assert int(sc.flags.sum()) == 0


# ---- 6: the replays on constructed logs -----------------------------------------------------------------------------------------------------
FQ, RQ, QQ = 16, 512, 4096


def _fabricated(logs, max_gt_tracks=64):
    """A centre scorer whose log and pair-log tensors hold `logs`, written as rtk_track_score_pairs_centre packs them."""
    sc = TS.TrackScorer(streams=len(logs), max_objects=8, max_boxes=8, max_gt_tracks=max_gt_tracks, sweep_frames=FQ, sweep_records=RQ, sweep_pairs=QQ,
                        similarity="centre")
    for k, a in C.pack(logs, FQ, RQ, QQ).items():
        getattr(sc, k).copy_(_dev(a))
    return sc


def _check_replays(sc, logs, threshold=None, min_iou=0.5, sweep=True):
    """The four calls against the (substituted) host statements: integers ==, the ordered float64 sums bit for bit, as the GPU tests of
    the plain kernels compare them."""
    scores = [W.track_scores(lb)[0] for lb in logs]
    plain = [[[0.0] * len(e["dets"]) for e in lb] for lb in logs]
    tau = -math.inf if threshold is None else threshold
    # clear_optimal
    res = sc.clear_optimal(min_iou, threshold=threshold)
    cn, iq, qs = O.host_replays(logs, plain if threshold is None else scores, [tau], min_iou)
    assert np.array_equal(np.stack([res["per_stream"][k] for k in O.COUNTERS], axis=1), cn[0])
    assert np.array_equal(res["per_stream"]["iou_q"], iq[0]) and np.array_equal(_bits(res["per_stream"]["iou_sum"]), _bits(qs[0]))
    # hota(matching="optimal")
    ho = sc.hota(alphas=19, threshold=threshold, matching="optimal")
    host = HO.host_hota_optimal(logs, None if threshold is None else scores, tau, 19)
    assert np.array_equal(ho.counters, host["counters"]) and np.array_equal(_bits(ho.sums), _bits(host["sums"]))
    assert (ho.similarity, ho.zero_distance, ho.matching) == ("centre", sc.zero_distance, "optimal")
    # identity(pairs="all")
    idn = sc.identity(alphas=LEVELS, threshold=threshold, pairs="all")
    ihost = HO.host_identity_all(logs, None if threshold is None else scores, tau, LEVELS)
    assert np.array_equal(idn.counters, ihost["counters"]) and idn.idtp.tolist() == ihost["idtp"] and idn.similarity == "centre"
    # sweep(matching="optimal")
    if sweep:
        sw, hs = sc.sweep(matching="optimal", min_iou=min_iou), O.host_sweep(logs, min_iou)
        assert sw.reached == hs["reached"] and np.array_equal(_bits(sw.thresholds), _bits(hs["thresholds"]))
        want = TS.optimal_sweep_values(hs["counters"], hs["iou_q"], hs["iou_sums"], hs["thresholds"], hs["reached"], 40)
        assert np.array_equal(sw.counters, want["counters"]) and np.array_equal(sw.iou_q_streams, want["iou_q_streams"])
        for k in ("iou_sums", "mota", "motp"):
            assert np.array_equal(_bits(getattr(sw, k)), _bits(want[k])), k
        assert (sw.similarity, sw.zero_distance, sw.min_iou) == ("centre", sc.zero_distance, min_iou)
    return res, ho, idn


@pytest.mark.parametrize("seed,streams", [(1, 4), (2, 3)])
def test_the_replays_on_constructed_similarity_logs_equal_the_host_statements(seed, streams, monkeypatch):
    logs = C.with_sims(O.random_logs(seed, streams=streams, frames=12, max_dets=12, max_objs=8), seed)
    sims = [s for lb in logs for e in lb for s in e["sims"]]
    assert len(sims) - len(set(sims)) > 50 and sims.count(0.5) > 3 and sims.count(0.25) > 3          # ties, and pairs exactly at the levels
    assert sum(1 for lb in logs for e in lb if e["reset"]) > streams                                  # clips that close at a reset
    sc = _fabricated(logs)
    C.patch_similarity(monkeypatch)
    res, ho, idn = _check_replays(sc, logs)
    assert res["overall"]["tp"] > 0 and ho.counters[0, :, HO.COUNTERS.index("tp")].sum() > ho.counters[14, :, HO.COUNTERS.index("tp")].sum() > 0
    _check_replays(sc, logs, min_iou=0.25, sweep=False)
    pool = sorted(s for lb in logs for f in W.track_scores(lb)[0] for s in f)
    _check_replays(sc, logs, threshold=pool[len(pool) // 2], sweep=False)                              # removed detections
    # the common counts (every third is 0) and the sizes are not read: other integers, the same numbers
    sc.pair_common.fill_(-7)
    sc.log_size.zero_()
    again = sc.hota(matching="optimal")
    assert np.array_equal(again.counters, ho.counters) and np.array_equal(_bits(again.sums), _bits(ho.sums)) and int(sc.flags.sum()) == 0
    assert np.array_equal(sc.identity(alphas=LEVELS, pairs="all").counters, idn.counters)
    assert all(sc.clear_optimal(0.5)["overall"][k] == res["overall"][k] for k in O.COUNTERS + ("iou_q", "iou_sum"))


def test_a_similarity_that_is_not_positive_makes_no_pair(monkeypatch):
    logs = C.with_sims(O.random_logs(3, streams=2, frames=8, max_dets=8, max_objs=6), 3)
    for lb in logs:
        for e in lb:
            e["sims"] = [(0.0, -0.25, float("nan"))[k % 7] if k % 7 < 3 else s for k, s in enumerate(e["sims"])]
    sc = _fabricated(logs)
    C.patch_similarity(monkeypatch)
    _check_replays(sc, logs, min_iou=0.25, sweep=False)


# ---- 7: end to end ----------------------------------------------------------------------------------------------------------------------------
def test_a_short_sequence_through_both_scorers_and_the_four_calls(monkeypatch):
    seq = O.small_sequence()
    K = seq["K"]
    mk = lambda **kw: TS.TrackScorer(streams=3, max_objects=8, max_boxes=5, max_gt_tracks=16, sweep_frames=16, sweep_records=128, sweep_pairs=512, **kw)
    iou, centre = mk(), mk(similarity="centre", zero_distance=1.0)
    for fr in seq["frames"]:
        pc1, nv = _dev(fr["pc1"]), _dev(fr["n_valid"])
        gobj = TS.gt_objects(pc1, G.pack_boxes(fr["per_stream"], K, DEV), TS.pack_box_types(fr["per_stream"], K, DEV), n_valid=nv,
                             min_obj_points=S.MIN_PTS)
        a, b = (sc.update_raw(pc1, _dev(fr["obj"]), _dev(fr["num"]), _dev(fr["ids"]), gobj, nv, _dev(fr["reset"]), _dev(fr["active"]),
                              object_conf=_dev(fr["conf"])) for sc in (iou, centre))
        _equal_tensors(a, b, OUT)
    iou.check()
    centre.check()
    _equal_tensors(centre, iou, STATE + LOG + SIZES)
    names = LOG + ("pair_frame", "pair_key", "pair_common") + SIZES
    # the "iou" scorer: the existing host statements, on its own downloaded log and on the host's log of the sequence
    ilogs = O.entries_from_logs(*(getattr(iou, k).cpu().numpy() for k in names))
    assert [[e["pairs"] for e in lb] for lb in ilogs] == [[e["pairs"] for e in lb] for lb in O.small_sequence_log(seq)]
    plain = [[[0.0] * len(e["dets"]) for e in lb] for lb in ilogs]
    res = iou.clear_optimal(0.25)
    cn, iq, qs = O.host_replays(ilogs, plain, [-math.inf], 0.25)
    assert np.array_equal(np.stack([res["per_stream"][k] for k in O.COUNTERS], axis=1), cn[0]) and np.array_equal(_bits(res["per_stream"]["iou_sum"]), _bits(qs[0]))
    assert (res["similarity"], res["zero_distance"]) == ("iou", None)
    ho, hh = iou.hota(matching="optimal"), HO.host_hota_optimal(ilogs)
    assert np.array_equal(ho.counters, hh["counters"]) and np.array_equal(_bits(ho.sums), _bits(hh["sums"])) and ho.similarity == "iou"
    idn, ih = iou.identity(alphas=LEVELS, pairs="all"), HO.host_identity_all(ilogs, alphas=LEVELS)
    assert np.array_equal(idn.counters, ih["counters"]) and idn.zero_distance is None
    sw, hs = iou.sweep(matching="optimal", min_iou=0.25), O.host_sweep(ilogs, 0.25)
    want = TS.optimal_sweep_values(hs["counters"], hs["iou_q"], hs["iou_sums"], hs["thresholds"], hs["reached"], 40)
    assert sw.reached == hs["reached"] and np.array_equal(sw.counters, want["counters"]) and np.array_equal(_bits(sw.motp), _bits(want["motp"]))
    assert (sw.similarity, sw.zero_distance) == ("iou", None)
    greedy = (iou.result(), iou.sweep(), iou.hota(), iou.identity())
    # the "centre" scorer: the same statements with the similarity substituted, on its downloaded log
    clogs = C.entries_from_logs(*(getattr(centre, k).cpu().numpy() for k in names + ("pair_sim",)))
    npairs = sum(len(e["pairs"]) for lb in clogs for e in lb)
    assert npairs > 60 and all(0.0 < s <= 1.0 for lb in clogs for e in lb for s in e["sims"])
    with monkeypatch.context() as m:
        C.patch_similarity(m)
        _, cho, _ = _check_replays(centre, clogs, min_iou=0.25)
    assert not np.array_equal(cho.counters, ho.counters)
    # the greedy calls read the main log only: the same under either similarity
    cg = (centre.result(), centre.sweep(), centre.hota(), centre.identity())
    assert all(cg[0]["overall"][k] == greedy[0]["overall"][k] for k in TS.COUNTERS) and np.array_equal(cg[1].counters, greedy[1].counters)
    assert np.array_equal(_bits(cg[2].sums), _bits(greedy[2].sums)) and np.array_equal(cg[3].counters, greedy[3].counters)
