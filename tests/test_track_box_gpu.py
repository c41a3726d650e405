"""GPU: the oriented-box IoU on the pair log (csrc/track_score.hip `rtk_track_score_pairs_box`, `TrackScorer(similarity="box")` /
`"box_bev"`) against the host statement of tests/_track_box_util.py.  The producer's integers and decisions exactly and its similarities
within SIM_BOUND (exact cases: bit for bit); everything but the pair log equal to the "iou" scorer's; the four replays on produced logs
against the existing host statements with their two similarity functions substituted.  The ground-truth objects are built by hand where
that is simpler (`GtObjects` is a plain holder of tensors)."""
import math

import numpy as np
import pytest
import torch

import _track_box_util as X
import _track_hota_optimal_util as HO
import _track_identity_util as I
import _track_optimal_util as O
import _track_score_util as S
import _track_sweep_util as W
from ratrack_amd import boxes as BX
from ratrack_amd import gt_device as G
from ratrack_amd import track_score as TS

pytestmark = pytest.mark.gpu
DEV = "cuda"
STATE = ("counters", "iou_sum", "table_key", "table_last", "table_seen", "table_matched", "table_used", "prev_gt_id", "prev_count", "prev_gt",
         "flags")
LOG = ("log_cursor", "log_frame", "log_label", "log_track", "log_best", "log_conf", "log_iou")
SIZES = ("log_size", "log_label_size")
PAIR_INTS = ("pair_cursor", "pair_frame", "pair_key", "pair_common")
PAIRS = PAIR_INTS + ("pair_sim",)
OUT = ("pred_gt_slot", "pred_gt_id", "gt_pred", "iou", "aff_target", "aff_defined")
LEVELS = (0.25, 0.5, 0.6, 0.75)
NAMES = ("box", "box_bev")


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
                        members=_dev(fr["members"].view(np.int32)), centre=_dev(fr["centre"]), boxes=_dev(fr["boxes"]),
                        flags=torch.zeros(len(fr["count"]), dtype=torch.int32, device=DEV), n_valid=_dev(fr["n_valid"]), max_boxes=K, points=N)


def _feed(frames, scorers, K, N, tables=None):
    """Every frame through every scorer; the MatchResults of one frame are equal bit for bit."""
    for f, fr in enumerate(frames):
        gobj = _gobj(fr, K, N)
        kw = {} if tables is None else dict(table_ids=_dev(tables[f][0]), table_count=_dev(tables[f][1]))
        outs = [sc.update_raw(_dev(fr["pc1"]), _dev(fr["obj"]), _dev(fr["num"]), _dev(fr["ids"]), gobj, _dev(fr["n_valid"]), _dev(fr["reset"]),
                              _dev(fr["active"]), object_conf=_dev(fr["conf"]), det_boxes=_dev(fr["det_box"]), det_box_valid=_dev(fr["det_valid"]),
                              **kw) for sc in scorers]
        for o in outs[1:]:
            _equal_tensors(outs[0], o, OUT)


def _holds_pair_log(sc, host, exact=False):
    """The scorer's pair log is the host statement's: the integers ==, no pair left out; pair_sim within SIM_BOUND (exact: bit for bit).
    -> the largest difference."""
    for k in PAIR_INTS:
        dev = getattr(sc, k).cpu().numpy()
        assert dev.shape == host[k].shape and np.array_equal(dev, host[k]), (k, np.argwhere(dev != host[k])[:6])
    dev, ref = sc.pair_sim.cpu().numpy(), np.asarray(host["pair_sim"], np.float64)
    worst = float(np.abs(dev - ref).max())
    print("pair_sim: largest |device - host| %.3e over %d pairs (bound %.3e)" % (worst, int(host["pair_cursor"].sum()), X.SIM_BOUND))
    if exact:
        assert np.array_equal(_bits(dev), _bits(ref)), np.argwhere(dev != ref)[:6]
    assert worst <= X.SIM_BOUND, worst
    return worst


# ---- 1: the producer on hand-built frames; everything else is rtk_track_score_pairs ---------------------------------------------------------
F1, R1, Q1 = 8, 512, 2048
_HOST = {}


def _host(key, frames, B, mode, Q=Q1):
    """The host statement of a scenario, computed once per session and left unchanged."""
    k = (key, mode, Q)
    if k not in _HOST:
        _HOST[k] = X.host_pair_log(frames, B, F1, R1, Q, mode)
    return _HOST[k]


@pytest.mark.parametrize("memory", [False, True])
@pytest.mark.parametrize("N,Kobj,seed,many", [(96, 16, 21, None), (320, 16, 21, None), (96, 80, 23, 70)])
def test_the_pair_log_is_the_host_statements_and_everything_else_is_the_iou_scorers(N, Kobj, seed, many, memory):
    B, K = 4, 8
    frames = X.scenario(seed, B=B, N=N, Kobj=Kobj, K=K, many=many)
    hosts = {name: _host((seed, N, Kobj, many), frames, B, X.MODES[name]) for name in NAMES}
    # the condition, on the host statement alone: no pair near s = 0, none near the prefilter's rim -- then the logged sets must be equal
    assert all(X.condition_holds(h) for h in hosts.values())
    tables = None
    if memory:                             # the tracker's new table: this frame's detections, then up to 3 coasted rows
        rng, tables = np.random.default_rng(seed), []
        for fr in frames:
            ids, count = fr["ids"].copy(), fr["num"].copy()
            for b in range(B):
                extra = min(int(rng.integers(0, 4)), Kobj - int(count[b]))
                ids[b, count[b]:count[b] + extra] = 100 + rng.choice(16, extra, replace=False)
                count[b] += extra
            tables.append((ids, count))
    mk = lambda **kw: TS.TrackScorer(streams=B, max_objects=Kobj, max_boxes=K, max_gt_tracks=32, sweep_frames=F1, sweep_records=R1, sweep_pairs=Q1,
                                     track_memory=memory, **kw)
    iou, box, bev, again = mk(), mk(similarity="box"), mk(similarity="box_bev"), mk(similarity="box")
    _feed(frames, (iou, box, bev, again), K, N, tables)
    extra = ("row_track", "labelled_coasted") if memory else ()
    for sc, name in ((box, "box"), (bev, "box_bev")):
        sc.check()
        host = hosts[name]
        _holds_pair_log(sc, host)
        # what the cases are there for: pairs without a common point and with one; detections without a box (valid 0 and -1, width 0);
        # objects with a degenerate box; P = 0, G = 0, an inactive stream (one frame fewer), a reset in the middle
        commons = [c for b in range(B) for ps, _ in host["entries"][b] for _, _, c in ps]
        assert min(commons) == 0 < max(commons) and int(host["pair_cursor"].sum()) > 40
        assert host["frames"].tolist() == [3, 3, 2, 3] and sc.log_cursor[:, 0].cpu().tolist() == [3, 3, 2, 3]
        assert all(i not in (1, 2, 3) for ps, _ in host["entries"][0] for i, _, _ in ps)
        assert all(j != 1 for ps, _ in host["entries"][2] for _, j, _ in ps) and all(j > 1 for ps, _ in host["entries"][3] for _, j, _ in ps)
        assert host["pair_frame"][0, 1, 1] == 0 and host["pair_frame"][1, 1, 1] == 0 and (sc.log_frame[3, 1, 2].item() >> 16) & 1 == 1
        # everything but the pair log: counters, iou_sum, the track table, the main log, the sizes, flags -- the "iou" scorer's bits
        _equal_tensors(sc, iou, STATE + LOG + SIZES + extra)
        assert not torch.equal(sc.pair_key, iou.pair_key) and int(sc.flags.sum()) == 0
    if many:                               # stream 1's last frame: more rows with pairs than one wave holds
        rows = {i for i, _, _ in hosts["box_bev"]["entries"][1][-1][0]}
        assert int(frames[2]["num"][1]) == many and len(rows) > 40 and max(rows) >= 64
    assert int(hosts["box_bev"]["pair_cursor"].sum()) > int(hosts["box"]["pair_cursor"].sum())
    # the same bits on a second run, pair_sim included
    _equal_tensors(box, again, STATE + LOG + SIZES + PAIRS + extra)


# ---- 2: exact cases, bit for bit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_exact_boxes_give_exact_similarities_and_sit_on_the_levels(name):
    fr, N, K, Kobj, want = X.exact_frame()
    mode = X.MODES[name]
    sc = TS.TrackScorer(streams=1, max_objects=Kobj, max_boxes=K, max_gt_tracks=16, sweep_frames=4, sweep_records=32, sweep_pairs=32, similarity=name)
    _feed([fr], (sc,), K, N)
    sc.check()
    n = int(sc.pair_cursor[0])
    got = [(int(k) >> 8, int(k) & 255, int(c), float(s)) for k, c, s in zip(sc.pair_key[0, :n].cpu(), sc.pair_common[0, :n].cpu(), sc.pair_sim[0, :n].cpu())]
    # s = 1, 1/2, 1/3, 1/7 as the float64 quotients; the touching pairs (an edge, a corner) and every distant pair absent; the pair
    # whose z ranges are apart only in the bird's-eye view
    assert got == want[mode] and [s for *_, s in got[:4]] == [1.0, 0.5, 1.0 / 3.0, 1.0 / 7.0]
    _holds_pair_log(sc, X.host_pair_log([fr], 1, 4, 32, 32, mode), exact=True)
    more = len(got) - 4                    # (BEV: one more pair of s = 1)
    # s = 0.5 stays at min_iou = 0.5 and at alpha = 0.5; just above, it does not
    at, above = sc.clear_optimal(0.5), sc.clear_optimal(math.nextafter(0.5, 1.0))
    assert at["overall"]["tp"] == 2 + more and at["overall"]["iou_sum"] == 1.5 + more and above["overall"]["tp"] == 1 + more
    assert (at["similarity"], at["zero_distance"]) == (name, None)
    idn = sc.identity(alphas=(1.0 / 7.0, 1.0 / 3.0, 0.5, math.nextafter(0.5, 1.0), 0.75, 1.0), pairs="all")
    assert idn.counters[:, 0, I.COUNTERS.index("pairs")].tolist() == [4 + more, 3 + more, 2 + more, 1 + more, 1 + more, 1 + more]
    assert (idn.similarity, idn.zero_distance) == (name, None)
    ho = sc.hota(alphas=19, matching="optimal")
    tp = ho.counters[:, 0, HO.COUNTERS.index("tp")]
    assert tp[9] == 2 + more and tp[10] == 1 + more and tp[1] == 4 + more and tp[2] == 3 + more          # alpha = 10/20, 11/20, 2/20, 3/20
    assert (ho.similarity, ho.zero_distance, ho.matching) == (name, None, "optimal")


# ---- 3: the overflows -----------------------------------------------------------------------------------------------------------------------
def test_a_frame_whose_pairs_do_not_fit_is_in_neither_log():
    B, N, Kobj, K = 4, 96, 16, 8
    frames = X.scenario(21, B=B, N=N, Kobj=Kobj, K=K)
    full = _host((21, N, Kobj, None), frames, B, X.MODE_BEV)
    Q = int(full["pair_frame"][3, 0, 1]) + 1          # stream 3's first frame fits, with one pair to spare
    host = _host((21, N, Kobj, None), frames, B, X.MODE_BEV, Q)
    assert host["dropped"].any()
    sc = TS.TrackScorer(streams=B, max_objects=Kobj, max_boxes=K, max_gt_tracks=32, sweep_frames=F1, sweep_records=R1, sweep_pairs=Q, similarity="box_bev")
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
    fr, B, N, Kobj, K = X.crowded_frame()
    sc = TS.TrackScorer(streams=B, max_objects=Kobj, max_boxes=K, max_gt_tracks=64, sweep_frames=2, sweep_records=128, sweep_pairs=4096,
                        similarity="box")
    _feed([fr], (sc,), K, N)
    sc.check()
    assert sc.pair_cursor.cpu().tolist() == [64 * K, 2 * 3] and 64 * K > TS.PAIR_EDGES
    host = X.host_pair_log([fr], B, 2, 128, 4096, X.MODE_3D)
    assert X.condition_holds(host)
    _holds_pair_log(sc, host)
    with pytest.raises(RuntimeError, match="stream 0 has a frame with more than %d candidate" % TS.PAIR_EDGES):
        sc.clear_optimal(0.25)
    assert sc.clear_optimal(0.25, check=False)["flags"].tolist() == [TS.FLAG_OPTIMAL, 0]
    ho = sc.hota(matching="optimal", check=False)
    assert ho.flags.tolist() == [TS.FLAG_OPTIMAL, 0] and ho.counters[0, 1, HO.COUNTERS.index("tp")] == 2
    assert int(sc.flags.sum()) == 0


# ---- 4: end to end --------------------------------------------------------------------------------------------------------------------------
def _check_replays(sc, logs, min_iou):
    """The four calls against the (substituted) host statements: integers ==, the ordered float64 sums bit for bit."""
    plain = [[[0.0] * len(e["dets"]) for e in lb] for lb in logs]
    res = sc.clear_optimal(min_iou)
    cn, iq, qs = O.host_replays(logs, plain, [-math.inf], min_iou)
    assert np.array_equal(np.stack([res["per_stream"][k] for k in O.COUNTERS], axis=1), cn[0])
    assert np.array_equal(res["per_stream"]["iou_q"], iq[0]) and np.array_equal(_bits(res["per_stream"]["iou_sum"]), _bits(qs[0]))
    ho = sc.hota(alphas=19, matching="optimal")
    host = HO.host_hota_optimal(logs, None, -math.inf, 19)
    assert np.array_equal(ho.counters, host["counters"]) and np.array_equal(_bits(ho.sums), _bits(host["sums"]))
    assert (ho.similarity, ho.zero_distance, ho.matching) == (sc.similarity, None, "optimal")
    idn = sc.identity(alphas=LEVELS, pairs="all")
    ihost = HO.host_identity_all(logs, None, -math.inf, LEVELS)
    assert np.array_equal(idn.counters, ihost["counters"]) and idn.idtp.tolist() == ihost["idtp"] and idn.similarity == sc.similarity
    sw, hs = sc.sweep(matching="optimal", min_iou=min_iou), O.host_sweep(logs, min_iou)
    assert sw.reached == hs["reached"] and np.array_equal(_bits(sw.thresholds), _bits(hs["thresholds"]))
    want = TS.optimal_sweep_values(hs["counters"], hs["iou_q"], hs["iou_sums"], hs["thresholds"], hs["reached"], 40)
    assert np.array_equal(sw.counters, want["counters"]) and np.array_equal(sw.iou_q_streams, want["iou_q_streams"])
    for k in ("iou_sums", "mota", "motp"):
        assert np.array_equal(_bits(getattr(sw, k)), _bits(want[k])), k
    assert (sw.similarity, sw.zero_distance, sw.min_iou) == (sc.similarity, None, min_iou)
    return res, ho, idn


def test_a_short_sequence_through_the_box_scorers_and_the_four_calls(monkeypatch):
    seq = O.small_sequence()
    K, Kobj = seq["K"], 8
    mk = lambda **kw: TS.TrackScorer(streams=3, max_objects=Kobj, max_boxes=5, max_gt_tracks=16, sweep_frames=16, sweep_records=128, sweep_pairs=512, **kw)
    iou, box, bev = mk(), mk(similarity="box"), mk(similarity="box_bev")
    for fr in seq["frames"]:
        pc1, nv = _dev(fr["pc1"]), _dev(fr["n_valid"])
        packed = G.pack_boxes(fr["per_stream"], K, DEV)
        gobj = TS.gt_objects(pc1, packed, TS.pack_box_types(fr["per_stream"], K, DEV), n_valid=nv, min_obj_points=S.MIN_PTS)
        # the frame-1 box table it was given: a reference, no copy
        assert gobj.boxes.shape == (3, K, 16) and gobj.boxes.dtype == torch.float64 and gobj.boxes.data_ptr() == packed.boxes[0].data_ptr()
        bx = BX.object_boxes_raw(pc1, _dev(fr["obj"]), _dev(fr["num"]), Kobj, active=_dev(fr["active"]), min_extent=0.5)
        outs = [sc.update_raw(pc1, _dev(fr["obj"]), _dev(fr["num"]), _dev(fr["ids"]), gobj, nv, _dev(fr["reset"]), _dev(fr["active"]),
                              object_conf=_dev(fr["conf"]), det_boxes=bx.box, det_box_valid=bx.valid) for sc in (iou, box, bev)]
        _equal_tensors(outs[0], outs[1], OUT)
        _equal_tensors(outs[0], outs[2], OUT)
    names = LOG + ("pair_frame", "pair_key", "pair_common") + SIZES
    greedy = (iou.result(), iou.sweep(), iou.hota(), iou.identity())
    iho = iou.hota(matching="optimal")
    for sc in (box, bev):
        sc.check()
        _equal_tensors(sc, iou, STATE + LOG + SIZES)
        logs = X.entries_from_logs(*(getattr(sc, k).cpu().numpy() for k in names + ("pair_sim",)))
        sims = [s for lb in logs for e in lb for s in e["sims"]]
        print("%s: %d pairs, s in [%.4f, %.4f]" % (sc.similarity, len(sims), min(sims), max(sims)))
        assert len(sims) > 20 and all(0.0 < s <= 1.0 for s in sims)
        with monkeypatch.context() as m:
            X.patch_similarity(m)
            _, ho, _ = _check_replays(sc, logs, min_iou=0.25)
        assert not np.array_equal(ho.counters, iho.counters)
        # the greedy calls read the main log only: the same under any similarity
        cg = (sc.result(), sc.sweep(), sc.hota(), sc.identity())
        assert all(cg[0]["overall"][k] == greedy[0]["overall"][k] for k in TS.COUNTERS) and np.array_equal(cg[1].counters, greedy[1].counters)
        assert np.array_equal(_bits(cg[2].sums), _bits(greedy[2].sums)) and np.array_equal(cg[3].counters, greedy[3].counters)
    assert sum(int(v) for v in bev.pair_cursor.cpu()) >= sum(int(v) for v in box.pair_cursor.cpu())

    # `update` takes the boxes from the step (the last frame, as a reset, through both doors: the same pair log); a step without
    # boxes names the tracker's keyword
    class Step:
        max_objects, object_boxes, object_box_valid = Kobj, None, None
    with pytest.raises(ValueError, match="BatchedTracker\\(boxes=True\\)"):
        box.update(Step(), gobj)
    step = Step()
    step.pc1, step.obj, step.num_objects, step.object_ids, step.active = pc1, _dev(fr["obj"]), _dev(fr["num"]), _dev(fr["ids"]), _dev(fr["active"])
    step.object_conf, step.object_boxes, step.object_box_valid = _dev(fr["conf"]), bx.box, bx.valid
    one, two = mk(similarity="box_bev"), mk(similarity="box_bev")
    rst = torch.ones(3, dtype=torch.uint8, device=DEV)
    a = one.update(step, gobj, reset=rst)
    b = two.update_raw(pc1, step.obj, step.num_objects, step.object_ids, gobj, nv, rst, step.active, object_conf=step.object_conf, det_boxes=bx.box,
                       det_box_valid=bx.valid)
    _equal_tensors(a, b, OUT)
    _equal_tensors(one, two, STATE + LOG + SIZES + PAIRS)
    assert int(one.log_cursor[:, 0].sum()) > 0
