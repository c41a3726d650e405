"""CPU: the native surface and the host half of the per-frame optimal matching at an IoU threshold (include/rtk_score.h,
csrc/track_score.hip, csrc/track_optimal.hip, ratrack_amd/track_score.py: `TrackScorer(sweep_pairs=...)`,
`sweep(matching="optimal")`, `clear_optimal`) -- the entry points and their constants are declared, built for gfx950 without scratch
and exported; the LDS the code object states is the figure the host function reports; the two host forms of
tests/_track_optimal_util.py agree with each other; the constructed frames have their known answers (greedy 1, optimal 2); the keywords are
validated."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import _track_optimal_util as O
from _util import SCORE_VARIANTS, kernel_notes, score_kernel_notes, template_flags
from ratrack_amd import _lib, abi, build as B
from ratrack_amd import track_score as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the native surface ------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_pair_log_and_the_optimal_replay():
    text = open(os.path.join(ROOT, "include", "rtk_score.h")).read()
    assert re.search(r"RTK_EXPORT int rtk_track_score_pairs\(const rtk_track_score_in_t \*in,", text)
    assert re.search(r"RTK_EXPORT int rtk_score_replay_optimal\(int B, int T, const rtk_score_log_t \*log, const rtk_score_pairs_t \*pairs,", text)
    assert re.search(r"RTK_EXPORT int rtk_score_optimal_lds_bytes\(int T\);", text)
    for name, value in (("RTK_SCORE_OPTIMAL_COUNTERS", len(TS.OPTIMAL_COUNTERS)), ("RTK_SCORE_PAIR_EDGES", TS.PAIR_EDGES),
                        ("RTK_SCORE_FLAG_OPTIMAL", TS.FLAG_OPTIMAL)):
        assert re.search(r"#define %s %d\b" % (name, value), text), name
    assert TS.FLAG_OPTIMAL == 512 and TS.PAIR_EDGES == 2048 == O.EDGES
    assert TS.OPTIMAL_COUNTERS == O.COUNTERS == ("frames", "gt", "pred", "tp", "fp", "fn", "idsw", "frag", "tracks", "mt", "pt", "ml")
    lib = ctypes.CDLL(B.build(verbose=False))
    for name, nargs in (("rtk_track_score_pairs", 7), ("rtk_score_replay_optimal", 15), ("rtk_score_optimal_lds_bytes", 1)):
        assert hasattr(lib, name) and len(abi.SIGNATURES[name]) == nargs, name
    assert [n for n, _ in abi.ScorePairs._fields_] == ["Q", "cursor", "frame_pair", "pair_key", "pair_common", "rec_size", "label_size"]
    assert abi.STRUCTS["rtk_score_pairs_t"] is abi.ScorePairs
    # what this is and what it is not is stated with the prototypes
    for word in ("ONE ASSIGNMENT", "THE CALLER CHOOSES", "still NOT a reproduction", "(1 << 23) + min(floor(iou * 65536), 65536)",
                 "tp * 2^23 + iou_q", "seen but unmatched in its previous seen frame", "logged whole or not at\n * all"):
        assert word in text, word
    for name in ("track_optimal.hip", "score_log_walk.h", "track_score.hip"):
        assert "asm" not in re.sub(r"//[^\n]*", "", open(os.path.join(B.CSRC, name)).read()), name


def test_optimal_replay_builds_for_gfx950_without_scratch_and_states_its_lds(tmp_path):
    found, _ = kernel_notes(os.path.join(B.CSRC, "track_optimal.hip"), tmp_path)
    # one instance per track-table capacity and similarity switch: no scratch, and the static LDS is the figure the host function reports
    assert len(found) == 4 and all("optimal_replay_kernel" in name and v.private == 0 for name, v in found.items()), found
    assert sorted(template_flags(name) for name in found) == [(False,), (False,), (True,), (True,)], sorted(found)
    lds = _lib._fn("rtk_score_optimal_lds_bytes")
    small = [v.lds for name, v in found.items() if "optimal_replay_kernelILi1024E" in name]
    assert small == [lds(1024)] * 2 and lds(1024) <= 65536 and lds(1) == lds(1024), (found, lds(1024))
    large = [v.lds for name, v in found.items() if "optimal_replay_kernelILi1024E" not in name]
    assert large == [lds(1025)] * 2 and lds(1024) < lds(1025) <= 65536
    assert lds(100000) > 65536 and lds(0) == -1
    # the figure, from its parts (ints): IoUs of the matches | edge list | solver tables at 256 x 64 x 2048 | track table 5 T | frame rows | scalars
    la_words = (256 + 1) + 2 * 2048 + 256 + 5 * 64
    assert lds(1024) == 4 * (2 * 64 + 2 * 2048 + la_words + 5 * 1024 + 2 * 256 + 3 * 64 + 8)


def test_pair_logging_kernels_build_without_scratch_and_with_no_static_lds(tmp_path):
    ts = score_kernel_notes(tmp_path)                # the ten instantiations of the one scoring kernel, and no other
    for k in ("pairs", "pairs_memory"):              # PAIRS with LOG, on the point IoU: without and with the memory block
        assert SCORE_VARIANTS[k][0] and SCORE_VARIANTS[k][2] and not any(SCORE_VARIANTS[k][3:]), k
        assert (ts[k].private, ts[k].lds) == (0, 0), (k, ts[k])          # dynamic LDS only: rtk_track_score_lds_bytes / _memory_lds_bytes


def test_entry_points_refuse_before_any_launch():
    lg = abi.ScoreLog(4, 32)
    keep = [(ctypes.c_int * 64)() for _ in range(5)] + [(ctypes.c_float * 64)(), (ctypes.c_double * 64)()]
    full = abi.ScoreLog(4, 8, None, *(ctypes.addressof(k) for k in keep))
    pk = [(ctypes.c_int * 64)() for _ in range(6)]
    pairs, empty = abi.ScorePairs(16, *(ctypes.addressof(k) for k in pk)), abi.ScorePairs(16)
    one = (ctypes.c_double * 1)(0.0)
    out = (ctypes.c_longlong * 64)()
    fl = (ctypes.c_int * 4)()
    a = ctypes.addressof

    def call(T=1024, log=full, pr=pairs, count=1, min_iou=0.5, counters=out, flags=fl):
        _lib.call("rtk_score_replay_optimal", 2, T, None if log is None else a(log), None if pr is None else a(pr), a(one), a(one), None, count,
                  min_iou, None if counters is None else a(counters), a(out), a(one), None, None if flags is None else a(flags), None)
    # (every pointer is host memory or null: a refusal touches none of them)
    with pytest.raises(_lib.RtkError, match="null or empty log"):
        call(log=lg)
    with pytest.raises(_lib.RtkError, match="null or empty pair log"):
        call(pr=empty)
    with pytest.raises(_lib.RtkError, match="null or empty pair log"):
        call(pr=None)
    with pytest.raises(_lib.RtkError, match="count=0"):
        call(count=0)
    with pytest.raises(_lib.RtkError, match="T=1304 track-table entries need \\d+ bytes of LDS per stream, the limit is 65536 \\(at most T=1303\\)"):
        call(T=1304)
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(_lib.RtkError, match="min_iou="):
            call(min_iou=bad)
    with pytest.raises(_lib.RtkError, match="null argument"):
        call(counters=None)
    with pytest.raises(_lib.RtkError, match="null argument"):
        call(flags=None)
    with pytest.raises(_lib.RtkError, match="null argument block"):
        _lib.call("rtk_track_score_pairs", None, None, None, a(full), None, a(pairs), None)


# ---- the keywords ------------------------------------------------------------------------------------------------------------------
def test_keyword_validation():
    with pytest.raises(ValueError, match="sweep_pairs=64 needs the log"):
        TS.TrackScorer(streams=2, max_objects=8, max_boxes=8, device="cpu", sweep_pairs=64)
    with pytest.raises(ValueError, match="sweep_pairs=0 must be at least 1"):
        TS.TrackScorer(streams=2, max_objects=8, max_boxes=8, device="cpu", sweep_frames=4, sweep_records=32, sweep_pairs=0)
    logged = TS.TrackScorer(streams=2, max_objects=8, max_boxes=8, device="cpu", sweep_frames=4, sweep_records=32)
    assert not logged.pairs and not hasattr(logged, "pair_key")
    with pytest.raises(RuntimeError, match="TrackScorer.sweep: the optimal matching needs the pair log \\(give sweep_pairs\\)"):
        logged.sweep(matching="optimal", min_iou=0.5)
    with pytest.raises(RuntimeError, match="TrackScorer.clear_optimal: the optimal matching needs the pair log"):
        logged.clear_optimal(0.5)
    s = TS.TrackScorer(streams=2, max_objects=8, max_boxes=8, device="cpu", sweep_frames=4, sweep_records=32, sweep_pairs=64)
    assert s.pairs and s.pair_key.shape == (2, 64) and s.pair_frame.shape == (2, 4, 2) and s.log_size.shape == s.log_label_size.shape == (2, 32)
    with pytest.raises(ValueError, match="needs an explicit min_iou in \\(0, 1\\]"):
        s.sweep(matching="optimal")
    with pytest.raises(TypeError):
        s.clear_optimal()
    for bad in (0.0, -0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="min_iou="):
            s.sweep(matching="optimal", min_iou=bad)
        with pytest.raises(ValueError, match="min_iou="):
            s.clear_optimal(bad)
    with pytest.raises(ValueError, match="matching='best'"):
        s.sweep(matching="best")
    with pytest.raises(ValueError, match="min_iou=0.5 goes with matching=\"optimal\""):
        s.sweep(min_iou=0.5)
    big = TS.TrackScorer(streams=1, max_objects=8, max_boxes=8, max_gt_tracks=1304, device="cpu", sweep_frames=4, sweep_records=32, sweep_pairs=8)
    with pytest.raises(ValueError, match="max_gt_tracks=1304 needs \\d+ bytes of LDS per stream for the optimal matching, the limit is 65536"):
        big.sweep(matching="optimal", min_iou=0.5)
    with pytest.raises(RuntimeError, match="stream 1 has a frame with more than 2048 candidate"):
        s._raise_on_flags([0, TS.FLAG_OPTIMAL])
    with pytest.raises(RuntimeError, match="or its pair log of sweep_pairs=64 pairs"):
        s._raise_on_flags([TS.FLAG_LOG, 0])


def test_optimal_sweep_values_carry_frag_and_iou_q():
    L, Bn = 2, 2
    c = np.zeros((L + 1, Bn, 12), dtype=np.int64)
    #          frames gt pred tp fp fn idsw frag tracks mt pt ml
    c[0, 0] = (4, 8, 9, 6, 3, 2, 1, 2, 2, 1, 1, 0)
    c[0, 1] = (4, 4, 4, 4, 0, 0, 0, 1, 1, 1, 0, 0)
    c[1, 0] = (4, 8, 5, 4, 1, 4, 0, 1, 2, 0, 2, 0)
    c[2] = 7                                                  # past `reached`: zeroed
    iq = np.array([[300000, 200000], [250000, 0], [9, 9]], dtype=np.int64)
    qs = np.array([[4.5, 3.0], [3.5, 0.0], [1.0, 1.0]])
    v = TS.optimal_sweep_values(c, iq, qs, np.array([-np.inf, 0.5, np.inf]), 1, L)
    assert v["frag"].tolist() == [3, 1, 0] and v["iou_q"].tolist() == [500000, 250000, 0]
    assert v["tp"].tolist() == [10, 4, 0] and v["idsw"].tolist() == [1, 0, 0] and v["motp"][0] == 7.5 / 10 and v["motp"][1] == 3.5 / 4
    assert v["counters"].shape == (3, 2, 11) and v["frag_streams"].shape == (3, 2) and v["best"]["frag"] == 1 and v["best"]["iou_q"] == 250000
    assert v["unfiltered"]["frag"] == 3 and v["mota"][1] == 1.0 - (1 + 4 + 0) / 8
    o = TS.optimal_values(c[0], qs[0])
    assert o["motp"].tolist() == [4.5 / 6, 3.0 / 4] and o["mota"][0] == 1.0 - 6 / 8 and o["mt_fraction"].tolist() == [0.5, 1.0]


# ---- the host statement ------------------------------------------------------------------------------------------------------------
def _two_on_one_frame(reset=True):
    """d0 has IoU 0.6 with A and 0.5 with B, d1 has 0.55 with A only (sizes chosen so that the three IoUs are the exact quotients
    15/25, 10/20 and 11/20)."""
    #                     A   B              d0  d1
    return O.make_frame([1, 2], [20, 10], [(10, 0.5, 20), (11, 0.5, 11)], [(0, 0, 15), (0, 1, 10), (1, 0, 11)], reset)


def test_the_constructed_frame_greedy_one_optimal_two():
    e = _two_on_one_frame()
    assert [O.pair_iou(e, i, j, c) for i, j, c in e["pairs"]] == [0.6, 0.5, 0.55]
    assert e["dets"][0][2:] == (1, 0.6) and e["dets"][1][2:] == (1, 0.55)          # both detections' best object is A
    assert O.greedy_tp(e) == 1
    sc = [[0.0, 0.0]]
    c, iou_q, iou_sum, tps, cps = O.replay([e], sc, -math.inf, 0.3)
    assert c["tp"] == 2 and c["fp"] == 0 and c["fn"] == 0 and cps[0] == [1, 0] and tps[0] == [0, 1]          # d1 on A, d0 on B
    assert iou_q == int(0.55 * 65536) + int(0.5 * 65536) and iou_sum == 0.55 + 0.5
    # an IoU equal to min_iou stays
    assert O.replay([e], sc, -math.inf, 0.5)[0]["tp"] == 2
    # above 0.5 the pair (d0, B) is refused: one match, and it is the heavier one, d0 on A
    for m in (0.5000001, 0.55):
        c, iou_q, iou_sum, tps, cps = O.replay([e], sc, -math.inf, m)
        assert c["tp"] == 1 and c["fp"] == 1 and c["fn"] == 1 and cps[0] == [0, -1] and iou_sum == 0.6 and iou_q == int(0.6 * 65536)
    assert O.replay([e], sc, -math.inf, 0.61)[0]["tp"] == 0
    # d0 removed by the threshold frees A for d1
    c, _, iou_sum, _, cps = O.replay([e], [[0.1, 0.9]], 0.5, 0.3)
    assert c["pred"] == 1 and c["tp"] == 1 and cps[0] == [1, -1] and iou_sum == 0.55
    # the independent solver sees the same unique quantities
    for m in (0.3, 0.5, 0.55):
        _, edges, _ = O.frame_edges(e, sc[0], -math.inf, m)
        assert O.independent_solve(2, 2, edges)[0] == O.la_solve(2, 2, edges)[0]


def test_id_switch_fragmentation_and_clip_close_in_the_host_statement():
    f = lambda tid, on=True, reset=False: O.frame_from_ious([7], [(tid, 0.5)], {(0, 0): 16} if on else {}, reset)
    sc = lambda lb: [[0.0] * len(e["dets"]) for e in lb]
    run = lambda lb: O.replay(lb, sc(lb), -math.inf, 0.5)[0]
    c = run([f(1, reset=True), f(1), f(2), f(2)])
    assert (c["tp"], c["idsw"], c["frag"], c["tracks"], c["mt"]) == (4, 1, 0, 1, 1)
    c = run([f(1, reset=True), f(1, on=False), f(1)])                        # matched, seen unmatched, matched again: one fragmentation
    assert (c["tp"], c["fn"], c["idsw"], c["frag"], c["pt"]) == (2, 1, 0, 1, 1)
    c = run([f(1, reset=True), f(1, on=False), f(1, on=False)])              # the same gap without a re-match
    assert (c["tp"], c["frag"], c["pt"]) == (1, 0, 1)
    c = run([f(1, on=False, reset=True), f(1)])                              # never matched before: no fragmentation
    assert (c["tp"], c["frag"]) == (1, 0)
    c = run([f(1, reset=True), f(1, on=False), f(1, reset=True)])            # the reset closes the clip: the gap is forgotten
    assert (c["tp"], c["frag"], c["idsw"], c["tracks"]) == (2, 0, 0, 2)


def _solvers_agree(e, sc, tau, min_iou, scipy=False):
    _, edges, _ = O.frame_edges(e, sc, tau, min_iou)
    P, G = len(e["dets"]), len(e["labels"])
    wa, cp = O.la_solve(P, G, edges)
    wb, match = O.independent_solve(P, G, edges, scipy=scipy)
    assert (wa >> 23, wa & (O.ONE - 1)) == (wb >> 23, wb & (O.ONE - 1)), (edges, wa, wb)
    assert wa >> 23 == sum(1 for r in cp if r >= 0) and all((cp[j], j) in {(i, k) for i, k, _ in edges} for j in range(G) if cp[j] >= 0)
    return edges, cp, match


def test_both_host_solvers_agree_on_200_random_frames():
    logs = O.random_logs(seed=2, streams=5, frames=40)
    frames = [e for lb in logs for e in lb]
    assert len(frames) == 200
    busy = differ = 0
    for k, e in enumerate(frames):
        sc = [float(d[1]) for d in e["dets"]]
        edges, cp, match = _solvers_agree(e, sc, 0.25 if k % 2 else -math.inf, (0.1, 0.3, 0.5)[k % 3])
        busy += len(edges) > 2
        differ += O.greedy_tp(e) != sum(1 for r in cp if r >= 0)
    assert busy >= 50 and differ >= 50, (busy, differ)          # a quarter of the frames have more than two candidates / another count than the greedy rule
    # a dense frame: 32 x 32 with every pair present
    rng = np.random.default_rng(4)
    dense = O.make_frame(range(32), [40] * 32, [(100 + i, 0.5, 40) for i in range(32)],
                         [(i, j, int(rng.integers(1, 41))) for i in range(32) for j in range(32)], True)
    edges, cp, _ = _solvers_agree(dense, [0.0] * 32, -math.inf, 0.01)
    assert len(edges) == 1024 and sum(1 for r in cp if r >= 0) == 32


def test_both_host_solvers_agree_with_scipy():
    pytest.importorskip("scipy.optimize")
    for e in [e for lb in O.random_logs(seed=3, streams=2, frames=30) for e in lb]:
        _solvers_agree(e, [0.0] * len(e["dets"]), -math.inf, 0.2, scipy=True)


def test_the_gpu_tests_random_logs_mostly_have_a_unique_optimum():
    """The seed tests/test_track_optimal_gpu.py uses: on at least half of the frames that have a candidate the optimum is unique (the
    matching itself can then be compared), and the sweep over them reaches levels."""
    logs = O.random_logs(O_SEED)
    scores = [[[0.0] * len(e["dets"]) for e in lb] for lb in logs]
    uniq, total = O.unique_share(logs, scores, -math.inf, 0.2)
    print("random logs, seed %d: %d of %d frames with a candidate have a unique optimum" % (O_SEED, uniq, total))
    assert total > 100 and 2 * uniq >= total
    assert O.host_sweep(logs, 0.2)["reached"] > 10


O_SEED = 1


def test_the_small_sequence_has_what_the_pair_log_must_meet():
    seq = O.small_sequence()
    logs = O.small_sequence_log(seq)
    assert (seq["B"], seq["N"], seq["Kobj"], seq["K"], len(seq["frames"])) == (3, 70, 8, 5, 12)
    assert [len(lb) for lb in logs] == [12, 12, 11] and sum(e["reset"] for e in logs[0]) == 2
    assert int(seq["frames"][0]["n_valid"][1]) < 70 and not seq["frames"][4]["active"][2]
    two = sum(1 for lb in logs for e in lb for i in range(len(e["dets"])) if sum(1 for p in e["pairs"] if p[0] == i) > 1)
    above_one = sum(1 for lb in logs for e in lb for i, j, c in e["pairs"] if O.pair_iou(e, i, j, c) > 1.0)
    assert two > 30 and above_one > 0                    # a detection over two kept objects; coincident points push an IoU past 1
    assert all(len(e["labels"]) == 4 for lb in logs for e in lb)          # the rider is merged into the cyclist: 5 boxes, 4 kept objects
    assert all(e["pairs"] == sorted(e["pairs"]) for lb in logs for e in lb)
    sw = O.host_sweep(logs, 0.3)
    assert sw["reached"] > 10 and sw["counters"][0, :, O.COUNTERS.index("idsw")].sum() > 0
