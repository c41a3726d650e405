"""CPU: the native surface and the host half of HOTA under the optimal matching and of the identity metrics over every pair
(include/rtk_score.h, csrc/track_hota_optimal.hip, csrc/track_identity_pairs.hip, ratrack_amd/track_score.py:
`TrackScorer.hota(matching="optimal")`, `TrackScorer.identity(pairs="all")`) -- the entry points and their constants are declared, built
for gfx950 without scratch and exported; the LDS the code objects state is within the limit and is the figure the host functions report;
the two host statements of tests/_track_hota_optimal_util.py agree bit for bit; the 28-bit weights keep the optimum within the stated
bound; the constructed cases have their known answers; the keywords are validated."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import _track_hota_optimal_util as HO
import _track_hota_util as H
import _track_identity_util as I
import _track_optimal_util as O
import _track_sweep_util as W
from _util import kernel_notes, template_flags
from ratrack_amd import _lib, abi, build as B
from ratrack_amd import track_score as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 65536


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


# ---- the native surface ------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_new_entry_points():
    text = open(os.path.join(ROOT, "include", "rtk_score.h")).read()
    assert re.search(r"RTK_EXPORT int rtk_score_alignment\(int B, int T, const rtk_score_log_t \*log, const rtk_score_pairs_t \*pairs,", text)
    assert re.search(r"RTK_EXPORT int rtk_score_hota_optimal\(int B, const rtk_score_log_t \*log, const rtk_score_pairs_t \*pairs,", text)
    assert re.search(r"RTK_EXPORT int rtk_score_identity_pairs\(int B, int T, const rtk_score_log_t \*log, const rtk_score_pairs_t \*pairs,", text)
    assert re.search(r"RTK_EXPORT int rtk_score_alignment_lds_bytes\(int T\);", text)
    assert re.search(r"RTK_EXPORT int rtk_score_identity_pairs_lds_bytes\(int T\);", text)
    # the header's constants are track_score.py's, and the host statement's
    for name, value in (("RTK_SCORE_ALIGN_PAIRS", TS.ALIGN_PAIRS), ("RTK_SCORE_PAIR_EDGES", TS.PAIR_EDGES), ("RTK_SCORE_FLAG_HOTA", TS.FLAG_HOTA),
                        ("RTK_SCORE_FLAG_IDENTITY", TS.FLAG_IDENTITY), ("RTK_SCORE_FLAG_OPTIMAL", TS.FLAG_OPTIMAL),
                        ("RTK_SCORE_HOTA_COUNTERS", len(TS.HOTA_COUNTERS)), ("RTK_SCORE_HOTA_SUMS", len(TS.HOTA_SUMS)),
                        ("RTK_SCORE_ID_COUNTERS", len(TS.IDENTITY_COUNTERS)), ("RTK_SCORE_LDS_LIMIT", TS.LDS_LIMIT)):
        assert re.search(r"#define %s %d\b" % (name, value), text), name
    assert TS.ALIGN_PAIRS == HO.ALIGN_PAIRS == 1024 and TS.PAIR_EDGES == HO.EDGES and TS.HOTA_COUNTERS == HO.COUNTERS and TS.HOTA_SUMS == HO.SUMS
    assert TS.IDENTITY_COUNTERS == I.COUNTERS
    lib = ctypes.CDLL(B.build(verbose=False))
    for name, nargs in (("rtk_score_alignment", 12), ("rtk_score_hota_optimal", 14), ("rtk_score_identity_pairs", 11),
                        ("rtk_score_alignment_lds_bytes", 1), ("rtk_score_identity_pairs_lds_bytes", 1)):
        assert hasattr(lib, name) and len(abi.SIGNATURES[name]) == nargs, name
    # what this is and what it is not is stated with the prototypes
    for word in ("ONE MATCHING FOR ALL ALPHA", "max(1, (int)floor(min(A[g,t] * sbar, 1.0) * 2^28))", "min(P, G) * 2^-28", "it is not measured",
                 "q = sbar / ((r_i + k_j) - sbar)", "A[g,t] = pmc / ((double)(cg + ct) - pmc)", "IN ORDER OF FIRST APPEARANCE AMONG THE VALID PAIRS",
                 "WHAT NOW AGREES WITH TrackEval", "WHAT STILL DOES NOT", "POINT IoU, not a box IoU", "28 BITS", "SOME REMAINING DETECTION"):
        assert word in text, word
    for name in ("track_hota_optimal.hip", "track_identity_pairs.hip", "score_log_walk.h", "lds_assignment.h"):
        code = re.sub(r"//[^\n]*", "", open(os.path.join(B.CSRC, name)).read())
        assert "asm" not in code and not re.search(r"atomic\w*\s*\(\s*&?\s*\w*(pmc|rsum|ksum|quot|miou|cq)\b", code), name


def test_the_new_kernels_build_for_gfx950_without_scratch_and_within_the_lds_limit(tmp_path):
    found, _ = kernel_notes(os.path.join(B.CSRC, "track_hota_optimal.hip"), tmp_path)
    # every kernel twice: on the point IoU and with the similarity switch on
    assert len(found) == 6 and all(v.private == 0 and 0 < v.lds <= LIMIT and (v.wavefront, v.max_threads) == (64, 64) for v in found.values()), found
    assert sorted(template_flags(name) for name in found) == [(False,)] * 3 + [(True,)] * 3, sorted(found)
    lds = _lib._fn("rtk_score_alignment_lds_bytes")
    small = [v.lds for name, v in found.items() if "alignment_kernelILi1024E" in name]
    large = [v.lds for name, v in found.items() if "alignment_kernel" in name and "ILi1024E" not in name]
    assert small == [lds(1024)] * 2 and lds(1) == lds(1024) and large == [lds(1025)] * 2 and lds(1024) < lds(1025) <= LIMIT
    assert lds(1404) == lds(1025) and lds(1405) > LIMIT and lds(0) == -1
    # the figures, from their parts (ints): r, k, a chunk's q, pmc as float64 | chunk key, index | pair list key, n | pair lookup | track
    # table key, ct | label table key, cg | rslot | glabel, entry | scalars
    assert lds(1024) == 4 * (2 * (256 + 64 + 64 + 1024) + 2 * 64 + 2 * 1024 + 2048 + 2 * 3072 + 2 * 1024 + 256 + 2 * 64 + 8) == 62496
    la_words = (256 + 1) + 2 * 2048 + 256 + 5 * 64
    match = [v.lds for name, v in found.items() if "hota_optimal_kernel" in name]
    assert match == [4 * (2 * (64 + 3 * 64) + 2 * 2048 + la_words + 1024 + 256 + 2 * 64 + 64 + 8)] * 2 == [44068] * 2
    found, _ = kernel_notes(os.path.join(B.CSRC, "track_identity_pairs.hip"), tmp_path)
    assert len(found) == 4 and all("identity_pairs_kernel" in name and v.private == 0 and v.lds <= LIMIT for name, v in found.items()), found
    assert sorted(template_flags(name) for name in found) == [(False,)] * 2 + [(True,)] * 2, sorted(found)
    ilds, plds = _lib._fn("rtk_score_identity_lds_bytes"), _lib._fn("rtk_score_identity_pairs_lds_bytes")
    assert sorted(v.lds for v in found.values()) == [plds(1024)] * 2 + [plds(1025)] * 2 and all(plds(T) == ilds(T) for T in (0, 1, 1024, 1025, 3583, 3584, 100000))


def test_entry_points_refuse_before_any_launch():
    keep = [(ctypes.c_int * 64)() for _ in range(5)] + [(ctypes.c_float * 64)(), (ctypes.c_double * 64)()]
    full, bare = abi.ScoreLog(4, 8, None, *(ctypes.addressof(k) for k in keep)), abi.ScoreLog(4, 32)
    pk = [(ctypes.c_int * 64)() for _ in range(6)]
    pairs, empty = abi.ScorePairs(16, *(ctypes.addressof(k) for k in pk)), abi.ScorePairs(16)
    dbl, out, ints = (ctypes.c_double * 64)(), (ctypes.c_longlong * 64)(), (ctypes.c_int * 64)()
    a = lambda x: None if x is None else ctypes.addressof(x)
    # (every pointer is host memory or null: a refusal touches none of them)

    def align(T=1024, log=full, pr=pairs, tables=ints, flags=ints):
        _lib.call("rtk_score_alignment", 2, T, a(log), a(pr), None, None, a(dbl), a(tables), a(ints), a(ints), a(flags), None)

    def match(alphas=19, log=full, pr=pairs, tables=ints, counters=out):
        _lib.call("rtk_score_hota_optimal", 2, a(log), a(pr), None, None, alphas, a(dbl), a(tables), a(ints), a(ints), a(counters), a(dbl), a(ints), None)

    def ident(T=1024, log=full, pr=pairs, count=1, levels=dbl):
        _lib.call("rtk_score_identity_pairs", 2, T, a(log), a(pr), None, None, a(levels), count, a(out), a(ints), None)
    for call in (align, match, ident):
        with pytest.raises(_lib.RtkError, match="null or empty log"):
            call(log=bare)
        with pytest.raises(_lib.RtkError, match="null or empty pair log"):
            call(pr=empty)
        with pytest.raises(_lib.RtkError, match="null or empty pair log"):
            call(pr=None)
    with pytest.raises(_lib.RtkError, match="T=1405 label-table entries need \\d+ bytes of LDS per stream, the limit is 65536 \\(at most T=1404\\)"):
        align(T=1405)
    with pytest.raises(_lib.RtkError, match="null output"):
        align(tables=None)
    with pytest.raises(_lib.RtkError, match="null output"):
        align(flags=None)
    with pytest.raises(_lib.RtkError, match="alphas=64"):
        match(alphas=64)
    with pytest.raises(_lib.RtkError, match="null alignment tables"):
        match(tables=None)
    with pytest.raises(_lib.RtkError, match="null output"):
        match(counters=None)
    with pytest.raises(_lib.RtkError, match="T=3584 label-table entries need"):
        ident(T=3584)
    with pytest.raises(_lib.RtkError, match="count=0"):
        ident(count=0)
    with pytest.raises(_lib.RtkError, match="null levels or null output"):
        ident(levels=None)


def test_keyword_validation():
    logged = TS.TrackScorer(streams=2, max_objects=8, max_boxes=8, device="cpu", sweep_frames=4, sweep_records=32)
    with pytest.raises(RuntimeError, match="TrackScorer.hota: the optimal matching needs the pair log \\(give sweep_pairs\\)"):
        logged.hota(matching="optimal")
    with pytest.raises(RuntimeError, match="TrackScorer.identity: the optimal matching needs the pair log \\(give sweep_pairs\\)"):
        logged.identity(pairs="all")
    s = TS.TrackScorer(streams=2, max_objects=8, max_boxes=8, device="cpu", sweep_frames=4, sweep_records=32, sweep_pairs=64)
    with pytest.raises(ValueError, match="TrackScorer.hota: matching='best' is neither \"greedy\" nor \"optimal\""):
        s.hota(matching="best")
    with pytest.raises(ValueError, match="TrackScorer.identity: pairs='optimal' is neither \"best\" nor \"all\""):
        s.identity(pairs="optimal")
    with pytest.raises(ValueError, match="alphas=0 outside"):
        s.hota(alphas=0, matching="optimal")
    big = TS.TrackScorer(streams=2, max_objects=8, max_boxes=8, max_gt_tracks=1405, device="cpu", sweep_frames=4, sweep_records=32, sweep_pairs=64)
    with pytest.raises(ValueError, match="max_gt_tracks=1405 needs \\d+ bytes of LDS per stream for the alignment pass"):
        big.hota(matching="optimal")


# ---- the two host statements -------------------------------------------------------------------------------------------------------
def _same(a, d):
    assert np.array_equal(a["counters"], d["counters"]), np.argwhere(a["counters"] != d["counters"])[:8]
    assert np.array_equal(_bits(a["sums"]), _bits(d["sums"])), np.argwhere(_bits(a["sums"]) != _bits(d["sums"]))[:8]


def test_the_two_host_statements_agree_bit_for_bit():
    logs = list(HO.constructed_logs().values())
    for A in (19, 1):
        _same(HO.host_hota_optimal(logs, A=A), HO.dense_hota_optimal(logs, A=A))
    scores = [W.track_scores(lb)[0] for lb in logs]
    _same(HO.host_hota_optimal(logs, scores, 0.5), HO.dense_hota_optimal(logs, scores, 0.5))
    levels = (0.3, 0.5, 0.6, 0.7)
    for sc, tau in ((None, -math.inf), (scores, 0.5)):
        sparse, dense = HO.host_identity_all(logs, sc, tau, levels), HO.dense_identity_all(logs, sc, tau, levels)
        assert (sparse["idtp"], sparse["idfn"], sparse["idfp"]) == tuple([d[k] for d in dense] for k in ("idtp", "idfn", "idfp"))
    total = 0
    for seed, streams in ((1, 4), (2, 2), (3, 3)):          # the logs of tests/test_track_hota_optimal_gpu.py
        logs = O.random_logs(seed, streams=streams, frames=12, max_dets=12, max_objs=8)
        scores = [W.track_scores(lb)[0] for lb in logs]
        pool = sorted(s for sb in scores for f in sb for s in f)
        for sc, tau in ((None, -math.inf), (scores, pool[len(pool) // 2])):
            a = HO.host_hota_optimal(logs, sc, tau)
            _same(a, HO.dense_hota_optimal(logs, sc, tau))
            tp = a["counters"][:, :, HO.COUNTERS.index("tp")].sum(axis=1)
            assert tp[0] > tp[14] > 0 and a["counters"][0, :, 1].sum() > streams          # levels that differ, resets in the middle
            total += int(tp[0])
            sparse, dense = HO.host_identity_all(logs, sc, tau, levels), HO.dense_identity_all(logs, sc, tau, levels)
            assert (sparse["idtp"], sparse["idfn"], sparse["idfp"]) == tuple([d[k] for d in dense] for k in ("idtp", "idfn", "idfp"))
            best = I.host_identity(logs, sc if sc is not None else None, tau, levels)
            assert all(x >= y for x, y in zip(sparse["idtp"], best["idtp"]))
    assert total > 200


def test_the_truncated_optimum_lies_within_the_stated_bound():
    """On random frames of at most 6 x 6 the quantised optimum times 2^-28 lies within min(P, G) * 2^-28 of the optimum of the float64
    scores; the bound follows from the truncation: every weight is below its score * 2^28 by less than 1, or is the 1 of max(1, ...)."""
    rng = np.random.default_rng(7)
    seen = 0
    for _ in range(300):
        P, G = int(rng.integers(1, 7)), int(rng.integers(1, 7))
        present = rng.random((P, G)) < 0.6
        scores = np.where(present, rng.random((P, G)) * rng.choice([1.0, 1e-3, 1e-9], (P, G)), 0.0)
        edges = [(i, j, HO.score_weight(float(scores[i, j]))) for i in range(P) for j in range(G) if present[i, j]]
        if not edges:
            continue
        seen += 1
        got, cp = O.la_solve(P, G, edges)
        assert got == O.independent_solve(P, G, edges)[0]
        bound = min(P, G) * 2.0 ** -28
        assert abs(got * 2.0 ** -28 - HO.float_optimum(scores)) <= bound
        # and the float score of the matching found is within the bound of the untruncated optimum
        found = sum(float(scores[i, j]) for j, i in enumerate(cp) if i >= 0)
        assert HO.float_optimum(scores) - found <= bound
    assert seen > 250


# ---- the constructed cases ---------------------------------------------------------------------------------------------------------
def test_the_alignment_case():
    clip = HO.alignment_case()
    e = clip[2]
    sims = {(i, j): s for i, j, s in HO.valid_pairs(e, [0.0, 0.0], -math.inf)}
    assert sims == {(0, 0): 15 / 25, (1, 0): 16 / 24} and sims[(0, 0)] == 3 / 5 == 12 / 20 < 13 / 20 < sims[(1, 0)]
    # an IoU-only optimal matching of that frame takes the intruder, detection 1
    _, cp = O.la_solve(2, 1, [(i, j, HO.score_weight(s)) for (i, j), s in sims.items()])
    assert cp == [1]
    # the statement takes detection 0: the track that follows the object through the clip
    host = HO.host_hota_optimal([clip])
    tr = host["trace"][0][2]
    assert tr["cp"] == [0] and tr["A"][(5, 1)] > 0.7 and tr["A"][(5, 2)] < 0.2
    tp = host["counters"][:, 0, HO.COUNTERS.index("tp")]
    assert tp[11] == 4 and tp[12] == 0          # 3/5 counts at 12/20; at 13/20 no frame has a true positive, frame 2 included
    assert all(t["cp"] == [0] for t in host["trace"][0])
    # the greedy rule finds frame 2's intruder at 13/20, and its HOTA differs
    greedy = H.host_hota([clip])
    assert greedy["counters"][12, 0, H.COUNTERS.index("tp")] == 1
    assert TS.hota_values(host["counters"], host["sums"])["hota"] != greedy["hota"]
    # after a reset the one-frame clip takes the intruder: no score crosses the reset
    leak = HO.host_hota_optimal([HO.leak_case()])["trace"][0]
    assert [t["cp"] for t in leak] == [[0], [0], [0], [0], [1]] and leak[4]["A"] != leak[0]["A"]


def test_the_identity_case():
    clip = HO.identity_case()
    every, best = HO.host_identity_all([clip]), I.host_identity([clip])
    assert every["idtp"] == [3] and best["idtp"] == [2] and every["pairs"] == [2] and every["gt"] == best["gt"] == [6]
    n, _, _ = HO.clip_pairs_all([(e, [0.0]) for e in clip], -math.inf, 0.5)
    assert n == {(1, 7): 2, (2, 7): 3}


def test_the_other_constructed_cases():
    cases = HO.constructed_logs()
    # the threshold removes track 10, which changes k of object 1 and with it A of (1, 11)
    clip = cases["threshold"]
    scores = W.track_scores(clip)[0]
    assert scores[0] == [0.125, 0.875]
    with_all, without = HO.clip_alignment(list(zip(clip, scores)), -math.inf)[0], HO.clip_alignment(list(zip(clip, scores)), 0.5)[0]
    assert set(with_all) == {(1, 10), (2, 10), (1, 11)} and set(without) == {(1, 11)} and with_all[(1, 11)] != without[(1, 11)]
    # the clamp: IoU 3 enters r, k and the weight as 1 and LocA as 3
    host = HO.host_hota_optimal([cases["clamp"]])
    assert host["trace"][0][0]["sims"][(0, 0)] == 3.0 and host["trace"][0][0]["cp"] == [0]
    assert host["sums"][18, 0, HO.SUMS.index("loc")] == 6.0 and max(w for _, _, w in host["trace"][0][0]["edges"]) <= HO.ONE
    # the tie: two edges of one weight, the smaller column wins
    tr = HO.host_hota_optimal([cases["tie"]])["trace"][0][0]
    assert tr["edges"][0][2] == tr["edges"][1][2] and tr["cp"] == [0, -1] and tr["sims"] == {(0, 0): 1.0, (0, 1): 3.0}
    # the overflow frames are what the GPU tests take them for
    edge, pair = HO.edge_overflow_frame(), HO.pair_overflow_frame()
    assert len(HO.valid_pairs(edge, [0.0] * 65, -math.inf)) == TS.PAIR_EDGES + 1
    assert len({(edge["labels"][j], edge["dets"][i][0]) for i, j, _ in edge["pairs"]}) == 512 <= TS.ALIGN_PAIRS
    assert len({(pair["labels"][j], pair["dets"][i][0]) for i, j, _ in pair["pairs"]}) == 1088 > TS.ALIGN_PAIRS and len(pair["pairs"]) <= TS.PAIR_EDGES
