"""CPU: the native surface and the host half of TrackEval's centre-distance similarity on the pair log (include/rtk_score.h, the last
section; csrc/track_score.hip and the three replay files; ratrack_amd/track_score.py: `TrackScorer(similarity="centre")`) -- the
entry points are declared, mirrored in abi.py, built for gfx950 and exported; the producer builds as exactly two kernels without scratch
and without static LDS; the similarity replays build without scratch, as one wave of 64 threads, with the static LDS of their plain
counterparts; the entry points refuse before any launch; `check_similarity` validates the keywords; the host statement of
tests/_track_centre_util.py agrees with its dense (TrackEval-form) twin."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import _track_centre_util as C
import _track_hota_optimal_util as HO
import _track_optimal_util as O
from _util import SCORE_VARIANTS, kernel_notes, score_kernel_notes, template_flags
from ratrack_amd import _lib, abi, build as B
from ratrack_amd import track_score as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 65536
SIM_ENTRY_POINTS = (("rtk_score_replay_optimal_sim", 16), ("rtk_score_alignment_sim", 13), ("rtk_score_hota_optimal_sim", 15),
                    ("rtk_score_identity_pairs_sim", 12))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


# ---- the native surface ------------------------------------------------------------------------------------------------------------
def test_header_declares_binding_mirrors_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "rtk_score.h")).read()
    assert re.search(r"RTK_EXPORT int rtk_track_score_pairs_centre\(const rtk_track_score_in_t \*in,", text)
    assert re.search(r"const rtk_score_pairs_t \*pairs, double \*pair_sim /\* \(B,Q\) \*/, const double \*gt_centre /\* \(B,K,3\) \*/,\s+double zero_distance, rtk_stream_t stream\);", text)
    assert re.search(r"RTK_EXPORT int rtk_track_score_centre_lds_bytes\(int Kobj, int K, int N, int memory", text)
    lib = ctypes.CDLL(B.build(verbose=False))
    for name, nargs in (("rtk_track_score_pairs_centre", 10), ("rtk_track_score_centre_lds_bytes", 4)) + SIM_ENTRY_POINTS:
        assert re.search(r"RTK_EXPORT int %s\(" % name, text), name
        assert hasattr(lib, name) and len(abi.SIGNATURES[name]) == nargs, name
    # each similarity replay takes its plain counterpart's arguments plus pair_sim, right behind the pair log
    for name, _ in SIM_ENTRY_POINTS:
        plain, sim = abi.SIGNATURES[name[:-4]], abi.SIGNATURES[name]
        at = 4 if name != "rtk_score_hota_optimal_sim" else 3
        assert sim == plain[:at] + [ctypes.c_void_p] + plain[at:], name
    assert abi.SIGNATURES["rtk_track_score_pairs_centre"] == abi.SIGNATURES["rtk_track_score_pairs"][:6] + [ctypes.c_void_p, ctypes.c_void_p,
                                                                                                              ctypes.c_double, ctypes.c_void_p]
    # the definitions are stated with the prototypes
    for word in ("_calculate_euclidean_similarity", "d2 = (dx * dx + dy * dy) + dz * dz", "s = 1.0 - d / zero_distance", "logged iff s > 0.0",
                 "a NaN is not logged", "may now be 0", "DEPARTURES FROM TrackEval AFTER THIS", "point\n * centroids rather than label-box centres",
                 "(1 << 23) + min(floor(s * 65536), 65536)", "ONE similarity"):
        assert word in text, word
    for name in ("track_score.hip", "track_optimal.hip", "track_hota_optimal.hip", "track_identity_pairs.hip", "track_score_body.h",
                 "track_optimal_body.h", "track_hota_optimal_body.h", "track_identity_pairs_body.h"):
        code = re.sub(r"//[^\n]*", "", open(os.path.join(B.CSRC, name)).read())
        assert "asm" not in code and not re.search(r"atomic\w*\s*\(\s*&?\s*\w*(pair_sim|gpos|pmc|rsum|ksum|quot|miou|cq)\b", code), name


def test_the_producer_builds_as_two_kernels_without_scratch_and_without_static_lds(tmp_path):
    ts = score_kernel_notes(tmp_path)                # the ten instantiations of the one scoring kernel, and no other
    assert [k for k, flags in SCORE_VARIANTS.items() if flags[3]] == ["centre", "centre_memory"]       # CENTRE: without and with the memory block
    assert all((ts[k].private, ts[k].lds) == (0, 0) for k in ("centre", "centre_memory")), ts
    # dynamic LDS: the plain figure rounded up to 8 bytes, plus the kept objects' positions, zero_distance and one address
    plain, memory, centre = (_lib._fn(n) for n in ("rtk_track_score_lds_bytes", "rtk_track_score_memory_lds_bytes", "rtk_track_score_centre_lds_bytes"))
    for Kobj, K, N in ((16, 8, 96), (7, 5, 33), (64, 40, 128), (128, 32, 256), (256, 64, 1)):
        up = lambda x: (x + 7) // 8 * 8
        assert centre(Kobj, K, N, 0) == up(plain(Kobj, K, N)) + 24 * K + 16 and centre(Kobj, K, N, 1) == up(memory(Kobj, K, N)) + 24 * K + 16
    assert centre(0, 8, 96, 0) == -1 and centre(16, 65, 96, 0) == -1 and centre(16, 8, 0, 1) == -1


def test_the_similarity_replays_build_without_scratch_as_one_wave_with_their_counterparts_lds(tmp_path):
    found = {}
    for name in ("track_optimal.hip", "track_hota_optimal.hip", "track_identity_pairs.hip"):
        found.update(kernel_notes(os.path.join(B.CSRC, name), tmp_path)[0])
    assert len(found) == 14, sorted(found)
    assert all(v.private == 0 and (v.wavefront, v.max_threads) == (64, 64) and 0 < v.lds <= LIMIT for v in found.values()), found
    # a similarity kernel is its counterpart's template with the switch on (optimal_replay_kernel<1024, true> for <1024, false>, ...)
    key = lambda n: re.search(r"_Z\d+(\w+?)_kernelI(?:Li(\d+)E)?Lb[01]EEv", n).groups()
    sim = {key(n): v for n, v in found.items() if template_flags(n) == (True,)}
    plain = {key(n): v for n, v in found.items() if template_flags(n) == (False,)}
    assert len(sim) == 7 and sorted(sim) == sorted(plain)
    assert all(plain[k].lds == v.lds for k, v in sim.items()), found


def test_entry_points_refuse_before_any_launch():
    keep = [(ctypes.c_int * 64)() for _ in range(5)] + [(ctypes.c_float * 64)(), (ctypes.c_double * 64)()]
    full, bare = abi.ScoreLog(4, 8, None, *(ctypes.addressof(k) for k in keep)), abi.ScoreLog(4, 32)
    pk = [(ctypes.c_int * 64)() for _ in range(6)]
    pairs, empty = abi.ScorePairs(16, *(ctypes.addressof(k) for k in pk)), abi.ScorePairs(16)
    dbl, out, ints = (ctypes.c_double * 64)(), (ctypes.c_longlong * 64)(), (ctypes.c_int * 64)()
    a = lambda x: None if x is None else ctypes.addressof(x)
    # (every pointer is host memory or null: a refusal touches none of them)

    def replay(T=1024, log=full, pr=pairs, sim=dbl, count=1, min_iou=0.5):
        _lib.call("rtk_score_replay_optimal_sim", 2, T, a(log), a(pr), a(sim), a(dbl), a(dbl), None, count, min_iou, a(out), a(out), a(dbl), None,
                  a(ints), None)

    def align(T=1024, log=full, pr=pairs, sim=dbl):
        _lib.call("rtk_score_alignment_sim", 2, T, a(log), a(pr), a(sim), None, None, a(dbl), a(ints), a(ints), a(ints), a(ints), None)

    def match(alphas=19, log=full, pr=pairs, sim=dbl):
        _lib.call("rtk_score_hota_optimal_sim", 2, a(log), a(pr), a(sim), None, None, alphas, a(dbl), a(ints), a(ints), a(ints), a(out), a(dbl), a(ints),
                  None)

    def ident(T=1024, log=full, pr=pairs, sim=dbl, count=1):
        _lib.call("rtk_score_identity_pairs_sim", 2, T, a(log), a(pr), a(sim), None, None, a(dbl), count, a(out), a(ints), None)
    for call in (replay, align, match, ident):
        with pytest.raises(_lib.RtkError, match="_sim: null or empty log"):
            call(log=bare)
        with pytest.raises(_lib.RtkError, match="_sim: null or empty pair log"):
            call(pr=empty)
        with pytest.raises(_lib.RtkError, match="_sim: null pair_sim"):
            call(sim=None)
    with pytest.raises(_lib.RtkError, match="score_replay_optimal_sim: T=1304 track-table entries need"):
        replay(T=1304)
    for bad in (0.0, float("nan"), float("inf")):
        with pytest.raises(_lib.RtkError, match="min_iou="):
            replay(min_iou=bad)
    with pytest.raises(_lib.RtkError, match="score_alignment_sim: T=1405 label-table entries need"):
        align(T=1405)
    with pytest.raises(_lib.RtkError, match="alphas=64"):
        match(alphas=64)
    with pytest.raises(_lib.RtkError, match="score_identity_pairs_sim: T=3584 label-table entries need"):
        ident(T=3584)

    # the producer: the three refusals of its own come first, then rtk_track_score_pairs' checks
    blocks = [abi.ScoreIn(2, 64, 8, 8, 16), abi.ScoreState(), abi.ScoreOut()]

    def produce(blocks=blocks, log=full, pr=pairs, sim=dbl, centre=dbl, zero_distance=2.0):
        i, s, o = (None, None, None) if blocks is None else (a(x) for x in blocks)
        _lib.call("rtk_track_score_pairs_centre", i, s, o, a(log), None, a(pr), a(sim), a(centre), zero_distance, None)
    with pytest.raises(_lib.RtkError, match="null argument block"):
        produce(blocks=None)
    with pytest.raises(_lib.RtkError, match="null log block"):
        produce(log=None)
    with pytest.raises(_lib.RtkError, match="null pair-log block"):
        produce(pr=None)
    with pytest.raises(_lib.RtkError, match="null pair_sim"):
        produce(sim=None)
    with pytest.raises(_lib.RtkError, match="null gt_centre"):
        produce(centre=None)
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(_lib.RtkError, match="zero_distance=.* must be finite and above 0"):
            produce(zero_distance=bad)
    with pytest.raises(_lib.RtkError, match="track_score: null input"):          # everything of its own in order: the shared checks refuse
        produce()


# ---- the keywords ------------------------------------------------------------------------------------------------------------------
def test_check_similarity_and_the_keywords():
    assert TS.check_similarity() == ("iou", None) and TS.check_similarity("iou", None, 64) == ("iou", None)
    assert TS.check_similarity("centre", None, 64) == ("centre", 2.0) and TS.check_similarity("centre", 0.5, 64) == ("centre", 0.5)
    assert TS.check_similarity("centre", np.float32(3.0), 1) == ("centre", 3.0)
    with pytest.raises(ValueError, match="zero_distance=2.0 goes with similarity=\"centre\""):
        TS.check_similarity("iou", 2.0, 64)
    with pytest.raises(ValueError, match="similarity=\"centre\" lives in the pair log \\(give sweep_pairs"):
        TS.check_similarity("centre", None, None)
    for bad in ("box", "Centre", None, 1):
        with pytest.raises(ValueError, match="is neither \"iou\" nor \"centre\""):
            TS.check_similarity(bad, None, 64)
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="must be finite and above 0"):
            TS.check_similarity("centre", bad, 64)
    with pytest.raises(ValueError, match="is not a number"):
        TS.check_similarity("centre", "far", 64)
    # the constructor runs the same checks before it allocates anything (device="nowhere" would fail at the first tensor)
    with pytest.raises(ValueError, match="lives in the pair log"):
        TS.TrackScorer(streams=2, max_objects=8, max_boxes=8, device="nowhere", sweep_frames=4, sweep_records=32, similarity="centre")
    with pytest.raises(ValueError, match="goes with similarity=\"centre\""):
        TS.TrackScorer(streams=2, max_objects=8, max_boxes=8, device="nowhere", zero_distance=2.0)
    kw = dict(streams=2, max_objects=8, max_boxes=8, device="cpu", sweep_frames=4, sweep_records=32, sweep_pairs=64)
    plain, centre = TS.TrackScorer(**kw), TS.TrackScorer(similarity="centre", zero_distance=3, **kw)
    assert (plain.similarity, plain.zero_distance, plain.centre) == ("iou", None, False) and not hasattr(plain, "pair_sim")
    assert (centre.similarity, centre.zero_distance, centre.centre) == ("centre", 3.0, True)
    assert centre.pair_sim.shape == (2, 64) and str(centre.pair_sim.dtype) == "torch.float64" and not centre.pair_sim.any()
    # the distance a similarity stands for
    assert TS.similarity_distance(1.0, 2.0) == 0.0 and TS.similarity_distance(0.5, 2.0) == 1.0 and TS.similarity_distance(0.25, 4.0) == 3.0
    assert np.array_equal(TS.similarity_distance([0.0, 0.75], 2.0), [2.0, 0.5])
    # a configuration the plain scorer takes and the centre variant's positions push over the LDS limit is refused by name
    fits = dict(max_boxes=64, points=1446, max_objects=64)
    TS.check_fit(**fits)
    with pytest.raises(ValueError, match="need \\d+ bytes of LDS per stream, the limit is 65536"):
        TS.check_fit(centre=True, **fits)


# ---- the host statement -------------------------------------------------------------------------------------------------------------
def test_centres_add_in_column_order_and_the_similarity_is_the_dense_forms():
    pc = np.zeros((3, 6), np.float32)
    pc[0] = [1e7 / 3, 1.0 / 3, 1e-7 / 3, -1e7 / 7, 1.0 / 7, 1e-7 / 7]      # (float32 values 1e4 .. 1e-4 apart add exactly in float64)
    c = C.centre_of(pc, [0, 1, 2, 3, 4, 5])
    x = y = 0.0
    for v in pc[0]:
        x += float(v)
    for v in pc[0][::-1]:
        y += float(v)
    assert c[0] == x / 6.0 and x != y                           # the sum in column order: another order gives other bits
    assert C.centre_of(pc, [1])[0] == float(np.float32(1.0 / 3)) and C.centre_of(pc, [0, 0])[0] == float(np.float32(1e7 / 3))
    # exact cases: offsets whose squares are powers of four
    g = np.zeros(3)
    assert C.similarity([0, 0, 0], g) == 1.0 and C.similarity([0, 1, 0], g) == 0.5 and C.similarity([0, 0, 2], g) == 0.0
    assert C.similarity([0.5, 0, 0], g) == 0.75 and C.similarity([0, 0, 4], g, 8.0) == 0.5 and C.similarity([9, 0, 0], g) < 0.0
    assert not C.similarity([float("nan"), 0, 0], g) > 0.0
    # against TrackEval's matrix form: the same pairs have s > 0 (none within 1e-9 of the rim here), the values agree to rounding
    rng = np.random.default_rng(5)
    a, b = rng.normal(size=(40, 3)) * 1.5, rng.normal(size=(30, 3)) * 1.5
    dense = C.dense_similarity(a, b)
    sparse = np.array([[C.similarity(x, y) for y in b] for x in a])
    assert np.abs(sparse).min() > 1e-9 and np.array_equal(dense > 0, sparse > 0) and 100 < (dense > 0).sum() < 1100
    assert np.allclose(dense, np.maximum(sparse, 0.0), rtol=0, atol=4 * np.finfo(np.float64).eps)


def test_the_frame_pair_list_and_the_fit_rule():
    frames = C.scenario(7)
    fr = frames[0]
    pairs, sims = C.frame_pairs(fr["pc1"][3], fr["obj"][3], int(fr["n_valid"][3]), int(fr["num"][3]), fr["members"][3], fr["centre"][3], int(fr["count"][3]))
    assert pairs == sorted(pairs) and len(pairs) == len(sims) > 0 and all(0.0 < s <= 1.0 for s in sims)
    P, G = int(fr["num"][3]), int(fr["count"][3])
    assert len(pairs) < P * G                                   # some positions are out of reach
    log = C.host_pair_log(frames, 4, 8, 256, 4096)
    zero = sum(1 for b in range(4) for ps, _ in log["entries"][b] for _, _, c in ps if c == 0)
    some = sum(1 for b in range(4) for ps, _ in log["entries"][b] for _, _, c in ps if c > 0)
    assert zero > 0 and some > 0 and not log["dropped"].any() and log["frames"].tolist() == [3, 3, 2, 3]
    # stream 2's detection 1 has no live column: no pair of any frame names it; stream 0's frame 1 has no detection, stream 1's no object
    assert all(i != 1 for ps, _ in log["entries"][2] for i, _, _ in ps)
    assert log["pair_frame"][0, 1, 1] == 0 and log["pair_frame"][1, 1, 1] == 0
    # a pair log that is too small drops whole frames and keeps later, smaller ones
    small = C.host_pair_log(frames, 4, 8, 256, int(log["pair_frame"][3, 0, 1]) + 1)
    assert small["dropped"].any() and (small["frames"] <= log["frames"]).all() and small["pair_cursor"][3] == log["pair_frame"][3, 0, 1]


@pytest.mark.parametrize("seed", [1, 2])
def test_the_replays_on_a_similarity_log_agree_with_their_dense_twins(seed, monkeypatch):
    logs = C.with_sims(O.random_logs(seed, streams=3, frames=10, max_dets=8, max_objs=6), seed)
    iou_hota = HO.host_hota_optimal(logs)                      # before the substitution: the point IoU of the integers
    C.patch_similarity(monkeypatch)
    sparse, dense = HO.host_hota_optimal(logs), HO.dense_hota_optimal(logs)
    assert np.array_equal(sparse["counters"], dense["counters"]) and np.array_equal(_bits(sparse["sums"]), _bits(dense["sums"]))
    assert sparse["counters"][0, :, HO.COUNTERS.index("tp")].sum() > 0 and not np.array_equal(sparse["counters"], iou_hota["counters"])
    levels = (0.25, 0.5, 0.75)
    ids, dense_ids = HO.host_identity_all(logs, alphas=levels), HO.dense_identity_all(logs, alphas=levels)
    assert [int(v) for v in ids["idtp"]] == [d["idtp"] for d in dense_ids] and ids["idtp"][0] > ids["idtp"][2] >= 0
    # the per-frame optimal matching: the unique quantities of every frame against an independent solver, ties included
    scores = [[[0.0] * len(e["dets"]) for e in lb] for lb in logs]
    for min_iou in (0.25, 0.5):
        for lb, sb in zip(logs, scores):
            _, _, _, _, cps = O.replay(lb, sb, -math.inf, min_iou)
            for e, sc, cp in zip(lb, sb, cps):
                _, edges, ious = O.frame_edges(e, sc, -math.inf, min_iou)
                assert all(v >= min_iou for v in ious.values()) and len(edges) == sum(1 for s in e["sims"] if s >= min_iou)
                assert sum(w for i, j, w in edges if cp[j] == i) == O.independent_solve(len(e["dets"]), len(e["labels"]), edges)[0]
    # pairs exactly at a level count at it; a pair whose common count is 0 is a pair like any other
    at_half = sum(1 for lb in logs for e in lb for s in e["sims"] if s == 0.5)
    assert at_half > 0 and any(c == 0 and s >= 0.5 for lb in logs for e in lb for (_, _, c), s in zip(e["pairs"], e["sims"]))
