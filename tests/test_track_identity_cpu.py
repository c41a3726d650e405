"""CPU: the native surface and the host half of the identity metrics over the scorer's log (include/rtk_score.h,
csrc/track_identity.hip, csrc/lds_assignment.h, ratrack_amd/track_score.py: `TrackScorer.identity`, `identity_values`) -- the entry
points and their constants are declared, built for gfx950 without scratch and exported; `identity_values` is the header's host
arithmetic; the two host forms of tests/_track_identity_util.py agree with each other and with scipy; the planned sequence meets its
numbers and does not need the solver, and the clips of tests/test_track_identity_gpu.py do."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import _track_identity_util as I
import _track_sweep_util as W
from _util import kernel_notes
from ratrack_amd import _lib, abi, build as B
from ratrack_amd import track_score as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOTA_LEVELS = tuple(a / 20 for a in range(1, 20))


# ---- the native surface ------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_identity():
    text = open(os.path.join(ROOT, "include", "rtk_score.h")).read()
    assert re.search(r"RTK_EXPORT int rtk_score_identity_lds_bytes\(int T\);", text)
    assert re.search(r"RTK_EXPORT int rtk_score_identity\(int B, int T, const rtk_score_log_t \*log, const double \*rec_score", text)
    for name, value in (("RTK_SCORE_ID_COUNTERS", len(TS.IDENTITY_COUNTERS)), ("RTK_SCORE_ID_PAIRS", TS.IDENTITY_PAIRS),
                        ("RTK_SCORE_FLAG_IDENTITY", TS.FLAG_IDENTITY)):
        assert re.search(r"#define %s %d\b" % (name, value), text), name
    assert TS.FLAG_IDENTITY == 256 and TS.IDENTITY_PAIRS == 1024
    assert TS.IDENTITY_COUNTERS == I.COUNTERS == ("frames", "clips", "gt", "pred", "idtp", "pairs")
    lib = ctypes.CDLL(B.build(verbose=False))
    assert hasattr(lib, "rtk_score_identity") and hasattr(lib, "rtk_score_identity_lds_bytes")
    assert len(abi.SIGNATURES["rtk_score_identity"]) == 10 and len(abi.SIGNATURES["rtk_score_identity_lds_bytes"]) == 1
    # the definitions are stated with the prototype, and what these numbers are not
    for word in ("THERE IS NO\n *                GREEDY PASS", "MAXIMUM-WEIGHT ONE-TO-ONE MATCHING", "sum cg + sum ct - 2 sum n(matched)",
                 "IDF1 = 2 idtp / (gt + pred)", "box\n * IoU at 0.5: these are NOT those", "only a detection's BEST object"):
        assert word in text, word
    # the solver's contract is written down with it
    solver = open(os.path.join(B.CSRC, "lds_assignment.h")).read()
    for word in ("The contract.", "Exact: integers only", "Bounded:", "no floating point, no scratch, no inline assembly"):
        assert word in solver, word
    assert "asm" not in re.sub(r"//[^\n]*", "", solver)
    for name in ("track_identity.hip", "score_log_walk.h"):          # the kernel's device code lives in both
        assert "asm" not in re.sub(r"//[^\n]*", "", open(os.path.join(B.CSRC, name)).read()), name


def test_identity_kernel_builds_for_gfx950_without_scratch_and_states_its_lds(tmp_path):
    found, _ = kernel_notes(os.path.join(B.CSRC, "track_identity.hip"), tmp_path)
    # one instance per label capacity, each "identity_kernel<capacity>": no scratch, and the LDS the host function reports
    assert len(found) == 2 and all("identity_kernel" in name and v.private == 0 for name, v in found.items()), found
    lds = _lib._fn("rtk_score_identity_lds_bytes")
    small = [v.lds for name, v in found.items() if "identity_kernelILi1024E" in name]
    assert small == [lds(1024)] and lds(1024) <= 65536 and lds(1) == lds(1024), (found, lds(1024))
    large = [v.lds for name, v in found.items() if "identity_kernelILi1024E" not in name]
    assert large == [lds(1025)] and lds(1024) < lds(1025) <= 65536
    assert lds(100000) > 65536 and lds(0) == -1


def test_entry_point_refuses_before_any_launch():
    lg, empty = abi.ScoreLog(4, 32), abi.ScoreLog(4, 32)
    one = (ctypes.c_double * 1)(0.5)
    out = (ctypes.c_longlong * 64)()
    fl = (ctypes.c_int * 4)()
    call = lambda *a: _lib.call("rtk_score_identity", *a)
    # (every pointer is host memory or null: a refusal touches none of them)
    with pytest.raises(_lib.RtkError, match="null or empty log"):
        call(2, 1024, None, None, None, ctypes.addressof(one), 1, ctypes.addressof(out), ctypes.addressof(fl), None)
    with pytest.raises(_lib.RtkError, match="null or empty log"):          # T = 1024 fits
        call(2, 1024, ctypes.addressof(empty), None, None, ctypes.addressof(one), 1, ctypes.addressof(out), ctypes.addressof(fl), None)
    for bad in (0, 64):
        with pytest.raises(_lib.RtkError, match="count=%d" % bad):
            call(2, 1024, ctypes.addressof(lg), None, None, ctypes.addressof(one), bad, ctypes.addressof(out), ctypes.addressof(fl), None)
    with pytest.raises(_lib.RtkError, match="T=100000 label-table entries need \\d+ bytes of LDS per stream, the limit is 65536"):
        call(2, 100000, ctypes.addressof(lg), None, None, ctypes.addressof(one), 1, ctypes.addressof(out), ctypes.addressof(fl), None)
    # a log whose tables are all there (host arrays: the refusal comes before any of them is read) and a null output
    keep = [(ctypes.c_int * 8)() for _ in range(5)] + [(ctypes.c_float * 8)(), (ctypes.c_double * 8)()]
    full = abi.ScoreLog(4, 8, None, *(ctypes.addressof(k) for k in keep))
    with pytest.raises(_lib.RtkError, match="null output"):
        call(2, 1024, ctypes.addressof(full), None, None, ctypes.addressof(one), 1, None, ctypes.addressof(fl), None)
    with pytest.raises(_lib.RtkError, match="null output"):
        call(2, 1024, ctypes.addressof(full), None, None, ctypes.addressof(one), 1, ctypes.addressof(out), None, None)


def test_identity_refusals():
    plain = TS.TrackScorer(streams=2, max_objects=8, max_boxes=8, device="cpu")
    with pytest.raises(RuntimeError, match="TrackScorer.identity: the scorer keeps no log"):
        plain.identity()
    s = TS.TrackScorer(streams=2, max_objects=8, max_boxes=8, device="cpu", sweep_frames=4, sweep_records=32)
    for bad in ((), [0.5] * 64, 0.0, 1.5, float("nan"), (0.5, 0.0), (0.5, float("inf")), -0.25):
        with pytest.raises(ValueError, match="alphas="):
            s.identity(alphas=bad)
    with pytest.raises(RuntimeError, match="TrackScorer.identity: stream 1 has a clip with more than max_gt_tracks=1024 label ids, 2048 track ids or "
                                           "1024 \\(label id, track id\\) pairs"):
        s._raise_on_flags([0, TS.FLAG_IDENTITY])


# ---- identity_values ---------------------------------------------------------------------------------------------------------------
def test_identity_values_against_hand_numbers():
    #              frames clips gt pred idtp pairs
    c = np.array([[[6, 1, 18, 16, 14, 4]],
                  [[6, 1, 18, 16, 0, 0]],
                  [[0, 0, 0, 0, 0, 0]]], dtype=np.int64)
    v = TS.identity_values(c, (0.5, 0.75, 1.0))
    assert v["alpha"].tolist() == [0.5, 0.75, 1.0]
    assert v["idtp"].tolist() == [14, 0, 0] and v["idfn"].tolist() == [4, 18, 0] and v["idfp"].tolist() == [2, 16, 0]
    assert v["gt"].tolist() == [18, 18, 0] and v["pred"].tolist() == [16, 16, 0] and v["pairs"].tolist() == [4, 0, 0]
    assert v["idf1"][0] == 28 / 34 and v["idr"][0] == 14 / 18 and v["idp"][0] == 14 / 16
    assert v["idf1"][1] == 0.0 and v["idr"][1] == 0.0 and v["idp"][1] == 0.0
    assert all(np.isnan(v[k][2]) for k in ("idf1", "idr", "idp"))                 # all-zero counters: no denominator
    # the streams are pooled before any ratio
    two = np.concatenate([c, c[::-1]], axis=1)
    w = TS.identity_values(two, (0.5, 0.75, 1.0))
    assert w["idtp"].tolist() == [14, 0, 14] and w["idf1"][0] == 28 / 34 and w["idf1"][1] == 0.0 and w["gt"].tolist() == [18, 36, 18]
    none = TS.identity_values(c[:, :0], (0.5, 0.75, 1.0))
    assert none["idtp"].tolist() == [0, 0, 0] and np.isnan(none["idf1"]).all()
    for bad in ((c[:, :, :5], (0.5, 0.75, 1.0)), (c, (0.5,)), (c[0], (0.5,))):
        with pytest.raises(ValueError, match="identity_values"):
            TS.identity_values(*bad)


# ---- the host statement ----------------------------------------------------------------------------------------------------------------
def _random_logs(seed=5, streams=4):
    rng = np.random.default_rng(seed)
    return [[e for k in range(3) for e in I.random_clip(rng, *I.RANDOM_SHAPES[(b + k) % 3], ious=(0.3, 0.6, 0.9))] for b in range(streams)]


def _forms_agree(logs, scores, tau, alphas, scipy=False):
    fast, mat = I.host_identity(logs, scores, tau, alphas), I.matrix_identity(logs, scores, tau, alphas, scipy=scipy)
    for a, m in enumerate(mat):
        assert (m["idtp"], m["idfn"], m["idfp"]) == (fast["idtp"][a], fast["idfn"][a], fast["idfp"][a]), (a, m, fast["idtp"][a])
    return fast


def test_own_solver_on_small_cases():
    assert I.max_weight({}) == 0 and I.max_weight({("A", 1): 5, ("A", 2): 4, ("B", 1): 4}) == 8
    assert I.greedy_weight({("A", 1): 5, ("A", 2): 4, ("B", 1): 4}) == 5
    assert I.max_weight({(g, 0): g + 1 for g in range(5)}) == 5 and I.max_weight({(0, t): t + 1 for t in range(5)}) == 5
    assert I.min_assignment([[4, 1, 3], [2, 0, 5]]) == [1, 0]


@pytest.mark.parametrize("filtered", [False, True])
def test_fast_and_matrix_forms_agree(filtered):
    _, _, logs, sw = W.planned()
    scores, tau = (sw["scores"], float(sw["thresholds"][sw["best"]])) if filtered else (None, -math.inf)
    fast = _forms_agree(logs, scores, tau, (0.05, 0.5, 0.8))
    assert fast["idtp"][0] > fast["idtp"][2] > 0
    rnd = _random_logs()
    scores = [W.track_scores(lb)[0] for lb in rnd] if filtered else None
    tau = float(np.median([s for sb in scores for f in sb for s in f])) if filtered else -math.inf
    fast = _forms_agree(rnd, scores, tau, (0.3, 0.5, 0.7))
    assert fast["idtp"][0] > fast["idtp"][1] > fast["idtp"][2] > 0


def test_both_forms_agree_with_scipy():
    pytest.importorskip("scipy.optimize")
    _, _, logs, sw = W.planned()
    _forms_agree(logs, None, -math.inf, (0.05, 0.5), scipy=True)
    _forms_agree(logs, sw["scores"], float(sw["thresholds"][sw["best"]]), (0.5,), scipy=True)
    _forms_agree(_random_logs(), None, -math.inf, (0.3, 0.5, 0.7), scipy=True)
    for sticky in (False, True):
        _forms_agree([I.dense_clip(sticky=sticky, frames=64)], None, -math.inf, (0.5,), scipy=True)


def test_planned_sequence_meets_its_numbers_and_does_not_need_the_solver():
    _, _, logs, sw = W.planned()
    h = I.host_identity(logs, alphas=(0.5, 0.05))
    assert len(logs) == 16 and int(h["counters"][0, :, I.COUNTERS.index("clips")].sum()) == 22
    assert (h["gt"][0], h["pred"][0], h["idtp"][0]) == (363, 617, 229) and h["idf1"][0] == 458 / 980
    assert h["idtp"][1] == 262 and h["gt"][1] == 363 and h["pred"][1] == 617
    assert sw["best"] == 9 and sw["thresholds"][9] == 0.55234375
    f = I.host_identity(logs, sw["scores"], 0.55234375, alphas=(0.5, 0.05))
    assert (f["gt"][0], f["pred"][0], f["idtp"][0]) == (363, 149, 54) and f["idtp"][1] == 118
    # heaviest pair first already reaches the optimum in every one of its clips: this sequence cannot tell a solver from a greedy pairing
    for res in (h, f):
        for a in range(2):
            assert len(res["clips"][a]) == 22 and all(best == greedy for best, greedy, _ in res["clips"][a])
    # the counts that do not depend on the level
    for k in ("frames", "clips", "gt", "pred"):
        i = I.COUNTERS.index(k)
        assert (h["counters"][0, :, i] == h["counters"][1, :, i]).all(), k


def test_the_gpu_tests_clips_beat_a_greedy_pairing():
    """The inputs of tests/test_track_identity_gpu.py must be able to fail: heaviest pair first falls short of the optimum in at least
    a quarter of the generator's clips (600 of them, 200 of each shape: 47, 94 and 127 with this seed), and in both dense clips."""
    rng = np.random.default_rng(1)
    total = 0
    for n, frames in I.RANDOM_SHAPES:
        short = 0
        for _ in range(200):
            clip = I.random_clip(rng, n, frames)
            pairs, _, _ = I.clip_pairs([(e, [0.0] * len(e["dets"])) for e in clip], -math.inf, 0.5)
            best, greedy = I.max_weight(pairs), I.greedy_weight(pairs)
            assert greedy <= best
            short += greedy < best
        print("n %d, %d frames: heaviest-pair-first below the optimum in %d of 200 clips" % (n, frames, short))
        total += short
    assert total >= 600 // 4, total
    for sticky in (False, True):
        (best, greedy, pairs), = I.host_identity([I.dense_clip(sticky=sticky)])["clips"][0]
        print("dense clip, sticky %s: %d pairs, optimum %d, heaviest-pair-first %d" % (sticky, pairs, best, greedy))
        assert greedy < best and (pairs == 1024 if not sticky else 900 < pairs <= 1024)
