"""CPU: the native surface and the host half of the batched tracker's exact association (include/rtk_fused.h rtk_associate_optimal,
csrc/track_assign.hip, csrc/lds_assignment.h la_solve_dense, ratrack_amd/tracker.py `BatchedTracker(assign="optimal")`) -- the entry
point is declared, bound, built for gfx950 without scratch and exported; its LDS at the largest K is within the limit; the host
solvers of tests/_track_assign_util.py agree on every case table; every case whose decisions the GPU test compares has a unique optimum;
the statement differs from mutual-best, from greedy, from an fp32 gate and from rounding where it must; the keywords are validated."""
import ctypes
import os
import re

import numpy as np
import pytest

import _track_assign_util as U
from _util import kernel_notes
from ratrack_amd import _lib, abi, build as B
from ratrack_amd import tracker as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMAX = 197


# ---- the native surface ------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_point():
    text = open(os.path.join(ROOT, "include", "rtk_fused.h")).read()
    assert re.search(r"RTK_EXPORT int rtk_associate_optimal\(int B, int N, int K, const unsigned char \*active, const unsigned char \*reset, "
                     r"const float \*aff,", text)
    assert re.search(r"double min_affinity, int \*counter,", text) and re.search(r"long long \*total, rtk_stream_t stream\);", text)
    assert re.search(r"RTK_EXPORT int rtk_associate_optimal_lds_bytes\(int K\);", text)
    lib = ctypes.CDLL(B.build(verbose=False))
    for name, nargs in (("rtk_associate_optimal", 21), ("rtk_associate_optimal_lds_bytes", 1)):
        assert hasattr(lib, name) and len(abi.SIGNATURES[name]) == nargs, name
    assert abi.SIGNATURES["rtk_associate_optimal"][10] is ctypes.c_double
    # every sentence of the contract that the GPU test asserts is in the header
    for word in ("(double)aff[b][i][j] >= min_affinity", "A NaN is not admissible", "(int)(aff * 268435456.0f)", "2 684 354",
                 "that total is unique", "ties go to the smaller column index", "Plain stores only", "untouched for an inactive stream",
                 "aff is read inside the live (m_b, n_b) block only"):
        assert word in text, word
    for name in ("track_assign.hip", "lds_assignment.h"):
        code = re.sub(r"//[^\n]*", "", open(os.path.join(B.CSRC, name)).read())
        assert "asm" not in code and "atomic" not in code.split("la_solve_dense(int R")[-1], name


def test_the_kernel_builds_for_gfx950_without_scratch_and_states_its_lds(tmp_path):
    found, asm = kernel_notes(os.path.join(B.CSRC, "track_assign.hip"), tmp_path)
    # one kernel, one wave, no scratch, no static LDS: all of it is dynamic and rtk_associate_optimal_lds_bytes states it
    assert len(found) == 1 and "associate_optimal_kernel" in list(found)[0] and list(found.values())[0] == (0, 0, 64, 64), found
    body = re.sub(r";[^\n]*", "", asm)
    assert not re.search(r"^\s+(flat_|scratch_)", body, flags=re.M)          # the tables are addressed as LDS, nothing spills
    lds = _lib._fn("rtk_associate_optimal_lds_bytes")
    assert _lib.load().rtk_track_max_objects() == KMAX
    # the figure, from its parts (ints): the K x K weight block | u [K] | v, dist, way, cp, done [K] each | the new IDs [K]
    for K in (1, 8, 128, KMAX):
        assert lds(K) == 4 * (K * K + K + 5 * K + K), K
    assert 4 * (KMAX * KMAX + KMAX + 5 * KMAX) == 159964 and lds(KMAX) == 160752 <= 160 * 1024
    assert lds(0) == -1 and lds(-3) == -1


def test_entry_point_refuses_before_any_launch():
    fake = 4096          # never dereferenced: every call below is refused on the host
    def call(B_=2, N=16, K=8, aff=fake, gate=0.01):
        _lib.call("rtk_associate_optimal", B_, N, K, None, None, aff, fake, fake, fake, fake, gate, fake, fake, fake, fake, fake, fake, fake,
                  fake, None, None)
    for bad in (0.0, 0.009999, 1.0000001, -1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.RtkError, match="min_affinity="):
            call(gate=bad)
    with pytest.raises(_lib.RtkError, match="K=198 object slots outside \\[1, 197\\]"):
        call(K=KMAX + 1)
    with pytest.raises(_lib.RtkError, match="K=0"):
        call(K=0)
    with pytest.raises(_lib.RtkError, match="bad arguments"):
        call(aff=None)
    with pytest.raises(_lib.RtkError, match="bad arguments"):
        call(B_=0)


# ---- the host statement ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    return [(c,) + U.expected(c) for c in U.cases()]


def test_the_case_table_covers_what_it_must(table):
    shapes = {(c["m"], c["n"]) for c, _, _, _ in table}
    assert set(U.SHAPES) <= shapes
    names = [c["name"] for c, _, _, _ in table]
    assert len(set(names)) == len(names)
    for need in ("two_by_two", "product_64x64", "ties_5x7", "float32_gate", "exactly_at_gate", "nan_inside", "dense_197x197", "diagonal_197x197"):
        assert need in names, need
    assert {c["K"] for c, _, _, _ in table} == {8, 128, KMAX} and all(max(c["m"], c["n"]) <= c["K"] for c, _, _, _ in table)
    for c, w, total, idx in table:
        assert w.shape == (c["m"], c["n"]) and w.min(initial=0) >= 0 and w.max(initial=0) <= U.ONE
        assert ((w == 0) | (w >= 2684354)).all(), c["name"]
        if c["name"].startswith("dense"):
            assert (w > 0).all(), c["name"]                       # everything admissible
    by = {c["name"]: (c, w, total, idx) for c, w, total, idx in table}
    assert by["float32_gate"][1].tolist() == [[0, 0], [0, 2684354]]
    assert by["exactly_at_gate"][1].tolist() == [[U.ONE // 2, 0], [0, int(np.float32(0.6) * np.float32(U.ONE))]]
    assert by["nan_inside"][1][2, 3] == 0 and (by["nan_inside"][1] > 0).sum() == 34
    assert by["two_by_two"][3] == [1, 0] and by["two_by_two"][2] == 2 * int(np.float32(0.8) * np.float32(U.ONE))


def test_the_host_solvers_agree_on_every_case(table):
    for c, w, total, idx in table:
        assert U.check_matching(w, idx) == total, c["name"]
        assert U.fast_total(w) == total, c["name"]
        dev_total, cp, rounds = U.device_method(w)
        assert dev_total == total and U.check_matching(w, cp) == total, c["name"]
        assert rounds <= c["m"] * (c["n"] + 1), c["name"]                     # the counted loops
        if max(c["m"], c["n"]) <= 6:
            assert U.brute_total(w) == total, c["name"]


def test_the_host_solvers_agree_with_scipy(table):
    pytest.importorskip("scipy.optimize")
    for c, w, total, _ in table:
        assert U.scipy_total(w) == total, c["name"]


def test_the_host_solvers_agree_on_random_blocks_with_holes():
    rng = np.random.default_rng(5)
    for k in range(60):
        m, n = int(rng.integers(1, 7)), int(rng.integers(1, 7))
        aff = rng.random((m, n)).astype(np.float32)
        aff[rng.random((m, n)) < 0.3] = 0.001                                  # holes: rows and columns without an edge occur
        if k % 3 == 0:
            aff = np.round(aff * 4) / 4                                          # few distinct values: ties
        w = U.quantise(aff, 0.2)
        total, idx = U.host_solve(w)
        assert total == U.brute_total(w) == U.fast_total(w) == U.device_method(w)[0], (k, w)
        assert U.check_matching(w, idx) == total
        if U.is_unique(w):
            assert U.device_method(w)[1] == idx, (k, w)


def test_every_decision_case_has_a_unique_optimum(table):
    decided = [c["name"] for c, w, _, _ in table if c["decision"]]
    assert len(decided) >= 20 and "product_64x64" in decided and "dense_64x64" in decided
    for c, w, total, idx in table:
        if c["decision"]:
            assert U.is_unique(w), c["name"]
            assert U.device_method(w)[1] == idx, c["name"]
    by = {c["name"]: w for c, w, _, _ in table}
    assert not U.is_unique(by["ties_5x7"])                                       # and is_unique can say no
    assert not U.is_unique(np.array([[5, 5], [5, 5]])) and U.is_unique(np.array([[5, 4], [4, 5]]))
    assert not U.is_unique(np.array([[3, 0], [5, 2]]))                           # 3 + 2 = 5: two matchings of one weight
    # the product matrix is what it is for: searches many columns long
    assert U.device_method(by["product_64x64"])[2] > 4 * U.device_method(by["dense_64x64"])[2]


# ---- teeth -------------------------------------------------------------------------------------------------------------------------
def test_mutual_best_and_greedy_fall_short_on_the_two_by_two():
    w = U.quantise(U.TWO_BY_TWO)
    total, idx = U.host_solve(w)
    assert idx == [1, 0]
    # mutual-best keeps (0, 0) and has nothing left for object 1; greedy takes 0.9 first and is left with the 0.1
    for rule, want in ((U.mutual_best, [0, -1]), (U.greedy, [0, 1])):
        other = rule(U.TWO_BY_TWO)
        assert other == want and U.check_matching(w, other) < total, rule.__name__
    assert U.greedy(U.TWO_BY_TWO, gate=0.5) == [0, -1]


def test_an_fp32_gate_flips_the_float32_case_and_rounding_changes_a_total():
    case = {c["name"]: c for c in U.cases()}["float32_gate"]
    w = U.quantise(case["aff"])
    assert float(U.F32_GATE) < 0.01 <= float(U.F32_ABOVE)
    wrong = U.quantise_fp32_gate(case["aff"])
    assert wrong[0, 0] > 0 and w[0, 0] == 0 and U.host_solve(wrong) != U.host_solve(w)
    assert U.host_solve(wrong)[1] == [0, 1] and U.host_solve(w)[1] == [-1, 1]
    rounded = U.quantise_rounded(case["aff"])
    assert U.host_solve(rounded)[0] == U.host_solve(w)[0] + 1 == 2684355
    # an affinity of 0.5 or more has no bits below 2^-28: nothing to round
    big = np.array([[0.5, 0.75], [0.9, 0.6]], dtype=np.float32)
    assert (U.quantise_rounded(big) == U.quantise(big)).all()


def test_bookkeeping_by_hand():
    aff = np.array([[0.9, 0.8, 0.1], [0.8, 0.1, 0.1]], dtype=np.float32)
    got = U.bookkeeping([1, 0, -1], aff, [41, 42], 7, [0, 0, 2, 1, -1, 3], 4)
    assert got["object_ids"] == [42, 41, 7, -1] and got["indices1"] == [1, 0, -1, -1] and got["counter"] == 8
    assert got["object_conf"].tolist() == [np.float32(0.8), np.float32(0.8), 0.0, 0.0]
    assert got["ids"] == [42, 41, 7] and got["count"] == 3 and got["point_track_id"] == [42, 42, 7, 41, -1, -1]


# ---- the keywords ------------------------------------------------------------------------------------------------------------------
def test_check_assign():
    for ok in (("sinkhorn", 0.01), ("optimal", 0.01), ("optimal", 0.5), ("optimal", 1), ("optimal", 1.0)):
        T.check_assign(*ok)
    for bad in ("hungarian", None, "", "Optimal", 1):
        with pytest.raises(ValueError, match="assign="):
            T.check_assign(bad, 0.01)
    for bad in (0.0, 0.005, 1.5, -0.1, float("nan"), float("inf"), None, "0.5", True):
        with pytest.raises(ValueError, match="min_affinity="):
            T.check_assign("optimal", bad)
    with pytest.raises(ValueError, match="min_affinity=0.5 without assign=\"optimal\""):
        T.check_assign("sinkhorn", 0.5)
    doc = T.BatchedTracker.__init__.__doc__
    assert "`iters` and `alpha` are ignored" in doc and "assign_total" in T.StepResult.__doc__
