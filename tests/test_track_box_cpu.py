"""CPU: the native surface and the host half of the oriented-box IoU on the pair log (include/rtk_score.h, the last section;
csrc/track_score.hip; ratrack_amd/track_score.py: `TrackScorer(similarity="box")` / `"box_bev"`) -- the host statement of
tests/_track_box_util.py against exact rational arithmetic; the keywords and the host-side refusals; header, abi.py and exports; the
producer's code object; the replays on a constructed similarity log against their dense twins; and the bound on pair_sim, measured
again."""
import ctypes
import fractions
import math
import os
import re

import numpy as np
import pytest

import _track_box_util as X
import _track_hota_optimal_util as HO
import _track_optimal_util as O
from _util import SCORE_VARIANTS, score_kernel_notes
from ratrack_amd import _lib, abi, build as B
from ratrack_amd import track_score as TS

F = fractions.Fraction
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T345, T51213, T81517 = (F(3, 5), F(4, 5)), (F(5, 13), F(12, 13)), (F(8, 17), F(15, 17))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _box(c, heading, size):
    return dict(c=tuple(F(v) for v in c), heading=heading, size=tuple(F(v) for v in size))


def _both(det, gt, mode, valid=3):
    """(the float64 statement, the exact value as a float) of one rational pair of boxes."""
    s = X.similarity(X.det_row(det), valid, X.gt_row(gt), mode)
    e = X.exact_iou(det, gt, mode)
    return float(s), float(e)


# ---- the host statement against exact rational arithmetic -----------------------------------------------------------------------------------
def _along(heading, along, across=0):
    """The point `along` the heading and `across` it (to its left), both Fractions."""
    return (along * heading[0] - across * heading[1], along * heading[1] + across * heading[0])


CASES = []
for _h in ((F(1), F(0)), T345, T51213, T81517):
    _o = _along(_h, F(1, 2), F(1, 4))
    CASES += [
        ("identical", _box((1, 2, 0), _h, (4, 2, 1.5)), _box((1, 2, 0), _h, (4, 2, 1.5))),
        ("inside", _box((1 + _o[0], 2 + _o[1], F(1, 8)), _h, (2, 1, 1)), _box((1, 2, 0), _h, (4, 2, 1.5))),
        ("outside", _box((1, 2, 0), _h, (4, 2, 1.5)), _box((1 + _o[0], 2 + _o[1], F(1, 8)), _h, (2, 1, 1))),
        ("offset", _box((1 + _o[0], 2 + _o[1], F(1, 4)), _h, (4, 2, 1.5)), _box((1, 2, 0), _h, (4, 2, 1.5))),
        ("plus", _box((1, 2, 0), (-_h[1], _h[0]), (6, F(1, 2), 1)), _box((1, 2, 0), _h, (6, F(1, 2), 1))),
        ("crossed", _box((F(3, 2), F(5, 2), 0), T51213, (5, 2, 2)), _box((1, 2, F(1, 2)), _h, (4, 3, 2))),
        ("skew", _box((2, 1, 0), T81517, (3, 1, 2)), _box((1, 2, F(1, 4)), (_h[1], _h[0]), (4, 2, 1))),
    ]


@pytest.mark.parametrize("mode", [X.MODE_3D, X.MODE_BEV])
def test_the_statement_agrees_with_exact_rational_arithmetic(mode):
    seen = set()
    for name, det, gt in CASES:
        s, e = _both(det, gt, mode)
        assert abs(s - e) <= X.SIM_BOUND, (name, det["heading"], s, e, s - e)
        assert 0.0 < e <= 1.0 and s > 0.0, (name, s, e)
        seen.add(name)
        if name == "identical":
            assert e == 1.0
        if name in ("inside", "outside"):          # the ratio of the volumes (of the areas)
            assert e == (2 * 1 * (1 if mode == X.MODE_3D else 1)) / (4 * 2 * (1.5 if mode == X.MODE_3D else 1))
        if name == "plus":                         # two 6 x 1/2 bars crossing at right angles share a 1/2 x 1/2 square
            assert e == float(F(1, 4) / (3 + 3 - F(1, 4)))
    assert len(seen) == 7
    # axis-aligned with dyadic coordinates: exact but for the last division
    s, e = _both(_box((1, 0, 0), (F(1), F(0)), (2, 2, 2)), _box((0, 0, 0), (F(1), F(0)), (2, 2, 2)), mode)
    assert s == e == 1.0 / 3.0
    s, e = _both(_box((1, 1, 0), (F(1), F(0)), (2, 2, 2)), _box((0, 0, 0), (F(1), F(0)), (2, 2, 2)), mode)
    assert s == e == 1.0 / 7.0


@pytest.mark.parametrize("mode", [X.MODE_3D, X.MODE_BEV])
def test_touching_boxes_a_gap_in_z_and_boxes_without_extent(mode):
    flat = (F(1), F(0))
    gt = _box((0, 0, 0), flat, (4, 2, 2))
    # touching along an edge (from either side, and a shorter edge on a longer one) and at a corner: exactly 0, so not logged
    for c, size in (((4, 0, 0), (4, 2, 2)), ((-3, 0, 0), (2, 2, 2)), ((0, 2, 0), (4, 2, 2)), ((0, -1.5, 0), (1, 1, 2)), ((1, 1.5, 0), (1, 1, 1)),
                    ((4, 2, 0), (4, 2, 2)), ((-3, -1.5, 0), (2, 1, 2))):
        s, e = _both(_box(c, flat, size), gt, mode)
        assert s == 0.0 and e == 0.0, (c, size, s)
    # the same with both boxes turned by a Pythagorean heading: the exact value is 0, the statement's within the bound of it
    for h in (T345, T51213, T81517):
        g = _box((0, 0, 0), h, (4, 2, 2))
        for along, across in ((4, 0), (0, 2), (4, 2)):
            c = _along(h, F(along), F(across))
            s, e = _both(_box((c[0], c[1], 0), h, (4, 2, 2)), g, mode)
            assert e == 0.0 and abs(s) <= X.SIM_BOUND, (h, along, across, s)
    # overlapping footprints, z ranges apart (and touching in z): 0 in three dimensions, positive in the bird's-eye view
    for z in (2, 5):
        s, e = _both(_box((1, 0, z), T345, (4, 2, 2)), gt, mode)
        assert (s == 0.0 and e == 0.0) if mode == X.MODE_3D else (s > 0.2 and abs(s - e) <= X.SIM_BOUND)
    # a detection of zero width (two points, or collinear points, fitted with min_extent = 0), without points, or with a word that is
    # not finite has no pairs; so has an object with a half-extent 0, without a heading, or with a word that is not finite
    row, grow = X.det_row(_box((0, 0, 0), T345, (4, 2, 2))), X.gt_row(gt)
    assert X.similarity(row, 3, grow, mode) > 0.3
    for k, v in ((4, 0.0), (3, 0.0), (3, -1.0), (0, np.nan), (6, np.inf), (2, np.nan)):
        bad = row.copy()
        bad[k] = v
        assert X.similarity(bad, 3, grow, mode) == 0.0 and X.detection(bad, 3, mode) is None, k
    assert X.similarity(row, 0, grow, mode) == 0.0 and X.similarity(row, -1, grow, mode) == 0.0
    flat_det = row.copy()
    flat_det[5] = 0.0                              # no height: no box in three dimensions, a footprint in the bird's-eye view
    assert (X.similarity(flat_det, 3, grow, mode) == 0.0) == (mode == X.MODE_3D)
    for k, v in ((12, 0.0), (13, 0.0), (14, -1.0), (0, np.nan), (2, np.inf), (3, np.nan)):
        bad = grow.copy()
        bad[k] = v
        assert X.similarity(row, 3, bad, mode) == 0.0 and X.upright(bad) is None, k
    bad = grow.copy()
    bad[3] = bad[6] = 0.0
    assert X.upright(bad) is None
    # the upright reading: a tilt shortens R's first column, the heading is its direction; the pad word and the area word are not read
    tilted = X.gt_row(gt, tilt=0.3)
    tilted[15], row[7] = np.nan, np.nan
    assert abs(float(X.similarity(row, 3, tilted, mode)) - float(X.similarity(row, 3, grow, mode))) <= X.SIM_BOUND


def test_the_bound_is_measured_on_the_tests_own_scenarios():
    """SIM_D bounds the float64 statement's own rounding, measured against numpy.longdouble over every scenario the GPU tests compare
    pair_sim on, and over the rational cases above; SIM_BOUND = 64 * SIM_D is far below any level spacing."""
    d = 0.0
    for mode in (X.MODE_3D, X.MODE_BEV):
        for kw in (dict(seed=21, N=96), dict(seed=21, N=320), dict(seed=23, N=96, Kobj=80, many=70), dict(seed=24, N=96, frames=4)):
            d = max(d, X.measure_d(X.scenario(**kw), 4, mode))
        d = max(d, X.measure_d([X.exact_frame()[0]], 1, mode), X.measure_d([X.crowded_frame()[0]], 2, mode))
        for _, det, gt in CASES:
            lo, hi = (X.similarity(X.det_row(det), 3, X.gt_row(gt), mode, T) for T in (np.float64, np.longdouble))
            d = max(d, abs(float(np.longdouble(lo) - hi)))
    print("largest |s(float64) - s(longdouble)|: %.3e; SIM_D %.3e, SIM_BOUND %.3e" % (d, X.SIM_D, X.SIM_BOUND))
    assert d <= X.SIM_D and X.SIM_BOUND == 64 * X.SIM_D and X.SIM_BOUND < 1e-12
    if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps:
        assert d > 0.0          # (where long double is wider than double the yardstick is a real one)


def test_the_frame_pair_list_the_condition_and_the_fit_rule():
    frames = X.scenario(21)
    for mode in (X.MODE_3D, X.MODE_BEV):
        log = X.host_pair_log(frames, 4, 8, 256, 1024, mode)
        assert X.condition_holds(log) and not log["dropped"].any() and log["frames"].tolist() == [3, 3, 2, 3]
        commons = [c for b in range(4) for ps, _ in log["entries"][b] for _, _, c in ps]
        assert min(commons) == 0 < max(commons) and all(0.0 < s <= 1.0 for s in log["all_sims"]) and len(commons) > 40
        # stream 0's detections 1 (valid 0), 2 (valid -1, a NaN) and 3 (width 0) have no pairs; nor have the objects without a box
        assert all(i not in (1, 2, 3) for ps, _ in log["entries"][0] for i, _, _ in ps)
        assert all(j != 1 for ps, _ in log["entries"][2] for _, j, _ in ps) and all(j > 1 for ps, _ in log["entries"][3] for _, j, _ in ps)
        assert log["pair_frame"][0, 1, 1] == 0 and log["pair_frame"][1, 1, 1] == 0
        for b in range(4):
            for ps, _ in log["entries"][b]:
                assert ps == sorted(ps)
    bev, box = (X.host_pair_log(frames, 4, 8, 256, 1024, m) for m in (X.MODE_BEV, X.MODE_3D))
    assert bev["pair_cursor"].sum() > box["pair_cursor"].sum()          # footprints that overlap under z ranges that do not
    # a pair log that is too small drops whole frames and keeps later, smaller ones
    small = X.host_pair_log(frames, 4, 8, 256, int(bev["pair_frame"][3, 0, 1]) + 1, X.MODE_BEV)
    assert small["dropped"].any() and (small["frames"] <= bev["frames"]).all() and small["pair_cursor"][3] == bev["pair_frame"][3, 0, 1]


# ---- the keywords -----------------------------------------------------------------------------------------------------------------------
def test_check_pair_similarity_and_the_keywords():
    assert TS.SIMILARITIES == ("iou", "centre", "box", "box_bev") and TS.BOX_MODES == {"box": 0, "box_bev": 1}
    check = TS.check_pair_similarity
    assert check("box", None, 64) == ("box", None) and check("box_bev", None, 1) == ("box_bev", None)
    for name in ("box", "box_bev"):
        with pytest.raises(ValueError, match="similarity=\"%s\" lives in the pair log \\(give sweep_pairs" % name):
            check(name, None, None)
        with pytest.raises(ValueError, match="a box IoU has no distance scale"):
            check(name, 2.0, 64)
    for bad in ("Box", "box3d", "bev", None, 1, ("box",)):
        with pytest.raises(ValueError, match="is none of \"iou\", \"centre\", \"box\", \"box_bev\""):
            check(bad, None, 64)
    # the defaults stay what they are, through `check_similarity`, which is itself what it was: it still refuses everything but its two
    assert check() == ("iou", None) and check("centre", None, 64) == ("centre", 2.0) and check("centre", 0.5, 64) == ("centre", 0.5)
    with pytest.raises(ValueError, match="goes with similarity=\"centre\"; the point IoU has no distance scale"):
        check("iou", 2.0, 64)
    with pytest.raises(ValueError, match="similarity=\"centre\" lives in the pair log"):
        check("centre", None, None)
    with pytest.raises(ValueError, match="is neither \"iou\" nor \"centre\""):
        TS.check_similarity("box_bev", None, 64)
    # the constructor runs the same checks before it allocates anything (device="nowhere" would fail at the first tensor)
    with pytest.raises(ValueError, match="lives in the pair log"):
        TS.TrackScorer(streams=2, max_objects=8, max_boxes=8, device="nowhere", sweep_frames=4, sweep_records=32, similarity="box")
    with pytest.raises(ValueError, match="no distance scale"):
        TS.TrackScorer(streams=2, max_objects=8, max_boxes=8, device="nowhere", sweep_frames=4, sweep_records=32, sweep_pairs=8, similarity="box_bev",
                       zero_distance=2.0)
    kw = dict(streams=2, max_objects=8, max_boxes=8, device="cpu", sweep_frames=4, sweep_records=32, sweep_pairs=64)
    plain, centre, box, bev = TS.TrackScorer(**kw), TS.TrackScorer(similarity="centre", **kw), TS.TrackScorer(similarity="box", **kw), \
        TS.TrackScorer(similarity="box_bev", **kw)
    assert (plain.box, plain.has_sim, centre.box, centre.has_sim) == (False, False, False, True) and not hasattr(plain, "pair_sim")
    for sc, name in ((box, "box"), (bev, "box_bev")):
        assert (sc.similarity, sc.zero_distance, sc.centre, sc.box, sc.has_sim) == (name, None, False, True, True)
        assert sc.pair_sim.shape == (2, 64) and str(sc.pair_sim.dtype) == "torch.float64" and not sc.pair_sim.any()
    # a configuration the centre scorer takes and the box variant's upright boxes push over the LDS limit is refused by name
    fits = dict(max_boxes=64, points=1350, max_objects=64)
    TS.check_fit(centre=True, **fits)
    with pytest.raises(ValueError, match="need \\d+ bytes of LDS per stream, the limit is 65536"):
        TS.check_fit(box=True, **fits)
    # update_raw refuses, before anything reaches the device, ground-truth objects without the box table and a step without boxes
    import torch
    z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt)
    gobj = TS.GtObjects(slot=z(2, 8), label_id=z(2, 8), count=z(2), size=z(2, 8), members=z(2, 8, 2), centre=z(2, 8, 3, dt=torch.float64), flags=z(2),
                        n_valid=None, max_boxes=8, points=64)
    args = (z(2, 3, 64, dt=torch.float32), z(2, 64), z(2), z(2, 8), gobj)
    with pytest.raises(ValueError, match="gobj.boxes must be the \\(2,8,16\\) float64 frame-1 box table, got None"):
        box.update_raw(*args, object_conf=z(2, 8, dt=torch.float32))
    gobj.boxes = z(2, 8, 16, dt=torch.float64)
    with pytest.raises(ValueError, match="update_raw needs the detections' boxes, det_boxes \\(2,8,8\\) float64 and det_box_valid \\(2,8\\), got None"):
        bev.update_raw(*args, object_conf=z(2, 8, dt=torch.float32))
    with pytest.raises(ValueError, match="det_boxes \\(2,8,8\\) float64"):
        bev.update_raw(*args, object_conf=z(2, 8, dt=torch.float32), det_boxes=z(2, 8, 8, dt=torch.float32), det_box_valid=z(2, 8))

    class Step:
        max_objects, object_boxes, object_box_valid = 8, None, None
    with pytest.raises(ValueError, match="similarity=\"box\"\\) scores the detections' boxes, and this step has none: build the tracker with "
                                         "BatchedTracker\\(boxes=True\\)"):
        box.update(Step(), gobj)
    # where the keyword is documented, the rule for a detection without a box is stated with its remedy
    assert "A DETECTION WITHOUT A BOX\n    HAS NO PAIRS" in TS.TrackScorer.__doc__ and "BatchedTracker(box_min_extent=...)" in TS.TrackScorer.__doc__


# ---- the native surface ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_binding_mirrors_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "rtk_score.h")).read()
    assert re.search(r"RTK_EXPORT int rtk_track_score_pairs_box\(const rtk_track_score_in_t \*in,", text)
    assert re.search(r"const rtk_score_pairs_t \*pairs, double \*pair_sim /\* \(B,Q\) \*/, const double \*det_box /\* \(B,Kobj,8\) \*/,\s+"
                     r"const int \*det_valid /\* \(B,Kobj\) \*/, const double \*gt_boxes /\* \(B,K,16\) \*/, int mode,\s+rtk_stream_t stream\);", text)
    assert re.search(r"RTK_EXPORT int rtk_track_score_box_lds_bytes\(int Kobj, int K, int N, int memory", text)
    assert re.search(r"#define RTK_SCORE_BOX_3D 0\n#define RTK_SCORE_BOX_BEV 1\n", text)
    lib = ctypes.CDLL(B.build(verbose=False))
    for name, nargs in (("rtk_track_score_pairs_box", 12), ("rtk_track_score_box_lds_bytes", 4)):
        assert hasattr(lib, name) and len(abi.SIGNATURES[name]) == nargs, name
    assert abi.SIGNATURES["rtk_track_score_pairs_box"] == abi.SIGNATURES["rtk_track_score_pairs"][:6] + [ctypes.c_void_p] * 4 + [ctypes.c_int,
                                                                                                                                 ctypes.c_void_p]
    assert (TS.BOX_MODES["box"], TS.BOX_MODES["box_bev"]) == (X.MODE_3D, X.MODE_BEV) == (0, 1)
    # the section is the header's last, and states the definition the tests hold the kernel to
    last = text[text.rindex("/* ----"):]
    for word in ("The oriented-box IoU on the pair log", "UPRIGHT IN\n *                THE RADAR FRAME", "rr = ri + rj", "(dx * dx + dy * dy) > rr * rr",
                 "zo = min(top_i, top_j) - max(bottom_i, bottom_j)", "SET TO THE BOUND ITSELF", "I2 = 0.5 * acc", "s = I2 / ((A_i + A_j) - I2)",
                 "s = I3 / ((V_i + V_j) - I3)", "s = min(s, 1.0)", "logged iff s > 0.0", "a NaN is not logged", "fit with a positive min_extent",
                 "DEPARTURES FROM\n * TrackEval AFTER THIS", "arccos(R[2][2])"):
        assert word in last, word
    assert "A box IoU is not built here" not in text
    for name in ("track_score.hip", "track_score_body.h"):
        code = re.sub(r"//[^\n]*", "", open(os.path.join(B.CSRC, name)).read())
        assert "asm" not in code and not re.search(r"atomic\w*\s*\(\s*&?\s*\w*(pair_sim|gpos|sim)\b", code), name


def test_the_producer_builds_as_two_kernels_without_scratch_and_without_static_lds(tmp_path):
    ts = score_kernel_notes(tmp_path)                # the ten instantiations of the one scoring kernel, each (0, 0, 64, 256), and no other
    box = [k for k, flags in SCORE_VARIANTS.items() if flags[4]]
    centre = [k for k, flags in SCORE_VARIANTS.items() if flags[3]]
    assert box == ["box", "box_memory"] and centre == ["centre", "centre_memory"]       # each without and with the memory block
    assert all((ts[k].private, ts[k].lds, ts[k].wavefront, ts[k].max_threads) == (0, 0, 64, 256) for k in box), ts
    # the box code stays in the instantiations with BOX, the centre code in those with CENTRE: every other instantiation of the one
    # body needs strictly fewer registers than either of them (at most 75 against 143 and 144; at most 44 against 73 and 75)
    assert max(ts[k].vgpr for k in ts if k not in box) < min(ts[k].vgpr for k in box), ts
    assert max(ts[k].vgpr for k in ts if k not in box + centre) < min(ts[k].vgpr for k in centre), ts
    # dynamic LDS: the plain figure rounded up to 8 bytes, plus eight float64 per kept object, the mode and one address
    plain, memory, box = (_lib._fn(n) for n in ("rtk_track_score_lds_bytes", "rtk_track_score_memory_lds_bytes", "rtk_track_score_box_lds_bytes"))
    for Kobj, K, N in ((16, 8, 96), (7, 5, 33), (64, 40, 128), (128, 32, 256), (256, 64, 1)):
        up = lambda x: (x + 7) // 8 * 8
        assert box(Kobj, K, N, 0) == up(plain(Kobj, K, N)) + 64 * K + 16 and box(Kobj, K, N, 1) == up(memory(Kobj, K, N)) + 64 * K + 16
    assert box(0, 8, 96, 0) == -1 and box(16, 65, 96, 0) == -1 and box(16, 8, 0, 1) == -1 and box(257, 8, 96, 0) == -1


def test_the_entry_point_refuses_before_any_launch():
    keep = [(ctypes.c_int * 64)() for _ in range(5)] + [(ctypes.c_float * 64)(), (ctypes.c_double * 64)()]
    full = abi.ScoreLog(4, 8, None, *(ctypes.addressof(k) for k in keep))
    pk = [(ctypes.c_int * 64)() for _ in range(6)]
    pairs = abi.ScorePairs(16, *(ctypes.addressof(k) for k in pk))
    dbl, ints = (ctypes.c_double * 64)(), (ctypes.c_int * 64)()
    a = lambda x: None if x is None else ctypes.addressof(x)
    blocks = [abi.ScoreIn(2, 64, 8, 8, 16), abi.ScoreState(), abi.ScoreOut()]
    # (every pointer is host memory or null: a refusal touches none of them)

    def produce(blocks=blocks, log=full, pr=pairs, sim=dbl, det=dbl, valid=ints, gt=dbl, mode=0):
        i, s, o = (None, None, None) if blocks is None else (a(x) for x in blocks)
        _lib.call("rtk_track_score_pairs_box", i, s, o, a(log), None, a(pr), a(sim), a(det), a(valid), a(gt), mode, None)
    with pytest.raises(_lib.RtkError, match="track_score_pairs_box: null argument block"):
        produce(blocks=None)
    with pytest.raises(_lib.RtkError, match="null log block"):
        produce(log=None)
    with pytest.raises(_lib.RtkError, match="null pair-log block"):
        produce(pr=None)
    with pytest.raises(_lib.RtkError, match="null pair_sim"):
        produce(sim=None)
    with pytest.raises(_lib.RtkError, match="null det_box or det_valid"):
        produce(det=None)
    with pytest.raises(_lib.RtkError, match="null det_box or det_valid"):
        produce(valid=None)
    with pytest.raises(_lib.RtkError, match="null gt_boxes"):
        produce(gt=None)
    for bad in (-1, 2, 7):
        with pytest.raises(_lib.RtkError, match="mode=%d is neither RTK_SCORE_BOX_3D nor RTK_SCORE_BOX_BEV" % bad):
            produce(mode=bad)
    # sizes whose tables exceed the LDS limit: the plain scorer's largest cloud at these counts does not leave room for the boxes
    with pytest.raises(_lib.RtkError, match="need \\d+ bytes of LDS per stream, the limit is 65536"):
        produce(blocks=[abi.ScoreIn(2, 1446, 64, 64, 16), abi.ScoreState(), abi.ScoreOut()], mode=1)
    with pytest.raises(_lib.RtkError, match="track_score: null input"):          # everything of its own in order: the shared checks refuse
        produce(mode=1)


# ---- the replays on a log that carries a similarity -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [4, 5])
def test_the_replays_on_a_similarity_log_agree_with_their_dense_twins(seed, monkeypatch):
    logs = X.with_sims(O.random_logs(seed, streams=3, frames=10, max_dets=8, max_objs=6), seed)
    iou_hota = HO.host_hota_optimal(logs)                      # before the substitution: the point IoU of the integers
    X.patch_similarity(monkeypatch)
    sparse, dense = HO.host_hota_optimal(logs), HO.dense_hota_optimal(logs)
    assert np.array_equal(sparse["counters"], dense["counters"]) and np.array_equal(_bits(sparse["sums"]), _bits(dense["sums"]))
    assert sparse["counters"][0, :, HO.COUNTERS.index("tp")].sum() > 0 and not np.array_equal(sparse["counters"], iou_hota["counters"])
    levels = (0.25, 0.5, 0.75)
    ids, dense_ids = HO.host_identity_all(logs, alphas=levels), HO.dense_identity_all(logs, alphas=levels)
    assert [int(v) for v in ids["idtp"]] == [d["idtp"] for d in dense_ids] and ids["idtp"][0] > ids["idtp"][2] >= 0
    scores = [[[0.0] * len(e["dets"]) for e in lb] for lb in logs]
    for min_iou in (0.25, 0.5):
        for lb, sb in zip(logs, scores):
            _, _, _, _, cps = O.replay(lb, sb, -math.inf, min_iou)
            for e, sc, cp in zip(lb, sb, cps):
                _, edges, ious = O.frame_edges(e, sc, -math.inf, min_iou)
                assert all(v >= min_iou for v in ious.values()) and len(edges) == sum(1 for s in e["sims"] if s >= min_iou)
                assert sum(w for i, j, w in edges if cp[j] == i) == O.independent_solve(len(e["dets"]), len(e["labels"]), edges)[0]


# ---- the departure: the upright reading of the label box -------------------------------------------------------------------------------------
def test_the_upright_reading_drops_the_calibrations_tilt_on_the_shipped_frames():
    """On the three shipped frames every label box in the radar frame is tilted by arccos(R[2][2]) = 0.54 degrees, the radar-lidar
    calibration's; the upright reading keeps the heading of the box's first axis (whose projection is shorter than 1 by < 1e-4), the
    centre and the half-extents, and a detection that is the label's own upright box has s = 1 within the bound."""
    from _gt_util import EX, tf_of
    from ratrack_amd import gt_device, vod_gt
    tilts = []
    for f in ("00549", "01047", "01201"):
        tf = tf_of(f)
        det = open(os.path.join(EX, "label_%s.txt" % f)).read().splitlines()
        labels = vod_gt.parse_tracking_labels([" ".join([line.split(" ")[0], str(i)] + line.split(" ")[2:15]) for i, line in enumerate(det)])
        for lab in labels.values():
            box = vod_gt.box_in_radar_frame(lab, tf)
            row = gt_device._box_row(box)
            tilts.append(math.degrees(math.acos(min(1.0, float(box.R[2, 2])))))
            gx, gy, hx, hy, a, b, bottom, top = X.upright(row)
            n = math.hypot(float(box.R[0, 0]), float(box.R[1, 0]))
            assert 1.0 - 1e-4 < n <= 1.0 and abs(math.hypot(hx, hy) - 1.0) < 1e-15
            assert (gx, gy, a, b) == (box.center[0], box.center[1], box.extent[0] / 2, box.extent[1] / 2)
            assert bottom == box.center[2] - box.extent[2] / 2 and top == box.center[2] + box.extent[2] / 2
            own = np.array([gx, gy, box.center[2], box.extent[0], box.extent[1], box.extent[2], math.atan2(hy, hx), 0.0])
            for mode in (X.MODE_3D, X.MODE_BEV):
                assert abs(float(X.similarity(own, 2, row, mode)) - 1.0) <= X.SIM_BOUND
    print("labels %d, tilt %.4f .. %.4f degrees" % (len(tilts), min(tilts), max(tilts)))
    assert len(tilts) > 50 and 0.535 < min(tilts) and max(tilts) < 0.545
