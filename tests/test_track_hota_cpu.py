"""CPU: the native surface and the host half of HOTA over the scorer's log (include/rtk_score.h, csrc/track_hota.hip,
ratrack_amd/track_score.py: `TrackScorer.hota`, `hota_values`) -- the entry point and its constants are declared, built for gfx950
without scratch and exported; `hota_values` is the header's host arithmetic; the two host forms of tests/_track_hota_util.py agree at
every level; the planned sequence of tests/test_track_hota_gpu.py holds every situation it is there for; and `hota` refuses what it
cannot evaluate."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import _track_hota_util as H
import _track_sweep_util as W
from _util import kernel_notes
from ratrack_amd import _lib, abi, build as B
from ratrack_amd import track_score as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


# ---- the native surface ------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_hota():
    text = open(os.path.join(ROOT, "include", "rtk_score.h")).read()
    assert re.search(r"RTK_EXPORT int rtk_score_hota\(int B, int T, const rtk_score_log_t \*log, const double \*rec_score", text)
    for name, value in (("RTK_SCORE_HOTA_COUNTERS", len(TS.HOTA_COUNTERS)), ("RTK_SCORE_HOTA_SUMS", len(TS.HOTA_SUMS)),
                        ("RTK_SCORE_HOTA_PAIRS", TS.HOTA_PAIRS), ("RTK_SCORE_FLAG_HOTA", TS.FLAG_HOTA)):
        assert re.search(r"#define %s %d\b" % (name, value), text), name
    assert TS.FLAG_HOTA == 128 and TS.HOTA_PAIRS >= 1024
    assert TS.HOTA_COUNTERS == H.COUNTERS == ("frames", "clips", "gt", "pred", "tp", "pairs") and TS.HOTA_SUMS == H.SUMS
    lib = ctypes.CDLL(B.build(verbose=False))
    assert hasattr(lib, "rtk_score_hota")
    assert _lib.SIGNATURES["rtk_score_hota"] == abi.SIGNATURES["rtk_score_hota"] and len(abi.SIGNATURES["rtk_score_hota"]) == 10
    # the definitions are stated with the prototype, and what this HOTA is
    for word in ("alpha_a = (double)a / (double)(A + 1)", "THE OBJECT STAYS FREE", "ORDER OF FIRST APPEARANCE", "N / (double)(cg + ct - n)",
                 "sqrt(DetA * AssA)", "Hungarian assignment on box IoU", "divided by A"):
        assert word in text, word


def test_hota_kernel_builds_for_gfx950_without_scratch(tmp_path):
    found = {k: v.private for k, v in kernel_notes(os.path.join(B.CSRC, "track_hota.hip"), tmp_path)[0].items()}
    assert len(found) == 1 and [v for name, v in found.items() if "hota_kernel" in name] == [0], found


def test_entry_point_refuses_before_any_launch():
    lg = abi.ScoreLog(4, 32)
    with pytest.raises(_lib.RtkError, match="T=100000 label-table entries need \\d+ bytes of LDS per stream, the limit is 65536"):
        _lib.call("rtk_score_hota", 2, 100000, ctypes.addressof(lg), None, None, 19, None, None, None, None)
    with pytest.raises(_lib.RtkError, match="alphas=64"):
        _lib.call("rtk_score_hota", 2, 1024, ctypes.addressof(lg), None, None, 64, None, None, None, None)
    with pytest.raises(_lib.RtkError, match="null or empty log"):          # T = 1024 fits
        _lib.call("rtk_score_hota", 2, 1024, ctypes.addressof(lg), None, None, 19, None, None, None, None)


def test_hota_and_alphas_refusals():
    plain = TS.TrackScorer(streams=2, max_objects=8, max_boxes=8, device="cpu")
    with pytest.raises(RuntimeError, match="TrackScorer.hota: the scorer keeps no log"):
        plain.hota()
    s = TS.TrackScorer(streams=2, max_objects=8, max_boxes=8, device="cpu", sweep_frames=4, sweep_records=32)
    for bad in (0, 64, -3):
        with pytest.raises(ValueError, match=r"alphas=%d outside \[1, 63\]" % bad):
            s.hota(alphas=bad)
    with pytest.raises(RuntimeError, match="TrackScorer.hota: stream 1 has a clip with more than max_gt_tracks=1024 label ids, 2048 track ids or "
                                           "1024 \\(label id, track id\\) pairs"):
        s._raise_on_flags([0, TS.FLAG_HOTA])


# ---- hota_values -------------------------------------------------------------------------------------------------------------------
def test_hota_values_against_hand_numbers():
    #              frames clips gt pred tp pairs
    c = np.array([[[10, 1, 20, 25, 15, 3], [5, 2, 10, 5, 5, 2]],          # level 1: TP 20, FN 10, FP 10
                  [[10, 1, 20, 25, 8, 2], [5, 2, 10, 5, 2, 1]],           # level 2: TP 10, FN 20, FP 20
                  [[10, 1, 20, 0, 0, 0], [5, 2, 10, 0, 0, 0]]],           # level 3: no prediction: TP 0 -> NaN where TP divides
                 dtype=np.int64)
    q = np.array([[[7.5, 9.0, 10.5, 12.0], [2.5, 3.0, 3.5, 4.0]],
                  [[3.0, 4.0, 5.0, 6.5], [1.0, 1.5, 2.0, 1.5]],
                  [[0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]]])
    v = TS.hota_values(c, q)
    assert v["alphas"] == 3 and v["alpha"].tolist() == [0.25, 0.5, 0.75]
    assert v["tp"].tolist() == [20, 10, 0] and v["fn"].tolist() == [10, 20, 30] and v["fp"].tolist() == [10, 20, 0]
    assert v["gt"].tolist() == [30, 30, 30] and v["pred"].tolist() == [30, 30, 0] and v["pairs"].tolist() == [5, 3, 0]
    assert v["deta"][0] == 20 / 40 and v["detre"][0] == 20 / 30 and v["detpr"][0] == 20 / 30
    assert v["assa"][0] == 10.0 / 20 and v["assre"][0] == 12.0 / 20 and v["asspr"][0] == 14.0 / 20 and v["loca"][0] == 16.0 / 20
    assert v["hota_alpha"][0] == math.sqrt(0.5 * 0.5) and v["hota_alpha"][1] == math.sqrt((10 / 50) * (4.0 / 10))
    assert v["deta"][2] == 0.0 and v["detre"][2] == 0.0 and np.isnan(v["detpr"][2])                 # 0/30, 0/30, 0/0
    assert all(np.isnan(v[k][2]) for k in ("assa", "assre", "asspr", "loca", "hota_alpha"))
    # the means: the non-NaN terms in level order, divided by A
    assert v["hota"] == (math.sqrt(0.25) + math.sqrt((10 / 50) * (4.0 / 10))) / 3
    assert v["deta_mean"] == (20 / 40 + 10 / 50 + 0.0) / 3 and v["detpr_mean"] == (20 / 30 + 10 / 30) / 3
    assert v["assa_mean"] == (0.5 + 0.4) / 3 and v["loca_mean"] == (16.0 / 20 + 8.0 / 10) / 3
    assert v["assre_mean"] == (12.0 / 20 + 5.5 / 10) / 3 and v["asspr_mean"] == (14.0 / 20 + 7.0 / 10) / 3
    # one stream of it, and no stream at all
    one = TS.hota_values(c[:, 1:2], q[:, 1:2])
    assert one["tp"].tolist() == [5, 2, 0] and one["assa"][0] == 2.5 / 5 and one["deta"][0] == 5 / 10 and one["fp"].tolist() == [0, 3, 0]
    none = TS.hota_values(c[:, :0], q[:, :0])
    assert none["hota"] == 0.0 and np.isnan(none["deta"]).all() and none["tp"].tolist() == [0, 0, 0]
    # the sums of the streams are added in stream order
    q2 = q.copy()
    q2[0, :, 0] = (0.1, 0.2)
    assert TS.hota_values(c, q2)["assa"][0] == (0.1 + 0.2) / 20
    with pytest.raises(ValueError, match="hota_values"):
        TS.hota_values(c, q[:, :, :3])


def test_hota_values_is_the_host_statements_arithmetic():
    _, _, logs, _ = W.planned()
    h = H.host_hota(logs)
    v = TS.hota_values(h["counters"], h["sums"])
    for k in ("tp", "fn", "fp", "gt", "pred", "pairs", "deta", "detre", "detpr", "assa", "assre", "asspr", "loca", "hota_alpha"):
        assert all(_same(float(x), float(y)) for x, y in zip(v[k], h[k])), k
    for k in ("hota", "deta_mean", "assa_mean", "detre_mean", "detpr_mean", "assre_mean", "asspr_mean", "loca_mean"):
        assert v[k] == h[k], k
    assert v["alpha"].tolist() == H.alpha_levels(19) and v["alpha"][11] == 3.0 / 5.0


# ---- the host statement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filtered", [False, True])
def test_fast_and_matrix_forms_agree_at_every_level(filtered):
    _, _, logs, sw = W.planned()
    scores, tau = (sw["scores"], float(sw["thresholds"][sw["best"]])) if filtered else (None, -math.inf)
    fast, mat = H.host_hota(logs, scores, tau), H.matrix_hota(logs, scores, tau)
    close = lambda x, y: (math.isnan(x) and math.isnan(y)) or abs(x - y) <= 1e-12 * abs(y)
    for a, m in enumerate(mat):
        assert (m["tp"], m["fn"], m["fp"]) == (fast["tp"][a], fast["fn"][a], fast["fp"][a]), a
        for k in ("assa", "assre", "asspr", "loca", "deta", "hota_alpha"):
            assert close(m[k], fast[k][a]), (a, k, m[k], fast[k][a])
    assert fast["tp"][0] > 0 and fast["assa"][0] > 0


def test_planned_sequence_meets_its_conditions():
    _, _, logs, sw = W.planned()
    h = H.host_hota(logs)
    pooled = h["counters"][0].sum(axis=0)
    assert len(logs) == 16 and pooled[H.COUNTERS.index("clips")] == 22 and pooled[H.COUNTERS.index("gt")] == 363
    # a later detection wins an object whose first taker fell below alpha
    assert h["freed"][3:10] == [2, 6, 20, 31, 34, 21, 21] and all(v > 0 for v in h["freed"][3:13]) and h["freed"][:3] == [0, 0, 0]
    ious = [d[3] for lb in logs for e in lb for d in e["dets"] if d[2] != -1]
    assert sum(v == 0.5 for v in ious) == 96 and sum(v == 0.8 for v in ious) == 36           # IoUs that ARE a level: >= decides
    assert h["tp"][0] == 273 and h["tp"][-1] == 81 and all(x >= y for x, y in zip(h["tp"], h["tp"][1:])) and len(set(h["tp"])) > 8
    assert h["pairs"][0] == 66 and h["pairs"][-1] == 17 and len(set(h["pairs"])) > 8
    assert abs(h["hota"] - 0.41369681694671) < 1e-13
    # the counts that do not depend on the level
    for k in ("frames", "clips", "gt", "pred"):
        i = H.COUNTERS.index(k)
        assert (h["counters"][:, :, i] == h["counters"][0, :, i]).all(), k
    # the order of the association sums shows in their bits somewhere
    assert any(m["assa"] != f for m, f in zip(H.matrix_hota(logs), h["assa"]))
    # at the sweep's best level
    assert sw["best"] == 9 and sw["thresholds"][9] == 0.55234375
    f = H.host_hota(logs, sw["scores"], float(sw["thresholds"][9]))
    assert f["tp"][0] == 118 and f["tp"][-1] == 19 and [a for a, v in enumerate(f["freed"]) if v > 0] == [2, 3, 4, 5, 6, 7]
    assert f["pred"][0] < h["pred"][0] and f["gt"][0] == 363
