"""CPU: the native surface and the host half of the confidence sweep (include/rtk_score.h, csrc/track_sweep.hip,
ratrack_amd/track_score.py: sAMOTA / AMOTA / AMOTP) -- the new entry points and the flag are declared, built for gfx950 without
scratch and exported; `sweep_values` is the host statement's arithmetic; the two host forms of the replay agree at every threshold;
the planned sequence of tests/test_track_sweep_gpu.py holds every situation it is there for; and the constructor refuses half a log."""
import ctypes
import os
import re

import numpy as np
import pytest

import _track_score_util as S
import _track_sweep_util as W
from _util import SCORE_VARIANTS, kernel_notes, score_kernel_notes
from ratrack_amd import _lib, abi, build as B
from ratrack_amd import track_score as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ["rtk_track_score_logged", "rtk_score_track_means", "rtk_score_thresholds", "rtk_score_replay"]


def test_header_declares_and_library_exports_the_sweep():
    text = open(os.path.join(ROOT, "include", "rtk_score.h")).read()
    assert re.search(r"RTK_EXPORT int rtk_track_score_logged\(const rtk_track_score_in_t \*in, const rtk_track_score_state_t \*state,\s+"
                     r"const rtk_track_score_out_t \*out,\s+const rtk_score_log_t \*log, rtk_stream_t stream\);", text)
    for name in ENTRY[1:]:
        assert re.search(r"RTK_EXPORT int %s\(" % name, text), name
    for name, value in (("RTK_SCORE_FLAG_LOG", TS.FLAG_LOG), ("RTK_SCORE_FLAG_SWEEP", TS.FLAG_SWEEP), ("RTK_SCORE_SWEEP_TRACKS", TS.SWEEP_TRACKS)):
        assert re.search(r"#define %s %d\b" % (name, value), text), name
    assert TS.FLAG_LOG == 16
    lib = ctypes.CDLL(B.build(verbose=False))
    for name in ENTRY:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["rtk_track_score_logged"] == [ctypes.c_void_p] * 5
    assert abi.STRUCTS["rtk_score_log_t"] is abi.ScoreLog
    # the definitions are stated with the prototypes
    for word in ("track score", "replay at t", "thresholds", "r_k = k/L", "sMOTA_k", "divided by L"):
        assert word in text, word


def test_sweep_kernels_and_the_logged_wrapper_build_for_gfx950_without_scratch(tmp_path):
    found = {k: v.private for k, v in kernel_notes(os.path.join(B.CSRC, "track_sweep.hip"), tmp_path)[0].items()}
    for k in ("sweep_means_kernel", "sweep_thresholds_kernel", "sweep_replay_kernel"):
        assert [v for name, v in found.items() if k in name] == [0], (k, found)
    assert len(found) == 3, found
    # the logged variant is an instantiation of its own among the ten of the one scoring kernel (and gt_objects_kernel: nothing else)
    ts = score_kernel_notes(tmp_path)
    assert SCORE_VARIANTS["logged"] == (True, False, False, False, False) != SCORE_VARIANTS["plain"]
    assert (ts["logged"].private, ts["logged"].lds, ts["logged"].wavefront, ts["logged"].max_threads) == (0, 0, 64, 256), ts["logged"]


# ---- sweep_values ------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


def test_sweep_values_is_the_host_statements_arithmetic():
    _, _, _, sw = W.planned()
    L = 40
    v = TS.sweep_values(sw["counters"], sw["iou_sums"], sw["thresholds"], sw["reached"], L)
    assert v["reached"] == sw["reached"] == 31 and v["levels"] == L
    assert v["amota"] == sw["amota"] and v["samota"] == sw["samota"] and v["amotp"] == sw["amotp"]
    for k in range(1, sw["reached"] + 1):
        assert v["mota"][k] == sw["mota"][k] and v["smota"][k] == sw["smota"][k] and _same(v["motp"][k], sw["motp"][k]), k
    for k in range(sw["reached"] + 1, L + 1):                 # unreached levels count 0
        assert np.isnan(v["mota"][k]) and np.isnan(v["smota"][k]) and np.isnan(v["motp"][k])
        assert all(v[n][k] == 0 for n in TS.COUNTERS[1:]), k
    assert np.isnan(v["smota"][0]) and v["mota"][0] == 1 - (344 + 90 + 91) / 363
    assert v["best"]["level"] == sw["best"] and v["best"]["mota"] == sw["mota"][sw["best"]]
    assert v["best"]["threshold"] == sw["thresholds"][sw["best"]] and v["best"]["tp"] == int(sw["counters"][sw["best"]].sum(0)[3])
    assert v["unfiltered"]["tp"] == 273 and v["unfiltered"]["gt"] == 363
    # unreached levels add nothing whatever their counters hold; the divisor stays L
    junk = sw["counters"].copy()
    junk[sw["reached"] + 1:] = 12345
    w = TS.sweep_values(junk, sw["iou_sums"], sw["thresholds"], sw["reached"], L)
    assert w["amota"] == v["amota"] and w["samota"] == v["samota"] and w["amotp"] == v["amotp"] and w["tp"][L] == 0


def test_sweep_values_ties_empty_levels_and_no_level():
    #            frames gt  pred tp  fp fn idsw tracks mt pt ml
    rows = [[10, 40, 50, 30, 20, 10, 4, 8, 5, 2, 1],          # unfiltered
            [10, 40, 0, 0, 0, 40, 0, 8, 0, 0, 8],             # level 1: nothing remains -> TP = 0
            [10, 40, 20, 18, 2, 22, 1, 8, 2, 2, 4],           # level 2 and 3: the same MOTA
            [10, 40, 22, 19, 3, 21, 1, 8, 2, 3, 3],
            [10, 40, 99, 9, 90, 31, 9, 8, 0, 0, 8]]           # level 4: not reached
    c = np.array(rows, dtype=np.int64).reshape(5, 1, 11)
    q = np.array([[21.0], [0.0], [9.0], [9.5], [7.0]])
    thr = np.array([-np.inf, 0.9, 0.5, 0.25, np.inf])
    v = TS.sweep_values(c, q, thr, 3, 4)
    assert np.isnan(v["motp"][1]) and v["mota"][1] == 0.0 and v["smota"][1] == max(0.0, 1 - (40 - 0.75 * 40) / (0.25 * 40))
    assert v["mota"][2] == v["mota"][3] == 1 - 25 / 40
    assert v["best"]["level"] == 2 and v["best"]["threshold"] == 0.5 and v["best"]["mt_fraction"] == 0.25       # the lowest of equals
    assert v["amotp"] == (9.0 / 18 + 9.5 / 19) / 4                                  # the TP = 0 level is left out, the divisor is L
    assert v["amota"] == (0.0 + (1 - 25 / 40) + (1 - 25 / 40)) / 4
    assert v["samota"] == (v["smota"][1] + v["smota"][2] + v["smota"][3]) / 4
    assert v["tp"].tolist() == [30, 0, 18, 19, 0] and np.isnan(v["mota"][4])
    none = TS.sweep_values(c, q, thr, 0, 4)
    assert none["best"] is None and none["amota"] == 0.0 and none["samota"] == 0.0 and none["amotp"] == 0.0
    with pytest.raises(ValueError, match="reached=5"):
        TS.sweep_values(c, q, thr, 5, 4)
    # the IoU sums of the streams are added in stream order
    two = TS.sweep_values(np.concatenate([c, c], axis=1), np.concatenate([q, q * 0.1], axis=1), thr, 3, 4)
    assert two["motp"][2] == (9.0 + 9.0 * 0.1) / 36


# ---- the host statement ---------------------------------------------------------------------------------------------------------------
def test_fast_and_full_definition_forms_agree_at_every_threshold():
    _, _, logs, sw = W.planned()
    W.host_sweep(logs, full=range(0, 41))                     # asserts counters and IoU-sum bits per (threshold, stream)
    _, _, logs, sw = W.planned(raw=True)
    W.host_sweep(logs, full=range(0, 41, 4))


def test_planned_sequence_meets_its_conditions():
    seq, confs, logs, sw = W.planned()
    assert all(float(c) * 256 == int(float(c) * 256) and 0 <= c < 1 for conf in confs for c in conf.reshape(-1))
    pooled = sw["counters"][0].sum(axis=0)
    assert pooled[W.COUNTERS.index("tp")] == 273 and pooled[W.COUNTERS.index("gt")] == 363
    assert len(sw["walked"]) == 32 and sw["reached"] == 31
    assert sw["thresholds"][30] == sw["thresholds"][31] == 0.0 and sw["thresholds"][29] > 0 and np.isinf(sw["thresholds"][32:]).all()
    assert (np.diff(sw["thresholds"][1:32]) <= 0).all()
    # the unfiltered replay is the per-frame score's host statement, exactly
    _, scorers, _ = S.host_sequence(**W.SHAPE)
    for b, s in enumerate(scorers):
        assert [s.final()[k] for k in W.COUNTERS] == sw["counters"][0, b].tolist() and s.iou_sum == sw["iou_sums"][0, b], b
    cen = W.census(logs, sw)
    print("census:", cen)
    assert cen["freed_matches"] > 0 and cen["idsw_values"] > 10 and cen["mt_values"] > 1 and cen["ml_values"] > 1, cen
    assert cen["tracks_sharing_a_score"] >= 24, cen
    # a clip boundary separates the scores of one track id
    assert any(len({c for c, t in tab if t == tid}) > 1 for tab in sw["tables"] for _, tid in tab)
    # the raw confidences are there for the order of the sums: some track's sum depends on it
    _, _, rlogs, rsw = W.planned(raw=True)
    differ = 0
    for lb in rlogs:
        acc = {}
        clip = 0
        for e in lb:
            clip += int(e["reset"])
            for tid, c, _, _ in e["dets"]:
                acc.setdefault((clip, tid), []).append(float(c))
        differ += sum(1 for v in acc.values() if sum(v) != sum(reversed(v)))
    assert differ > 0 and rsw["reached"] > 0


# ---- the constructor -------------------------------------------------------------------------------------------------------------------
def test_constructor_and_update_raw_refuse_half_a_log():
    with pytest.raises(ValueError, match="sweep_frames=8 and sweep_records=None must be given together"):
        TS.TrackScorer(streams=2, device="cpu", sweep_frames=8)
    with pytest.raises(ValueError, match="sweep_frames=None and sweep_records=64 must be given together"):
        TS.TrackScorer(streams=2, device="cpu", sweep_records=64)
    with pytest.raises(ValueError, match="must be at least 1"):
        TS.TrackScorer(streams=2, device="cpu", sweep_frames=0, sweep_records=64)
    plain = TS.TrackScorer(streams=2, max_objects=8, max_boxes=8, device="cpu")
    assert not plain.logging and not hasattr(plain, "log_cursor")
    with pytest.raises(RuntimeError, match="keeps no log"):
        plain.sweep()
    s = TS.TrackScorer(streams=2, max_objects=8, max_boxes=8, device="cpu", sweep_frames=4, sweep_records=32)
    assert s.logging and tuple(s.log_frame.shape) == (2, 4, 4) and tuple(s.log_iou.shape) == (2, 32) and int(s.log_cursor.sum()) == 0
    import torch
    gobj = TS.GtObjects(max_boxes=8, points=16, count=torch.zeros(2, dtype=torch.int32), n_valid=None)
    pc1, obj = torch.zeros(2, 3, 16), torch.zeros(2, 16, dtype=torch.int32)
    num, ids = torch.zeros(2, dtype=torch.int32), torch.zeros(2, 8, dtype=torch.int32)
    with pytest.raises(ValueError, match="update_raw needs object_conf"):
        s.update_raw(pc1, obj, num, ids, gobj)
    with pytest.raises(ValueError, match="update_raw needs object_conf"):
        s.update_raw(pc1, obj, num, ids, gobj, object_conf=torch.zeros(2, 4))
    # the native side refuses a null log before any launch
    a = TS.ScoreIn(2, 256, 8, 8, 8)
    with pytest.raises(_lib.RtkError, match="null log block"):
        _lib.call("rtk_track_score_logged", ctypes.addressof(a), ctypes.addressof(TS.ScoreState()), ctypes.addressof(TS.ScoreOut()), None, None)
    lg = abi.ScoreLog(4, 32)
    with pytest.raises(_lib.RtkError, match="T=100000 track-table entries need \\d+ bytes of LDS per stream, the limit is 65536"):
        _lib.call("rtk_score_replay", 2, 100000, ctypes.addressof(lg), None, None, None, 1, None, None, None, None)
