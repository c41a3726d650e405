"""CPU: the native surface and the host half of ratrack_amd/track_score.py -- the two entry points are declared, built for gfx950
without scratch and exported; `pack_box_types` follows `pack_boxes`' slot order on the three shipped frames (which contain riders);
the values-from-counters formulae; oversize configurations are refused with the limit stated; and the synthetic sequence of
tests/test_track_score_gpu.py meets its input conditions and holds every situation it is there for."""
import ctypes
import os
import re

import numpy as np
import pytest

import _gt_util as U
import _track_score_util as S
from _util import kernel_notes, score_kernel_notes
from ratrack_amd import build as B
from ratrack_amd import gt_device as G
from ratrack_amd import track_score as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ["rtk_gt_objects", "rtk_track_score", "rtk_gt_objects_lds_bytes", "rtk_track_score_lds_bytes"]


def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "rtk_score.h")).read()
    assert re.search(r"RTK_EXPORT int rtk_gt_objects\(const rtk_gt_objects_in_t \*in, const rtk_gt_objects_out_t \*out, rtk_stream_t stream\);", text)
    assert re.search(r"RTK_EXPORT int rtk_track_score\(const rtk_track_score_in_t \*in, const rtk_track_score_state_t \*state,\s+"
                     r"const rtk_track_score_out_t \*out,\s+rtk_stream_t stream\);", text)
    assert "rtk_bcn_view_t pc1" in text and '#include "rtk_gt.h"' in text
    lib = ctypes.CDLL(B.build(verbose=False))
    for name in ENTRY:
        assert hasattr(lib, name), name
    from ratrack_amd import _lib, fused  # noqa: F401
    assert _lib.SIGNATURES["rtk_gt_objects"] == [ctypes.c_void_p] * 3 and _lib.SIGNATURES["rtk_track_score"] == [ctypes.c_void_p] * 4
    # the constants the Python side restates
    for name, value in (("RTK_SCORE_LDS_LIMIT", TS.LDS_LIMIT), ("RTK_SCORE_MAX_BOXES", TS.MAX_BOXES), ("RTK_SCORE_MAX_OBJECTS", TS.MAX_OBJECTS),
                        ("RTK_SCORE_MAX_POINTS", TS.MAX_POINTS), ("RTK_SCORE_COUNTERS", len(TS.COUNTERS)), ("RTK_SCORE_FLAG_TRACKS", TS.FLAG_TRACKS)):
        assert re.search(r"#define %s %d\b" % (name, value), text), name
    assert TS.COUNTERS == S.COUNTERS


def test_kernels_build_for_gfx950_without_scratch(tmp_path):
    found, _ = kernel_notes(os.path.join(B.CSRC, "track_score.hip"), tmp_path)
    assert [v.private for name, v in found.items() if "gt_objects_kernel" in name] == [0], found
    # the scoring launch: gt_objects_kernel aside, the file holds exactly the ten instantiations of the one kernel template
    ts = score_kernel_notes(tmp_path)
    assert (ts["plain"].private, ts["plain"].lds, ts["plain"].wavefront, ts["plain"].max_threads) == (0, 0, 64, 256), ts["plain"]


def test_pack_box_types_follows_pack_boxes_slot_order_on_the_shipped_frames():
    per_stream, _, _ = U.real_streams()
    bb = G.pack_boxes(per_stream, max_boxes=16, device="cpu")
    types = TS.pack_box_types(per_stream, max_boxes=16, device="cpu")
    assert tuple(types.shape) == (3, 16) and str(types.dtype) == "torch.uint8"
    riders = 0
    for b, item in enumerate(per_stream):
        ids = bb.box_id[0, b].tolist()
        for k, obj_id in enumerate(ids):
            assert int(types[b, k]) == int(obj_id >= 0 and item[0][obj_id].type == "rider"), (b, k)
        riders += int(types[b].sum())
    assert riders >= 1
    assert TS.pack_box_types([None, per_stream[0]], 16, "cpu")[0].sum() == 0
    with pytest.raises(ValueError, match="stream 0, frame 1: .* boxes > max_boxes=1"):
        TS.pack_box_types(per_stream[:1], 1, "cpu")


def test_values_from_counters_and_track_classes():
    #            frames gt  pred tp  fp fn idsw tracks mt pt ml
    c = np.array([10, 40, 50, 30, 20, 10, 4, 8, 5, 2, 1])
    v = TS.values_from_counters(c, 21.0)
    assert v["mota"] == 1 - 34 / 40 and v["moda"] == 1 - 30 / 40 and v["recall"] == 0.75 and v["precision"] == 0.6
    assert v["mt_fraction"] == 0.625 and v["pt_fraction"] == 0.25 and v["ml_fraction"] == 0.125 and v["mean_iou"] == 0.7
    two = TS.values_from_counters(np.stack([c, np.zeros(11, dtype=np.int64)]), np.array([21.0, 0.0]))
    assert two["mota"][0] == v["mota"] and np.isnan(two["mota"][1]) and np.isnan(two["mean_iou"][1]) and np.isnan(two["mt_fraction"][1])
    # matched / seen: 0.8 is not "mostly tracked", 0.2 is not "mostly lost"
    assert TS.classify_tracks([10, 10, 10, 10, 5, 1], [9, 8, 2, 1, 5, 0]) == (2, 2, 2)
    assert S.HostScorer.classify([(None, 10, 9), (None, 10, 8), (None, 10, 2), (None, 10, 1), (None, 5, 5), (None, 1, 0)]) == (6, 2, 2, 2)


def test_oversize_configurations_are_refused_with_the_limit():
    TS.check_fit(32, 1024, 128)                                   # the default case fits
    TS.TrackScorer(streams=2, max_objects=128, max_boxes=32, max_gt_tracks=1024, device="cpu")
    lib = ctypes.CDLL(B.build(verbose=False))
    assert 0 < lib.rtk_gt_objects_lds_bytes(32, 1024) <= TS.LDS_LIMIT and 0 < lib.rtk_track_score_lds_bytes(128, 32, 1024) <= TS.LDS_LIMIT
    with pytest.raises(ValueError, match=r"max_boxes=65 outside \[1, 64\]"):
        TS.check_fit(65, 256)
    with pytest.raises(ValueError, match=r"max_objects=257 outside \[1, 256\]"):
        TS.TrackScorer(streams=2, max_objects=257, max_boxes=32, device="cpu")
    with pytest.raises(ValueError, match=r"need \d+ bytes of LDS per stream, the limit is 65536"):
        TS.check_fit(32, 4096)
    with pytest.raises(ValueError, match=r"max_objects=256, max_boxes=64 and N=256 need \d+ bytes of LDS per stream, the limit is 65536"):
        TS.check_fit(64, 256, 256)
    with pytest.raises(ValueError, match="max_gt_tracks"):
        TS.TrackScorer(streams=2, max_gt_tracks=0, device="cpu")
    # the native side refuses the same sizes before any launch
    from ratrack_amd import _lib
    a = TS.GtObjectsIn(2, 4096, 32)
    o = TS.GtObjectsOut()
    with pytest.raises(_lib.RtkError, match="the limit is 65536"):
        _lib.call("rtk_gt_objects", ctypes.addressof(a), ctypes.addressof(o), None)
    s = TS.ScoreIn(2, 256, 256, 64, 8)
    with pytest.raises(_lib.RtkError, match="the limit is 65536"):
        _lib.call("rtk_track_score", ctypes.addressof(s), ctypes.addressof(TS.ScoreState()), ctypes.addressof(TS.ScoreOut()), None)


def test_synthetic_sequence_meets_its_conditions_and_holds_every_situation():
    seq = S.synthetic_sequence()
    cond = S.input_conditions(seq)
    assert cond["rider_gap"] >= 1e-3 and cond["point_gap"] >= 1e-3 and cond["face_margin"] >= 1e-6 and cond["negative_zero"] == 0, cond
    _, scorers, census = S.host_sequence()
    assert all(v > 0 for v in census.values()), census
    padded = sum(int((fr["n_valid"] < seq["N"]).sum()) for fr in seq["frames"])
    none = sum(1 for fr in seq["frames"] for item in fr["per_stream"] if item is None)
    inactive = sum(int((fr["active"] == 0).sum()) for fr in seq["frames"])
    resets = sum(int(fr["reset"].sum()) for fr in seq["frames"][1:])
    assert padded > 0 and none > 0 and inactive > 0 and resets > 0
    assert len({tuple(fr["active"].tolist()) for fr in seq["frames"]}) > 1      # a changing mask
