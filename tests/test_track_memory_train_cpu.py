"""CPU: training the re-acquisition -- rtk_track_score_memory (csrc/track_score.hip), TrackScorer(track_memory=True) and
SequenceTrainer(reacquire=...): declared, exported, built without scratch; the host statement of the record on hand-written cases;
arguments refused before any device is touched."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import _track_memory_train_util as M
from _util import SCORE_VARIANTS, score_kernel_notes
from ratrack_amd import _lib, abi, build as B, track_score as TS, track_train as TT, tracker as T
from ratrack_amd.track4d import Args, Track4D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 6


# ---- 1. surface -----------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_point():
    text = open(os.path.join(ROOT, "include", "rtk_score.h")).read()
    assert re.search(r"RTK_EXPORT int rtk_track_score_memory\(const rtk_track_score_in_t \*in, const rtk_track_score_state_t \*state,\s+"
                     r"const rtk_track_score_out_t \*out,\s+const rtk_score_log_t \*log[^,]*,\s+const rtk_score_memory_t \*mem,\s+"
                     r"rtk_stream_t stream\);", text)
    assert re.search(r"RTK_EXPORT int rtk_track_score_memory_lds_bytes\(int Kobj, int K, int N\);", text)
    assert re.search(r"#define RTK_SCORE_FLAG_TABLE %d\b" % TS.FLAG_TABLE, text) and TS.FLAG_TABLE == M.FLAG_TABLE == 64
    for field in ("table_ids", "table_count", "row_track", "labelled_coasted"):
        assert re.search(r"\b%s;" % field, text), field
    lib = ctypes.CDLL(B.build(verbose=False))
    for name in ("rtk_track_score_memory", "rtk_track_score_memory_lds_bytes", "rtk_track_score", "rtk_track_score_logged"):
        assert hasattr(lib, name), name
    assert _lib.SIGNATURES["rtk_track_score_memory"] == [ctypes.c_void_p] * 6
    assert [f[0] for f in abi.ScoreMemory._fields_] == ["table_ids", "table_count", "row_track", "labelled_coasted"]
    # the variant keeps Kobj more words of LDS; the plain function keeps its values
    plain, memory = _lib._fn("rtk_track_score_lds_bytes"), _lib._fn("rtk_track_score_memory_lds_bytes")
    for Kobj, Kb, N in ((8, 8, 32), (128, 32, 256), (256, 64, 512)):
        assert memory(Kobj, Kb, N) == plain(Kobj, Kb, N) + 4 * Kobj
    assert memory(257, 8, 32) == -1 and memory(8, 65, 32) == -1
    assert inspect.signature(TS.TrackScorer.__init__).parameters["track_memory"].default is False
    assert inspect.signature(TT.SequenceTrainer.__init__).parameters["reacquire"].default is None
    p = inspect.signature(TS.TrackScorer.update_raw).parameters
    assert p["table_ids"].default is None and p["table_count"].default is None


def test_memory_kernels_build_for_gfx950_without_scratch(tmp_path):
    ts = score_kernel_notes(tmp_path)                # the ten instantiations of the one scoring kernel, and no other
    for k in ("memory", "memory_logged"):            # one instantiation per variant: without and with the log
        assert SCORE_VARIANTS[k][1] and not any(SCORE_VARIANTS[k][2:]), k
        assert (ts[k].private, ts[k].lds, ts[k].wavefront, ts[k].max_threads) == (0, 0, 64, 256), (k, ts[k])


# ---- 2. the host statement on hand-written cases ----------------------------------------------------------------------------------------
def pad(v, fill=-1):
    return list(v) + [fill] * (K - len(v))


def test_a_survivor_is_found_by_its_track_id_and_a_dropped_one_is_not():
    # frame 0: tracks 10, 11, 12 matched to labels 5, 6, -1; nothing coasts
    rec, target, defined, flag = M.host_score_memory(M.empty_record(), [10, 11, 12], [5, 6, -1], 2, pad([10, 11, 12]), 3, K)
    assert (rec["count"], rec["track"], rec["label"], rec["gt"], rec["labelled"]) == (3, [10, 11, 12], [5, 6, -1], 2, 0)
    assert M.ones(target) == [] and defined == 0 and flag == 0
    # frame 1: only track 11 is detected; the table keeps 12 and 10 -- in that order, not the old one: found by id, not by position
    rec1, target, defined, flag = M.host_score_memory(rec, [11], [6], 2, pad([11, 12, 10]), 3, K)
    assert (rec1["count"], rec1["track"], rec1["label"], rec1["labelled"]) == (3, [11, 12, 10], [6, -1, 5], 1)
    assert M.ones(target) == [(1, 0)] and defined == 1 and flag == 0
    # frame 2: label 5 is detected again under track 10 (re-acquired): its one sits on the coasted row 2; track 12, which never matched
    # an object, has an all-zero row; the table dropped track 11's coasted row (truncation): the record follows the table
    rec2, target, defined, flag = M.host_score_memory(rec1, [10], [5], 2, pad([10, 12]), 2, K)
    assert M.ones(target) == [(2, 0)] and target[1] == [0] * K and defined == 1
    assert (rec2["count"], rec2["track"], rec2["label"], rec2["labelled"]) == (2, [10, 12], [5, -1], 0)
    # frame 3: a table that names a track the old record does not hold (it was dropped): not found, -1, no row invented
    rec3, target, _, flag = M.host_score_memory(rec2, [10], [5], 1, pad([10, 11]), 2, K)
    assert (rec3["track"], rec3["label"], rec3["labelled"]) == ([10, 11], [5, -1], 0) and M.ones(target) == [(0, 0)] and flag == 0


def test_a_reset_drops_the_record_and_an_inactive_stream_keeps_it():
    rec, _, _, _ = M.host_score_memory(M.empty_record(), [10, 11], [5, 6], 2, pad([10, 11]), 2, K)
    rec, _, _, _ = M.host_score_memory(rec, [11], [6], 2, pad([11, 10]), 2, K)
    assert rec["label"] == [6, 5] and rec["labelled"] == 1
    same, target, defined, flag = M.host_score_memory(rec, [], [], 0, pad([]), 0, K, active=False)
    assert same is rec and M.ones(target) == [] and (defined, flag) == (0, 0)
    # the reset stream: no target, and a survivor named by the table (a reset tracker has none) is not looked up in the dropped record
    new, target, defined, _ = M.host_score_memory(rec, [20], [5], 2, pad([20, 10]), 2, K, reset=True)
    assert M.ones(target) == [] and defined == 0
    assert (new["count"], new["track"], new["label"], new["labelled"]) == (2, [20, 10], [5, -1], 0)


def test_two_rows_of_one_label_both_get_the_one():
    # the old track 10 (label 5) coasts while label 5 was detected again under the fresh id 30
    rec = dict(count=3, track=[30, 11, 10], label=[5, 6, 5], gt=2, labelled=1)
    new, target, defined, _ = M.host_score_memory(rec, [30, 11], [5, 6], 2, pad([30, 11, 10]), 3, K)
    assert M.ones(target) == [(0, 0), (1, 1), (2, 0)] and defined == 1
    assert new["label"] == [5, 6, 5] and new["labelled"] == 1       # the coasted row keeps its label: the FIRST row of track 10


def test_the_first_row_of_a_track_id_wins():
    rec = dict(count=3, track=[10, 10, 11], label=[7, 8, 9], gt=3, labelled=0)       # (ids are unique in a real table)
    new, _, _, _ = M.host_score_memory(rec, [], [], 1, pad([10, 11]), 2, K)
    assert new["label"] == [7, 9] and new["labelled"] == 2


@pytest.mark.parametrize("count,P,G,gt,labelled,want", [
    (3, 2, 2, 2, 0, 1),          # today's rule
    (3, 2, 2, 0, 1, 1),          # no kept object in the previous frame, but a coasted row remembers one
    (3, 2, 2, 0, 0, 0),          # neither
    (0, 2, 2, 2, 1, 0),          # an empty record
    (-1, 2, 2, 0, 0, 0),         # no record
    (3, 0, 2, 2, 1, 0),          # no detection
    (3, 2, 0, 2, 1, 0),          # no kept object in this frame
])
def test_every_branch_of_aff_defined(count, P, G, gt, labelled, want):
    rows = max(count, 0)
    rec = dict(count=count, track=list(range(rows)), label=[-1] * rows, gt=gt, labelled=labelled)
    _, _, defined, _ = M.host_score_memory(rec, list(range(100, 100 + P)), [-1] * P, G, pad(range(100, 100 + P)), P, K)
    assert defined == want


def test_a_table_count_outside_its_range_is_clamped_and_flagged():
    rec = M.empty_record()
    new, _, _, flag = M.host_score_memory(rec, [10, 11], [5, 6], 2, pad([10, 11]), 1, K)          # below P
    assert flag == M.FLAG_TABLE and new["count"] == 2 and new["track"] == [10, 11]
    new, _, _, flag = M.host_score_memory(rec, [10, 11], [5, 6], 2, pad([10, 11, 12, 13, 14, 15]), K + 3, K)      # above Kobj
    assert flag == M.FLAG_TABLE and new["count"] == K and new["track"] == [10, 11, 12, 13, 14, 15]
    new, _, _, flag = M.host_score_memory(rec, [10, 11], [5, 6], 2, pad([10, 11]), -4, K)
    assert flag == M.FLAG_TABLE and new["count"] == 2


# ---- 3. argument checks ---------------------------------------------------------------------------------------------------------------
def test_bad_reacquire_values_are_refused_before_any_device_check():
    net = Track4D(Args())                       # on the CPU: the refusal comes first
    for bad in (-1, True, False, 1.5, "2"):
        with pytest.raises(ValueError, match="reacquire"):
            TT.SequenceTrainer(net, streams=2, reacquire=bad)
    with pytest.raises(ValueError, match="max_age.*previous frame's detections.*reacquire"):
        TT.SequenceTrainer(net, streams=2, max_age=2)
    with pytest.raises(ValueError, match="needs a model on the GPU"):      # a good value passes on to the checks that were there
        TT.SequenceTrainer(net, streams=2, reacquire=2)


def test_a_memory_scorer_refuses_a_step_without_a_table():
    scorer = TS.TrackScorer(streams=2, max_objects=8, max_boxes=8, max_gt_tracks=16, device="cpu", track_memory=True)
    assert tuple(scorer.row_track.shape) == (2, 8) and scorer.row_track.dtype == torch.int32 and bool((scorer.row_track == -1).all())
    assert tuple(scorer.labelled_coasted.shape) == (2,) and int(scorer.labelled_coasted.sum()) == 0
    plain = TS.TrackScorer(streams=2, max_objects=8, max_boxes=8, max_gt_tracks=16, device="cpu")
    assert not hasattr(plain, "row_track") and not hasattr(plain, "labelled_coasted") and plain.track_memory is False
    out = T.StepResult(max_objects=8, table_ids=None, table_count=None)
    with pytest.raises(ValueError, match="max_age"):
        scorer.update(out, None)
    with pytest.raises(ValueError, match="max_age"):
        scorer.update(T.StepResult(max_objects=8), None)            # a result from before the fields existed
