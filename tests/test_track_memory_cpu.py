"""CPU: track memory (BatchedTracker(max_age=...), rtk_track_memory) -- declared, built without scratch, arguments refused before any
launch, and the host statement of its rules (tests/_track_memory_util.py) on hand-written tables."""
import inspect
import os
import re
import subprocess

import pytest
import torch

import _track_memory_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_track_memory_and_the_tracker_takes_max_age():
    from ratrack_amd import abi, tracker as T, track_train as TT
    text = open(os.path.join(ROOT, "include", "rtk_fused.h")).read()
    assert re.search(r"RTK_EXPORT int rtk_track_memory\(", text)
    assert "rtk_track_memory" in abi.SIGNATURES
    assert inspect.signature(T.BatchedTracker.__init__).parameters["max_age"].default is None
    assert inspect.signature(T.BatchedTracker.write_results).parameters["min_hits"].default == 1
    assert inspect.signature(TT.SequenceTrainer.__init__).parameters["max_age"].default is None


def test_track_memory_kernel_builds_for_gfx950_without_scratch(tmp_path):
    from ratrack_amd import build as B
    hipcc = B._hipcc()
    src = os.path.join(B.CSRC, "track_batched.hip")
    out = str(tmp_path / "track_batched.s")
    cmd = [hipcc] + [f for f in B.flags_for(src) if f != "-fPIC"] + ["-I", os.path.join(ROOT, "include"), "-I", B.CSRC, "-S",
                                                                    "--cuda-device-only", "-o", out, src]
    subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
    asm = open(out).read()
    notes = asm[asm.index("amdhsa.kernels"):]
    found = {}
    for e in re.split(r"\n\s+- \.", notes):
        m = re.search(r"\.name:\s+(\S+)", e)
        p = re.search(r"\.private_segment_fixed_size:\s+(\d+)", e)
        if m and p:
            found[m.group(1)] = int(p.group(1))
    assert [v for k, v in found.items() if "track_memory_kernel" in k] == [0], found


def test_bad_max_age_and_min_hits_are_refused():
    from ratrack_amd import tracker as T, track_train as TT
    from ratrack_amd.track4d import Args, Track4D
    net = Track4D(Args()).eval()
    for bad in (-1, 1.5, "2", True):
        with pytest.raises(ValueError, match="max_age"):
            T.BatchedTracker(net, streams=2, max_age=bad)
    with pytest.raises(ValueError, match="max_age.*previous frame's detections"):
        TT.SequenceTrainer(net, streams=2, max_age=2)
    with pytest.raises(ValueError, match="max_age.*previous frame's detections"):
        TT.SequenceTrainer(net, streams=2, max_age=0)
    # write_results: min_hits is checked before anything is read
    trk = T.BatchedTracker.__new__(T.BatchedTracker)
    plain = T.StepResult(object_hits=None)
    for bad in (0, -3, 2.0, True):
        with pytest.raises(ValueError, match="min_hits"):
            trk.write_results("/nonexistent-root", ["a"], [0], plain, min_hits=bad)
    with pytest.raises(ValueError, match="min_hits=2 needs"):
        trk.write_results("/nonexistent-root", ["a"], [0], plain, min_hits=2)
    # the truncation flag: check() names the stream, the accessors whose output is complete do not raise
    with pytest.raises(RuntimeError, match="stream 1 dropped coasted tracks"):
        T.raise_on_flags([0, 4], 8)
    T.raise_on_flags([0, 4], 8, truncation=False)
    with pytest.raises(RuntimeError, match="stream 1 has more than max_objects=8"):
        T.raise_on_flags([0, 5], 8, truncation=False)


def _call_fails(name, *args):
    from ratrack_amd import _lib, fused  # noqa: F401
    with pytest.raises(_lib.RtkError) as e:
        _lib.call(name, *args)
    return str(e.value)


def test_track_memory_arguments_are_validated_before_any_launch():
    from ratrack_amd import tracker as T
    kmax = T.max_objects_limit()
    fake, other = 4096, 8192          # never dereferenced: the checks fail first
    def args(B=2, K=8, max_age=2, **over):
        names = ["active", "reset", "num_objects", "indices1", "object_conf", "prev_ids", "prev_age", "prev_hits", "prev_n_det", "prev_count",
                 "desc_prev", "ids", "age", "hits", "n_det", "count", "desc", "flags", "object_hits", "object_gap", "num_coasted"]
        vals = {n: (other if n in ("ids", "age", "hits", "n_det", "count", "desc") else fake) for n in names}
        vals.update(active=None, reset=None)
        vals.update(over)
        return [B, K, max_age] + [vals[n] for n in names] + [None]
    assert "K=%d" % (kmax + 1) in _call_fails("rtk_track_memory", *args(K=kmax + 1))
    assert "K=0" in _call_fails("rtk_track_memory", *args(K=0))
    assert "max_age=-1" in _call_fails("rtk_track_memory", *args(max_age=-1))
    assert "bad arguments" in _call_fails("rtk_track_memory", *args(B=0))
    for name in ("num_objects", "indices1", "object_conf", "prev_ids", "prev_age", "prev_hits", "prev_n_det", "prev_count", "desc_prev", "ids",
                 "age", "hits", "n_det", "count", "desc", "flags", "object_hits", "object_gap", "num_coasted"):
        assert "bad arguments" in _call_fails("rtk_track_memory", *args(**{name: None})), name
    assert "alias" in _call_fails("rtk_track_memory", *args(ids=fake))


# ---- the host statement on hand-written tables --------------------------------------------------------------------------------------
def table(K, ids, age, hits, n_det):
    t = U.empty_table(K)
    c = len(ids)
    t["ids"][:c], t["age"][:c], t["hits"][:c] = ids, age, hits
    t.update(n_det=n_det, count=c)
    return t


def pad(x, K, fill):
    return list(x) + [fill] * (K - len(x))


def test_host_statement_matched_aged_and_dying_rows():
    K = 8
    prev = table(K, ids=[10, 11, 12, 13], age=[0, 0, 1, 2], hits=[3, 1, 5, 2], n_det=2)
    # object 0 inherits row 1 (id 11); object 1 points at row 0 with conf 0: a fresh id, row 0 stays unmatched
    new, out = U.host_step(prev, pad([1, 0], K, -1), pad([0.8, 0.0], K, 0.0), 2, pad([11, 40], K, -1), False, True, max_age=2)
    # survivors in increasing i: row 0 (age 0 -> 1), row 2 (age 1 -> 2); row 3 (age 2 -> 3 > max_age) dies
    assert new["ids"] == [11, 40, 10, 12, -1, -1, -1, -1]
    assert new["age"] == [0, 0, 1, 2, 0, 0, 0, 0]
    assert new["hits"] == [2, 1, 3, 5, 0, 0, 0, 0]
    assert (new["n_det"], new["count"]) == (2, 4)
    assert out["object_hits"] == pad([2, 1], K, 0) and out["object_gap"] == pad([0, -1], K, -1)
    assert out["num_coasted"] == 2 and not out["truncated"]
    assert out["src"] == [None, None, 0, 2, None, None, None, None]
    # max_age = 0: the bookkeeping without coasting
    new0, out0 = U.host_step(prev, pad([1, 0], K, -1), pad([0.8, 0.0], K, 0.0), 2, pad([11, 40], K, -1), False, True, max_age=0)
    assert new0["ids"] == pad([11, 40], K, -1) and new0["count"] == 2 and new0["hits"] == pad([2, 1], K, 0)
    assert out0["object_hits"] == out["object_hits"] and out0["object_gap"] == out["object_gap"] and out0["num_coasted"] == 0


def test_host_statement_reacquired_track_reports_its_gap():
    K = 6
    prev = table(K, ids=[7, 8, 9], age=[0, 2, 1], hits=[4, 6, 2], n_det=1)
    new, out = U.host_step(prev, pad([1, 0], K, -1), pad([0.7, 0.9], K, 0.0), 2, pad([8, 7], K, -1), False, True, max_age=3)
    assert out["object_gap"] == pad([2, 0], K, -1)            # id 8 comes back after 2 missed frames, id 7 was seen last frame
    assert out["object_hits"] == pad([7, 5], K, 0)
    assert new["ids"] == [8, 7, 9, -1, -1, -1] and new["age"] == [0, 0, 2, 0, 0, 0] and new["hits"] == [7, 5, 2, 0, 0, 0]


def test_host_statement_truncates_at_k_and_says_so():
    K = 4
    prev = table(K, ids=[1, 2, 3, 4], age=[0, 0, 1, 0], hits=[1, 1, 2, 1], n_det=3)
    new, out = U.host_step(prev, pad([-1, -1], K, -1), pad([0.0, 0.0], K, 0.0), 2, pad([20, 21], K, -1), False, True, max_age=5)
    assert new["ids"] == [20, 21, 1, 2] and new["age"] == [0, 0, 1, 1] and new["count"] == 4       # rows 2, 3 of prev do not fit
    assert out["truncated"] and out["num_coasted"] == 2 and out["src"] == [None, None, 0, 1]
    full, out_full = U.host_step(prev, pad([], K, -1), pad([], K, 0.0), 0, pad([], K, -1), False, True, max_age=5)
    assert not out_full["truncated"] and full["count"] == 4                                      # exactly K rows: nothing dropped


def test_host_statement_reset_inactive_and_empty_frames():
    K = 5
    prev = table(K, ids=[1, 2, 3], age=[0, 1, 0], hits=[2, 3, 1], n_det=2)
    prev["ids"][4] = 77                                       # beyond count: carried by an inactive frame bit for bit, dropped otherwise
    # reset: the previous table is ignored, even where indices1 names a row
    new, out = U.host_step(prev, pad([0], K, -1), pad([0.9], K, 0.0), 1, pad([30], K, -1), True, True, max_age=3)
    assert new == dict(ids=[30, -1, -1, -1, -1], age=[0] * K, hits=[1, 0, 0, 0, 0], n_det=1, count=1)
    assert out["object_gap"] == [-1] * K and out["num_coasted"] == 0
    # inactive: the table is the previous one, nothing ages
    new, out = U.host_step(prev, pad([], K, -1), pad([], K, 0.0), 0, pad([], K, -1), False, False, max_age=3)
    assert new == prev and new is not prev and out["num_coasted"] == 1 and out["object_hits"] == [0] * K
    # an active frame without objects ages every row; max_age = 1 lets the row of age 1 die
    new, out = U.host_step(prev, pad([], K, -1), pad([], K, 0.0), 0, pad([], K, -1), False, True, max_age=1)
    assert new["ids"] == [1, 3, -1, -1, -1] and new["age"] == [1, 1, 0, 0, 0] and new["hits"] == [2, 1, 0, 0, 0]
    assert (new["n_det"], new["count"], out["num_coasted"]) == (0, 2, 2)


def test_distance_affinity_is_the_closed_form():
    aff = U.distance_affinity(4.0, 4.0)
    g = torch.Generator().manual_seed(1)
    d = torch.randn(32, U.DESC, generator=g) * 3.0
    with torch.no_grad():
        got = aff.affinity(d).reshape(-1)
    want = torch.sigmoid(4.0 - 4.0 * d[:, :3].abs().sum(dim=1))
    assert torch.allclose(got, want, rtol=0, atol=1e-6)
    from ratrack_amd import tracker as T
    assert T.pack_affinity(aff).numel() == 141 * 564 + 564 + 564 * 282 + 282 + 282 * 70 + 70 + 70 * 35 + 35 + 35 + 1
