"""CPU: the native surface and the host half of the result log (include/rtk_fused.h "The result log", csrc/track_results.hip,
ratrack_amd/result_log.py) -- the entry points are declared, built for gfx950 without scratch and exported; `write_frames` writes the
reference's own result files back byte for byte and agrees with vod_io.write_track_results; the formatter is str(float(x)) at the
edges of fp32; every ValueError comes before a device is touched; and the host statement of select splits a track id at a clip
boundary."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _result_log_util as U
from _util import GOLDEN, kernel_notes
from ratrack_amd import _lib, abi, build as B, result_log as RL, vod_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ["rtk_result_log_append", "rtk_result_log_select"]


def test_header_declares_and_library_exports_the_result_log():
    text = open(os.path.join(ROOT, "include", "rtk_fused.h")).read()
    for name in ENTRY:
        assert re.search(r"RTK_EXPORT int %s\(" % name, text), name
    for name, value in (("RTK_RESULT_MAX_OBJECTS", RL.MAX_OBJECTS), ("RTK_RESULT_FLAG_OBJECTS", RL.FLAG_OBJECTS), ("RTK_RESULT_FLAG_STEP", RL.FLAG_STEP),
                        ("RTK_RESULT_FLAG_FULL", RL.FLAG_FULL), ("RTK_RESULT_FLAG_TRACKS", RL.FLAG_TRACKS)):
        assert re.search(r"#define %s %d\b" % (name, value), text), name
    score = open(os.path.join(ROOT, "include", "rtk_score.h")).read()
    assert re.search(r"#define RTK_SCORE_MAX_OBJECTS %d\b" % RL.MAX_OBJECTS, score) and re.search(r"#define RTK_SCORE_SWEEP_TRACKS %d\b" % RL.TRACKS, score)
    assert (U.FLAG_OBJECTS, U.FLAG_STEP, U.FLAG_FULL, U.FLAG_TRACKS, U.TRACKS) == (RL.FLAG_OBJECTS, RL.FLAG_STEP, RL.FLAG_FULL, RL.FLAG_TRACKS, RL.TRACKS)
    lib = ctypes.CDLL(B.build(verbose=False))
    for name in ENTRY:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert abi.STRUCTS["rtk_result_log_t"] is abi.ResultLog
    assert [f[0] for f in abi.ResultLog._fields_][3:] == list(U.TABLES)      # the host statement's tables are the block's, in its order


def test_both_kernels_build_for_gfx950_without_scratch(tmp_path):
    found = {k: v.private for k, v in kernel_notes(os.path.join(B.CSRC, "track_results.hip"), tmp_path)[0].items()}
    for k in ("result_append_kernel", "result_select_kernel"):
        assert [v for name, v in found.items() if k in name] == [0], (k, found)
    assert len(found) == 2, found


# ---- the file text -----------------------------------------------------------------------------------------------------------------
def test_write_frames_writes_the_shipped_result_files_back_byte_for_byte(tmp_path):
    d = os.path.join(GOLDEN, "result_files")
    names = sorted(os.listdir(d))
    assert len(names) == 3
    frames = []
    for name in names:
        rows = vod_io.read_track_results(os.path.join(d, name))
        assert rows
        frames.append((0, int(name.split("_")[-1][:5]), rows))
    tables = U.pack_frames(frames)
    paths = RL.write_frames(str(tmp_path), ["delft_1"], tables)
    assert [os.path.relpath(p, str(tmp_path)) for p in paths] == [os.path.join("delft_1", n.split("_")[-1]) for n in names]
    for name, p in zip(names, paths):
        assert open(p, "rb").read() == open(os.path.join(d, name), "rb").read(), name
    # and the structure read_track_results returns
    got = RL.host_frames(tables, 0)
    for (seq, index, rows), (gseq, gindex, grows) in zip(frames, got):
        assert (seq, index) == (gseq, gindex) and len(rows) == len(grows)
        for (i, c, p), (gi, gc, gp) in zip(rows, grows):
            assert i == gi and c == gc and gp.dtype == np.float64 and np.array_equal(p, gp)


def random_frames(rng, count, max_objects, max_points):
    frames = []
    for f in range(count):
        objects = []
        for j in range(int(rng.integers(0, max_objects + 1))):
            n = int(rng.integers(0 if j % 3 == 1 else 1, max_points + 1))
            conf = np.float32(0.0) if j % 4 == 0 else np.float32(rng.uniform(0.01, 1.0))
            objects.append((int(rng.integers(0, 5000)) * 10 + j, float(conf), (rng.normal(size=(n, 3)) * 40.0).astype(np.float32).astype(np.float64)))
        frames.append((f % 2, 7 + f, objects))
    return frames


def test_write_frames_against_write_track_results_on_random_objects(tmp_path):
    frames = random_frames(np.random.default_rng(5), 9, 6, 5)
    frames.append((1, 99, []))                                         # a frame without objects still gets its (empty) file
    tables = U.pack_frames(frames)
    got_root, want_root = tmp_path / "log", tmp_path / "vod"
    paths = RL.write_frames(str(got_root), ["a", "b"], tables)
    assert len(paths) == len(frames)
    for seq, index, objects in frames:
        objs, confs = {}, []
        for tid, conf, pts in objects:
            t = torch.zeros(1, 6, pts.shape[0], dtype=torch.float32)
            t[0, 3:6] = torch.from_numpy(pts.T).float()
            objs[tid] = t
            confs.append(torch.tensor(conf, dtype=torch.float32))
        vod_io.write_track_results(str(want_root), ["a", "b"][seq], index, objs, confs)
    got, want = U.read_tree(str(got_root)), U.read_tree(str(want_root))
    assert got == want and len(got) == len(frames) and got[os.path.join("b", "00099.txt")] == b""
    assert any(len(v) > 200 for v in got.values())
    # the host statement of the text says the same
    texts = U.file_texts(tables)
    assert {os.path.join(["a", "b"][s], "%05d.txt" % i): t.encode() for (s, i), t in texts.items()} == got
    # keep: a dropped record leaves the file, a frame that loses all of them keeps its empty file
    keep = np.ones(tables["rec_track"].shape, np.uint8)
    keep[0, ::2] = 0
    RL.write_frames(str(tmp_path / "kept"), ["a", "b"], tables, keep)
    texts = U.file_texts(tables, keep)
    assert {os.path.join(["a", "b"][s], "%05d.txt" % i): t.encode() for (s, i), t in texts.items()} == U.read_tree(str(tmp_path / "kept"))
    assert U.read_tree(str(tmp_path / "kept")) != got


def test_the_formatter_is_str_float_at_the_edges_of_fp32():
    tiny = np.array([1, 2, 0x7fffff, 0x800000, 0x80000001], dtype=np.uint32).view(np.float32)      # subnormals, the smallest normal, a negative subnormal
    values = np.concatenate([np.array([0.0, -0.0, 1e-5, 1e16, np.finfo(np.float32).max, -np.finfo(np.float32).max, np.inf, -np.inf, np.nan,
                                       0.1, 1.0, 123456.789, 1e-45, 16777216.0, 0.01], dtype=np.float32), tiny,
                             np.random.default_rng(0).normal(size=200).astype(np.float32) * np.float32(1e3)])
    got = RL.format_values(values)
    want = [str(float(v)) for v in values]
    assert got == want
    assert got[:2] == ["0.0", "-0.0"] and got[2] == "9.999999747378752e-06" and got[3] == "1.0000000272564224e+16"
    assert got[4] == "3.4028234663852886e+38" and got[6:9] == ["inf", "-inf", "nan"] and got[15] == "1.401298464324817e-45"


# ---- every ValueError, before a device is touched -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(streams=0), dict(max_objects=0), dict(max_objects=257), dict(frames=0), dict(records=0), dict(points=0),
                                dict(frames=-3), dict(records=2.5), dict(streams=True), dict(streams=1024, frames=2 ** 19),
                                dict(streams=1024, records=2 ** 21), dict(streams=1024, points=699051)])
def test_the_constructor_refuses_before_any_allocation(kw, monkeypatch):
    def no_allocation(*a, **k):
        raise AssertionError("allocated")
    monkeypatch.setattr(torch, "zeros", no_allocation)
    args = dict(streams=2, max_objects=8, frames=4, records=16, points=64)
    args.update(kw)
    with pytest.raises(ValueError):
        RL.ResultLog(device="cuda", **args)


def test_the_largest_sizes_the_constructor_accepts_are_the_stated_ones():
    RL.check_sizes(1024, 256, 2 ** 19 - 1, 2 ** 21 - 1, 699050)
    RL.check_sizes(1, 256, 1, 1, 1)


@pytest.mark.parametrize("kw", [dict(min_hits=0), dict(min_hits=1.0), dict(min_hits=True), dict(min_track_frames=0), dict(min_track_frames=None),
                                dict(threshold=float("nan")), dict(threshold="0.5"), dict(threshold=torch.zeros(2)),
                                dict(threshold=torch.zeros((), dtype=torch.int64))])
def test_select_and_write_refuse_before_a_launch(kw, tmp_path):
    log = RL.ResultLog(streams=2, max_objects=4, frames=2, records=4, points=8, device="cpu")      # host tensors: a launch would fail
    with pytest.raises(ValueError):
        log.select(**kw)
    with pytest.raises(ValueError):
        log.write(str(tmp_path), ["a"], **kw)
    with pytest.raises(ValueError):
        log.frames(0, **kw)


def test_min_hits_needs_hit_counts_in_every_logged_frame():
    log = RL.ResultLog(streams=1, max_objects=4, frames=2, records=4, points=8, device="cpu")
    assert RL.check_filters(None, 2, 1, hits_logged=True) and not RL.check_filters(None, 1, 1) and RL.check_filters(float("-inf"), 1, 1)
    log.hits_logged = False                      # what an append without object_hits leaves behind
    with pytest.raises(ValueError, match="max_age"):
        log.select(min_hits=2)
    assert RL.check_filters(0.5, 1, 3, hits_logged=False)
    log.clear()
    assert log.hits_logged


def test_append_refuses_other_sizes_before_a_launch():
    log = RL.ResultLog(streams=2, max_objects=4, frames=2, records=4, points=8, device="cpu")
    z = lambda *s: torch.zeros(*s, dtype=torch.int32)
    ok = dict(pc1=torch.zeros(2, 3, 5), obj=z(2, 5), num_objects=z(2), object_ids=z(2, 4), object_conf=torch.zeros(2, 4), seq=0, index=0)
    for bad in (dict(pc1=torch.zeros(2, 4, 5)), dict(obj=z(2, 6)), dict(num_objects=z(3)), dict(object_ids=z(2, 5)), dict(object_conf=torch.zeros(2, 3)),
                dict(object_hits=z(2, 3)), dict(step_flags=z(3))):
        with pytest.raises(ValueError):
            log.append_raw(**dict(ok, **bad))

    class Step:
        max_objects = 5
    with pytest.raises(ValueError, match="max_objects"):
        log.append(Step(), 0, 0)


def test_two_frames_with_one_path_are_refused_before_anything_is_written(tmp_path):
    frames = [(0, 3, [(1, 0.5, np.ones((2, 3)))]), (1, 3, []), (0, 3, [])]
    tables = U.pack_frames(frames)
    with pytest.raises(ValueError, match=r"frame 0 of stream 0 and frame 2 of stream 0"):
        RL.write_frames(str(tmp_path), ["a", "b"], tables)
    assert os.listdir(str(tmp_path)) == []
    two = {k: np.concatenate([v[:, :2], v[:, :2]]) if k not in ("cursor",) else np.array([[1, 1, 2, 0], [1, 1, 2, 0]], np.int32) for k, v in tables.items()
           if k != "flags"}
    with pytest.raises(ValueError, match=r"stream 0 and frame 0 of stream 1"):
        RL.write_frames(str(tmp_path), ["a", "b"], two)
    assert len(RL.write_frames(str(tmp_path), ["a", "b"], two, streams=[1])) == 1      # one of the two streams alone is fine


# ---- the host statement ------------------------------------------------------------------------------------------------------------
def hand_made_log():
    """One stream, five frames, a clip mark on frame 3: id 7 is one track of three records (conf .2 .4 .9) before the mark and another of
    two (.8 .6) after it; id 9 lives in the first clip only, id 4 appears once in the second."""
    log = U.HostLog(1, 4, 8, 16, 32)
    plan = [(False, [(7, 0.2, 2), (9, 0.5, 1)]), (False, [(9, 0.75, 1), (7, 0.4, 2)]), (False, [(7, 0.9, 3)]),
            (True, [(7, 0.8, 1), (4, 0.3, 2)]), (False, [(7, 0.6, 1)])]
    for t, (mark, objects) in enumerate(plan):
        ids, conf, hits = np.zeros((1, 4), np.int32), np.zeros((1, 4), np.float32), np.zeros((1, 4), np.int32)
        obj = np.full((1, 6), -1, np.int32)
        at = 0
        for j, (tid, c, n) in enumerate(objects):
            ids[0, j], conf[0, j], hits[0, j] = tid, c, t + 1
            obj[0, at:at + n] = j
            at += n
        log.append(np.arange(18, dtype=np.float32).reshape(1, 3, 6), obj, [len(objects)], ids, conf, [0], [t], object_hits=hits, reset=[mark])
    return log


def test_the_host_statement_splits_a_track_id_at_a_clip_boundary():
    log = hand_made_log()
    t = log.tables()
    assert t["cursor"][0].tolist() == [5, 8, 13, 0]
    assert U.clips([(int(w[0]), int(w[2]) & 0xffff, int(w[2]) >> 16) for w in t["frame"][0, :5]]) == [[0, 1, 2], [3, 4]]
    keep, score, length, flags = U.select(t)
    f32 = lambda v: np.float64(np.float32(v))
    first = ((f32(0.2) + f32(0.4)) + f32(0.9)) / 3.0
    second = (f32(0.8) + f32(0.6)) / 2.0
    nine = (f32(0.5) + f32(0.75)) / 2.0
    assert first != second
    assert score[0, :8].tolist() == [first, nine, nine, first, first, second, f32(0.3), second]
    assert length[0, :8].tolist() == [3, 2, 2, 3, 3, 2, 1, 2] and keep[0, :8].all() and not keep[0, 8:].any() and not flags.any()
    # a threshold between the two scores of id 7 removes its first track whole and keeps its second
    assert first < 0.6 < second
    keep = U.select(t, threshold=0.6)[0]
    assert keep[0, :8].tolist() == [0, 1, 1, 0, 0, 1, 0, 1]
    # an equal score stays; min_track_frames takes a short track with its first frame; min_hits looks at the record
    assert U.select(t, threshold=second)[0][0, :8].tolist() == [0, 0, 0, 0, 0, 1, 0, 1]
    assert U.select(t, min_track_frames=3)[0][0, :8].tolist() == [1, 0, 0, 1, 1, 0, 0, 0]
    assert U.select(t, min_hits=3)[0][0, :8].tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    # min_hits = 1 asks nothing, as in write_results: records logged without hit counts (rec_hits = 0) are not emptied by it
    bare = dict(t, rec_hits=np.zeros_like(t["rec_hits"]))
    assert U.select(bare, threshold=0.6)[0][0, :8].tolist() == [0, 1, 1, 0, 0, 1, 0, 1] and not U.select(bare, min_hits=2)[0].any()
    # the files at that operating point
    texts = U.file_texts(t, U.select(t, threshold=0.6)[0])
    assert texts[(0, 2)] == "" and texts[(0, 0)].startswith("NA 1 -1 -1 0.5 9 2.0 8.0 14.0\n")
    assert texts[(0, 3)] == "NA 1 -1 -1 %s 7 0.0 6.0 12.0\n" % str(float(np.float32(0.8)))
