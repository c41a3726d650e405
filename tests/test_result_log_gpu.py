"""GPU: the result log (ratrack_amd/result_log.py, csrc/track_results.hip) against the host statement of tests/_result_log_util.py
and against the per-step writer it replaces.  Everything is compared with ==, floats by their bits: the log after every append
(poisoned buffers: the words an append must not touch are compared too), the refusals, the selection, the track scores against the
scorer's own, the files of a tracked sequence against `BatchedTracker.write_results`, and a captured append against eager ones."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _result_log_util as U
import _track_score_util as S
import _track_sweep_util as W
import test_tracker_graph_gpu as TG
from ratrack_amd import _lib, gt_device as G
from ratrack_amd import result_log as RL, tracker as T, track_score as TS, vod_io
from ratrack_amd.captured import capture_graph

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else (a.view(np.int64) if a.dtype == np.float64 else a)


def new_logs(B, K, F, R, P):
    """A device log whose tables hold the poison pattern, and the host statement's log in the same state."""
    log, host = RL.ResultLog(B, K, F, R, P, device=DEV), U.HostLog(B, K, F, R, P, poison=True)
    for name in U.TABLES[1:-1]:
        getattr(log, name).view(torch.int32).fill_(U.POISON)
    return log, host


def assert_same_log(log, host, where):
    """Every word of every table, the ones behind the cursors included; then, stated on its own, that those still hold the poison."""
    got = {n: getattr(log, n).cpu().numpy() for n in U.TABLES}
    for n, want in host.tables().items():
        assert got[n].dtype == want.dtype and np.array_equal(_words(got[n]), _words(want)), (where, n, np.argwhere(_words(got[n]) != _words(want))[:6])
    for b in range(log.B):
        f, r, p = got["cursor"][b, :3]
        assert (got["frame"][b, f:] == U.POISON).all() and (got["tag"][b, f:] == U.POISON).all(), (where, b)
        for n in ("rec_track", "rec_conf", "rec_hits", "rec_size"):
            assert (_words(got[n])[b, r:] == U.POISON).all(), (where, b, n)
        assert (_words(got["points"])[b, p:] == U.POISON).all(), (where, b)


def step(rng, B, N, K, num=None, obj=None, hits=True):
    """One frame of random detections: coordinates, ids, confidences, hits; obj in [-1, num] (num itself belongs to nothing)."""
    num = np.asarray(rng.integers(0, K + 1, size=B) if num is None else num, dtype=np.int32)
    if obj is None:
        obj = np.stack([rng.integers(-1, num[b] + 1, size=N) for b in range(B)]).astype(np.int32)
    return dict(pc1=(rng.normal(size=(B, 3, N)) * 30.0).astype(np.float32), obj=np.asarray(obj, np.int32), num_objects=num,
                object_ids=rng.integers(0, 10 ** 6, size=(B, K)).astype(np.int32), object_conf=rng.uniform(0.0, 1.0, size=(B, K)).astype(np.float32),
                object_hits=rng.integers(1, 5, size=(B, K)).astype(np.int32) if hits else None)


def append_both(log, host, fr, seq, index, step_flags=None, reset=None, active=None, pc1_dev=None):
    B = log.B
    seq, index = np.broadcast_to(np.asarray(seq), (B,)), np.broadcast_to(np.asarray(index), (B,))
    opt = lambda x: None if x is None else _dev(np.asarray(x))
    log.append_raw(_dev(fr["pc1"]) if pc1_dev is None else pc1_dev, _dev(fr["obj"]), _dev(fr["num_objects"]), _dev(fr["object_ids"]),
                   _dev(fr["object_conf"]), seq.tolist(), index.tolist(), object_hits=opt(fr["object_hits"]),
                   step_flags=opt(None if step_flags is None else np.asarray(step_flags, np.int32)), reset=opt(reset), active=opt(active))
    host.append(fr["pc1"], fr["obj"], fr["num_objects"], fr["object_ids"], fr["object_conf"], seq, index, object_hits=fr["object_hits"],
                step_flags=step_flags, reset=reset, active=active)


# ---- append against the host statement ----------------------------------------------------------------------------------------
def case_lane_boundary(rng):
    """N = 65, K = 4, three objects: object 1's columns lie on both sides of the lane 63 / 64 boundary with object 0's and 2's between
    them, -1 columns, and a column whose obj is num_objects (and one above K)."""
    obj = np.full((1, 65), -1, np.int32)
    obj[0, [3, 59, 61, 63, 64]] = 1
    obj[0, [0, 60, 62]] = 0
    obj[0, [1, 2, 58]] = 2
    obj[0, 57], obj[0, 5] = 3, 9
    return 1, 65, 4, [step(rng, 1, 65, 4, num=[3], obj=obj)]


def case_one_column(rng):
    return 1, 1, 3, [step(rng, 1, 1, 3, num=[2], obj=[[1]]), step(rng, 1, 1, 3, num=[1], obj=[[-1]])]


def case_one_point_objects(rng):
    return 1, 256, 256, [step(rng, 1, 256, 256, num=[256], obj=[rng.permutation(256)])]


def case_one_object_owns_every_column(rng):
    return 1, 256, 2, [step(rng, 1, 256, 2, num=[1], obj=np.zeros((1, 256)))]


def case_no_objects_and_an_empty_object(rng):
    obj = rng.choice(np.array([-1, 0, 2]), size=(2, 40))
    return 2, 40, 5, [step(rng, 2, 40, 5, num=[0, 3], obj=obj), step(rng, 2, 40, 5, num=[3, 0], obj=obj)]


def case_many_chunks_per_wave(rng):
    """N = 700: every wave walks three 64-column chunks, the last wave's last one partial."""
    return 2, 700, 9, [step(rng, 2, 700, 9), step(rng, 2, 700, 9, num=[9, 1])]


def case_n_257(rng):
    """N = 257: two chunks each for the first two waves, one column for the third, nothing for the fourth."""
    return 1, 257, 40, [step(rng, 1, 257, 40, num=[40])]


CASES = [case_lane_boundary, case_one_column, case_one_point_objects, case_one_object_owns_every_column, case_no_objects_and_an_empty_object,
         case_many_chunks_per_wave, case_n_257]


@pytest.mark.parametrize("case", CASES, ids=[c.__name__[5:] for c in CASES])
def test_append_equals_the_host_statement(case):
    B, N, K, steps = case(np.random.default_rng(11))
    total = sum(int((s["obj"] >= 0).sum()) for s in steps)
    log, host = new_logs(B, K, len(steps) + 1, K * len(steps) + 2, total + 3)
    assert_same_log(log, host, "empty")
    for t, fr in enumerate(steps):
        append_both(log, host, fr, seq=np.arange(B) + 5, index=100 + t, step_flags=[4] * B)      # (bit 2, dropped coasted tracks: logged)
        assert_same_log(log, host, t)
    log.check()
    assert host.cursor[:, 0].tolist() == [len(steps)] * B and host.cursor[:, 2].sum() > 0 and not host.flags.any()
    if case is case_lane_boundary:
        assert host.rec_size[0, :3].tolist() == [3, 5, 3] and host.cursor[0].tolist() == [1, 3, 11, 0]
        pc1 = steps[0]["pc1"]
        assert np.array_equal(host.points[0, 3:8], pc1[0][:, [3, 59, 61, 63, 64]].T)


def test_append_reads_a_permuted_view_and_skips_an_inactive_stream():
    """pc1 as the (B,3,N) view of a point-major (B,N,3) buffer; B = 3 with stream 1 inactive in the second frame and stream 2 reset."""
    rng = np.random.default_rng(12)
    B, N, K = 3, 130, 6
    log, host = new_logs(B, K, 4, 20, 400)
    for t in range(3):
        fr = step(rng, B, N, K, hits=(t != 1))
        point_major = _dev(np.ascontiguousarray(fr["pc1"].transpose(0, 2, 1)))
        view = point_major.permute(0, 2, 1)
        assert not view.is_contiguous() and view.shape == (B, 3, N)
        active, reset = ([1, 0, 1], [0, 1, 1]) if t == 1 else ([1, 1, 1], [0, 0, 0])
        append_both(log, host, fr, seq=[0, 1, 2], index=t, reset=np.array(reset, np.uint8), active=np.array(active, np.uint8), pc1_dev=view)
        assert_same_log(log, host, t)
    assert host.cursor[:, 0].tolist() == [3, 2, 3] and host.frame[2, 1, 2] >> 16 == 1 and host.frame[1, 1, 2] >> 16 == 0
    assert not log.hits_logged
    with pytest.raises(ValueError, match="max_age"):
        log.select(min_hits=2)
    # min_hits = 1 asks nothing: the records of the frame that came without hit counts (rec_hits = 0) stay under a threshold
    tables = host.tables()
    score = U.select(tables)[1]
    tau = float(np.median(score[0, :tables["cursor"][0, 1]]))
    want = U.select(tables, threshold=tau)
    no_hits = tables["frame"][0, 1, 0]
    assert tables["rec_hits"][0, no_hits] == 0 and want[0][0, no_hits:no_hits + (tables["frame"][0, 1, 2] & 0xffff)].any()
    sel = log.select(threshold=tau)
    assert np.array_equal(sel.keep.cpu().numpy(), want[0]) and np.array_equal(_words(sel.track_score.cpu().numpy()), _words(want[1]))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _refusal(kind, rng, B, N, K):
    """(F, R, P, the frames, per frame the step flags and the active mask, the flag stream 1 must end with)."""
    full = lambda num: step(rng, B, N, K, num=num, obj=np.stack([np.arange(N) % max(n, 1) if n else np.full(N, -1) for n in num]))
    if kind == "frames":          # stream 1 has logged F frames when the others have logged F - 1
        return 2, 40, 100, [full([1, 1, 1]), full([2, 2, 2]), full([3, 3, 3])], [None] * 3, [[0, 1, 0], None, None], U.FLAG_FULL
    if kind == "records":         # 4 + 3 records fit R = 7, 4 + 4 do not
        return 4, 7, 100, [full([4, 4, 4]), full([3, 4, 2])], [None] * 2, [None] * 2, U.FLAG_FULL
    if kind == "points":          # 10 + 10 points fit P = 20, but stream 1's second frame has 11
        a, b = full([2, 2, 2]), full([2, 2, 2])
        a["obj"][:, 10:], b["obj"][:, 10:] = -1, -1
        b["obj"][1, 10] = 1
        return 4, 40, 20, [a, b], [None] * 2, [None] * 2, U.FLAG_FULL
    if kind in ("overflow", "n_valid"):
        word = 1 if kind == "overflow" else 2
        return 4, 40, 100, [full([2, 2, 2]), full([2, 3, 2])], [None, [4, word | 4, 0]], [None] * 2, U.FLAG_STEP
    assert kind == "objects"
    return 4, 40, 100, [full([2, 2, 2]), full([K, K + 1, 0])], [None] * 2, [None] * 2, U.FLAG_OBJECTS


@pytest.mark.parametrize("kind", ["frames", "records", "points", "overflow", "n_valid", "objects"])
def test_a_refused_frame_leaves_its_stream_as_it_was_and_the_others_go_on(kind, tmp_path):
    rng = np.random.default_rng(13)
    B, N, K = 3, 12, 4
    F, R, P, steps, flags, actives, want_flag = _refusal(kind, rng, B, N, K)
    log, host = new_logs(B, K, F, R, P)
    for t, fr in enumerate(steps):
        before = {n: getattr(log, n)[1].clone() for n in U.TABLES}
        append_both(log, host, fr, seq=[0, 1, 2], index=t, step_flags=flags[t], active=None if actives[t] is None else np.array(actives[t], np.uint8))
        assert_same_log(log, host, t)
    # the last frame: stream 1 was refused -- not a word or a cursor of it moved but the flag -- and streams 0 and 2 logged theirs
    assert log.flags.tolist() == [0, want_flag, 0]
    for n in U.TABLES[:-1]:
        assert torch.equal(getattr(log, n)[1], before[n]), n
    frames = log.cursor[:, 0].tolist()
    assert frames[0] == frames[2] == (len(steps) - 1 if kind == "frames" else len(steps)) and frames[1] == (F if kind == "frames" else len(steps) - 1)
    with pytest.raises(RuntimeError, match="stream 1 "):
        log.check()
    with pytest.raises(RuntimeError, match="stream 1 "):
        log.write(str(tmp_path / "checked"), ["a", "b", "c"])
    assert not os.path.exists(str(tmp_path / "checked"))
    paths = log.write(str(tmp_path / "rest"), ["a", "b", "c"], check=False)
    texts = {os.path.join("abc"[s], "%05d.txt" % i): t.encode() for (s, i), t in U.file_texts(host.tables()).items() if s != 1}
    assert U.read_tree(str(tmp_path / "rest")) == texts and len(paths) == len(texts) == frames[0] + frames[2]
    log.clear()
    log.check()
    assert log.cursor.sum().item() == 0


# ---- select -------------------------------------------------------------------------------------------------------------------------
def selection_log():
    """B = 3, ten frames of up to six detections with ids from a pool of eight, so that tracks last; clip marks on stream 0 at frame 4
    and on stream 2 at frames 3 and 7; stream 1 sits frame 5 out."""
    rng = np.random.default_rng(14)
    B, N, K, T_ = 3, 48, 6, 10
    log, host = new_logs(B, K, T_, T_ * K, T_ * N)
    for t in range(T_):
        fr = step(rng, B, N, K)
        for b in range(B):
            fr["object_ids"][b] = rng.permutation(8)[:K]
        fr["object_conf"] = (rng.integers(0, 64, size=(B, K)) / 64.0).astype(np.float32) * rng.uniform(0.9, 1.0, size=(B, K)).astype(np.float32)
        reset = np.array([t == 4, False, t in (3, 7)], np.uint8)
        active = np.array([True, t != 5, True], np.uint8)
        append_both(log, host, fr, seq=[0, 1, 2], index=t, reset=reset, active=active)
    return log, host


@pytest.fixture(scope="module")
def selected():
    log, host = selection_log()
    return log, host, host.tables(), U.select(host.tables())


def assert_same_selection(sel, want, tables, where):
    keep, score, length, flags = want
    assert sel.flags.tolist() == flags.tolist(), where
    assert np.array_equal(sel.keep.cpu().numpy(), keep), (where, "keep")
    assert np.array_equal(_words(sel.track_score.cpu().numpy()), _words(score)), (where, "track_score")
    assert np.array_equal(sel.track_frames.cpu().numpy(), length), (where, "track_frames")


def test_select_equals_the_host_statement(selected):
    log, host, tables, (keep, score, length, flags) = selected
    assert_same_log(log, host, "selection log")
    records = tables["cursor"][:, 1]
    assert keep.sum() == records.sum() and not flags.any()
    assert_same_selection(log.select(), (keep, score, length, flags), tables, "no filter")
    # the same id in two clips of stream 0 is two tracks with two scores
    first, second = tables["frame"][0, 4, 0], records[0]
    ids = tables["rec_track"][0]
    split = [i for i in set(ids[:first].tolist()) & set(ids[first:second].tolist())
             if score[0, :first][ids[:first] == i][0] != score[0, first:second][ids[first:second] == i][0]]
    assert split and tables["frame"][0, 4, 2] >> 16 == 1
    # a threshold equal to a track's score: the track stays
    live = np.sort(np.unique(score[1, :records[1]]))
    tau = float(live[len(live) // 2])
    want = U.select(tables, threshold=tau)
    assert want[0][1, :records[1]][score[1, :records[1]] == tau].all() and 0 < want[0].sum() < keep.sum()
    assert_same_selection(log.select(threshold=tau), want, tables, "equal")
    # between two scores, as a float and as a 0-dim device tensor
    mid = float((live[2] + live[3]) / 2.0)
    assert live[2] < mid < live[3]
    want = U.select(tables, threshold=mid)
    assert_same_selection(log.select(threshold=mid), want, tables, "between")
    assert_same_selection(log.select(threshold=torch.tensor(mid, dtype=torch.float64, device=DEV)), want, tables, "device threshold")
    assert_same_selection(log.select(threshold=float("-inf")), (keep, score, length, flags), tables, "-inf")
    # min_track_frames takes a short track whole, its first frame included
    want = U.select(tables, min_track_frames=3)
    short = (length[0, :records[0]] < 3)
    assert short.any() and not want[0][0, :records[0]][short].any() and want[0][0, :records[0]][~short].all()
    assert_same_selection(log.select(min_track_frames=3), want, tables, "min_track_frames")
    # min_hits together with a threshold
    want = U.select(tables, threshold=mid, min_hits=3)
    assert 0 < want[0].sum() < U.select(tables, threshold=mid)[0].sum()
    assert_same_selection(log.select(threshold=mid, min_hits=3), want, tables, "min_hits and threshold")


def test_filtered_files_are_the_host_statements(selected, tmp_path):
    log, host, tables, (keep, score, length, flags) = selected
    tau = float(np.median(score[keep.astype(bool)]))
    want = U.select(tables, threshold=tau, min_track_frames=2)
    log.write(str(tmp_path), ["a", "b", "c"], threshold=tau, min_track_frames=2)
    texts = {os.path.join("abc"[s], "%05d.txt" % i): t.encode() for (s, i), t in U.file_texts(tables, want[0]).items()}
    assert U.read_tree(str(tmp_path)) == texts and len(texts) == 29
    got = log.frames(2, threshold=tau, min_track_frames=2)
    for seq, index, objects in got:
        rows = vod_io.read_track_results(os.path.join(str(tmp_path), "c", "%05d.txt" % index))
        assert seq == 2 and len(rows) == len(objects)
        for (i, c, p), (gi, gc, gp) in zip(rows, objects):
            assert i == gi and c == gc and np.array_equal(p, gp)


def test_a_clip_with_more_than_2048_track_ids_is_flagged():
    """Stream 0: nine frames of 256 fresh ids in one clip (2304 ids); stream 1: the same frames with a clip mark on each (256 ids a clip)."""
    rng = np.random.default_rng(15)
    B, N, K, T_ = 2, 256, 256, 9
    log, host = RL.ResultLog(B, K, T_, T_ * K, T_ * N, device=DEV), U.HostLog(B, K, T_, T_ * K, T_ * N)
    for t in range(T_):
        fr = step(rng, B, N, K, num=[K, K], obj=np.stack([np.arange(N), np.arange(N)]))
        fr["object_ids"][:] = np.arange(K) + K * t
        append_both(log, host, fr, seq=[0, 1], index=t, reset=np.array([0, 1], np.uint8))
    log.check()
    want = U.select(host.tables(), threshold=0.25)
    assert want[3].tolist() == [U.FLAG_TRACKS, 0] and want[0][1].sum() > 0 and want[0][0].sum() == 0
    sel = log.select(threshold=0.25, check=False)
    assert_same_selection(sel, want, host.tables(), "tracks")
    with pytest.raises(RuntimeError, match="stream 0 .*2048"):
        log.select(threshold=0.25)
    with pytest.raises(RuntimeError, match="stream 0 "):
        log.write("/nonexistent/never/written", ["a", "b"], threshold=0.25)


# ---- the scorer's own track scores ----------------------------------------------------------------------------------------------
def test_track_scores_are_the_scorers_bits():
    """The sweep's planned sequence through a logging TrackScorer and through the result log: every record's track score equals what
    rtk_score_track_means -- the launch `TrackScorer.sweep` starts with -- gives for the scorer's log, record for record."""
    seq, confs, logs, _ = W.planned()
    B, N, K = seq["B"], seq["N"], seq["K"]
    scorer = TS.TrackScorer(streams=B, max_objects=K, max_boxes=K, max_gt_tracks=64, sweep_frames=16, sweep_records=128)
    log = RL.ResultLog(B, K, 16, 128, 16 * N, device=DEV)
    for t, (fr, conf) in enumerate(zip(seq["frames"], confs)):
        pc1, nv = _dev(fr["pc1"]), _dev(fr["n_valid"])
        gobj = TS.gt_objects(pc1, G.pack_boxes(fr["per_stream"], K, DEV), TS.pack_box_types(fr["per_stream"], K, DEV), n_valid=nv, min_obj_points=S.MIN_PTS)
        obj, num, ids, reset, active = (_dev(fr[k]) for k in ("obj", "num", "ids", "reset", "active"))
        scorer.update_raw(pc1, obj, num, ids, gobj, nv, reset, active, object_conf=_dev(conf))
        log.append_raw(pc1, obj, num, ids, _dev(conf), seq=list(range(B)), index=t, reset=reset, active=active)
    scorer.check()
    log.check()
    score = torch.zeros(B, scorer.R, dtype=torch.float64, device=DEV)
    flags = torch.zeros(B, dtype=torch.int32, device=DEV)
    block = scorer._log_block()
    _lib.call("rtk_score_track_means", B, ctypes.addressof(block), score.data_ptr(), flags.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert int(flags.sum()) == 0
    sel = log.select()
    cursor = log.cursor.cpu().numpy()
    assert np.array_equal(cursor[:, :2], scorer.log_cursor.cpu().numpy()[:, :2]) and cursor[:, 1].sum() > 300
    assert torch.equal(log.rec_track, scorer.log_track) and torch.equal(log.rec_conf.view(torch.int32), scorer.log_conf.view(torch.int32))
    assert torch.equal(log.frame[:, :, 0], scorer.log_frame[:, :, 0]) and torch.equal(log.frame[:, :, 2] & 0xffff, scorer.log_frame[:, :, 2] & 0xffff)
    got, want = sel.track_score.cpu().numpy(), score.cpu().numpy()
    for b in range(B):
        r = cursor[b, 1]
        assert np.array_equal(_words(got[b, :r]), _words(want[b, :r])), b
    assert len(np.unique(want)) > 20


# ---- a tracked sequence ------------------------------------------------------------------------------------------------------------
SIZES = [200, 160, 97]
NAMES = ["seq0", "seq1", "seq2"]


def track(net, seq, root, min_hits=None, **kw):
    """The sequence through a BatchedTracker with per-step write_results (into root/steps, and with min_hits into root/steps_hits) and
    with append; -> the log."""
    B = len(SIZES)
    trk = T.BatchedTracker(net, streams=B, **kw)
    log = RL.ResultLog(B, trk.K, TG.STEPS, TG.STEPS * trk.K, TG.STEPS * max(SIZES), device=DEV)
    objects = 0
    with torch.no_grad():
        for t, (pc1, pc2, f1, f2, nv) in enumerate(seq):
            reset, active = TG.masks(t, B)
            out = trk.step(pc1, pc2, f1, f2, n_valid=nv, reset=reset, active=active)
            trk.write_results(os.path.join(root, "steps"), NAMES, [t] * B, out)
            if min_hits is not None:
                trk.write_results(os.path.join(root, "steps_hits"), NAMES, [t] * B, out, min_hits=min_hits)
            log.append(out, seq=[0, 1, 2], index=t, reset=reset)
            objects += int(out.num_objects.sum())
    assert objects > 0
    return log


@pytest.fixture(scope="module")
def tracked(tmp_path_factory):
    net = TG.new_net()
    seq = TG.frames(SIZES, TG.STEPS, 40)
    plain_root, memory_root = str(tmp_path_factory.mktemp("plain")), str(tmp_path_factory.mktemp("memory"))
    return dict(plain=(track(net, seq, plain_root), plain_root), memory=(track(net, seq, memory_root, min_hits=2, max_age=2), memory_root))


@pytest.mark.parametrize("which", ["plain", "memory"])
def test_one_write_gives_the_files_of_per_step_write_results(tracked, which):
    log, root = tracked[which]
    log.check()
    paths = log.write(os.path.join(root, "log"), NAMES)
    want, got = U.read_tree(os.path.join(root, "steps")), U.read_tree(os.path.join(root, "log"))
    assert len(want) == 3 * TG.STEPS - 1 == len(paths) and sum(len(v) for v in want.values()) > 1000      # (one inactive frame)
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
    assert log.hits_logged == (which == "memory")
    # frames(b) is read_track_results of those files
    for b in range(3):
        frames = log.frames(b)
        assert [(s, i) for s, i, _ in frames] == [(b, t) for t in range(TG.STEPS) if not (b == TG.INACTIVE[0] and t == TG.INACTIVE[1])]
        for s, i, objects in frames:
            rows = vod_io.read_track_results(os.path.join(root, "steps", NAMES[s], "%05d.txt" % i))
            assert len(rows) == len(objects)
            for (tid, c, p), (gtid, gc, gp) in zip(rows, objects):
                assert tid == gtid and c == gc and np.array_equal(p, gp) and gp.dtype == np.float64
    # the clip mark of the reset and the frame words
    assert int(log.frame[TG.RESET[0], TG.RESET[1], 2]) >> 16 == 1 and int((log.frame[:, :, 2] >> 16).sum()) == 1


def test_min_hits_gives_the_files_of_write_results_with_min_hits(tracked):
    log, root = tracked["memory"]
    log.write(os.path.join(root, "log_hits"), NAMES, min_hits=2)
    want, got = U.read_tree(os.path.join(root, "steps_hits")), U.read_tree(os.path.join(root, "log_hits"))
    assert sorted(got) == sorted(want) and len(want) == 3 * TG.STEPS - 1
    for name in want:
        assert got[name] == want[name], name
    assert want != U.read_tree(os.path.join(root, "steps"))      # the filter removed something
    # what write_results cannot do: a track of fewer than three frames goes with its first frames
    sel = log.select(min_track_frames=3)
    tables = {n: getattr(log, n).cpu().numpy() for n in U.TABLES}
    assert_same_selection(sel, U.select(tables, min_track_frames=3), tables, "tracked")
    with pytest.raises(ValueError, match="max_age"):
        tracked["plain"][0].write(os.path.join(root, "never"), NAMES, min_hits=2)


# ---- stream capture ---------------------------------------------------------------------------------------------------------------
def test_a_captured_append_replays_with_new_contents():
    rng = np.random.default_rng(16)
    B, N, K = 3, 150, 7
    steps = [step(rng, B, N, K) for _ in range(3)]
    eager, host = new_logs(B, K, 4, 30, 500)
    for t, fr in enumerate(steps):
        append_both(eager, host, fr, seq=[3, 4, 5], index=10 + t, step_flags=[0, 4, 0], reset=np.array([t == 1, 0, 0], np.uint8),
                    active=np.array([1, 1, t != 2], np.uint8))
    assert_same_log(eager, host, "eager")

    log, _ = new_logs(B, K, 4, 30, 500)
    keys = ("pc1", "obj", "num_objects", "object_ids", "object_conf", "object_hits")
    static = {k: torch.zeros_like(_dev(steps[0][k])) for k in keys}
    words = {k: torch.zeros(B, dtype=torch.int32, device=DEV) for k in ("seq", "index", "step_flags")}
    masks = {k: torch.zeros(B, dtype=torch.uint8, device=DEV) for k in ("reset", "active")}
    torch.cuda.synchronize()
    graph, _ = capture_graph(lambda: log.append_raw(static["pc1"], static["obj"], static["num_objects"], static["object_ids"], static["object_conf"],
                                                    words["seq"], words["index"], object_hits=static["object_hits"],
                                                    step_flags=words["step_flags"], reset=masks["reset"], active=masks["active"]))
    assert int(log.cursor.sum()) == 0                        # the capture recorded the launch and executed nothing
    for t, fr in enumerate(steps):
        for k in keys:
            static[k].copy_(_dev(fr[k]))
        words["seq"].copy_(_dev(np.array([3, 4, 5], np.int32)))
        words["index"].fill_(10 + t)
        words["step_flags"].copy_(_dev(np.array([0, 4, 0], np.int32)))
        masks["reset"].copy_(_dev(np.array([t == 1, 0, 0], np.uint8)))
        masks["active"].copy_(_dev(np.array([1, 1, t != 2], np.uint8)))
        graph.replay()
    torch.cuda.synchronize()
    assert_same_log(log, host, "replayed")
