"""GPU: the track box filter (ResultLog.filter_boxes, csrc/track_box_filter.hip, csrc/box_filter.h) against the host statement of
tests/_box_filter_util.py.  Every word of box, valid, vel, state, aligned, link and flags is compared by its bits: the rule has no
transcendental function and rounds every operation on its own, so there is no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

import _box_filter_util as K
import _box_fit_util as F
import _result_log_util as U
import test_track_boxes_gpu as TBG
from ratrack_amd import boxes as BX, result_log as RL
from ratrack_amd.captured import capture_graph

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAX_GAP = 3
FLOATS, INTS = ("box", "vel", "state", "aligned"), ("valid", "link", "flags")
MODES = [(sym, sm, sz) for sym in (2, 4) for sm in (0, 1) for sz in (0, 1)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def poisoned(B, rows):
    into = BX.FilteredBoxes.empty(B, rows, DEV)
    for n in FLOATS + INTS:
        getattr(into, n).view(torch.int32).fill_(K.POISON)
    return into


def device_boxes(box, valid):
    """The statement's per-record boxes as the ObjectBoxes the launch reads."""
    B, R = valid.shape
    return BX.ObjectBoxes(_dev(box), torch.zeros(B, R, dtype=torch.int32, device=DEV), _dev(valid), torch.zeros(B, dtype=torch.int32, device=DEV))


def assert_same(got, want, where):
    """got: a FilteredBoxes; want: the statement's dict.  Every word of every row, the poison behind the cursors included."""
    for n in INTS:
        g = getattr(got, n).cpu().numpy()
        assert np.array_equal(g, want[n]), (where, n, np.argwhere(g != want[n])[:6].tolist())
    for n in FLOATS:
        g = getattr(got, n).cpu().numpy().view(np.int64)
        w = np.ascontiguousarray(want[n]).view(np.int64)
        assert np.array_equal(g, w), (where, n, np.argwhere(g != w)[:6].tolist())


def spec(rng, shift=0):
    """B = 3 streams.  Stream 0: 24 frames in one clip, frame 12 with 70 records whose duplicates straddle a wave, frame numbers with
    gaps of 1, 2, max_gap, max_gap + 1, 0 and -2.  Stream 1: two clips that share their ids.  Stream 2: five frames."""
    pool = [3, 4, 5, 8, 9, 11, 12, 20, 21, 30]
    gaps = [1, 1, 2, 1, MAX_GAP, 1, MAX_GAP + 1, 1, 1, 0, 1, 2, 1, -2, 1, 1, MAX_GAP, 2, 1, 1, MAX_GAP + 1, 1, 1]
    ids = lambda: [int(v) + shift for v in rng.permutation(pool)[:int(rng.integers(3, 9))]]
    s0, n = [], 5
    for f in range(24):
        row = ids()
        if f == 12:
            row = [100 + i + shift for i in range(70)]
            row[66], row[64], row[69] = row[10], row[63], pool[0] + shift      # lanes 10 | 66 and 63 | 64 of one id; 69: a pool id
            row[2] = pool[1] + shift
        if f == 5:
            row = row + [row[0]]                                             # a duplicate in a small frame
        s0.append((n, f == 0, row))
        n += gaps[f] if f < len(gaps) else 1
    s1 = [(10 + 2 * f if f < 9 else 7 + f, f in (0, 9), ids()) for f in range(20)]
    s2 = [(f, f == 0, ids()) for f in range(5)]
    return [s0, s1, s2]


def inputs(rng, tables):
    """Random boxes for every record slot, a valid word of -1 and one of 0, and a keep mask that drops a tenth."""
    B, R = tables["rec_track"].shape
    box, valid = K.random_boxes(rng, B, R), rng.integers(1, 9, size=(B, R)).astype(np.int32)
    valid[0, 7], valid[0, 20], valid[1, 3] = -1, 0, -1
    keep = (rng.uniform(size=(B, R)) >= 0.1).astype(np.uint8)
    return box, valid, keep


@pytest.fixture(scope="module")
def logged():
    rng = np.random.default_rng(31)
    host = K.ids_log(spec(rng), poison=True)
    tables = host.tables()
    assert tables["cursor"][:, 0].tolist() == [24, 20, 5] and tables["cursor"][0, 1] < host.R - 2 and host.K == 70
    box, valid, keep = inputs(rng, tables)
    return TBG.upload(host), tables, box, valid, keep


@pytest.mark.parametrize("symmetry,smooth,size_rule", MODES)
def test_the_launch_equals_the_statement(logged, symmetry, smooth, size_rule):
    log, tables, box, valid, keep = logged
    par = dict(symmetry=symmetry, smooth=smooth, size_rule=size_rule, size_percent=90, max_gap=MAX_GAP, q_vel=0.25, r_yaw=0.5)
    src = device_boxes(box, valid)
    for mask in (None, keep):
        want = K.filter_log(tables, box, valid, keep=mask, par=K.Par(**par), poison=True)
        into = poisoned(log.B, log.R)
        got = log.filter_boxes(src, keep=None if mask is None else _dev(mask), filter=BX.BoxFilter(**par), into=into)
        assert got is into and got.cand is src.cand
        assert_same(got, want, (symmetry, smooth, size_rule, mask is not None))
        assert want["flags"].tolist() == [K.FLAG_DUPLICATE, 0, 0]
    # the log has what the test is about: every gap case, segments of many members, duplicates on both sides of lane 63
    link = want["link"][0, :int(tables["cursor"][0, 1])]
    assert set(link[:, 1].tolist()) >= {-1, 1, 2, MAX_GAP} and (link[:, 0] >= 0).sum() > 40
    r12 = int(tables["frame"][0, 12, 0])
    full = K.filter_log(tables, box, valid, par=K.Par(**par))
    assert full["valid"][0, r12 + 10] > 0 and full["valid"][0, r12 + 66] == 0 and full["valid"][0, r12 + 63] > 0 and full["valid"][0, r12 + 64] == 0


def test_nothing_at_or_beyond_a_cursor_is_written_and_two_runs_agree(logged):
    log, tables, box, valid, keep = logged
    flt = BX.BoxFilter(smooth=1, size_rule=1, max_gap=MAX_GAP)
    src = device_boxes(box, valid)
    a, b = log.filter_boxes(src, filter=flt, into=poisoned(log.B, log.R)), log.filter_boxes(src, filter=flt, into=poisoned(log.B, log.R))
    for s in range(log.B):
        r = int(tables["cursor"][s, 1])
        assert r < log.R
        for n in FLOATS + ("valid", "link"):
            assert (getattr(a, n)[s, r:].view(torch.int32) == K.POISON).all(), (s, n)
            assert not (getattr(a, n)[s, :r].reshape(r, -1).view(torch.int32) == K.POISON).all(dim=1).any(), (s, n)
    for n in FLOATS + INTS:
        assert torch.equal(getattr(a, n).view(torch.int32), getattr(b, n).view(torch.int32)), n
    # without into= the rows behind the cursors are zero, and check() names the stream with the duplicate
    fresh = log.filter_boxes(src, filter=flt)
    r = int(tables["cursor"][2, 1])
    assert int(fresh.box[2, r:].abs().sum()) == 0 and int(fresh.link[2, r:].abs().sum()) == 0 and torch.equal(fresh.box[2, :r], a.box[2, :r])
    with pytest.raises(RuntimeError, match="stream 0 .*one track id"):
        fresh.check()


def test_a_clip_of_too_many_ids_is_refused_for_its_stream_only():
    """33 frames x 64 distinct ids in one clip (2112 > 2048 + a wave) behind a small clip.  The second stream is filtered: 64 tracks
    over 36 frames, 2304 records, with a break after frame 32, so that 64 segments begin beyond record 2048 -- the extent rule serves
    segments in windows of 2048 first members, and these are in the second."""
    rng = np.random.default_rng(32)
    s0 = [(0, True, [1, 2, 3]), (1, False, [3, 2])] + [(f, f == 2, [1000 + 64 * f + i for i in range(64)]) for f in range(2, 35)] + [(40, True, [5])]
    s1 = [(f if f < 33 else f + 10, f == 0, list(range(64))) for f in range(36)]
    host = K.ids_log([s0, s1], poison=True)
    tables = host.tables()
    box, valid = K.random_boxes(rng, 2, host.R), np.ones((2, host.R), np.int32)
    par = dict(smooth=1, size_rule=1, size_percent=60)
    want = K.filter_log(tables, box, valid, par=K.Par(**par), poison=True)
    assert want["flags"].tolist() == [K.FLAG_TRACKS, 0] and want["valid"][0, :5].tolist() == [1] * 5 and (want["valid"][0, 5:5 + 33 * 64 + 1] == 0).all()
    first = want["link"][1, :2304, 3]
    assert (first < 64).sum() == 33 * 64 and ((first >= 2112) & (first < 2176)).sum() == 3 * 64 and tables["cursor"][1, 1] == 2304
    got = TBG.upload(host).filter_boxes(device_boxes(box, valid), filter=BX.BoxFilter(**par), into=poisoned(2, host.R))
    assert_same(got, want, "overflow")
    with pytest.raises(RuntimeError, match="stream 0 .*2048"):
        got.check()


def test_a_captured_launch_replays_on_another_logs_contents():
    rng = np.random.default_rng(33)
    specs = [spec(rng, shift) for shift in (0, 50)]
    dims = tuple(max(d) for d in zip(*(K.ids_dims(s) for s in specs)))
    hosts = [K.ids_log(s, dims=dims) for s in specs]
    assert not np.array_equal(hosts[0].cursor, hosts[1].cursor)
    log = TBG.upload(hosts[0])
    src = device_boxes(np.zeros((log.B, log.R, 8)), np.zeros((log.B, log.R), np.int32))
    keep = torch.ones(log.B, log.R, dtype=torch.uint8, device=DEV)
    flt = BX.BoxFilter(smooth=1, size_rule=1, max_gap=MAX_GAP, size_percent=75)
    into = poisoned(log.B, log.R)
    torch.cuda.synchronize()
    graph, out = capture_graph(lambda: log.filter_boxes(src, keep=keep, filter=flt, into=into))
    assert out is into and int(into.link[0, 0, 0]) == K.POISON                   # the capture recorded the launch and executed nothing
    for host in reversed(hosts):
        tables = host.tables()
        box, valid, mask = inputs(rng, tables)
        for n in U.TABLES:
            getattr(log, n).copy_(_dev(getattr(host, n)))
        src.box.copy_(_dev(box)); src.valid.copy_(_dev(valid)); keep.copy_(_dev(mask))
        for n in FLOATS + INTS:
            getattr(into, n).view(torch.int32).fill_(K.POISON)
        graph.replay()
        torch.cuda.synchronize()
        assert_same(into, K.filter_log(tables, box, valid, keep=mask, par=K.Par(**{n: getattr(flt, n) for n in BX.BoxFilter.FIELDS}), poison=True),
                    "replay")


def test_write_kitti_with_a_filter_and_without(tmp_path):
    """Integer grids (exact ties: the fitted yaw is exactly 0 or -pi/2, so the per-frame boxes are the statement's bit for bit) on four
    tracks per stream; with a filter the files hold the statement's filtered boxes, without one today's files."""
    rng = np.random.default_rng(34)
    B, N, Kobj, frames = 2, 80, 4, 6
    host = U.HostLog(B, Kobj, frames, frames * Kobj, frames * N)
    for t in range(frames):
        records = [[TBG.grid(int(rng.integers(1, 5)), int(rng.integers(1, 5)), at=(3 * t + int(rng.integers(-2, 3)), 10 * j + int(rng.integers(-2, 3))), z=j)
                    for j in range(3)] + [np.zeros((0, 3), np.float32) if t % 2 else np.array([[t, 40, 1]], np.float32)] for _ in range(B)]
        pc1, obj, num = TBG.frame_of(rng, records, N, Kobj)
        ids = np.tile(np.array([11, 12, 13, 14], np.int32), (B, 1))
        host.append(pc1, obj, num, ids, (rng.integers(1, 64, size=(B, Kobj)) / 64.0).astype(np.float32), seq=[1, 0], index=[7 + t + (t > 3)] * B,
                    object_hits=np.ones((B, Kobj), np.int32), reset=[t == 0, t in (0, 3)])
    tables = host.tables()
    log = TBG.upload(host)
    names = ["second", "first"]
    plain = F.log_boxes(tables, min_extent=0.5)
    log.write_kitti(str(tmp_path / "plain"), names, min_extent=0.5)
    texts = F.kitti_text(tables, plain[0], plain[2])
    assert U.read_tree(str(tmp_path / "plain")) == {names[s] + ".txt": t.encode() for s, t in texts.items()}
    for k, (flt, sel) in enumerate(((BX.BoxFilter(), {}), (BX.BoxFilter(smooth=1, size_rule=1, size_percent=100), dict(min_track_frames=4)))):
        keep = U.select(tables, **sel)[0] if sel else None
        fitted = F.log_boxes(tables, keep=keep, min_extent=0.5)
        want = K.filter_log(tables, fitted[0], fitted[2], keep=keep, par=K.Par(**{n: getattr(flt, n) for n in BX.BoxFilter.FIELDS}))
        assert want["flags"].tolist() == [0, 0] and (want["valid"] > 0).sum() >= 20
        log.write_kitti(str(tmp_path / str(k)), names, min_extent=0.5, filter=flt, **sel)
        filtered = F.kitti_text(tables, want["box"], want["valid"], keep)
        # (a sequence whose every record was dropped still gets its file, empty, as without a filter)
        assert U.read_tree(str(tmp_path / str(k))) == {names[s] + ".txt": filtered.get(s, "").encode() for s in (0, 1)}
        assert filtered != texts and sum(t.count("\n") for t in filtered.values()) == int((want["valid"] > 0).sum())
    # the filtered result goes through download as an ObjectBoxes does, with its velocity rows
    fb = log.filter_boxes(log.boxes(min_extent=0.5))
    hostd, _, _ = log.download(boxes=fb)
    r = hostd["box"].shape[1]
    assert np.array_equal(hostd["box_vel"].view(np.int64), fb.vel[:, :r].cpu().numpy().view(np.int64)) and hostd["box_flags"].tolist() == [0, 0]
    assert np.array_equal(hostd["box_valid"], fb.valid[:, :r].cpu().numpy())
