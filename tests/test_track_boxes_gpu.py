"""GPU: oriented boxes (ratrack_amd/boxes.py, csrc/track_boxes.hip, csrc/box_fit.h) against the host statement of
tests/_box_fit_util.py.  cand, valid and flags are compared with ==, every float but yaw by its bits, yaw within 4e-15 (3 ulp at
|yaw| <= pi: the device's atan2 is good to 2 ulp, the host's to 1).  Random clouds are drawn so that the statement's runner-up area
exceeds the winner's by a relative 1e-6 (asserted; a cloud that misses it is redrawn), exact ties use small-integer coordinates only."""
import os

import numpy as np
import pytest
import torch

import _box_fit_util as F
import _result_log_util as U
import test_tracker_graph_gpu as TG
from ratrack_amd import boxes as BX, result_log as RL, tracker as T
from ratrack_amd.captured import capture_graph

pytestmark = pytest.mark.gpu
DEV = "cuda"
YAW_TOL = 4e-15
YAW = 6


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def poisoned(B, rows):
    into = BX.ObjectBoxes.empty(B, rows, DEV)
    for t in (into.box, into.cand, into.valid, into.flags):
        t.view(torch.int32).fill_(F.POISON)
    return into


def assert_same_boxes(got, want, where):
    """got: an ObjectBoxes; want: the statement's (box, cand, valid, flags).  Every word of every row, poison included."""
    box, cand, valid, flags = want[:4]
    g = got.box.cpu().numpy()
    assert got.flags.cpu().tolist() == flags.tolist(), (where, "flags")
    assert np.array_equal(got.cand.cpu().numpy(), cand), (where, "cand", np.argwhere(got.cand.cpu().numpy() != cand)[:6])
    assert np.array_equal(got.valid.cpu().numpy(), valid), (where, "valid")
    rest = [k for k in range(8) if k != YAW]
    same = np.ascontiguousarray(g[..., rest]).view(np.int64) == np.ascontiguousarray(box[..., rest]).view(np.int64)
    assert same.all(), (where, "box", np.argwhere(~same)[:6])
    off = np.abs(g[..., YAW] - box[..., YAW])
    print("   %s: yaw differs in %d of %d rows, at most %.3g" % (where, int((off > 0).sum()), off.size, float(off.max()) if off.size else 0.0))
    assert (off <= YAW_TOL).all(), (where, "yaw", float(off.max()))


def cloud(rng, n):
    """n points of an elongated cluster somewhere within 30 m, fp32; redrawn until the statement's margin holds."""
    while True:
        a = rng.uniform(0.0, np.pi)
        rot = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        xy = (rng.normal(size=(n, 2)) * [2.0, 0.6]) @ rot.T + rng.uniform(-30.0, 30.0, size=2)
        pts = np.column_stack([xy, rng.uniform(-1.0, 1.0, size=n)]).astype(np.float32)
        box, _, _, runner = F.fit(pts)
        if F.margin_ok(box[7], runner):
            return pts


def grid(w, h, at=(0, 0), z=0):
    """The integer points of a w x h grid: its corners tie exactly, so candidate 0 wins."""
    return np.array([[at[0] + i, at[1] + j, z + (i + j) % 2] for i in range(w + 1) for j in range(h + 1)], np.float32)


def frame_of(rng, records, N, K):
    """Per stream a list of point sets -> (pc1 (B,3,N), obj (B,N), num_objects (B)): the objects' columns scattered over the frame."""
    B = len(records)
    pc1, obj = (rng.normal(size=(B, 3, N)) * 30.0).astype(np.float32), np.full((B, N), -1, np.int32)
    for b, recs in enumerate(records):
        assert len(recs) <= K and sum(len(r) for r in recs) <= N
        cols = rng.permutation(N)[:sum(len(r) for r in recs)]
        at = 0
        for j, pts in enumerate(recs):
            mine = np.sort(cols[at:at + len(pts)])
            pc1[b][:, mine], obj[b, mine] = np.asarray(pts, np.float32).reshape(-1, 3).T, j
            at += len(pts)
    return pc1, obj, np.array([len(r) for r in records], np.int32)


def upload(host):
    log = RL.ResultLog(host.B, host.K, host.F, host.R, host.P, device=DEV)
    for n in U.TABLES:
        getattr(log, n).copy_(_dev(getattr(host, n)))
    return log


# ---- a log against the statement ---------------------------------------------------------------------------------------------------
SIZES = [[[0, 1, 2, 3], [63, 64], [65, 128], [129, 5]],            # stream 0: four frames, the cap in the last
         [[2, 64, "rect"], [3, 65, 1, "grid"]],                    # stream 1: two frames, the exact ties
         []]                                                       # stream 2: nothing logged


@pytest.fixture(scope="module")
def logged():
    """B = 3, record sizes on the lane and wave boundaries of the candidate loop and on the cap; -> the device log, the host tables
    and the statement's boxes, computed once."""
    rng = np.random.default_rng(21)
    B, N, K, frames = 3, 200, 4, 4
    host = U.HostLog(B, K, frames, 12, 4 * N, poison=True)
    for t in range(frames):
        records = []
        for b in range(B):
            sizes = SIZES[b][t] if t < len(SIZES[b]) else []
            records.append([grid(6, 3, at=(-2, 5)) if s == "grid" else grid(1, 1, at=(3, -4), z=2) * [4, 2, 1] if s == "rect" else cloud(rng, s)
                            for s in sizes])
        pc1, obj, num = frame_of(rng, records, N, K)
        host.append(pc1, obj, num, rng.integers(0, 99, size=(B, K)).astype(np.int32), rng.uniform(0, 1, size=(B, K)).astype(np.float32),
                    seq=[0, 1, 2], index=[t] * B, active=[t < len(SIZES[b]) for b in range(B)])
    tables = host.tables()
    assert tables["cursor"][:, :2].tolist() == [[4, 10], [2, 7], [0, 0]]
    assert sorted(tables["rec_size"][0, :10].tolist() + tables["rec_size"][1, :7].tolist()) == sorted([0, 1, 2, 3, 63, 64, 65, 128, 129, 5, 2, 64, 4, 3, 65, 1, 28])
    want = F.log_boxes(tables, poison=True)
    for b, r, area, runner in want[4]:
        assert F.margin_ok(area, runner), (b, r, area, runner)
    return upload(host), tables, want


def test_log_boxes_equal_the_statement(logged):
    log, tables, want = logged
    into = poisoned(log.B, log.R)
    got = log.boxes(into=into)
    assert got is into
    assert_same_boxes(got, want, "log")
    # stated on its own: the words at or beyond each cursor still hold the poison, the flags word of every stream was written
    for b in range(log.B):
        r = int(tables["cursor"][b, 1])
        assert (got.box[b, r:].view(torch.int32) == F.POISON).all() and (got.cand[b, r:] == F.POISON).all() and (got.valid[b, r:] == F.POISON).all()
    box, cand, valid, flags, _ = want
    # the exact ties went to candidate 0, the searches did not (stream 1's records: 2, 64, rect | 3, 65, 1, grid)
    assert valid[1, 2] == 4 and valid[1, 6] == 28 and cand[1, 2] == 0 and cand[1, 6] == 0
    assert box[1, 2].tolist() == [14.0, -7.0, 2.5, 4.0, 2.0, 1.0, 0.0, 8.0] and box[1, 6, 3:].tolist() == [6.0, 3.0, 1.0, 0.0, 18.0]
    assert (cand[0, [4, 5, 6, 7]] > 0).all() and valid[0, :10].tolist() == [0, 1, 2, 3, 63, 64, 65, 128, 129, 5] and cand[0, 0] == -1
    # a second run gives the same bits, yaw included
    again = log.boxes()
    for b in range(log.B):
        r = int(tables["cursor"][b, 1])
        assert torch.equal(again.box[b, :r].view(torch.int64), got.box[b, :r].view(torch.int64)) and int(again.box[b, r:].abs().sum()) == 0


def test_the_cap_is_reported(logged):
    log, tables, (box, cand, valid, flags, _) = logged
    got = log.boxes()
    assert flags.tolist() == [F.FLAG_AXIS, 0, 0] and got.flags.tolist() == [BX.FLAG_AXIS, 0, 0]
    mask = got.axis_only.cpu().numpy()
    assert mask.sum() == 1 and mask[0, 8] and valid[0, 8] == 129 and cand[0, 8] == 0
    pts = tables["points"][0, int(tables["rec_size"][0, :8].sum()):][:129].astype(np.float64)
    assert box[0, 8, 7] == np.ptp(pts[:, 0]) * np.ptp(pts[:, 1]) and box[0, 8, YAW] in (0.0, -F.PI / 2.0)      # axis-aligned
    with pytest.raises(RuntimeError, match="stream 0 .*128"):
        got.check()
    BX.ObjectBoxes(got.box[1:], got.cand[1:], got.valid[1:], got.flags[1:]).check()


def test_keep_fits_only_the_marked_records(logged):
    log, tables, want = logged
    rng = np.random.default_rng(22)
    keep = rng.integers(0, 2, size=(log.B, log.R)).astype(np.uint8)
    keep[0, 8], keep[0, 7], keep[1, 2] = 0, 1, 1          # the record above the cap is not fitted: no flag
    masked = F.log_boxes(tables, keep=keep, poison=True)
    assert masked[3].tolist() == [0, 0, 0] and (masked[2][0, :10][keep[0, :10] == 0] == 0).all()
    got = log.boxes(keep=_dev(keep), into=poisoned(log.B, log.R))
    assert_same_boxes(got, masked, "keep")
    full = log.boxes()
    for b in range(log.B):
        for r in range(int(tables["cursor"][b, 1])):
            if keep[b, r]:
                assert torch.equal(got.box[b, r].view(torch.int64), full.box[b, r].view(torch.int64)) and got.cand[b, r] == full.cand[b, r]
            else:
                assert got.box[b, r].tolist() == [0.0] * 8 and (int(got.cand[b, r]), int(got.valid[b, r])) == (-1, 0)
    with pytest.raises(ValueError, match="keep"):
        log.boxes(keep=_dev(keep[:, :5]))
    with pytest.raises(ValueError, match="min_extent"):
        log.boxes(min_extent=-1.0)


def test_min_extent_pads_the_lengths_and_nothing_else(logged):
    log, tables, _ = logged
    want = F.log_boxes(tables, min_extent=1.5, poison=True)
    assert_same_boxes(log.boxes(min_extent=1.5, into=poisoned(log.B, log.R)), want, "min_extent")
    r = int(tables["cursor"][0, 1])
    assert (want[0][0, 1:r, 3:6] >= 1.5).all() and (want[0][0, 1:r, 3:6] == 1.5).any() and want[0][0, 0].tolist() == [0.0] * 8


# ---- a live step ---------------------------------------------------------------------------------------------------------------------
def live_step(rng, B=3, N=64, K=8, num=(5, 8, 3)):
    """obj in [-1, num]: columns of no object, and columns whose object is num_objects itself (none either); redrawn for the margin."""
    while True:
        pc1 = np.zeros((B, 3, N), np.float32)
        obj = np.stack([rng.integers(-1, num[b] + 1, size=N) for b in range(B)]).astype(np.int32)
        for b in range(B):
            for j in range(-1, num[b] + 1):
                cols = np.nonzero(obj[b] == j)[0]
                pc1[b][:, cols] = cloud(rng, len(cols)).T if len(cols) else 0
        want = F.step_boxes(pc1, obj, np.array(num, np.int32), K, active=[1, 1, 0])
        if all(F.margin_ok(area, runner) for _, _, area, runner in want[4]):
            return pc1, obj, np.array(num, np.int32), want


def test_object_boxes_equal_the_statement_and_the_logged_step():
    rng = np.random.default_rng(23)
    B, N, K = 3, 64, 8
    pc1, obj, num, want = live_step(rng)
    active = np.array([1, 1, 0], np.uint8)
    assert (want[2][:2] > 0).sum() >= 12 and (want[2][2] == 0).all() and (want[1][:2] > 0).sum() >= 8
    got = BX.object_boxes_raw(_dev(pc1), _dev(obj), _dev(num), K, active=_dev(active), into=poisoned(B, K))
    assert_same_boxes(got, want, "step")
    # a StepResult goes the same way, and a strided view of the cloud is read in place
    view = _dev(np.ascontiguousarray(pc1.transpose(0, 2, 1))).permute(0, 2, 1)
    assert not view.is_contiguous()
    out = T.StepResult(pc1=view, obj=_dev(obj), num_objects=_dev(num), max_objects=K, active=_dev(active))
    same = BX.object_boxes(out)
    assert torch.equal(same.box.view(torch.int64), got.box.view(torch.int64)) and torch.equal(same.cand, got.cand) and torch.equal(same.valid, got.valid)
    # the same step appended to a log: record for record the same bits, yaw included
    log = RL.ResultLog(B, K, 2, 2 * K, 2 * N, device=DEV)
    log.append_raw(_dev(pc1), _dev(obj), _dev(num), _dev(np.zeros((B, K), np.int32)), _dev(np.zeros((B, K), np.float32)), seq=[0, 1, 2], index=0,
                   active=_dev(active))
    log.check()
    assert log.cursor[:, 1].tolist() == [5, 8, 0]
    rec = log.boxes()
    for b in range(2):
        n = int(num[b])
        assert torch.equal(rec.box[b, :n].view(torch.int64), got.box[b, :n].view(torch.int64)), b
        assert torch.equal(rec.cand[b, :n], got.cand[b, :n]) and torch.equal(rec.valid[b, :n], got.valid[b, :n]), b
    # a num_objects outside [0, K] is refused as the log's append refuses it
    bad = np.array([K + 1, -1, 3], np.int32)
    want_bad = F.step_boxes(pc1, obj, bad, K)
    assert want_bad[3].tolist() == [F.FLAG_OBJECTS, F.FLAG_OBJECTS, 0] and (want_bad[2][:2] == 0).all() and (want_bad[2][2, :3] > 0).all()
    refused = BX.object_boxes_raw(_dev(pc1), _dev(obj), _dev(bad), K, into=poisoned(B, K))
    assert_same_boxes(refused, want_bad, "refused")
    with pytest.raises(RuntimeError, match="stream 0 .*num_objects"):
        refused.check()


def test_a_step_object_above_the_cap_and_one_that_is_not_finite():
    """N = 300: object 0 owns 129 columns (axis-aligned, flagged), object 1 owns 128 (searched), object 2 has a NaN."""
    rng = np.random.default_rng(24)
    B, N, K = 1, 300, 4
    pc1, obj, num = frame_of(rng, [[cloud(rng, 129), cloud(rng, 128), cloud(rng, 7), cloud(rng, 30)]], N, K)
    pc1[0, 1, np.nonzero(obj[0] == 2)[0][3]] = np.nan
    want = F.step_boxes(pc1, obj, num, K)
    assert want[2][0].tolist() == [129, 128, -1, 30] and want[1][0, 0] == 0 and want[1][0, 1] > 0 and want[1][0, 2] == -1 and want[3].tolist() == [F.FLAG_AXIS]
    got = BX.object_boxes_raw(_dev(pc1), _dev(obj), _dev(num), K, into=poisoned(B, K))
    assert_same_boxes(got, want, "cap")
    assert got.axis_only.tolist() == [[True, False, False, False]]
    with pytest.raises(RuntimeError, match="stream 0 .*128"):
        got.check()


# ---- stream capture ---------------------------------------------------------------------------------------------------------------
def test_a_captured_object_boxes_replays_on_new_inputs():
    rng = np.random.default_rng(25)
    B, N, K = 3, 64, 8
    steps = [live_step(rng, num=num) for num in ((5, 8, 3), (8, 0, 6))]
    static = dict(pc1=torch.zeros(B, 3, N, device=DEV), obj=torch.zeros(B, N, dtype=torch.int32, device=DEV),
                  num=torch.zeros(B, dtype=torch.int32, device=DEV), active=torch.ones(B, dtype=torch.uint8, device=DEV))
    into = poisoned(B, K)
    torch.cuda.synchronize()
    graph, out = capture_graph(lambda: BX.object_boxes_raw(static["pc1"], static["obj"], static["num"], K, active=static["active"], min_extent=0.25, into=into))
    assert out is into and int(into.cand[0, 0]) == F.POISON                       # the capture recorded the launch and executed nothing
    for (pc1, obj, num, _), active in zip(steps, ([1, 1, 0], [1, 1, 1])):
        eager = BX.object_boxes_raw(_dev(pc1), _dev(obj), _dev(num), K, active=_dev(np.array(active, np.uint8)), min_extent=0.25)
        static["pc1"].copy_(_dev(pc1)); static["obj"].copy_(_dev(obj)); static["num"].copy_(_dev(num)); static["active"].copy_(_dev(np.array(active, np.uint8)))
        graph.replay()
        torch.cuda.synchronize()
        for name in ("box", "cand", "valid", "flags"):
            g, e = getattr(into, name), getattr(eager, name)
            assert torch.equal(g.view(torch.int32), e.view(torch.int32)), name
        assert_same_boxes(into, F.step_boxes(pc1, obj, num, K, active=active, min_extent=0.25), "replay")


# ---- the tracker -----------------------------------------------------------------------------------------------------------------------
def test_the_tracker_fits_its_objects_eager_and_captured():
    """The small net of the tracker tests on three streams: boxes=True adds the boxes and changes nothing else, eager and replayed."""
    sizes, steps = [200, 160, 97], 4
    net, seq, B = TG.new_net(), TG.frames(sizes, steps, 40), len(sizes)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    plain = T.BatchedTracker(net, streams=B)
    eager = T.BatchedTracker(TG.new_net(sd), streams=B, boxes=True, box_min_extent=0.5)
    graph = T.BatchedTracker(TG.new_net(sd), streams=B, boxes=True, box_min_extent=0.5, graph=True, graph_warmup=1)
    objects = 0
    with torch.no_grad():
        for t, (pc1, pc2, f1, f2, nv) in enumerate(seq):
            reset, active = torch.tensor([False, t == 2, False]), torch.tensor([True, True, t != 1])
            outs = [trk.step(pc1, pc2, f1, f2, n_valid=nv, reset=reset, active=active) for trk in (plain, eager, graph)]
            assert outs[0].object_boxes is None and outs[0].object_box_valid is None and outs[0].object_box_cand is None
            want = TG.snapshot(outs[0], plain)
            for out, trk in zip(outs[1:], (eager, graph)):
                TG.assert_same(TG.snapshot(out, trk), want, t)
                ref = BX.object_boxes(out, min_extent=0.5)
                assert torch.equal(out.object_boxes.view(torch.int64), ref.box.view(torch.int64)), t
                assert torch.equal(out.object_box_valid, ref.valid) and torch.equal(out.object_box_cand, ref.cand), t
                assert torch.equal(out.object_box_flags, ref.flags), t
                n = out.num_objects.tolist()
                for b in range(B):
                    sizes_b = torch.bincount(out.obj[b][out.obj[b] >= 0], minlength=trk.K)[:n[b]]
                    assert out.object_box_valid[b, :n[b]].tolist() == sizes_b.tolist() and (out.object_box_valid[b, n[b]:] == 0).all()
                    assert (out.object_boxes[b, :n[b], 3:6] >= 0.5).all()
            assert graph.captured == (t >= 1)
            objects += sum(outs[0].num_objects.tolist())
    assert objects > 0


# ---- KITTI files -----------------------------------------------------------------------------------------------------------------------
def test_write_kitti_gives_the_statements_files(tmp_path):
    """A logged sequence of integer grids (exact ties: candidate 0 wins, yaw is exactly 0 or -pi/2, so the text of every field is
    fixed), single points and an empty object; the filters take what `select` takes."""
    rng = np.random.default_rng(26)
    B, N, K, frames = 2, 80, 4, 5
    host = U.HostLog(B, K, frames, frames * K, frames * N)
    for t in range(frames):
        records = [[grid(int(rng.integers(1, 5)), int(rng.integers(1, 5)), at=(int(rng.integers(-20, 20)), int(rng.integers(-20, 20))), z=t)
                    for _ in range(3)] + [np.zeros((0, 3), np.float32) if t % 2 else np.array([[t, 2, 1]], np.float32)] for _ in range(B)]
        pc1, obj, num = frame_of(rng, records, N, K)
        ids = np.stack([rng.permutation(6)[:K] for _ in range(B)]).astype(np.int32)
        host.append(pc1, obj, num, ids, (rng.integers(1, 64, size=(B, K)) / 64.0).astype(np.float32), seq=[1, 0], index=[7 + t] * B,
                    object_hits=np.ones((B, K), np.int32), reset=[t == 0, t in (0, 3)])
    tables = host.tables()
    box, cand, valid, flags, _ = F.log_boxes(tables)
    assert (cand[valid > 0] == 0).all() and set(box[..., YAW][valid > 0].tolist()) <= {0.0, -F.PI / 2.0} and (valid == 0).sum() == 4
    log = upload(host)
    names = ["second", "first"]
    paths = log.write_kitti(str(tmp_path / "all"), names)
    texts = F.kitti_text(tables, box, valid)
    assert U.read_tree(str(tmp_path / "all")) == {names[s] + ".txt": t.encode() for s, t in texts.items()} and len(paths) == 2
    assert sum(t.count("\n") for t in texts.values()) == int((valid > 0).sum()) == 2 * (5 * 3 + 3)
    first = texts[1].split("\n")[0].split()
    assert first[0] == "7" and first[2] == "Car" and len(first) == 18
    # filters: exactly the records `select` removes are gone
    score = U.select(tables)[1]
    tau = float(np.median(score[:, :int(tables["cursor"][0, 1])]))
    keep = U.select(tables, threshold=tau, min_track_frames=2)[0]
    assert 0 < keep.sum() < tables["cursor"][:, 1].sum()
    log.write_kitti(str(tmp_path / "filtered"), names, obj_type="Pedestrian", threshold=tau, min_track_frames=2, min_extent=0.75)
    box75 = F.log_boxes(tables, keep=keep, min_extent=0.75)
    texts = F.kitti_text(tables, box75[0], box75[2], keep, obj_type="Pedestrian")
    assert U.read_tree(str(tmp_path / "filtered")) == {names[s] + ".txt": t.encode() for s, t in texts.items()}
    assert sum(t.count("\n") for t in texts.values()) == int(((valid > 0) & (keep > 0)).sum())
    # a transforms mapping that misses a logged frame: nothing is written
    with pytest.raises(ValueError, match="transforms"):
        log.write_kitti(str(tmp_path / "never"), names, transforms={(0, 7): None})
    assert not os.path.exists(str(tmp_path / "never"))
