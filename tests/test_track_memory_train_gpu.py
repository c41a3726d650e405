"""GPU: training the re-acquisition -- rtk_track_score_memory (csrc/track_score.hip), TrackScorer(track_memory=True) behind
BatchedTracker(max_age=...) and SequenceTrainer(reacquire=...).

Every comparison is exact (== on integers, bit views on floats) except the gradient test, whose bound is the project's own
(tests/_track_train_util.py `bound`).  The scenes are those of tests/test_track_memory_gpu.py: blobs where the frame builder put them,
one `Car` box around every object, identity transforms and `distance_affinity(4, 4)`, so which object follows which is decided by
construction.  Only the trainer test runs a backbone.

The plain-kernel comparison runs `synthetic_sequence(B=4, N=96, K=8, frames=8)`: N = 96 is the smallest multiple of 32 the builder of
tests/_track_score_util.py can fill (a stream holds up to 69 clutter points besides its objects; at N = 64 it raises)."""
import os
import sys

import numpy as np
import pytest
import torch

import _gt_util as GU
import _track_memory_train_util as M
import _track_memory_util as U
import _track_score_util as S
import _track_train_util as TU
from _util import reference_state_dict
from ratrack_amd import gt_device as G, synth, track_score as TS, track_train as TT, tracker as T, vod_gt
from ratrack_amd.track4d import Affinity, Args, Track4D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = "cuda"
B3, N, K, KB = 3, 64, 16, 8
FRAMES = 8
RESET, INACTIVE = (1, 3), (2, (2, 4))          # (stream, frame): the pattern of tests/test_track_memory_gpu.py
CLUTTER = (0, 1)                               # (stream, frame) of the one-frame blob outside every box
MATCH = ("pred_gt_slot", "pred_gt_id", "gt_pred", "iou", "aff_target", "aff_defined")
STATE = ("counters", "iou_sum", "table_key", "table_last", "table_seen", "table_matched", "table_used", "prev_gt_id", "prev_count",
         "prev_gt", "flags")
MEMORY_STATE = ("row_track", "labelled_coasted")
LOG = ("log_cursor", "log_frame", "log_label", "log_track", "log_best", "log_conf", "log_iou")


def bits(t):
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32)
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def differing(a, b, keys):
    return [k for k in keys if not same(getattr(a, k), getattr(b, k))]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def affinity_net():
    net = Track4D(Args()).to(DEV).eval()
    net.affinity.load_state_dict(U.distance_affinity(4.0, 4.0).state_dict())
    net.invalidate_fused()
    return net


def masks(t, B=B3):
    reset = torch.tensor([b == RESET[0] and t == RESET[1] for b in range(B)], dtype=torch.uint8, device=DEV)
    active = torch.tensor([not (b == INACTIVE[0] and t in INACTIVE[1]) for b in range(B)], dtype=torch.uint8, device=DEV)
    return reset, active


def step_scene(trk, scorers, row, reset=None, active=None, boxes=KB):
    """One frame: row = [(blob_stream dict, per-stream item)] per stream -> (StepResult, GtObjects, [MatchResult per scorer])."""
    pc1, f1, flow, cls, prop, nv = U.batch([s for s, _ in row], DEV)
    B = len(row)
    reset = torch.zeros(B, dtype=torch.uint8, device=DEV) if reset is None else reset
    active = torch.ones(B, dtype=torch.uint8, device=DEV) if active is None else active
    out = trk.associate(pc1, f1, flow, cls, prop, nv, reset, active)
    per_stream = [item for _, item in row]
    bb = G.pack_boxes(per_stream, boxes, DEV)
    gobj = TS.gt_objects(out.pc1, bb, TS.pack_box_types(per_stream, boxes, DEV), n_valid=nv, min_obj_points=2)
    return out, gobj, [sc.update(out, gobj, reset=reset, active=active) for sc in scorers]


def pad(v, n, fill=-1):
    return list(v) + [fill] * (n - len(v))


# ---- 4. no coasted rows means the plain kernel ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("logging", [False, True])
def test_without_coasted_rows_it_is_the_plain_kernel(logging):
    seq = S.synthetic_sequence(B=4, N=96, K=8, frames=8)
    assert any(fr["reset"][1:].any() for fr in seq["frames"][1:]) and any(not fr["active"].all() for fr in seq["frames"])
    kw = dict(streams=4, max_objects=8, max_boxes=8, max_gt_tracks=16)
    if logging:
        kw.update(sweep_frames=8, sweep_records=64)
    plain, memory = TS.TrackScorer(**kw), TS.TrackScorer(track_memory=True, **kw)
    g = torch.Generator().manual_seed(11)
    for f, fr in enumerate(seq["frames"]):
        pc1, nv = _dev(fr["pc1"]), _dev(fr["n_valid"])
        bb = G.pack_boxes(fr["per_stream"], 8, DEV)
        gobj = TS.gt_objects(pc1, bb, TS.pack_box_types(fr["per_stream"], 8, DEV), n_valid=nv, min_obj_points=S.MIN_PTS)
        conf = torch.rand(4, 8, generator=g).to(DEV) if logging else None
        args = (pc1, _dev(fr["obj"]), _dev(fr["num"]), _dev(fr["ids"]), gobj, nv, _dev(fr["reset"]), _dev(fr["active"]))
        a = plain.update_raw(*args, object_conf=conf)
        b = memory.update_raw(*args, object_conf=conf, table_ids=_dev(fr["ids"]), table_count=_dev(fr["num"]))
        assert differing(a, b, MATCH) == [], f
        assert differing(plain, memory, STATE + (LOG if logging else ())) == [], f
        assert int(memory.labelled_coasted.sum()) == 0
    plain.check()
    memory.check()
    assert int(plain.counters[:, 3].sum()) > 0
    np.testing.assert_equal(plain.result(), memory.result())
    if logging:
        np.testing.assert_equal(plain.sweep(40).__dict__, memory.sweep(40).__dict__)
        assert int(plain.log_cursor[:, 1].sum()) > 0


# ---- 5. the kernel equals the host statement ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seq():
    """The sequence of tests/test_track_memory_gpu.py (3 streams, 6 / 7 / 8 five-point objects, seeded visibility) with its boxes, and
    a one-frame clutter blob outside every box in stream 0 at frame 1."""
    frames, vis = U.random_sequence(B=B3, frames=FRAMES, N=N, objects=(6, 7, 8), points=5, seed=7, min_visible=5)
    rows = []
    for t in range(FRAMES):
        row = []
        for b, objects in enumerate((6, 7, 8)):
            c = U.lattice(objects) + torch.tensor([0.2 * t, 0.0, 0.0])
            stream = frames[t][b]
            if (b, t) == CLUTTER:
                stream = M.with_clutter(c, vis[t][b], N, points=5, seed=7000 + 10 * t + b)
            row.append((stream, M.car_labels(c)))
        rows.append(row)
    return rows


def host_frame(out, gobj_count, row, b):
    """The host path of one stream's frame: -> dict(P, G, ids, gt_id, iou, slots, gt_pred)."""
    stream, item = row[b]
    r = S.host_gt_objects(item, stream["pc1"].numpy(), stream["n_valid"], min_pts=2)
    objects, _ = out.objects(b)
    objects = {k: v.cpu() for k, v in objects.items()}
    _, gt_id, iou = S.host_match(r, objects)
    labels = list(r[7].keys())
    assert len(labels) == gobj_count
    slot_of = {k: i for i, k in enumerate(item[0].keys())}
    pred_of = {k: i for i, k in enumerate(gt_id) if k >= 0}
    return dict(P=len(objects), G=len(labels), ids=list(objects.keys()), gt_id=gt_id, iou=iou, slots=[slot_of.get(k, -1) for k in gt_id],
                gt_pred=[pred_of.get(k, -1) for k in labels])


@pytest.mark.parametrize("max_age", [0, 1, 2])
def test_kernel_equals_the_host_statement(seq, max_age):
    trk = T.BatchedTracker(affinity_net(), streams=B3, max_objects=K, max_age=max_age)
    scorer = TS.TrackScorer(streams=B3, max_objects=K, max_boxes=KB, max_gt_tracks=32, track_memory=True)
    recs, n_det = [M.empty_record() for _ in range(B3)], [0] * B3
    coasted_ones = unlabelled_coasted = defined_frames = 0
    for t, row in enumerate(seq):
        reset_d, active_d = masks(t)
        reset, active = reset_d.tolist(), active_d.tolist()
        out, gobj, (m,) = step_scene(trk, [scorer], row, reset_d, active_d)
        trk.check()
        gobj.check()
        got = {k: getattr(m, k).cpu() for k in MATCH}
        st = {k: getattr(scorer, k).cpu() for k in STATE + MEMORY_STATE}
        slot = U.written_slot(trk)
        table_ids, table_count = trk.ids[slot].tolist(), trk.count[slot].tolist()
        assert out.table_ids.tolist() == table_ids and out.table_count.tolist() == table_count
        counts = gobj.count.tolist()
        for b in range(B3):
            where = (max_age, t, b)
            if active[b]:
                h = host_frame(out, counts[b], row, b)
                assert h["ids"] == out.object_ids[b, :h["P"]].tolist(), where
                new, target, defined, flag = M.host_score_memory(recs[b], h["ids"], h["gt_id"], h["G"], table_ids[b], table_count[b], K,
                                                                 bool(reset[b]), True)
                assert flag == 0, where
                assert got["pred_gt_id"][b].tolist() == pad(h["gt_id"], K), where
                assert got["pred_gt_slot"][b].tolist() == pad(h["slots"], K), where
                assert got["gt_pred"][b].tolist() == pad(h["gt_pred"], KB), where
                assert got["iou"][b].view(torch.int64).tolist() == torch.tensor(pad(h["iou"], K, 0.0), dtype=torch.float64).view(torch.int64).tolist(), where
                old_det = 0 if reset[b] else n_det[b]
                coasted_ones += sum(1 for i, _ in M.ones(target) if i >= old_det)
                unlabelled_coasted += sum(1 for v in new["label"][h["P"]:] if v < 0)
                n_det[b] = h["P"]
            else:
                new, target, defined, flag = M.host_score_memory(recs[b], [], [], 0, table_ids[b], table_count[b], K, False, False)
                assert got["pred_gt_id"][b].tolist() == [-1] * K and got["pred_gt_slot"][b].tolist() == [-1] * K, where
                assert got["gt_pred"][b].tolist() == [-1] * KB and got["iou"][b].tolist() == [0.0] * K, where
            assert got["aff_target"][b].tolist() == target, where
            assert int(got["aff_defined"][b]) == defined, where
            defined_frames += defined
            recs[b] = new
            assert int(st["prev_count"][b]) == new["count"] and int(st["prev_gt"][b]) == new["gt"], where
            assert st["prev_gt_id"][b].tolist() == pad(new["label"], K) and st["row_track"][b].tolist() == pad(new["track"], K), where
            assert int(st["labelled_coasted"][b]) == new["labelled"], where
            assert st["row_track"][b, :new["count"]].tolist() == table_ids[b][:table_count[b]] and new["count"] == table_count[b], where
    scorer.check()
    print("   max_age %d: %d defined stream-frames, %d target ones on coasted rows, %d coasted rows without a label"
          % (max_age, defined_frames, coasted_ones, unlabelled_coasted))
    assert defined_frames > 0
    if max_age == 0:
        assert coasted_ones == 0 and unlabelled_coasted == 0
    else:
        assert coasted_ones > 0 and unlabelled_coasted > 0, (coasted_ones, unlabelled_coasted)


# ---- 6. known by construction ---------------------------------------------------------------------------------------------------------
def run_scene(frames, max_age=2, track_memory=True, max_objects=8):
    """One stream through the tracker and one scorer.  -> per frame dict(P, prev_det, ids, gt_id, target (K,K) int, defined, prev_gt,
    labelled_coasted (the state the frame left))."""
    trk = T.BatchedTracker(affinity_net(), streams=1, max_objects=max_objects, max_age=max_age)
    scorer = TS.TrackScorer(streams=1, max_objects=max_objects, max_boxes=KB, max_gt_tracks=16, track_memory=track_memory)
    res, prev_det = [], 0
    for t, row in enumerate(frames):
        first = torch.tensor([t == 0], dtype=torch.uint8, device=DEV)
        out, gobj, (m,) = step_scene(trk, [scorer], [row], reset=first)
        trk.check()
        P = int(out.num_objects[0])
        res.append(dict(P=P, prev_det=prev_det, ids=out.object_ids[0, :P].tolist(), gt_id=m.pred_gt_id[0, :P].tolist(),
                        target=m.aff_target[0].to(torch.int32), defined=int(m.aff_defined[0]), prev_gt=int(scorer.prev_gt[0]),
                        labelled_coasted=int(scorer.labelled_coasted[0]) if track_memory else None, num_prev=int(out.num_prev[0])))
        prev_det = P
    scorer.check()
    return res


@pytest.mark.parametrize("g", [1, 2, 3])
def test_the_returning_object_has_its_one_on_the_coasted_row(g):
    back = 2 + g
    r = run_scene(M.scenario(g))[back]
    assert r["P"] == 3 and sorted(r["gt_id"]) == [0, 1, 2] and r["defined"] == 1
    col = r["gt_id"].index(0)                                    # A's detection
    ones = M.ones(r["target"].tolist())
    if g <= 2:
        assert len(ones) == 3 and r["num_prev"] == 3 and r["prev_det"] == 2
        (row,) = [i for i, j in ones if j == col]
        assert row >= r["prev_det"] and row < r["num_prev"]      # a coasted row of the previous table
        assert sorted(i for i, j in ones if j != col) == [0, 1]
    else:                                                        # A's row has died (max_age = 2): nothing to re-acquire
        assert len(ones) == 2 and r["num_prev"] == 2
        assert int(r["target"][:, col].sum()) == 0


def test_an_object_hidden_for_one_frame_keeps_the_frame_defined():
    with_memory = run_scene(M.single_object())
    plain = run_scene(M.single_object(), track_memory=False)
    assert [r["P"] for r in with_memory] == [1, 0, 1, 1] == [r["P"] for r in plain]
    assert with_memory[2]["defined"] == 1 and plain[2]["defined"] == 0
    assert M.ones(with_memory[2]["target"].tolist()) == [(0, 0)] and with_memory[2]["prev_det"] == 0      # row 0 of that table is coasted
    assert M.ones(plain[2]["target"].tolist()) == []
    assert with_memory[1]["prev_gt"] == 1 and with_memory[1]["labelled_coasted"] == 1
    assert with_memory[3]["defined"] == 1 and plain[3]["defined"] == 1
    # the hidden frame without any label: prev_gt = 0, and the labelled coasted row alone keeps the next frame defined
    bare = run_scene(M.single_object(unlabelled=(1,)))
    assert bare[1]["prev_gt"] == 0 and bare[1]["labelled_coasted"] == 1
    assert bare[2]["defined"] == 1 and M.ones(bare[2]["target"].tolist()) == [(0, 0)]


def test_a_duplicate_label_gives_both_rows_the_one():
    res = run_scene(M.duplicate_label())
    a = res[0]["ids"][res[0]["gt_id"].index(0)]
    fresh = res[3]["ids"][res[3]["gt_id"].index(0)]
    assert res[3]["P"] == 3 and fresh != a and fresh not in res[0]["ids"]      # displaced by 3 m: a fresh ID, while track a still coasts
    assert res[3]["labelled_coasted"] == 1
    r = res[4]
    assert r["ids"][r["gt_id"].index(0)] == fresh and r["num_prev"] == 4 and r["prev_det"] == 3
    col = r["gt_id"].index(0)
    rows = sorted(i for i, j in M.ones(r["target"].tolist()) if j == col)
    assert len(rows) == 2 and rows[0] < r["prev_det"] <= rows[1], rows          # one detection row, one coasted row
    assert len(M.ones(r["target"].tolist())) == 4 and r["defined"] == 1


# ---- 7. truncation and bad tables -----------------------------------------------------------------------------------------------------
def _labels_at(lat, t):
    """Boxes around the objects shown in frame t of the truncation scene, label id = lattice index."""
    shown = (range(0, 6), range(6, 12), range(0, 3))[t]
    c = lat.tolist()
    labels = {k: vod_gt.Label("Car", k, 0, 0, 0, 0, 0, 0, 3.0, 4.0, 6.0, c[k][0], c[k][1], c[k][2], 0.0) for k in shown}
    return (labels, GU.IDENTITY_TF, labels, GU.IDENTITY_TF)


def test_the_record_follows_a_truncated_table():
    lat = U.lattice(12)
    trk = T.BatchedTracker(affinity_net(), streams=1, max_objects=8, max_age=1)
    scorer = TS.TrackScorer(streams=1, max_objects=8, max_boxes=16, max_gt_tracks=16, track_memory=True)
    shown = [lat[:6], lat[6:], lat[:3]]
    outs, ms = [], []
    for t, c in enumerate(shown):
        out, gobj, (m,) = step_scene(trk, [scorer], [(U.blob_stream(c, [True] * len(c), 32, points=3, seed=300 + t), _labels_at(lat, t))], boxes=16)
        outs.append(out)
        ms.append(m)
        if t == 1:
            state1 = {k: getattr(scorer, k).clone() for k in ("prev_gt_id", "row_track", "prev_count", "labelled_coasted")}
            table1 = (trk.ids[U.written_slot(trk)].clone(), trk.count[U.written_slot(trk)].clone())
    ids0 = outs[0].object_ids[0, :6].tolist()
    # frame 1: six fresh objects and room for two of the six lost tracks; the record is the table, nothing more
    assert outs[1].flags.tolist() == [4] and table1[1].tolist() == [8]
    assert state1["prev_count"].tolist() == [8] and state1["row_track"][0].tolist() == table1[0][0].tolist()
    assert state1["row_track"][0, 6:].tolist() == ids0[:2] and state1["prev_gt_id"][0].tolist() == [6, 7, 8, 9, 10, 11, 0, 1]
    assert state1["labelled_coasted"].tolist() == [2]
    with pytest.raises(RuntimeError, match="dropped coasted tracks"):
        outs[1].check()
    # frame 2: objects 0 and 1 come back to their coasted rows; object 2's row was dropped: its column is zero, no row was invented
    m, gt_id = ms[2], ms[2].pred_gt_id[0, :3].tolist()
    assert gt_id == [0, 1, 2] and int(m.aff_defined[0]) == 1
    assert M.ones(m.aff_target[0].to(torch.int32).tolist()) == [(6, 0), (7, 1)]
    assert outs[2].object_ids[0, :2].tolist() == ids0[:2] and outs[2].object_ids[0, 2].item() not in ids0
    scorer.check()                                               # truncation is the tracker's flag, not the scorer's


def _table_run(bad):
    seq = S.synthetic_sequence(B=4, N=96, K=8, frames=8)
    scorer = TS.TrackScorer(streams=4, max_objects=8, max_boxes=8, max_gt_tracks=16, track_memory=True)
    kept = []
    for f, fr in enumerate(seq["frames"][:3]):
        pc1, nv = _dev(fr["pc1"]), _dev(fr["n_valid"])
        bb = G.pack_boxes(fr["per_stream"], 8, DEV)
        gobj = TS.gt_objects(pc1, bb, TS.pack_box_types(fr["per_stream"], 8, DEV), n_valid=nv, min_obj_points=S.MIN_PTS)
        count = fr["num"].copy()
        if bad and f == 1:
            assert fr["active"].tolist() == [1, 1, 1, 0] and fr["num"][1] >= 1 and fr["num"][2] < 8
            count[1], count[2], count[3] = fr["num"][1] - 1, 8 + 5, -7          # below P | above Kobj | an inactive stream: not looked at
        m = scorer.update_raw(pc1, _dev(fr["obj"]), _dev(fr["num"]), _dev(fr["ids"]), gobj, nv, _dev(fr["reset"]), _dev(fr["active"]),
                              table_ids=_dev(fr["ids"]), table_count=_dev(count))
        kept.append((m, {k: getattr(scorer, k).clone() for k in STATE + MEMORY_STATE}))
    return scorer, kept, seq


def test_a_table_count_out_of_range_is_clamped_flagged_and_named():
    clean, ref, seq = _table_run(False)
    clean.check()
    bad, got, _ = _table_run(True)
    assert bad.flags.tolist() == [0, TS.FLAG_TABLE, TS.FLAG_TABLE, 0]
    with pytest.raises(RuntimeError, match="stream 1 has a table_count outside"):
        bad.check()
    with pytest.raises(RuntimeError, match="stream 1 has a table_count outside"):
        bad.result()
    for f in range(3):
        assert differing(got[f][0], ref[f][0], MATCH) == [], f                 # clamped rows carry no label: no output changes
    num = seq["frames"][1]["num"].tolist()
    s, r = got[1][1], ref[1][1]
    assert s["prev_count"].tolist() == [num[0], num[1], 8, r["prev_count"][3].item()]      # clamped to [P, Kobj]
    assert s["row_track"][2].tolist() == seq["frames"][1]["ids"][2].tolist() and s["row_track"][2, num[2]:].tolist() == [-1] * (8 - num[2])
    assert s["prev_gt_id"][2, num[2]:].tolist() == [-1] * (8 - num[2]) and s["labelled_coasted"].tolist() == [0, 0, 0, 0]
    for k in STATE + MEMORY_STATE:
        if k not in ("flags", "prev_count"):
            assert same(s[k], r[k]), k
        assert same(got[1][1][k][[0, 3]], ref[1][1][k][[0, 3]]), k              # the other streams are untouched
    np.testing.assert_equal(bad.result(check=False)["per_stream"], clean.result()["per_stream"])


# ---- 8. gradients ---------------------------------------------------------------------------------------------------------------------
def test_the_term_over_coasted_rows_matches_the_float64_arbiter():
    """Stream 0 is scenario(1) at the frame A returns (its one sits on a coasted row), stream 1 the same scene with nothing hidden (no
    coasted row).  The last frame is associated with a randomly initialised Affinity -- the target does not depend on that frame's
    association -- so that the MLP under test has gradients everywhere.  (prop channel 0 is one value for every point: the max's
    gradient goes to the lowest index, in the kernel and in torch on the CPU.)"""
    hidden, shown = M.scenario(1), M.scenario(0, frames=5)
    trk = T.BatchedTracker(affinity_net(), streams=2, max_objects=8, max_age=2)
    scorer = TS.TrackScorer(streams=2, max_objects=8, max_boxes=KB, max_gt_tracks=16, track_memory=True)
    torch.manual_seed(5)
    affinity = Affinity(U.DESC).to(DEV)
    for t in range(4):
        if t == 3:
            trk.weights = T.pack_affinity(affinity)
        out, gobj, (match,) = step_scene(trk, [scorer], [hidden[t], shown[t]])
    trk.check()
    scorer.check()
    assert match.aff_defined.tolist() == [1, 1] and out.num_prev.tolist() == [3, 3] and out.num_objects.tolist() == [3, 3]
    coasted = [i for i, j in M.ones(match.aff_target[0].to(torch.int32).tolist()) if i >= 2]
    assert len(coasted) == 1 and int(out.prev_age[0, coasted[0]]) == 1 and out.prev_age[1, :3].tolist() == [0, 0, 0]
    params = [p for _, p in affinity.named_parameters()]

    def ours():
        flow, prop = out.flow.clone().requires_grad_(True), out.prop.clone().requires_grad_(True)
        for p in params:
            p.grad = None
        term = TT.affinity_term(affinity, out, match, flow, prop).sum() / 2
        term.backward()
        return [term.detach().clone(), flow.grad.clone(), prop.grad.clone()] + [p.grad.clone() for p in params]

    def torch_term(dtype, dev):
        c = lambda x: x.detach().to(device=dev, dtype=dtype)
        mlp = TU.mlp_copy(affinity, dtype).to(dev)
        flow, prop = c(out.flow).requires_grad_(True), c(out.prop).requires_grad_(True)
        term, _ = TU.frame_term(mlp, c(out.pc1), flow, c(out.feature1), prop, out.obj.to(dev), out.num_objects.tolist(), c(out.desc_prev),
                                out.num_prev.tolist(), c(match.aff_target), match.aff_defined.tolist())
        term.backward()
        return [term.detach(), flow.grad, prop.grad] + [p.grad for p in mlp.parameters()]

    first, second = ours(), ours()
    assert all(same(a, b) for a, b in zip(first, second))               # the same bits on every run
    r32, r64 = torch_term(torch.float32, "cpu"), torch_term(torch.float64, "cpu")      # on the CPU both: torch.max's tie rule there
    names = ["term", "d_flow", "d_prop"] + [n for n, _ in affinity.named_parameters()]
    assert float(r64[0]) > 0
    for name, a, g32, g64 in zip(names, first, r32, r64):
        TU.check_grad(name, a, g32, g64)


# ---- 9. the trainer -------------------------------------------------------------------------------------------------------------------
TB, STEPS = 4, 7
T_RESET, T_INACTIVE = (1, 5), (2, 6)          # (stream, step): both on replayed steps
ITEMS = ("Loss", "SceneFlowLoss", "SegLoss", "TrackingLoss")


def ref_net():
    sd = reference_state_dict(DEV)
    sd["fd_layer.cp.linear.bias"] = sd["fd_layer.cp.linear.bias"] + 0.09      # moving points in every frame (tests/test_tracker_gpu.py)
    net = Track4D(Args()).to(DEV)
    net.load_state_dict(sd, strict=True)
    return net.train()


def train_batches():
    """The recipe of tests/test_track_train_graph_gpu.py (synthetic pairs, six labelled boxes per stream), twice: the whole clouds, and
    the clouds cut to 60 % of their points through n_valid -- other detections, so that tracks are lost and found between steps."""
    t = {k: torch.from_numpy(v) for k, v in synth.make_frame_pairs(TB, 256, case_id=50).items()}
    pairs = [(t["pc1"][i:i + 1], t["pc2"][i:i + 1], t["feature1"][i:i + 1], t["feature2"][i:i + 1]) for i in range(TB)]
    per_stream = []
    for b in range(TB):
        p = t["pc1"][b].numpy()
        mk = lambda k: vod_gt.Label("rider" if k == 2 else "Car", k, 0, 0, 0, 0, 0, 0, 3.0, 4.0, 6.0, float(p[0, 10 * k]), float(p[1, 10 * k]),
                                    float(p[2, 10 * k]), 0.3 * k)
        labels = {k: mk(k) for k in range(6)}
        per_stream.append((labels, GU.IDENTITY_TF, labels, GU.IDENTITY_TF))
    pc1, pc2, f1, f2, nv = vod_gt.pad_frame_pairs(pairs, device=DEV)
    bb = G.pack_boxes(per_stream, 8, DEV)
    types = TS.pack_box_types(per_stream, 8, DEV)
    out = []
    for n_valid in (nv, (nv * 3) // 5):
        n_valid = n_valid.to(torch.int32).contiguous()
        gt = G.ground_truth(pc1, pc2, bb, n_valid=n_valid)
        gobj = TS.gt_objects(pc1, bb, types, n_valid=n_valid, min_obj_points=2)
        out.append(((pc1, pc2, f1, f2, gt.gt_warp, gt.gt_cls, gobj), n_valid))
    return out


def train_record(res, tr):
    items, h, out, match = res
    rec = {k: items[k].clone() for k in ITEMS}
    rec.update(h=h.clone(), point_track_id=out.point_track_id.clone(), object_ids=out.object_ids.clone(), num_prev=out.num_prev.clone(),
               num_coasted=out.num_coasted.clone(), table_ids=out.table_ids.clone(), table_count=out.table_count.clone())
    rec.update({k: getattr(match, k).clone() for k in MATCH})
    rec.update({"scorer/" + k: getattr(tr.scorer, k).clone() for k in STATE + MEMORY_STATE})
    return rec


def test_the_captured_reacquire_step_equals_the_eager_one():
    batches = train_batches()
    nets = [ref_net(), ref_net()]
    kw = dict(streams=TB, max_boxes=8, max_gt_tracks=32, deterministic=True, reacquire=2)
    eager = TT.SequenceTrainer(nets[0], **kw)
    graph = TT.SequenceTrainer(nets[1], graph=True, graph_warmup=2, **kw)
    assert eager.tracker.max_age == 2 and eager.scorer.track_memory and graph.tracker.static_state
    hs = [None, None]
    captured, coasted, coasted_ones, terms = [], [], [], []
    for t in range(STEPS):
        data, nv = batches[t % 2]
        mk = dict(n_valid=nv)
        if t == 0:
            mk["reset"] = torch.ones(TB, dtype=torch.bool)
        if t == T_RESET[1]:
            mk["reset"] = [s == T_RESET[0] for s in range(TB)]
        if t == T_INACTIVE[1]:
            mk["active"] = [s != T_INACTIVE[0] for s in range(TB)]
        recs = []
        for i, tr in enumerate((eager, graph)):
            # a replayed step without masks from the host: nothing may synchronise.  (The eager trainer's FusedAdam waits for the stream
            # whenever the gradients' addresses change, with or without the tracking term: it is left out of this check.)
            quiet = t == 4 and tr is graph
            if quiet:
                torch.cuda.synchronize()
                torch.cuda.set_sync_debug_mode("error")
            try:
                res = tr.step(*data, hs[i], **mk)
            finally:
                if quiet:
                    torch.cuda.set_sync_debug_mode(0)
            recs.append(train_record(res, tr))
            hs[i] = res[1]
        captured.append(graph.captured)
        bad = [k for k in recs[0] if not same(recs[0][k], recs[1][k])]
        assert bad == [], (t, bad)
        r = recs[1]
        coasted.append(int(r["num_coasted"].sum()))
        rows = torch.arange(r["aff_target"].shape[1], device=DEV).view(1, -1, 1)
        # (num_prev - the previous table's coasted rows) is its detection count; ones at or past it sit on coasted rows
        coasted_ones.append(int((r["aff_target"] * (rows >= (r["num_prev"] - prev_coasted).view(-1, 1, 1))).sum()) if t else 0)
        prev_coasted = r["num_coasted"].clone()
        terms.append(float(r["TrackingLoss"]))
    print("   captured", captured, "coasted rows", coasted, "target ones on coasted rows", coasted_ones, "TrackingLoss", terms)
    assert captured == [False, False, False, True, True, True, True]
    assert captured[T_RESET[1]] and captured[T_INACTIVE[1]]
    assert sum(coasted[3:]) > 0 and max(terms[3:]) > 0
    for (name, a), (_, b) in zip(nets[0].state_dict().items(), nets[1].state_dict().items()):
        assert torch.equal(a, b), name
    np.testing.assert_equal(eager.scorer.result(), graph.scorer.result())
    assert eager.scorer.result()["overall"]["frames"] > 0
    eager.scorer.check()
    graph.scorer.check()


# ---- 10. unwritten memory -------------------------------------------------------------------------------------------------------------
def test_the_memory_scorer_reads_no_unwritten_memory(seq):
    """The rule of tests/test_unwritten_memory_gpu.py on the new entry point behind the eager tracker with max_age = 2: two clean runs
    agree bit for bit, and under the fills (NaN, 1), (1e30, 3), (-7.5, 2) every output and every state tensor equals the clean run."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from hazard_harness import poison
    net = affinity_net()

    def run():
        trk = T.BatchedTracker(net, streams=B3, max_objects=K, max_age=2)
        scorer = TS.TrackScorer(streams=B3, max_objects=K, max_boxes=KB, max_gt_tracks=32, track_memory=True, sweep_frames=8, sweep_records=128)
        rec = {}
        for t, row in enumerate(seq):
            out, gobj, (m,) = step_scene(trk, [scorer], row, *masks(t))
            rec.update({"frame%d/%s" % (t, k): getattr(m, k).clone() for k in MATCH})
            rec.update({"frame%d/%s" % (t, k): getattr(scorer, k).clone() for k in STATE + MEMORY_STATE})
        rec.update({k: getattr(scorer, k).clone() for k in LOG})
        trk.check()
        scorer.check()
        torch.cuda.synchronize()
        return rec

    ref = run()
    assert sum(int(ref["frame%d/labelled_coasted" % t].sum()) for t in range(FRAMES)) > 0
    again = run()
    assert [k for k in ref if not same(ref[k], again[k])] == []
    for fill in ((float("nan"), 1), (1e30, 3), (-7.5, 2)):
        with poison(*fill) as active:
            cur = run()
        assert active.fills > 0
        assert [k for k in ref if not same(ref[k], cur[k])] == [], fill
