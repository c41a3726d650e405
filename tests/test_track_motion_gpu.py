"""GPU: coasted tracks that move -- BatchedTracker(motion="flow") and rtk_track_memory_motion (csrc/track_motion.hip).

Every comparison is exact (== on integers, int32 views on floats).  As in tests/test_track_memory_gpu.py the tests call
`trk.associate(...)` on synthetic backbone outputs whose objects are where the frame builder put them -- here with the flow the test
gave each object (tests/_track_motion_util.py) -- and the Affinity is a `distance_affinity`, so which object follows which is decided
by construction.  Only the execution-form tests and the trainer test run a backbone."""
import os
import sys

import numpy as np
import pytest
import torch

import _gt_util as GU
import _track_memory_util as U
import _track_motion_util as MU
from _util import reference_state_dict
from ratrack_amd import _lib, gt_device as G, synth, track_score as TS, track_train as TT, tracker as T, vod_gt
from ratrack_amd.track4d import Args, Track4D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = "cuda"
B3, N, K = 3, 64, 16
FRAMES = 8
RESET, INACTIVE = (1, 3), (2, (2, 4))          # (stream, frame): the masks of tests/test_track_memory_gpu.py
STEP_FIELDS = ("labels", "obj", "point_track_id", "num_objects", "num_prev", "object_ids", "object_conf", "flags", "h")
MEMORY_FIELDS = ("object_hits", "object_gap", "num_coasted")
MOTION_FIELDS = ("object_velocity", "table_velocity")


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def affinity_net(c=4.0, s=4.0, backbone=False):
    """A Track4D whose Affinity is distance_affinity(c, s); backbone: synthetic weights with the segmentation head's bias raised, so
    that every point is called moving."""
    net = Track4D(Args()).to(DEV).eval()
    if backbone:
        synth.fill_state_dict(net.state_dict())
        with torch.no_grad():
            net.fd_layer.cp.linear.bias += 4.0
    net.affinity.load_state_dict(U.distance_affinity(c, s).state_dict())
    net.invalidate_fused()
    return net


def masks(t, B=B3):
    reset = torch.tensor([b == RESET[0] and t == RESET[1] for b in range(B)], dtype=torch.uint8, device=DEV)
    active = torch.tensor([not (b == INACTIVE[0] and t in INACTIVE[1]) for b in range(B)], dtype=torch.uint8, device=DEV)
    return reset, active


def associate(trk, frame, reset=None, active=None):
    pc1, f1, flow, cls, prop, nv = U.batch(frame, DEV)
    B = pc1.shape[0]
    reset = torch.zeros(B, dtype=torch.uint8, device=DEV) if reset is None else reset
    active = torch.ones(B, dtype=torch.uint8, device=DEV) if active is None else active
    return trk.associate(pc1, f1, flow, cls, prop, nv, reset, active)


def state(trk):
    """Clones of the table the last step wrote: ids, age, hits (B,K), n_det, count (B), desc (B,K,141) and, with motion, vel (B,K,3)."""
    s = U.written_slot(trk)
    names = ("ids", "count", "desc") + (() if trk.max_age is None else ("age", "hits", "n_det")) + (() if trk.vel is None else ("vel",))
    return {k: getattr(trk, k)[s].clone() for k in names}


def rows(t, counts):
    """t (B, K, ...) with the rows from counts[b] on zeroed."""
    keep = torch.arange(t.shape[1], device=t.device)[None, :] < counts.long()[:, None]
    return torch.where(keep.view(keep.shape + (1,) * (t.dim() - 2)), t, torch.zeros_like(t))


def record(out, trk):
    """Everything a step defines, cloned: the StepResult's tensors (aff and the descriptors: their live part), the table with its
    velocities up to `count`, the counter."""
    rec = {k: getattr(out, k).clone() for k in STEP_FIELDS}
    rec["indices1"] = out.indices1().clone()
    rec["aff"] = rows(rows(out.aff, out.num_prev).transpose(1, 2), out.num_objects).transpose(1, 2)
    rec["descriptors"] = rows(out.descriptors, out.num_objects)
    rec["desc_prev"] = rows(out.desc_prev, out.num_prev)
    if out.object_hits is not None:
        rec.update({k: getattr(out, k).clone() for k in MEMORY_FIELDS})
        rec["prev_age"] = rows(out.prev_age, out.num_prev)
    st = state(trk)
    if out.object_velocity is not None:
        rec["object_velocity"] = out.object_velocity.clone()
        rec["table_velocity"] = rows(out.table_velocity, st["count"])
    for k in ("ids", "desc", "age", "hits", "vel"):
        if k in st:
            rec["state/" + k] = rows(st[k], st["count"])
    rec["state/count"] = st["count"]
    if "n_det" in st:
        rec["state/n_det"] = st["n_det"]
    rec["counter"] = trk.counter.clone()
    return rec


def differing(a, b, keys=None):
    keys = list(a) if keys is None else keys
    return [k for k in keys if not same(a[k], b[k])]


@pytest.fixture(scope="module")
def seq():
    """8 frames of 3 streams with 6, 7 and 8 five-point objects moving 0.2 m per frame, seeded visibility (at least 5 visible), every
    object with a flow of its own that changes a little from frame to frame."""
    frames, vis = MU.motion_sequence(B=B3, frames=FRAMES, N=N, objects=(6, 7, 8), points=5, seed=7, min_visible=5)
    return dict(frames=frames, vis=vis)


# ---- 1. off means off -----------------------------------------------------------------------------------------------------------------
def test_off_means_off(seq, monkeypatch):
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    net = affinity_net()
    runs = {}
    for name, kw in (("today", {}), ("none", dict(motion=None)), ("flow", dict(motion="flow"))):
        trk = T.BatchedTracker(net, streams=B3, max_objects=K, max_age=2, **kw)
        del calls[:]
        recs, fields = [], []
        for t in range(6):
            out = associate(trk, seq["frames"][t], *masks(t))
            recs.append(record(out, trk))
            fields.append({k: getattr(out, k) for k in MOTION_FIELDS})
        runs[name] = dict(recs=recs, calls=list(calls), fields=fields, vel=trk.vel)
    today, none, flow = runs["today"], runs["none"], runs["flow"]
    assert none["calls"] == today["calls"] and "rtk_track_memory_motion" not in none["calls"]
    assert today["calls"] == ["rtk_dbscan_batched", "rtk_object_descriptors", "rtk_affinity_pairs", "rtk_associate_batched",
                              "rtk_track_memory"] * 6
    assert none["vel"] is None and today["vel"] is None
    for t in range(6):
        assert all(v is None for v in none["fields"][t].values()) and len(none["fields"][t]) == 2
        assert list(none["recs"][t]) == list(today["recs"][t])
        assert differing(none["recs"][t], today["recs"][t]) == [], t
    assert sum(int(r["num_coasted"].sum()) for r in none["recs"]) > 0
    # and on means the other entry point, never both
    assert flow["calls"].count("rtk_track_memory_motion") == 6 and "rtk_track_memory" not in flow["calls"]
    assert tuple(flow["vel"].shape) == (2, B3, K, 3) and flow["vel"].dtype == torch.float32
    assert all(tuple(f["object_velocity"].shape) == (B3, K, 3) and tuple(f["table_velocity"].shape) == (B3, K, 3) for f in flow["fields"])


# ---- 2. the kernel equals the host statement ----------------------------------------------------------------------------------------
class HostTables:
    """The host statement carried along a run: per stream the table, its velocities and its descriptors."""

    def __init__(self, B, Kt, max_age, beta):
        self.B, self.K, self.max_age, self.beta = B, Kt, max_age, beta
        self.tables = [U.empty_table(Kt) for _ in range(B)]
        self.vel, self.desc = zip(*[MU.empty_motion(Kt) for _ in range(B)])
        self.vel, self.desc = list(self.vel), list(self.desc)
        self.counts = dict(coasted=0, twice=0, reacquired=0, moved=0, smoothed=0)

    def check(self, out, trk, reset, active, where):
        """Compares the step `out` of `trk` with the host statement, bit for bit, and advances the host's tables."""
        Kt = self.K
        st = {k: v.cpu() for k, v in state(trk).items()}
        idx, conf, num, oid = out.indices1().tolist(), out.object_conf.tolist(), out.num_objects.tolist(), out.object_ids.tolist()
        got = {k: st[k].tolist() for k in ("ids", "age", "hits", "n_det", "count")}
        got.update({k: getattr(out, k).tolist() for k in MEMORY_FIELDS})
        desc, vel, ovel = st["desc"].numpy(), st["vel"].numpy(), out.object_velocity.cpu().numpy()
        assert same(out.table_velocity, trk.vel[U.written_slot(trk)])
        for b in range(self.B):
            w = where + (b,)
            prev, prev_vel, prev_desc = self.tables[b], self.vel[b], self.desc[b]
            new, hvel, htab, want = MU.host_step_motion(prev, prev_vel, prev_desc, desc[b], idx[b], conf[b], num[b], oid[b], bool(reset[b]),
                                                        bool(active[b]), self.max_age, self.beta)
            for k in ("ids", "age", "hits", "n_det", "count"):
                assert got[k][b] == new[k], (w, k)
            for k in MEMORY_FIELDS:
                assert got[k][b] == want[k], (w, k)
            assert not want["truncated"], w
            c = new["count"]
            assert np.array_equal(MU.ibits(vel[b]), MU.ibits(hvel)), (w, "vel")                       # all K rows: zero past the count
            assert np.array_equal(MU.ibits(ovel[b]), MU.ibits(want["object_velocity"])), (w, "object_velocity")
            assert np.array_equal(MU.ibits(desc[b, :c]), MU.ibits(htab[:c])), (w, "desc")
            for r, i in enumerate(want["src"]):                                                       # (said again, without the helper)
                if i is not None:
                    assert np.array_equal(MU.ibits(desc[b, r, 3:]), MU.ibits(prev_desc[i, 3:])), (w, r, i)
                    assert np.array_equal(MU.ibits(desc[b, r, :3]), MU.ibits(prev_desc[i, :3] + prev_vel[i])), (w, r, i)
                    assert np.array_equal(MU.ibits(vel[b, r]), MU.ibits(prev_vel[i])), (w, r, i)
                    self.counts["moved"] += int(not np.array_equal(MU.ibits(desc[b, r, :3]), MU.ibits(prev_desc[i, :3])))
                    self.counts["twice"] += int(new["age"][r] >= 2)
            if active[b]:
                m = 0 if reset[b] else prev["count"]
                for j in range(num[b]):
                    if 0 <= idx[b][j] < m and conf[b][j] != 0:
                        self.counts["smoothed"] += int(not np.array_equal(MU.ibits(vel[b, j]), MU.ibits(desc[b, j, MU.FLOW])))
            self.tables[b], self.vel[b], self.desc[b] = new, hvel, htab
            self.counts["coasted"] += want["num_coasted"]
            self.counts["reacquired"] += sum(1 for g in want["object_gap"] if g > 0)


@pytest.mark.parametrize("beta", [1.0, 0.25])
@pytest.mark.parametrize("max_age", [1, 3])
def test_kernel_equals_the_host_statement(seq, max_age, beta):
    trk = T.BatchedTracker(affinity_net(), streams=B3, max_objects=K, max_age=max_age, motion="flow", motion_beta=beta)
    host = HostTables(B3, K, max_age, beta)
    for t in range(FRAMES):
        reset_d, active_d = masks(t)
        out = associate(trk, seq["frames"][t], reset_d, active_d)
        trk.check()
        host.check(out, trk, reset_d.tolist(), active_d.tolist(), (max_age, beta, t))
    c = host.counts
    print("   max_age %d beta %g:" % (max_age, beta), c)
    assert c["coasted"] > 0 and c["moved"] > 0 and c["reacquired"] > 0, c
    assert (c["twice"] > 0) == (max_age >= 2), c                   # (with max_age = 1 no row can coast twice)
    assert (c["smoothed"] > 0) == (beta != 1.0), c                 # beta = 1: every velocity is the measured flow, bit for bit


# ---- 3. compaction across wavefronts ------------------------------------------------------------------------------------------------
def test_compaction_across_wavefronts():
    n_obj, big = 70, 160
    trk = T.BatchedTracker(affinity_net(), streams=1, max_objects=big, max_age=2, motion="flow", motion_beta=0.25)
    assert trk.min_samples == 2
    host = HostTables(1, big, 2, 0.25)
    centres = U.lattice(n_obj)
    k = torch.arange(n_obj, dtype=torch.float32)
    flows = torch.stack((0.0137 * (k % 9) + 0.003 * k + 0.011, 0.0071 * (k % 7) - 0.019, -0.0053 * (k % 5) + 0.0171), dim=1)
    visible_by_frame = [[True] * n_obj, [j % 2 == 1 for j in range(n_obj)], [False] * n_obj]
    outs, states = [], []
    one = [1]
    for t, visible in enumerate(visible_by_frame):
        out = associate(trk, [MU.flow_stream(centres, visible, big, flows * (1.0 + 0.1 * t), points=2, seed=200 + t)])
        trk.check()
        host.check(out, trk, [0], one, ("wavefronts", t))
        outs.append(out)
        states.append({k_: v[0].clone() for k_, v in state(trk).items()})
    ids0 = outs[0].object_ids[0, :n_obj].tolist()
    assert int(outs[0].num_objects[0]) == n_obj and len(set(ids0)) == n_obj
    # frame 1: the 35 even objects coast into rows 35 .. 69, their source rows 0, 2, .. 68 in two wavefronts
    s1, s2 = states[1], states[2]
    assert int(s1["count"]) == 70 and int(s1["n_det"]) == 35 and s1["ids"][:70].tolist() == ids0[1::2] + ids0[0::2]
    # frame 2: nothing is detected: 70 survivors (more than a wavefront), source rows 0 .. 69
    assert int(outs[2].num_objects[0]) == 0 and int(s2["count"]) == 70 and s2["ids"][:70].tolist() == s1["ids"][:70].tolist()
    assert s2["age"][:70].tolist() == [1] * 35 + [2] * 35
    assert same(s2["vel"][:70], s1["vel"][:70])
    moved = s1["desc"][:70, :3] + s1["vel"][:70]
    assert same(s2["desc"][:70, :3], moved) and same(s2["desc"][:70, 3:], s1["desc"][:70, 3:])
    assert int((bits(s2["desc"][:70, :3]) != bits(s1["desc"][:70, :3])).any(dim=1).sum()) == 70       # every centre moved
    assert host.counts["moved"] >= 35 + 70 and host.counts["twice"] == 35


# ---- 4. IDs known by construction ---------------------------------------------------------------------------------------------------
SPEED = 1.2


def fast_centres(t):
    return U.lattice(3) + torch.tensor([SPEED * t, 0.0, 0.0])


def fast_scenario(g):
    """Three objects moving 1.2 m per frame along x, their flow (1.2, 0, 0); object A (index 0) is hidden in frames 2 .. 2 + g - 1 and
    back in frame 2 + g."""
    out = []
    for t in range(2 + g + 2):
        visible = [not 2 <= t < 2 + g, True, True]
        out.append([MU.flow_stream(fast_centres(t), visible, 32, [[SPEED, 0.0, 0.0]] * 3, points=3, seed=100 + t)])
    return out


def run_fast(g, motion):
    """distance_affinity(8, 4): sigmoid(8 - 4 |delta centre|_1) -- 0.96 one frame (1.2 m) stale, 0.17 two frames, 0.0017 three, and
    below 0.01 the association hands out a fresh ID."""
    trk = T.BatchedTracker(affinity_net(8.0, 4.0), streams=1, max_objects=8, max_age=2, motion=motion)
    res = []
    for frame in fast_scenario(g):
        out = associate(trk, frame)
        trk.check()
        n = int(out.num_objects[0])
        r = dict(ids=out.object_ids[0, :n].tolist(), gap=out.object_gap[0, :n].tolist(), hits=out.object_hits[0, :n].tolist(),
                 coasted=int(out.num_coasted[0]), conf=out.object_conf[0, :n].tolist())
        if motion is not None:
            r["velocity"] = out.object_velocity[0, :n].cpu()
        res.append(r)
    return res


@pytest.mark.parametrize("g", [1, 2])
def test_a_fast_object_keeps_its_id_only_when_its_coasted_track_moves(g):
    back = 2 + g
    held, moving = run_fast(g, None), run_fast(g, "flow")
    for res in (held, moving):
        a, b, c = res[0]["ids"]
        assert len({a, b, c}) == 3 and res[1]["ids"] == [a, b, c]
        for t in range(2, back):
            assert res[t]["ids"] == [b, c] and res[t]["coasted"] == 1, t       # B and C are followed throughout, A's row coasts
        assert res[back]["ids"][1:] == [b, c] and res[back + 1]["ids"][1:] == [b, c]
        print("   g %d:" % g, "conf at the return", res[back]["conf"], "ids", res[back]["ids"])
    a = moving[0]["ids"][0]
    # with motion the coasted row is one frame stale whatever g is: A keeps its ID
    assert moving[back]["ids"][0] == a and moving[back]["gap"] == [g, 0, 0] and moving[back]["hits"] == [3, back + 1, back + 1]
    assert moving[back + 1]["ids"][0] == a and moving[back + 1]["gap"] == [0, 0, 0]
    for r in moving:
        assert torch.allclose(r["velocity"], torch.tensor([SPEED, 0.0, 0.0]).expand_as(r["velocity"]), rtol=0, atol=1e-5)
    a = held[0]["ids"][0]
    if g == 1:      # 2.4 m stale: sigmoid(8 - 9.6) = 0.17, still above 0.01
        assert held[back]["ids"][0] == a and held[back]["gap"] == [1, 0, 0]
    else:           # 3.6 m stale: sigmoid(8 - 14.4) = 0.0017: a NEW ID although the track is still in the table
        new = held[back]["ids"][0]
        assert new != a and new not in held[0]["ids"] and held[back]["gap"] == [-1, 0, 0] and held[back]["hits"][0] == 1
        assert held[back + 1]["ids"][0] == new


def scored(motion):
    trk = T.BatchedTracker(affinity_net(8.0, 4.0), streams=1, max_objects=8, max_age=2, motion=motion)
    scorer = TS.TrackScorer(streams=1, max_objects=8, max_boxes=8, max_gt_tracks=16)
    frames = fast_scenario(2)
    for t, frame in enumerate(frames):
        first = torch.tensor([t == 0], dtype=torch.uint8, device=DEV)
        out = associate(trk, frame, reset=first)
        c = fast_centres(t).tolist()
        labels = {k: vod_gt.Label("Car", k, 0, 0, 0, 0, 0, 0, 3.0, 4.0, 6.0, c[k][0], c[k][1], c[k][2], 0.0) for k in range(3)}
        per_stream = [(labels, GU.IDENTITY_TF, labels, GU.IDENTITY_TF)]
        bb = G.pack_boxes(per_stream, 8, DEV)
        nv = torch.tensor([frame[0]["n_valid"]], dtype=torch.int32, device=DEV)
        gobj = TS.gt_objects(out.pc1, bb, TS.pack_box_types(per_stream, 8, DEV), n_valid=nv, min_obj_points=2)
        scorer.update(out, gobj, reset=first)
    trk.check()
    return scorer.result()["overall"], len(frames)


def test_the_score_sees_the_gap_that_only_motion_bridges():
    held, frames = scored(None)
    moving, _ = scored("flow")
    assert int(held["idsw"]) == 1 and int(moving["idsw"]) == 0
    for k in ("tp", "fp", "fn", "gt", "pred"):
        assert int(held[k]) == int(moving[k]), k
    assert int(held["gt"]) == 3 * frames and int(held["fn"]) == 2 and int(held["fp"]) == 0


# ---- 5. static state, captured step, pipeline ---------------------------------------------------------------------------------------
MOTION_KW = dict(max_age=2, motion="flow", motion_beta=0.25)


def net_inputs(seq):
    """The frames of `seq` as backbone inputs (tests/test_track_memory_gpu.py `net_inputs`): per frame (pc1, pc2, feature1, feature2,
    n_valid), a hidden object's points left out, every frame padded to N columns with copies of column 0."""
    frames = []
    for row in seq["frames"]:
        pc1, f1, counts = [], [], []
        for s in row:
            keep = torch.nonzero(s["cls"][:s["n_valid"]] > 0.5).reshape(-1)
            pad = torch.cat([keep, keep[:1].expand(N - keep.numel())])
            pc1.append(s["pc1"][:, pad])
            f1.append(s["feature1"][:, pad])
            counts.append(keep.numel())
        pc1, f1 = torch.stack(pc1).to(DEV), torch.stack(f1).to(DEV)
        nv = torch.tensor([counts, counts], dtype=torch.int32, device=DEV)
        frames.append((pc1, pc1 + torch.tensor([0.2, 0.0, 0.0], device=DEV).view(1, 3, 1), f1, f1.clone(), nv))
    return frames


@pytest.fixture(scope="module")
def stepped(seq):
    """The eager double-buffered tracker with max_age = 2, motion and beta = 0.25 through step(), computed once."""
    net = affinity_net(backbone=True)
    frames = net_inputs(seq)
    trk = T.BatchedTracker(net, streams=B3, max_objects=K, **MOTION_KW)
    recs = []
    with torch.no_grad():
        for t, (pc1, pc2, f1, f2, nv) in enumerate(frames):
            reset, active = masks(t)
            out = trk.step(pc1, pc2, f1, f2, n_valid=nv, reset=reset, active=active)
            trk.check()
            recs.append(record(out, trk))
    objects = sum(int(r["num_objects"].sum()) for r in recs)
    coasted = sum(int(r["num_coasted"].sum()) for r in recs)
    moving = sum(int((r["state/vel"] != 0).sum()) for r in recs)
    print("   stepped: objects", objects, "coasted rows", coasted, "non-zero velocity components", moving)
    assert objects > 0 and coasted > 0 and moving > 0, (objects, coasted, moving)
    assert all("state/vel" in r and "object_velocity" in r and "table_velocity" in r for r in recs)
    return dict(sd={k: v.clone() for k, v in net.state_dict().items()}, frames=frames, recs=recs)


def clone_net(sd):
    net = Track4D(Args()).to(DEV)
    net.load_state_dict(sd, strict=True)
    return net.eval()


def test_static_state_equals_the_swap(stepped, monkeypatch):
    from ratrack_amd import fused
    jobs = []
    real = fused.copy_multi
    monkeypatch.setattr(fused, "copy_multi", lambda pairs: (jobs.append(pairs), real(pairs))[1])
    trk = T.BatchedTracker(clone_net(stepped["sd"]), streams=B3, max_objects=K, static_state=True, **MOTION_KW)
    with torch.no_grad():
        for t, (pc1, pc2, f1, f2, nv) in enumerate(stepped["frames"]):
            reset, active = masks(t)
            out = trk.step(pc1, pc2, f1, f2, n_valid=nv, reset=reset, active=active)
            assert differing(record(out, trk), stepped["recs"][t]) == [], t
    assert trk.cur == 0 and not trk.captured
    # the state advance, vel with it: seven jobs of ONE rtk_copy_multi launch (which takes eight) per step
    advance = [p for p in jobs if p[0][0].data_ptr() == trk.desc[1].data_ptr()]
    assert len(advance) == FRAMES and all(len(p) == 7 for p in advance)
    assert all(p[-1][0].data_ptr() == trk.vel[1].data_ptr() and p[-1][1].data_ptr() == trk.vel[0].data_ptr() for p in advance)


def test_replay_equals_eager(stepped):
    trk = T.BatchedTracker(clone_net(stepped["sd"]), streams=B3, max_objects=K, graph=True, graph_warmup=2, **MOTION_KW)
    captured = []
    with torch.no_grad():
        for t, (pc1, pc2, f1, f2, nv) in enumerate(stepped["frames"]):
            reset, active = masks(t)
            out = trk.step(pc1, pc2, f1, f2, n_valid=nv, reset=reset, active=active)
            captured.append(trk.captured)
            assert differing(record(out, trk), stepped["recs"][t]) == [], t
            trk.check()
    assert captured == [False, False] + [True] * (FRAMES - 2) and trk.captured


def test_pipeline_groups_equal_eager(stepped):
    groups = 2
    pipe = T.TrackerPipeline(clone_net(stepped["sd"]), groups=groups, streams=B3, max_objects=K, graph_warmup=2, **MOTION_KW)
    got = [[] for _ in range(groups)]
    with torch.no_grad():
        for t, (pc1, pc2, f1, f2, nv) in enumerate(stepped["frames"]):
            reset, active = masks(t)
            outs = [pipe.submit(g, pc1, pc2, f1, f2, n_valid=nv, reset=reset, active=active) for g in range(groups)]      # both in flight
            for g in range(groups):
                with torch.cuda.stream(pipe.streams[g]):
                    got[g].append(record(outs[g], pipe.trackers[g]))
        pipe.drain()
        torch.cuda.synchronize()
    assert all(trk.captured and trk.motion == "flow" for trk in pipe.trackers)
    for g in range(groups):
        for t in range(FRAMES):
            assert differing(got[g][t], stepped["recs"][t]) == [], (g, t)


# ---- 6. unwritten memory ------------------------------------------------------------------------------------------------------------
def test_track_motion_reads_no_unwritten_memory(seq):
    """The rule of tests/test_unwritten_memory_gpu.py on the eager tracker with max_age = 2 and motion: two clean runs agree bit for
    bit, and under the fills (NaN, 1), (1e30, 3), (-7.5, 2) every recorded tensor and the state tables, vel included, up to `count`
    equal the clean run."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from hazard_harness import poison
    net = affinity_net()
    inputs = [U.batch(frame, DEV) for frame in seq["frames"]]
    assert min(K, N, min(s["n_valid"] for row in seq["frames"] for s in row)) >= 4

    def run():
        trk = T.BatchedTracker(net, streams=B3, max_objects=K, **MOTION_KW)
        rec = {}
        for t, (pc1, f1, flow, cls, prop, nv) in enumerate(inputs):
            out = trk.associate(pc1, f1, flow, cls, prop, nv, *masks(t))
            rec.update({"frame%d/%s" % (t, k): v for k, v in record(out, trk).items()})
        trk.check()
        torch.cuda.synchronize()
        return rec
    ref = run()
    for t in range(FRAMES):
        live = [c for c in ref["frame%d/num_objects" % t].tolist() + ref["frame%d/state/count" % t].tolist()]
        assert all(c >= 4 or c == 0 for c in live), (t, live)
    assert sum(int(ref["frame%d/num_coasted" % t].sum()) for t in range(FRAMES)) > 0
    assert "frame0/state/vel" in ref and "frame0/object_velocity" in ref
    assert differing(ref, run()) == []
    for fill in ((float("nan"), 1), (1e30, 3), (-7.5, 2)):
        with poison(*fill) as active:
            cur = run()
        assert active.fills > 0
        assert differing(ref, cur) == [], fill


# ---- 7. the trainer -------------------------------------------------------------------------------------------------------------------
TB, STEPS = 2, 6
ITEMS = ("Loss", "SceneFlowLoss", "SegLoss", "TrackingLoss")


def ref_net():
    sd = reference_state_dict(DEV)
    sd["fd_layer.cp.linear.bias"] = sd["fd_layer.cp.linear.bias"] + 0.09      # moving points in every frame (tests/test_tracker_gpu.py)
    net = Track4D(Args()).to(DEV)
    net.load_state_dict(sd, strict=True)
    return net.train()


def train_batches():
    """The recipe of tests/test_track_memory_train_gpu.py at B = 2 (synthetic pairs, six labelled boxes per stream), twice: the whole
    clouds, and the clouds cut to 60 % of their points through n_valid -- other detections, so that tracks are lost between steps."""
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
    st = state(tr.tracker)
    rec.update(h=h.clone(), point_track_id=out.point_track_id.clone(), object_ids=out.object_ids.clone(), num_prev=out.num_prev.clone(),
               num_coasted=out.num_coasted.clone(), table_ids=out.table_ids.clone(), table_count=out.table_count.clone(),
               desc_prev=rows(out.desc_prev, out.num_prev), object_velocity=out.object_velocity.clone(),
               table_velocity=rows(out.table_velocity, st["count"]), aff_target=match.aff_target.clone())
    rec.update({"state/" + k: (rows(v, st["count"]) if v.dim() > 1 else v) for k, v in st.items()})
    return rec


def test_the_trainer_trains_on_moved_rows_and_its_captured_step_equals_the_eager_one():
    batches = train_batches()
    nets = [ref_net(), ref_net()]
    kw = dict(streams=TB, max_boxes=8, max_gt_tracks=32, deterministic=True, reacquire=2, motion="flow", motion_beta=0.25)
    eager = TT.SequenceTrainer(nets[0], **kw)
    graph = TT.SequenceTrainer(nets[1], graph=True, graph_warmup=2, **kw)
    for tr in (eager, graph):
        assert tr.tracker.max_age == 2 and tr.tracker.motion == "flow" and tr.tracker.motion_beta == 0.25 and tr.scorer.track_memory
    hs = [None, None]
    history, captured, terms = [], [], []
    coasted_rows = moved_rows = 0
    for t in range(STEPS):
        data, nv = batches[t % 2]
        mk = dict(n_valid=nv)
        if t == 0:
            mk["reset"] = torch.ones(TB, dtype=torch.bool)
        recs = []
        for i, tr in enumerate((eager, graph)):
            res = tr.step(*data, hs[i], **mk)
            assert not res[2].desc_prev.requires_grad
            recs.append(train_record(res, tr))
            hs[i] = res[1]
        captured.append(graph.captured)
        bad = [k for k in recs[0] if not same(recs[0][k], recs[1][k])]
        assert bad == [], (t, bad)
        r = {k: v.cpu() for k, v in recs[0].items()}
        assert bool(torch.isfinite(r["TrackingLoss"]).all()), t
        terms.append(float(r["TrackingLoss"]))
        if t >= 1:      # out.desc_prev is the table the step before wrote
            p = history[-1]
            for b in range(TB):
                c = int(p["state/count"][b])
                assert int(r["num_prev"][b]) == c and same(r["desc_prev"][b, :c], p["state/desc"][b, :c]), (t, b)
        if t >= 2:      # ... and its coasted rows are their source rows of the table before that, the centre moved by the velocity
            p, q = history[-1], history[-2]
            for b in range(TB):
                ids_q = q["state/ids"][b, :int(q["state/count"][b])].tolist()
                for row in range(int(p["state/n_det"][b]), int(p["state/count"][b])):
                    i = ids_q.index(int(p["state/ids"][b, row]))
                    assert same(r["desc_prev"][b, row, :3], q["state/desc"][b, i, :3] + q["state/vel"][b, i]), (t, b, row)
                    assert same(r["desc_prev"][b, row, 3:], q["state/desc"][b, i, 3:]) and same(p["state/vel"][b, row], q["state/vel"][b, i])
                    coasted_rows += 1
                    moved_rows += int(not same(r["desc_prev"][b, row, :3], q["state/desc"][b, i, :3]))
        history.append(r)
    print("   captured", captured, "coasted rows checked", coasted_rows, "moved", moved_rows, "TrackingLoss", terms)
    assert captured == [False, False, False] + [True] * (STEPS - 3)
    assert coasted_rows > 0 and moved_rows > 0
    for (name, a), (_, b) in zip(nets[0].state_dict().items(), nets[1].state_dict().items()):
        assert torch.equal(a, b), name
    eager.check()
    graph.check()
