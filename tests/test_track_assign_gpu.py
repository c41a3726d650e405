"""GPU: the batched tracker's exact association -- rtk_associate_optimal (csrc/track_assign.hip) called directly on the crafted blocks
of tests/_track_assign_util.py, and `BatchedTracker(assign="optimal")` on a short synthetic sequence.

Every comparison is between integers (floats by their bits) with ==.  The device's matching must be a one-to-one matching of
admissible pairs whose weight equals the host optimum; where that optimum is unique (tests/test_track_assign_cpu.py holds every
decision case to it) the matching itself equals the host's; everything else the launch writes equals the host bookkeeping applied to
the device's own matching."""
import numpy as np
import pytest
import torch

import _track_assign_util as U
import _track_memory_util as M
from ratrack_amd import _lib, synth, tracker as T
from ratrack_amd.track4d import Args, Track4D

pytestmark = pytest.mark.gpu
DEV = "cuda"
NPTS = 96                      # points per stream of the direct launches: more than one pass of the wave
SENTINEL = -12345


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


# ---- 1. the entry point on crafted blocks ----------------------------------------------------------------------------------------------
def launch(K, streams):
    """streams: [dict(aff (m,n) float32, gate is shared, kind "live" | "inactive" | "reset")] with one gate per launch -> the host copy of
    everything the launch wrote, twice (two runs), and the inputs."""
    B = len(streams)
    gate = streams[0]["gate"]
    assert all(s["gate"] == gate for s in streams)
    rng = np.random.default_rng(1000 + K + B)
    aff = np.full((B, K, K), np.nan, dtype=np.float32)               # NaN outside every live block
    num, pc = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    prev_ids = np.full((B, K), -1, dtype=np.int32)
    obj = np.full((B, NPTS), -1, dtype=np.int32)
    counter0 = np.zeros(B, dtype=np.int32)
    for b, s in enumerate(streams):
        m, n = s["aff"].shape
        aff[b, :m, :n] = s["aff"]
        num[b], pc[b] = n, m
        prev_ids[b, :m] = 1000 * (b + 1) + 3 * rng.permutation(m)
        obj[b] = rng.integers(-1, n + 2, NPTS)                       # some points without an object, some with one past n_b
        counter0[b] = 50 + 7 * b
    active = np.array([s["kind"] != "inactive" for s in streams], dtype=np.uint8)
    reset = np.array([s["kind"] == "reset" for s in streams], dtype=np.uint8)
    d = lambda x: torch.from_numpy(x).to(DEV)
    aff_d, num_d, pc_d, prev_d, obj_d, act_d, rst_d = d(aff), d(num), d(pc), d(prev_ids), d(obj), d(active), d(reset)
    runs = []
    for _ in range(2):
        counter = d(counter0.copy())
        i32 = lambda *s: torch.full(s, SENTINEL, dtype=torch.int32, device=DEV)
        out = dict(counter=counter, ids=i32(B, K), count=i32(B), object_ids=i32(B, K), object_conf=torch.full((B, K), -7.0, device=DEV),
                   indices1=i32(B, K), num_prev=i32(B), point_track_id=i32(B, NPTS),
                   total=torch.full((B,), SENTINEL, dtype=torch.int64, device=DEV))
        _lib.call("rtk_associate_optimal", B, NPTS, K, act_d.data_ptr(), rst_d.data_ptr(), aff_d.data_ptr(), num_d.data_ptr(), obj_d.data_ptr(),
                  prev_d.data_ptr(), pc_d.data_ptr(), gate, counter.data_ptr(), out["ids"].data_ptr(), out["count"].data_ptr(),
                  out["object_ids"].data_ptr(), out["object_conf"].data_ptr(), out["indices1"].data_ptr(), out["num_prev"].data_ptr(),
                  out["point_track_id"].data_ptr(), out["total"].data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        runs.append({k: v.cpu() for k, v in out.items()})
    return runs, dict(prev_ids=prev_ids, obj=obj, counter=counter0, aff=aff)


def check_stream(name, s, b, K, got, inp, want):
    """One stream of a launch against the statement; want = (w, total, indices1) of its block (None for a stream that solves nothing)."""
    m, n = s["aff"].shape
    conf_bits = lambda x: np.asarray(x, dtype=np.float32).view(np.int32).tolist()
    if s["kind"] == "inactive":
        assert got["ids"][b].tolist() == inp["prev_ids"][b].tolist(), name
        assert got["object_ids"][b].tolist() == [-1] * K and got["indices1"][b].tolist() == [-1] * K, name
        assert conf_bits(got["object_conf"][b].numpy()) == [0] * K, name
        assert got["point_track_id"][b].tolist() == [-1] * NPTS, name
        assert (int(got["count"][b]), int(got["num_prev"][b]), int(got["counter"][b])) == (m, 0, int(inp["counter"][b])), name
        assert int(got["total"][b]) == SENTINEL, name                 # untouched
        return
    live_m = 0 if s["kind"] == "reset" else m
    idx = got["indices1"][b, :n].tolist()
    if live_m == 0 or n == 0:
        assert idx == [-1] * n and int(got["total"][b]) == 0, name    # no solve ran: every object is fresh
    else:
        w, total, host_idx = want
        assert U.check_matching(w, idx) == int(got["total"][b]), name           # one-to-one, admissible pairs only, and its weight
        assert int(got["total"][b]) == total, name                              # the host optimum
        if s["decision"]:
            assert idx == host_idx, name
    book = U.bookkeeping(idx, s["aff"], inp["prev_ids"][b], int(inp["counter"][b]), inp["obj"][b].tolist(), K)
    assert got["indices1"][b].tolist() == book["indices1"], name
    assert got["object_ids"][b].tolist() == book["object_ids"], name
    assert conf_bits(got["object_conf"][b].numpy()) == conf_bits(book["object_conf"]), name
    assert int(got["counter"][b]) == book["counter"] and int(got["count"][b]) == n and int(got["num_prev"][b]) == live_m, name
    assert got["ids"][b, :n].tolist() == book["ids"] and got["ids"][b, n:].tolist() == [SENTINEL] * (K - n), name      # nothing past the stated rows
    assert got["point_track_id"][b].tolist() == book["point_track_id"], name
    matched = [j for j in range(n) if idx[j] >= 0]
    assert all(float(s["aff"][idx[j], j]) >= s["gate"] and got["object_conf"][b, j].item() != 0.0 for j in matched), name


@pytest.fixture(scope="module")
def table():
    return [(c,) + U.expected(c) for c in U.cases()]


@pytest.mark.parametrize("K", [8, 128, 197])
def test_the_entry_point_equals_the_statement(table, K):
    mine = [(c, w, total, idx) for c, w, total, idx in table if c["K"] == K]
    assert mine
    decided = 0
    for gate in sorted({c["gate"] for c, _, _, _ in mine}):
        group = [(c, (w, total, idx)) for c, w, total, idx in mine if c["gate"] == gate]
        streams = [dict(aff=c["aff"], gate=gate, kind="live", decision=c["decision"], name=c["name"]) for c, _ in group]
        wants = [want for _, want in group]
        # an inactive and a reset stream among them, each holding a block that WOULD be solved
        for kind in ("inactive", "reset"):
            c, want = group[len(group) // 2]
            streams.insert(1, dict(aff=c["aff"], gate=gate, kind=kind, decision=False, name=kind + ":" + c["name"]))
            wants.insert(1, None)
        runs, inp = launch(K, streams)
        for k in runs[0]:
            assert same(runs[0][k], runs[1][k]), (K, gate, k)          # a second run gives identical bits
        for b, (s, want) in enumerate(zip(streams, wants)):
            check_stream(s["name"], s, b, K, runs[0], inp, want)
            decided += bool(s["decision"])
    assert decided == sum(1 for c, _, _, _ in mine if c["decision"]) and decided > 0          # no decision case is left out


def test_total_may_be_null():
    aff = U.TWO_BY_TWO
    K, B = 8, 1
    d = lambda x: torch.from_numpy(x).to(DEV)
    full = np.full((B, K, K), np.nan, dtype=np.float32)
    full[0, :2, :2] = aff
    i32 = lambda *s: torch.full(s, SENTINEL, dtype=torch.int32, device=DEV)
    out = [i32(B), i32(B, K), i32(B), i32(B, K), torch.zeros(B, K, device=DEV), i32(B, K), i32(B), i32(B, 4)]
    out[0].zero_()
    two = torch.tensor([2], dtype=torch.int32, device=DEV)
    prev = d(np.array([[41, 42, -1, -1, -1, -1, -1, -1]], dtype=np.int32))
    obj = d(np.array([[0, 1, 1, -1]], dtype=np.int32))
    _lib.call("rtk_associate_optimal", B, 4, K, None, None, d(full).data_ptr(), two.data_ptr(), obj.data_ptr(), prev.data_ptr(), two.data_ptr(),
              0.01, *(t.data_ptr() for t in out), None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert out[5][0, :2].tolist() == [1, 0] and out[3][0, :3].tolist() == [42, 41, -1] and int(out[0][0]) == 0
    assert out[7][0].tolist() == [42, 41, 41, -1]


# ---- 2. the tracker --------------------------------------------------------------------------------------------------------------------
B3, N, K = 3, 64, 8
FRAMES = 7
RESET, INACTIVE = (1, 3), (2, (2, 4))          # (stream, frame): stream 1 is reset at frame 3, stream 2 sits frames 2 and 4 out
STEP_FIELDS = ("labels", "obj", "point_track_id", "num_objects", "num_prev", "object_ids", "object_conf", "flags", "h")
MEMORY_FIELDS = ("object_hits", "object_gap", "num_coasted")


def soft_net(backbone=False):
    """A Track4D whose Affinity is sigmoid(4 - 0.3 |delta centre|_1): objects 10 m apart still score 0.73 and 20 m apart 0.12, so every
    pair is admissible and the assignment is a real one.  backbone: synthetic weights, every point called moving."""
    net = Track4D(Args()).to(DEV).eval()
    if backbone:
        synth.fill_state_dict(net.state_dict())
        with torch.no_grad():
            net.fd_layer.cp.linear.bias += 4.0
    net.affinity.load_state_dict(M.distance_affinity(4.0, 0.3).state_dict())
    net.invalidate_fused()
    return net


def masks(t):
    reset = torch.tensor([b == RESET[0] and t == RESET[1] for b in range(B3)], dtype=torch.uint8, device=DEV)
    active = torch.tensor([not (b == INACTIVE[0] and t in INACTIVE[1]) for b in range(B3)], dtype=torch.uint8, device=DEV)
    return reset, active


@pytest.fixture(scope="module")
def seq():
    """7 frames of 3 streams with 4, 5 and 6 five-point objects moving 0.2 m per frame, visibility drawn from a seeded generator."""
    frames, vis = M.random_sequence(B=B3, frames=FRAMES, N=N, objects=(4, 5, 6), points=5, seed=11, min_visible=3)
    return dict(frames=frames, vis=vis)


def associate(trk, frame, t):
    pc1, f1, flow, cls, prop, nv = M.batch(frame, DEV)
    return trk.associate(pc1, f1, flow, cls, prop, nv, *masks(t))


def rows(t, counts):
    """t (B, K, ...) with the rows from counts[b] on zeroed."""
    keep = torch.arange(t.shape[1], device=t.device)[None, :] < counts.long()[:, None]
    return torch.where(keep.view(keep.shape + (1,) * (t.dim() - 2)), t, torch.zeros_like(t))


def record(out, trk):
    rec = {k: getattr(out, k).clone() for k in STEP_FIELDS}
    rec["indices1"] = out.indices1().clone()
    rec["aff"] = rows(rows(out.aff, out.num_prev).transpose(1, 2), out.num_objects).transpose(1, 2)
    s = M.written_slot(trk)
    rec["state/count"] = trk.count[s].clone()
    rec["state/ids"] = rows(trk.ids[s], trk.count[s])
    rec["counter"] = trk.counter.clone()
    if out.assign_total is not None:
        rec["assign_total"] = out.assign_total.clone()
    if out.object_hits is not None:
        rec.update({k: getattr(out, k).clone() for k in MEMORY_FIELDS})
    return rec


def differing(a, b):
    assert list(a) == list(b)
    return [k for k in a if not same(a[k], b[k])]


def check_step_against_statement(out, prev_ids, prev_count, counter, reset, active, where, gate=0.01):
    """One step's association outputs against the statement applied to the step's own out.aff -> how many blocks were solved and how
    many of them had a unique optimum."""
    aff = out.aff.cpu().numpy()
    num, nprev = out.num_objects.tolist(), out.num_prev.tolist()
    idx_d, oid, conf = out.indices1().tolist(), out.object_ids.tolist(), bits(out.object_conf).tolist()
    pid, obj, tot = out.point_track_id.tolist(), out.obj.tolist(), out.assign_total.tolist()
    solved = unique = 0
    for b in range(B3):
        if not active[b]:
            assert num[b] == 0 and nprev[b] == 0 and oid[b] == [-1] * K and idx_d[b] == [-1] * K and pid[b] == [-1] * N, where
            continue
        m, n = (0 if reset[b] else prev_count[b]), num[b]
        assert nprev[b] == m, where
        block = aff[b, :m, :n]
        idx = idx_d[b][:n]
        if m and n:
            w = U.quantise(block, gate)
            total, host_idx = U.host_solve(w)
            assert U.check_matching(w, idx) == tot[b] == total, (where, b)
            solved += 1
            if U.is_unique(w):
                unique += 1
                assert idx == host_idx, (where, b)
        else:
            assert idx == [-1] * n and tot[b] == 0, (where, b)
        book = U.bookkeeping(idx, block, prev_ids[b], counter[b], obj[b], K)
        assert idx_d[b] == book["indices1"] and oid[b] == book["object_ids"], (where, b)
        assert conf[b] == book["object_conf"].view(np.int32).tolist() and pid[b] == book["point_track_id"], (where, b)
    return solved, unique


def test_every_step_equals_the_statement_applied_to_its_aff(seq):
    trk = T.BatchedTracker(soft_net(), streams=B3, max_objects=K, assign="optimal")
    solved = unique = inherited = 0
    for t in range(FRAMES):
        reset_d, active_d = masks(t)
        prev_ids, prev_count = trk.ids[1 - trk.cur].tolist(), trk.count[1 - trk.cur].tolist()
        counter = trk.counter.tolist()
        out = associate(trk, seq["frames"][t], t)
        trk.check()
        a, u = check_step_against_statement(out, prev_ids, prev_count, counter, reset_d.tolist(), active_d.tolist(), t)
        solved, unique = solved + a, unique + u
        inherited += int((out.indices1() >= 0).sum())
        # the state the step left: this frame's IDs and count (an inactive stream: carried over)
        w = M.written_slot(trk)
        for b in range(B3):
            if active_d[b]:
                n = int(out.num_objects[b])
                assert int(trk.count[w][b]) == n and trk.ids[w][b, :n].tolist() == out.object_ids[b, :n].tolist(), (t, b)
            else:
                assert int(trk.count[w][b]) == prev_count[b] and trk.ids[w][b].tolist() == prev_ids[b], (t, b)
    assert solved >= 10 and unique >= 8 and inherited >= 20, (solved, unique, inherited)


def test_with_track_memory_the_lifecycle_equals_its_host_statement(seq):
    trk = T.BatchedTracker(soft_net(), streams=B3, max_objects=K, max_age=2, assign="optimal", min_affinity=0.5)
    tables = [M.empty_table(K) for _ in range(B3)]
    coasted = reacquired = solved = 0
    for t in range(FRAMES):
        reset_d, active_d = masks(t)
        reset, active = reset_d.tolist(), active_d.tolist()
        prev_ids, prev_count, counter = trk.ids[1 - trk.cur].tolist(), trk.count[1 - trk.cur].tolist(), trk.counter.tolist()
        out = associate(trk, seq["frames"][t], t)
        assert prev_count == [tb["count"] for tb in tables] and all(prev_ids[b][:tables[b]["count"]] == tables[b]["ids"][:tables[b]["count"]]
                                                                    for b in range(B3)), t
        solved += check_step_against_statement(out, prev_ids, prev_count, counter, reset, active, ("memory", t), gate=0.5)[0]
        w = M.written_slot(trk)
        idx, conf, num, oid = out.indices1().tolist(), out.object_conf.tolist(), out.num_objects.tolist(), out.object_ids.tolist()
        got = {k: getattr(trk, k)[w].tolist() for k in ("ids", "age", "hits", "n_det", "count")}
        got.update({k: getattr(out, k).tolist() for k in MEMORY_FIELDS})
        flags = out.flags.tolist()
        for b in range(B3):
            new, want = M.host_step(tables[b], idx[b], conf[b], num[b], oid[b], bool(reset[b]), bool(active[b]), 2)
            for k in ("ids", "age", "hits", "n_det", "count"):
                assert got[k][b] == new[k], (t, b, k)
            for k in MEMORY_FIELDS:
                assert got[k][b] == want[k], (t, b, k)
            assert bool(flags[b] & 4) == want["truncated"], (t, b)
            tables[b] = new
            coasted += want["num_coasted"]
            reacquired += sum(1 for g in want["object_gap"] if g > 0)
    assert solved >= 10 and coasted > 0 and reacquired > 0, (solved, coasted, reacquired)


def net_inputs(seq):
    """The frames of `seq` as backbone inputs (pc1, pc2, feature1, feature2, n_valid), a hidden object's points left out, every frame
    padded to N columns with copies of column 0 so that one captured graph serves them all."""
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


def test_replay_equals_eager(seq):
    net = soft_net(backbone=True)
    twin = Track4D(Args()).to(DEV)
    twin.load_state_dict({k: v.clone() for k, v in net.state_dict().items()}, strict=True)      # its own engine: the graph keeps it
    frames = net_inputs(seq)
    kw = dict(streams=B3, max_objects=K, max_age=2, assign="optimal")
    eager, graphed = T.BatchedTracker(net, **kw), T.BatchedTracker(twin.eval(), graph=True, graph_warmup=2, **kw)
    captured, objects, totals = [], 0, 0
    with torch.no_grad():
        for t, (pc1, pc2, f1, f2, nv) in enumerate(frames):
            reset, active = masks(t)
            a = record(eager.step(pc1, pc2, f1, f2, n_valid=nv, reset=reset, active=active), eager)
            b = record(graphed.step(pc1, pc2, f1, f2, n_valid=nv, reset=reset, active=active), graphed)
            captured.append(graphed.captured)
            assert differing(a, b) == [], t
            objects += int(a["num_objects"].sum())
            totals += int((a["assign_total"] > 0).sum())
    assert captured == [False, False] + [True] * (FRAMES - 2) and objects > 0 and totals > 0, (captured, objects, totals)


def test_sinkhorn_given_explicitly_is_the_tracker_without_the_keyword(seq, monkeypatch):
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    net = soft_net()
    runs = {}
    for name, kw in (("plain", {}), ("named", dict(assign="sinkhorn", min_affinity=0.01)), ("optimal", dict(assign="optimal"))):
        trk = T.BatchedTracker(net, streams=B3, max_objects=K, **kw)
        del calls[:]
        recs = []
        for t in range(FRAMES):
            out = associate(trk, seq["frames"][t], t)
            recs.append(record(out, trk))
            assert (out.assign_total is None) == (name != "optimal")
        runs[name] = dict(recs=recs, calls=list(calls), buffers=trk.assign_total)
    assert runs["plain"]["calls"] == runs["named"]["calls"] and "rtk_associate_optimal" not in runs["plain"]["calls"]
    assert runs["plain"]["calls"].count("rtk_associate_batched") == FRAMES and runs["plain"]["buffers"] is None
    # the same number of launches, one of them exchanged
    assert [c.replace("rtk_associate_optimal", "rtk_associate_batched") for c in runs["optimal"]["calls"]] == runs["plain"]["calls"]
    assert "rtk_associate_batched" not in runs["optimal"]["calls"]
    for t in range(FRAMES):
        assert differing(runs["plain"]["recs"][t], runs["named"]["recs"][t]) == [], t
