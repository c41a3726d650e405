"""GPU: the filter inside the tracked step (rtk_track_box_filter_step, csrc/track_box_step.hip; boxes.filter_step_raw;
BatchedTracker(box_filter=...)) against the host statement of tests/_box_filter_step_util.py and against the offline launch
(ResultLog.filter_boxes).  Every comparison is of bits: the arithmetic is a correctly rounded float64 chain shared through
csrc/box_filter.h, so there is no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

import _box_filter_step_util as S
import _box_filter_util as K
import _track_memory_util as M
import test_box_filter_gpu as FG
import test_track_boxes_gpu as TBG
import test_track_memory_gpu as TM
import test_tracker_graph_gpu as TG
from ratrack_amd import _lib, boxes as BX, result_log as RL, tracker as T
from ratrack_amd.captured import capture_graph

pytestmark = pytest.mark.gpu
DEV = "cuda"
GAP = 2
PAR = dict(max_gap=GAP, q_vel=0.25, r_yaw=0.5)
TABLES = ("ids_prev", "count_prev", "ids_new", "count_new", "num_objects", "box", "valid", "active", "reset")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def poisoned(B, rows):
    into = BX.StepBoxes.empty(B, rows, DEV)
    for n in S.FLOATS + S.INTS:
        getattr(into, n).view(torch.int32).fill_(S.POISON)
    return into


def device_state(B, rows):
    state, since = S.empty_state(B, rows)
    return _dev(state), _dev(since)


def host_of(out, state, since):
    """A StepBoxes and the state after the step in the form of `_box_filter_step_util.walk`'s entries."""
    return dict(out={n: getattr(out, n).cpu().numpy() for n in S.FLOATS + S.INTS}, state=state.cpu().numpy(), since=since.cpu().numpy())


def run(steps, flt):
    """The launch over a sequence, every output into poisoned buffers: -> walk's form."""
    B, rows = steps[0]["ids_new"].shape
    state, since = device_state(B, rows)
    res = []
    for s in steps:
        d = {n: _dev(s[n]) for n in TABLES}
        out = BX.filter_step_raw(d["ids_prev"], d["count_prev"], d["ids_new"], d["count_new"], d["num_objects"], d["box"], d["valid"], state, since,
                                 filter=flt, active=d["active"], reset=d["reset"], into=poisoned(B, rows))
        res.append(host_of(out, state, since))
    return res


def assert_same(got, want, where):
    """Two sequences in walk's form: all rows of every output, of the state and of since, by their bits."""
    assert len(got) == len(want)
    for t, (g, w) in enumerate(zip(got, want)):
        for n in S.INTS:
            assert np.array_equal(g["out"][n], w["out"][n]), (where, t, n, np.argwhere(g["out"][n] != w["out"][n])[:6].tolist())
        assert np.array_equal(g["since"], w["since"]), (where, t, "since", np.argwhere(g["since"] != w["since"])[:6].tolist())
        for n, a, b in [(n, g["out"][n], w["out"][n]) for n in S.FLOATS] + [("state", g["state"], w["state"])]:
            a, b = np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64)
            assert np.array_equal(a, b), (where, t, n, np.argwhere(a != b)[:6].tolist())


@pytest.fixture(scope="module")
def scripted():
    """The scripted sequence (B = 3, K = 8, twelve steps), the statement's walk and the launch's, for symmetry 2 and 4; computed once."""
    steps, marks = S.scripted(np.random.default_rng(43), rows=8, max_gap=GAP)
    runs = {}
    for symmetry in (2, 4):
        par = dict(PAR, symmetry=symmetry)
        runs[symmetry] = dict(par=par, want=S.walk(steps, K.Par(**par)), got=run(steps, BX.BoxFilter(**par)))
    return dict(steps=steps, marks=marks, runs=runs)


# ---- 1. the launch equals the statement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symmetry", [2, 4])
def test_the_launch_equals_the_statement(scripted, symmetry):
    """Births, rows that move up and down between tables (the in-place hazard), a track re-acquired at k = max_gap (continues) and one
    at max_gap + 1 (restarts), a detection with valid = -1 (carried, since + 1), a track that disappears, a reset, an inactive step
    across which the state keeps its bits, quarter-turn readings under both symmetries: `assert_cases` holds the sequence to all of it."""
    steps, marks, r = scripted["steps"], scripted["marks"], scripted["runs"][symmetry]
    S.assert_cases(steps, marks, GAP)
    assert_same(r["got"], r["want"], symmetry)
    b, t = marks["inactive"]
    assert np.array_equal(r["got"][t]["state"][b].view(np.int64), r["got"][t - 1]["state"][b].view(np.int64)) and r["got"][t]["state"][b].any()
    assert np.array_equal(r["got"][t]["since"][b], r["got"][t - 1]["since"][b])
    # stated on its own: no word of any output kept the poison, and the rows at or past count_new hold no filter
    for t, (s, g) in enumerate(zip(steps, r["got"])):
        for n in S.FLOATS + S.INTS:
            assert not (np.ascontiguousarray(g["out"][n]).view(np.int32) == S.POISON).any(), (t, n)
        for b in range(3):
            if s["active"][b]:
                c = int(s["count_new"][b])
                assert c < 8 and not g["state"][b, c:].any() and (g["since"][b, c:] == -1).all() and (g["since"][b, :c] >= 0).any()


# ---- 2. edge shapes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [64, 65, 197])
def test_full_tables_at_the_wave_boundaries(rows):
    """Full tables of 64, 65 and 197 rows (a wave of the id lookup, one row more, the tracker's largest table), five steps."""
    rng = np.random.default_rng(44 + rows)
    steps = S.tables_of(rng, 2, rows, S.random_frames(rng, 2, rows, 5, GAP))
    assert all(int(s["count_new"][b]) == rows for s in steps[:2] for b in range(2))
    par = dict(PAR, symmetry=4)
    want = S.walk(steps, K.Par(**par))
    assert sum(int((w["out"]["gap"] > 0).sum()) for w in want) > rows and sum(int((w["since"] > 0).sum()) for w in want) > rows // 4
    assert_same(run(steps, BX.BoxFilter(**par)), want, rows)


def test_counts_outside_the_table_are_clamped():
    """count_prev, count_new and num_objects below 0 and above K: the launch treats them as the statement's clamp does."""
    rng = np.random.default_rng(45)
    steps = S.tables_of(rng, 3, 8, S.random_frames(rng, 3, 8, 3, GAP))
    for s in steps[1:]:
        s["count_new"], s["num_objects"], s["count_prev"] = s["count_new"].copy(), s["num_objects"].copy(), s["count_prev"].copy()
        s["count_new"][0], s["num_objects"][1], s["count_prev"][2] = 2 ** 30, -5, 2 ** 31 - 1
    steps[2]["num_objects"][0], steps[2]["count_new"][1] = 2 ** 31 - 1, -1
    assert_same(run(steps, BX.BoxFilter(**PAR)), S.walk(steps, K.Par(**PAR)), "clamped")


# ---- 3. the launch equals the offline launch -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symmetry", [2, 4])
def test_the_launch_equals_the_offline_launch(scripted, symmetry):
    steps, r = scripted["steps"], scripted["runs"][symmetry]
    streams, where = S.as_log(steps)
    host = K.ids_log(streams)
    box, valid = S.record_boxes(steps, where, host.R)
    fb = TBG.upload(host).filter_boxes(FG.device_boxes(box, valid), filter=BX.BoxFilter(smooth=0, size_rule=0, **dict(r["par"])))
    offline = {n: getattr(fb, n).cpu().numpy() for n in ("box", "vel", "state", "aligned", "valid", "link")}
    assert fb.flags.tolist() == [0, 0, 0]
    members, continuing = S.compare_with_offline(steps, r["got"], offline, where)
    assert members > 60 and continuing > 40


# ---- 4. determinism and capture ---------------------------------------------------------------------------------------------------------
def test_two_runs_agree_and_a_captured_launch_replays(scripted):
    steps, r = scripted["steps"], scripted["runs"][4]
    flt = BX.BoxFilter(**r["par"])
    assert_same(run(steps, flt), r["got"], "again")
    B, rows = steps[0]["ids_new"].shape
    static = {n: torch.zeros_like(_dev(steps[0][n])) for n in TABLES}
    state, since = device_state(B, rows)
    into = poisoned(B, rows)
    torch.cuda.synchronize()
    graph, out = capture_graph(lambda: BX.filter_step_raw(static["ids_prev"], static["count_prev"], static["ids_new"], static["count_new"],
                                                          static["num_objects"], static["box"], static["valid"], state, since, filter=flt,
                                                          active=static["active"], reset=static["reset"], into=into))
    assert out is into and int(into.gap[0, 0]) == S.POISON and int(since[0, 0]) == -1      # the capture recorded the launch and executed nothing
    res = []
    for s in steps:
        for n in TABLES:
            static[n].copy_(_dev(s[n]))
        for n in S.FLOATS + S.INTS:
            getattr(into, n).view(torch.int32).fill_(S.POISON)
        graph.replay()
        torch.cuda.synchronize()
        res.append(host_of(into, state, since))
    assert_same(res, r["got"], "replay")


# ---- 5. the tracker -----------------------------------------------------------------------------------------------------------------------
FILTER = dict(max_gap=3)
FIELDS = ("filtered_boxes", "filtered_valid", "filtered_velocity", "filtered_aligned", "filtered_gap", "filtered_since", "filtered_state")
RESET, INACTIVE = (1, 3), (2, 4)          # (stream, step)


def tracked_net():
    """The small net of the tracker tests with the Affinity of the track-memory tests, sigmoid(4 - 4 |delta centre|_1), and every point
    called moving: which object follows which is decided by where the clip puts it."""
    sd = {k: v.clone() for k, v in TG.new_net().state_dict().items()}
    sd.update({"affinity." + k: v.to(DEV) for k, v in M.distance_affinity(4.0, 4.0).state_dict().items()})
    sd["fd_layer.cp.linear.bias"] = sd["fd_layer.cp.linear.bias"] + 4.0
    return sd


def masks(t, B=3):
    reset = torch.tensor([b == RESET[0] and t == RESET[1] for b in range(B)], dtype=torch.uint8, device=DEV)
    active = torch.tensor([not (b == INACTIVE[0] and t == INACTIVE[1]) for b in range(B)], dtype=torch.uint8, device=DEV)
    return reset, active


@pytest.fixture(scope="module")
def clip():
    frames, _ = M.random_sequence(B=3, frames=TM.FRAMES, N=TM.N, objects=(6, 7, 8), points=5, seed=7, min_visible=5)
    return dict(frames=TM.net_inputs(dict(frames=frames)), sd=tracked_net())


def filtered(out):
    return {n: getattr(out, n).clone() for n in FIELDS}


def test_the_tracker_eager_and_captured(clip, monkeypatch):
    """max_age = 2, boxes: the option changes nothing the tracker reports and adds one launch behind rtk_object_boxes; eager and captured agree; the measured rows are
    ResultLog.filter_boxes' over the logged clip; a carried row's box is the statement's prediction."""
    B, rows, sd = 3, TM.K, clip["sd"]
    kw = dict(streams=B, max_objects=rows, max_age=2, boxes=True, box_min_extent=0.5)
    flt = BX.BoxFilter(**FILTER)
    plain = T.BatchedTracker(TG.new_net(sd), **kw)
    eager = T.BatchedTracker(TG.new_net(sd), box_filter=flt, **kw)
    graph = T.BatchedTracker(TG.new_net(sd), box_filter=flt, graph=True, graph_warmup=1, **kw)
    assert plain.box_state is None and plain.box_since is None and tuple(eager.box_state.shape) == (B, rows, 16) and eager.box_state.dtype == torch.float64
    log = RL.ResultLog(B, rows, TM.FRAMES, TM.FRAMES * rows, TM.FRAMES * TM.N, device=DEV)
    index, steps, got, where = [0] * B, [], [], [[] for _ in range(B)]
    ids_prev, count_prev = np.full((B, rows), -1, np.int32), np.zeros(B, np.int32)
    reacquired = 0
    calls, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    with torch.no_grad():
        for t, (pc1, pc2, f1, f2, nv) in enumerate(clip["frames"]):
            reset, active = masks(t)
            outs, issued = [], []
            for trk in (plain, eager, graph):
                del calls[:]
                outs.append(trk.step(pc1, pc2, f1, f2, n_valid=nv, reset=reset, active=active))
                issued.append(list(calls))
            assert all(getattr(outs[0], n) is None for n in FIELDS)
            at = issued[0].index("rtk_object_boxes") + 1
            assert "rtk_track_box_filter_step" not in issued[0] and issued[1] == issued[0][:at] + ["rtk_track_box_filter_step"] + issued[0][at:]
            want = TG.snapshot(outs[0], plain)
            for out, trk in zip(outs[1:], (eager, graph)):
                TG.assert_same(TG.snapshot(out, trk), want, t)
                for n in TM.MEMORY_FIELDS + ("table_ids", "table_count", "object_boxes", "object_box_valid", "object_box_cand", "object_box_flags"):
                    assert torch.equal(getattr(out, n).view(torch.int32), getattr(outs[0], n).view(torch.int32)), (t, n)
                assert out.filtered_state is trk.box_state and out.filtered_since is trk.box_since
            a, b = filtered(outs[1]), filtered(outs[2])
            for n in FIELDS:
                assert torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)), (t, n)
            assert graph.captured == (t >= 1)
            out = outs[1]
            out.check()
            first = [index[s] == 0 for s in range(B)]
            log.append(out, seq=list(range(B)), index=list(index), reset=[bool(reset[s]) or first[s] for s in range(B)])
            act = active.cpu().numpy()
            for s in range(B):
                if act[s]:
                    index[s] += 1
                    where[s] += [(t, r) for r in range(int(out.num_objects[s]))]
            steps.append(dict(ids_prev=ids_prev, count_prev=count_prev, ids_new=out.table_ids.cpu().numpy().copy(), count_new=out.table_count.cpu().numpy().copy(),
                              num_objects=out.num_objects.cpu().numpy(), box=out.object_boxes.cpu().numpy(), valid=out.object_box_valid.cpu().numpy(),
                              active=act, reset=reset.cpu().numpy()))
            ids_prev, count_prev = steps[-1]["ids_new"], steps[-1]["count_new"]
            got.append(dict(out=dict(box=a["filtered_boxes"].cpu().numpy(), vel=a["filtered_velocity"].cpu().numpy(), aligned=a["filtered_aligned"].cpu().numpy(),
                                     valid=a["filtered_valid"].cpu().numpy(), gap=a["filtered_gap"].cpu().numpy()),
                            state=a["filtered_state"].cpu().numpy(), since=a["filtered_since"].cpu().numpy()))
            reacquired += int((out.object_gap > 0).sum())
    log.check()
    # the offline launch over the logged clip
    fb = log.filter_boxes(log.boxes(min_extent=0.5), filter=flt)
    offline = {n: getattr(fb, n).cpu().numpy() for n in ("box", "vel", "state", "aligned", "valid", "link")}
    assert fb.flags.tolist() == [0] * B
    members, continuing = S.compare_with_offline(steps, got, offline, where)
    bridged = sum(int((g["out"]["gap"] > 1).sum()) for g in got)
    print("   tracked: members", members, "continuing", continuing, "re-acquired", reacquired, "bridged by the filter", bridged)
    assert reacquired >= 1 and continuing >= 10 and bridged >= 1, (members, continuing, reacquired, bridged)
    # the host statement on the tracker's own tables: every row of every field, the carried rows' predicted boxes among them
    want = S.walk(steps, K.Par(**FILTER))
    assert_same(got, want, "tracker")
    carried = sum(int(((w["since"] > 0) & (w["out"]["box"][..., 3] > 0)).sum()) for w in want)
    assert carried >= 1, carried


# ---- 6. the pipeline ------------------------------------------------------------------------------------------------------------------------
def test_the_pipeline_forwards_the_option(clip):
    G, B, rows, sd = 2, 3, TM.K, clip["sd"]
    kw = dict(max_objects=rows, max_age=2, boxes=True, box_min_extent=0.5, box_filter=BX.BoxFilter(**FILTER))
    single = T.BatchedTracker(TG.new_net(sd), streams=B, **kw)
    pipe = T.TrackerPipeline(TG.new_net(sd), groups=G, streams=B, graph_warmup=1, **kw)
    assert all(trk.box_filter is kw["box_filter"] for trk in pipe.trackers)
    with torch.no_grad():
        for t, (pc1, pc2, f1, f2, nv) in enumerate(clip["frames"][:5]):
            reset, active = masks(t)
            want = filtered(single.step(pc1, pc2, f1, f2, n_valid=nv, reset=reset, active=active))
            outs = [pipe.submit(g, pc1, pc2, f1, f2, n_valid=nv, reset=reset, active=active) for g in range(G)]      # both in flight
            got = []
            for g in range(G):
                with torch.cuda.stream(pipe.streams[g]):
                    got.append(filtered(outs[g]))
            pipe.drain()
            torch.cuda.synchronize()
            for g in range(G):
                for n in FIELDS:
                    assert torch.equal(got[g][n].view(torch.int32), want[n].view(torch.int32)), (t, g, n)
    assert all(trk.captured for trk in pipe.trackers) and int((want["filtered_since"] >= 0).sum()) > 0
