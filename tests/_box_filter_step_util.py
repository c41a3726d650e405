"""A host statement of the filter inside the tracked step (include/rtk_fused.h, "Filtered boxes inside the step"): the step rule over
numpy tables, built from `_box_filter_util`'s State, predict, align, update and output -- the arithmetic is stated there and nowhere
else.  The kernel of csrc/track_box_step.hip is compared with it bit for bit.  Also here: sequences of synthetic tables (a scripted one
that contains every case of the rule, a random one with full tables) and their restatement as a result log, for the comparison with
the offline rule (`_box_filter_util.filter_log`, rtk_result_log_filter_boxes)."""
import numpy as np

import _box_filter_util as K

MAX_GAP = K.MAX_GAP
POISON = K.POISON
FLOATS, INTS = ("box", "vel", "aligned"), ("valid", "gap")
WIDTH = dict(box=8, vel=4, aligned=4)


def clamp(v, hi):
    return min(max(int(v), 0), hi)


def empty_state(B, rows):
    """The filter's state before the first step: (state (B,rows,16) float64 zeros, since (B,rows) int32 -1)."""
    return np.zeros((B, rows, 16), np.float64), np.full((B, rows), -1, np.int32)


def load(words, p):
    s = K.State.__new__(K.State)
    w = [float(x) for x in words]
    s.m, s.v = w[:7], w[7:10]
    s.P00, s.P01, s.P11, s.Py, s.Ps = w[10:15]
    return s


def host_step(state, since, ids_prev, count_prev, ids_new, count_new, num_objects, box, valid, par, active=None, reset=None):
    """rtk_track_box_filter_step.  state (B,rows,16) / since (B,rows) are NOT changed: -> (new state, new since, dict(box (B,rows,8),
    vel, aligned (B,rows,4) float64, valid, gap (B,rows) int32))."""
    B, rows = ids_new.shape
    new_state, new_since = state.copy(), since.copy()
    out = dict(box=np.zeros((B, rows, 8)), vel=np.zeros((B, rows, 4)), aligned=np.zeros((B, rows, 4)), valid=np.zeros((B, rows), np.int32),
               gap=np.full((B, rows), -1, np.int32))
    for b in range(B):
        if active is not None and not active[b]:
            continue                                         # no frame passed: state and since keep every bit, the outputs are empty
        m = 0 if (reset is not None and reset[b]) else clamp(count_prev[b], rows)
        c, n = clamp(count_new[b], rows), clamp(num_objects[b], rows)
        new_state[b], new_since[b] = 0.0, -1
        for r in range(c):
            tid = int(ids_new[b, r])
            prev = next((i for i in range(m) if tid >= 0 and int(ids_prev[b, i]) == tid), None)
            since_prev = min(int(since[b, prev]), MAX_GAP) if prev is not None else -1
            if r < n and valid[b, r] > 0:
                z = K.measurement(box[b, r])
                k = since_prev + 1
                if since_prev >= 0 and k <= par.max_gap:
                    s = load(state[b, prev], par)
                    for _ in range(k):
                        K.predict(s, par)
                    z = K.align(s, z, par)
                    K.update(s, z, par)
                    out["gap"][b, r] = k
                else:
                    s = K.State(z, par)
                new_state[b, r], new_since[b, r] = s.words(), 0
                out["valid"][b, r] = valid[b, r]
                out["aligned"][b, r] = [z[3], z[4], z[5], z[6]]
            elif since_prev >= 0:
                new_state[b, r], new_since[b, r] = state[b, prev], min(since_prev + 1, MAX_GAP)
            else:
                continue
            s = load(new_state[b, r], par)
            for _ in range(int(new_since[b, r])):
                for q in range(3):
                    s.m[q] = s.m[q] + s.v[q]
            out["box"][b, r], out["vel"][b, r] = K.output(s.m, s.v)
    return new_state, new_since, out


# ---- sequences of tables ------------------------------------------------------------------------------------------------------------
def tables_of(rng, B, rows, frames, garbage=True):
    """frames[t][b] = dict(det=[(id, valid), ...], coast=[id, ...], active=bool, reset=bool) -> the steps of a sequence: per step a
    dict(ids_prev, count_prev, ids_new, count_new, num_objects, box, valid, active, reset) of numpy arrays.  An inactive stream's table
    is carried over, as the tracker's kernels carry it.  garbage: the rows at or past a count hold ids of live tracks and boxes with
    valid > 0, and rows past num_objects a valid > 0 too: the counts alone decide."""
    ids_prev, count_prev = np.full((B, rows), -1, np.int32), np.zeros(B, np.int32)
    steps = []
    for row in frames:
        ids_new, count_new, num = ids_prev.copy(), count_prev.copy(), np.zeros(B, np.int32)
        box = K.random_boxes(rng, B, rows)
        valid = rng.integers(1, 9, size=(B, rows)).astype(np.int32) if garbage else np.zeros((B, rows), np.int32)
        active, reset = np.array([f["active"] for f in row], np.uint8), np.array([f["reset"] for f in row], np.uint8)
        for b, f in enumerate(row):
            if not f["active"]:
                continue
            table = [i for i, _ in f["det"]] + list(f["coast"])
            assert len(table) <= rows and len(set(table)) == len(table), (b, table)
            fill = table[0] if (garbage and table) else -1
            ids_new[b] = fill
            ids_new[b, :len(table)] = table
            count_new[b], num[b] = len(table), len(f["det"])
            for r, (_, v) in enumerate(f["det"]):
                valid[b, r] = v if v <= 0 else max(int(valid[b, r]), 1)
                if "box" in f and f["det"][r][0] in f["box"]:
                    box[b, r] = f["box"][f["det"][r][0]]
        steps.append(dict(ids_prev=ids_prev, count_prev=count_prev, ids_new=ids_new, count_new=count_new, num_objects=num, box=box, valid=valid,
                          active=active, reset=reset))
        ids_prev, count_prev = ids_new, count_new
    return steps


def turned(t, at):
    """The crafted reading of frame t: one rectangle (l 4, w 2) whose fitted yaw is 0.3 in even frames and a quarter turn back in odd ones."""
    yaw = 0.3 if t % 2 == 0 else 0.3 - K.PI / 2.0
    return [at + 0.5 * t, -at, 0.25, 4.0, 2.0, 1.5, yaw, 8.0]


def scripted(rng, rows=8, max_gap=2):
    """B = 3, twelve steps, every case of the rule (the docstrings of the tests that use it name them).  Detections are listed in
    increasing id order in even steps and decreasing order in odd ones, so rows move up and down between tables.
    -> (steps, dict of the (stream, step, id) triples the tests look up)."""
    g = max_gap
    T = 12
    frames = []
    for t in range(T):
        # stream 0: 1 always; 2 coasts one frame short of the limit (re-acquired at k = g); 3 coasts g frames (re-acquired at k = g + 1);
        # 4 has a box that is not valid at t = 3; 5 is born at 1 and disappears at 5; 6 is born at 5; 50 is the quarter-turn track
        det0 = [(1, 1), (50, 1)]
        coast0 = []
        if t <= 1 or t >= 1 + g:
            det0.append((2, 1))
        else:
            coast0.append(2)                                  # t = 2 ... g: g - 1 frames
        if t <= 1 or t >= 2 + g:
            det0.append((3, 1))
        else:
            coast0.append(3)                                  # t = 2 ... g + 1: g frames
        det0.append((4, -1 if t == 3 else 1))
        if 1 <= t <= 4:
            det0.append((5, 1))
        if t >= 5:
            det0.append((6, 1))
        # stream 1: 11, 12, 13 always, reset at t = 6; 14 is born at 3
        det1 = [(11, 1), (12, 1), (13, 1)] + ([(14, 1)] if t >= 3 else [])
        # stream 2: inactive at t = 4; 21 and 22 always; 23 coasts at t = 3 and 5, across the inactive step, and returns at t = 6
        det2 = [(21, 1), (22, 1)] + ([(23, 1)] if t not in (3, 4, 5) else [])
        coast2 = [23] if t in (3, 5) else []
        order = (lambda d: sorted(d)) if t % 2 == 0 else (lambda d: sorted(d, reverse=True))
        frames.append([dict(det=order(det0), coast=coast0, active=True, reset=False, box={50: turned(t, 7.0)}),
                       dict(det=order(det1), coast=[], active=True, reset=t == 6),
                       dict(det=order(det2), coast=coast2, active=t != 4, reset=False)])
    marks = dict(continues=(0, 1 + g, 2), restarts=(0, 2 + g, 3), invalid=(0, 3, 4), gone=(0, 5, 5), born=(0, 5, 6), reset=(1, 6), inactive=(2, 4),
                 turned=(0, 50))
    return tables_of(rng, 3, rows, frames), marks


def random_frames(rng, B, rows, steps, max_gap, detect=0.7):
    """Full tables: every stream keeps `rows` tracks alive -- a track is detected with probability `detect`, else coasts for up to
    max_gap + 1 frames and is then dropped; births fill the table; a detection's box is not valid now and then; the detections are in
    a random order.  One stream is reset and one inactive midway."""
    frames, nxt = [], 1000
    live = [dict() for _ in range(B)]                         # id -> frames coasted
    for t in range(steps):
        row = []
        for b in range(B):
            active, reset = not (b == B - 1 and t == steps // 2), (b == 0 and t == steps // 2)
            if not active:
                row.append(dict(det=[], coast=[], active=False, reset=False))
                continue
            if reset:
                live[b] = dict()
            det, coast = [], []
            for tid, age in list(live[b].items()):
                if rng.uniform() < detect:
                    det.append(tid)
                    live[b][tid] = 0
                elif age < max_gap + 1:
                    coast.append(tid)
                    live[b][tid] = age + 1
                else:
                    del live[b][tid]
            while len(det) + len(coast) < rows:
                det.append(nxt)
                live[b][nxt] = 0
                nxt += 1
            det = [det[i] for i in rng.permutation(len(det))]
            row.append(dict(det=[(tid, -1 if rng.uniform() < 0.05 else 1) for tid in det], coast=[coast[i] for i in rng.permutation(len(coast))],
                            active=True, reset=reset))
        frames.append(row)
    return frames


def walk(steps, par):
    """The host statement over a sequence: -> per step dict(out=host_step's outputs, state, since (after the step))."""
    B, rows = steps[0]["ids_new"].shape
    state, since = empty_state(B, rows)
    res = []
    for s in steps:
        state, since, out = host_step(state, since, s["ids_prev"], s["count_prev"], s["ids_new"], s["count_new"], s["num_objects"], s["box"], s["valid"],
                                      par, active=s["active"], reset=s["reset"])
        res.append(dict(out=out, state=state, since=since))
    return res


# ---- the same sequence as a result log -------------------------------------------------------------------------------------------------
def as_log(steps):
    """The detections of a sequence as the records a result log would hold: frame index = the stream's active-step count, a reset (and
    the first frame) begins a clip.  -> (streams for `_box_filter_util.ids_log`, where[b] = [(step, row), ...] per record of stream b)."""
    B = steps[0]["ids_new"].shape[0]
    streams, where = [[] for _ in range(B)], [[] for _ in range(B)]
    for t, s in enumerate(steps):
        for b in range(B):
            if not s["active"][b]:
                continue
            n = int(s["num_objects"][b])
            streams[b].append((len(streams[b]), bool(s["reset"][b]) or not streams[b], [int(i) for i in s["ids_new"][b, :n]]))
            where[b] += [(t, r) for r in range(n)]
    return streams, where


def record_boxes(steps, where, R):
    """The boxes of the records: (box (B,R,8), valid (B,R)) with the rows of `where`."""
    B = len(where)
    box, valid = np.zeros((B, R, 8)), np.zeros((B, R), np.int32)
    for b in range(B):
        for i, (t, r) in enumerate(where[b]):
            box[b, i], valid[b, i] = steps[t]["box"][b, r], steps[t]["valid"][b, r]
    return box, valid


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.int64), np.ascontiguousarray(b, np.float64).view(np.int64))


def compare_with_offline(steps, res, offline, where):
    """Every measured row of the walk `res` (or of a device run in the same form) against the offline result dict: box, vel, state,
    aligned by their bits, gap against link[..., 1].  -> (members compared, continuing members)."""
    members = continuing = 0
    for b in range(len(where)):
        for i, (t, r) in enumerate(where[b]):
            out = res[t]["out"]
            if out["valid"][b, r] <= 0:
                assert offline["valid"][b, i] == 0, (b, t, r)
                continue
            assert offline["valid"][b, i] == out["valid"][b, r], (b, t, r)
            for name, got in (("box", out["box"][b, r]), ("vel", out["vel"][b, r]), ("aligned", out["aligned"][b, r]), ("state", res[t]["state"][b, r])):
                assert same_bits(got, offline[name][b, i]), (name, b, t, r, got, offline[name][b, i])
            assert int(offline["link"][b, i, 1]) == int(out["gap"][b, r]), (b, t, r)
            members += 1
            continuing += int(out["gap"][b, r] > 0)
    return members, continuing


def assert_cases(steps, marks, g):
    """The cases the scripted sequence is meant to contain are in it (by the host statement): a re-acquisition at k = max_gap that
    continues and one at max_gap + 1 that restarts, a detection whose box is not valid, a track that disappears, a birth, a reset, an
    inactive step across which the state keeps its bits, rows that move up and down between tables, and the quarter-turn readings."""
    res = walk(steps, K.Par(max_gap=g))
    row = lambda b, t, tid: steps[t]["ids_new"][b, :int(steps[t]["count_new"][b])].tolist().index(tid)
    b, t, tid = marks["continues"]
    assert res[t]["out"]["gap"][b, row(b, t, tid)] == g and res[t - 1]["since"][b, row(b, t - 1, tid)] == g - 1
    b, t, tid = marks["restarts"]
    assert res[t]["out"]["gap"][b, row(b, t, tid)] == -1 and res[t]["since"][b, row(b, t, tid)] == 0 and res[t - 1]["since"][b, row(b, t - 1, tid)] == g
    b, t, tid = marks["invalid"]
    assert steps[t]["valid"][b, row(b, t, tid)] == -1 and res[t]["since"][b, row(b, t, tid)] == 1 and res[t + 1]["out"]["gap"][b, row(b, t + 1, tid)] == 2
    b, t, tid = marks["gone"]
    assert tid in steps[t - 1]["ids_new"][b, :int(steps[t - 1]["count_new"][b])] and tid not in steps[t]["ids_new"][b, :int(steps[t]["count_new"][b])]
    b, t, tid = marks["born"]
    assert res[t]["out"]["gap"][b, row(b, t, tid)] == -1 and res[t]["since"][b, row(b, t, tid)] == 0
    b, t = marks["reset"]
    assert steps[t]["reset"][b] and (res[t]["out"]["gap"][b] == -1).all() and (res[t - 1]["out"]["gap"][b, :3] == 1).all()
    b, t = marks["inactive"]
    assert not steps[t]["active"][b] and same_bits(res[t]["state"][b], res[t - 1]["state"][b]) and (res[t - 1]["since"][b] >= 0).sum() == 3
    assert (res[t]["out"]["valid"][b] == 0).all() and not res[t]["out"]["box"][b].any()
    # rows move in both directions between tables
    up = down = 0
    for t in range(1, len(steps)):
        for r in range(int(steps[t]["count_new"][0])):
            prev = steps[t]["ids_prev"][0, :int(steps[t]["count_prev"][0])].tolist()
            tid = int(steps[t]["ids_new"][0, r])
            if tid in prev and res[t - 1]["since"][0, prev.index(tid)] >= 0:
                up, down = up + (prev.index(tid) > r), down + (prev.index(tid) < r)
    assert up > 5 and down > 5
    # the quarter-turn track: under symmetry 4 the reading's l and w are swapped in odd frames, under symmetry 2 never
    b, tid = marks["turned"]
    for symmetry, swapped in ((4, True), (2, False)):
        res = walk(steps, K.Par(max_gap=g, symmetry=symmetry))
        seen = [res[t]["out"]["aligned"][b, row(b, t, tid)][1:3].tolist() for t in range(len(steps))]
        assert ([2.0, 4.0] in seen) == swapped and [4.0, 2.0] in seen, (symmetry, seen)
