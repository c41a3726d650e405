"""A host statement of the track box filter (include/rtk_fused.h, "Filtered boxes"): plain Python floats (float64), one operation per
expression step, in the order the header names, over the tables of a `_result_log_util.HostLog`.  The kernel of
csrc/track_box_filter.hip is compared with it bit for bit.  `dense_track` restates the same filter the textbook way -- 10 x 10 F, H, Q,
R, the Joseph-form update, dense Rauch-Tung-Striebel -- from the filter equations, for the CPU test that holds the decomposition to it."""
import math

import numpy as np

import _result_log_util as U

PI = math.pi
MAX_GAP = 64
TRACKS = U.TRACKS
FLAG_DUPLICATE, FLAG_TRACKS = 4, 8
POISON = 0x5a5a5a5a
INT_MIN = -2 ** 31


class Par:
    """rtk_box_filter_t with its defaults."""

    def __init__(self, r_pos=1.0, r_yaw=1.0, r_size=1.0, q_pos=1.0, q_vel=0.01, q_yaw=1.0, q_size=1.0, p0=10.0, p0_vel=10000.0, symmetry=4,
                 max_gap=2, smooth=0, size_rule=0, size_percent=90):
        self.__dict__.update({k: v for k, v in locals().items() if k != "self"})

    def kwargs(self):
        return dict(self.__dict__)


def floor(x):
    return float(np.floor(x))


# ---- the chain of one segment -------------------------------------------------------------------------------------------------------
class State:
    def __init__(self, z, p):
        self.m, self.v = [float(x) for x in z], [0.0, 0.0, 0.0]
        self.P00, self.P01, self.P11, self.Py, self.Ps = p.p0, 0.0, p.p0_vel, p.p0, p.p0

    def copy(self):
        s = State.__new__(State)
        s.m, s.v = list(self.m), list(self.v)
        s.P00, s.P01, s.P11, s.Py, s.Ps = self.P00, self.P01, self.P11, self.Py, self.Ps
        return s

    def words(self):
        return self.m + self.v + [self.P00, self.P01, self.P11, self.Py, self.Ps, 0.0]


def predict(s, p):
    for c in range(3):
        s.m[c] = s.m[c] + s.v[c]
    a = s.P00 + s.P01
    b = s.P01 + s.P11
    s.P00 = (a + b) + p.q_pos
    s.P01 = b
    s.P11 = s.P11 + p.q_vel
    s.Py = s.Py + p.q_yaw
    s.Ps = s.Ps + p.q_size


def align(s, z, p):
    """z = [x, y, z, yaw, l, w, h] -> the aligned copy."""
    z = list(z)
    H = (2.0 * PI) / float(p.symmetry)
    d = z[3] - s.m[3]
    t = floor(d / H + 0.5)
    z[3] = s.m[3] + (d - t * H)
    if p.symmetry == 4 and t - 2.0 * floor(t / 2.0) == 1.0:
        z[4], z[5] = z[5], z[4]
    return z


def update(s, z, p):
    S = s.P00 + p.r_pos
    K0 = s.P00 / S
    K1 = s.P01 / S
    for c in range(3):
        y = z[c] - s.m[c]
        s.m[c] = s.m[c] + K0 * y
        s.v[c] = s.v[c] + K1 * y
    s.P11 = s.P11 - K1 * s.P01
    s.P01 = (1.0 - K0) * s.P01
    s.P00 = (1.0 - K0) * s.P00
    Ky = s.Py / (s.Py + p.r_yaw)
    s.m[3] = s.m[3] + Ky * (z[3] - s.m[3])
    s.Py = (1.0 - Ky) * s.Py
    Ks = s.Ps / (s.Ps + p.r_size)
    for c in range(4, 7):
        s.m[c] = s.m[c] + Ks * (z[c] - s.m[c])
    s.Ps = (1.0 - Ks) * s.Ps


def smooth(s, k, nm, nv, p):
    """s: a member's filtered state (changed in place into its smoothed mean); nm, nv: its successor's smoothed mean, k frames on."""
    q = s.copy()
    for _ in range(k):
        predict(q, p)
    kk = float(k)
    C00 = s.P00 + kk * s.P01
    C01 = s.P01
    C10 = s.P01 + kk * s.P11
    C11 = s.P11
    det = q.P00 * q.P11 - q.P01 * q.P01
    G00 = (C00 * q.P11 - C01 * q.P01) / det
    G01 = (C01 * q.P00 - C00 * q.P01) / det
    G10 = (C10 * q.P11 - C11 * q.P01) / det
    G11 = (C11 * q.P00 - C10 * q.P01) / det
    for c in range(3):
        e0 = nm[c] - q.m[c]
        e1 = nv[c] - q.v[c]
        s.m[c] = s.m[c] + (G00 * e0 + G01 * e1)
        s.v[c] = s.v[c] + (G10 * e0 + G11 * e1)
    Gy = s.Py / q.Py
    Gs = s.Ps / q.Ps
    s.m[3] = s.m[3] + Gy * (nm[3] - s.m[3])
    for c in range(4, 7):
        s.m[c] = s.m[c] + Gs * (nm[c] - s.m[c])


def output(m, v):
    """A final mean -> (box (8), vel (4))."""
    l, w, yaw = m[4], m[5], m[3]
    if w > l:
        l, w = w, l
        yaw = yaw + PI / 2.0
    yaw = yaw - floor((yaw + PI / 2.0) / PI) * PI
    if yaw >= PI / 2.0:
        yaw = yaw - PI
    elif yaw < -(PI / 2.0):
        yaw = yaw + PI
    return [m[0], m[1], m[2], l, w, m[6], yaw, l * w], [v[0], v[1], v[2], m[3]]


def measurement(box):
    return [float(box[0]), float(box[1]), float(box[2]), float(box[6]), float(box[3]), float(box[4]), float(box[5])]


def extent_rank(n, percent):
    return (percent * (n - 1)) // 100


def run_segment(zs, gaps, ids, p):
    """zs: the members' measurements; gaps[i]: frames from member i - 1 to member i (gaps[0] unused); ids: their record indices (the
    extent's tie-break).  -> per member dict(box, vel, state, aligned)."""
    s = State(zs[0], p)
    filtered, aligned = [s.copy()], [[zs[0][3], zs[0][4], zs[0][5], zs[0][6]]]
    for i in range(1, len(zs)):
        for _ in range(gaps[i]):
            predict(s, p)
        z = align(s, zs[i], p)
        update(s, z, p)
        filtered.append(s.copy())
        aligned.append([z[3], z[4], z[5], z[6]])
    final = [f.copy() for f in filtered]
    if p.smooth:
        for i in range(len(zs) - 2, -1, -1):
            smooth(final[i], gaps[i + 1], final[i + 1].m, final[i + 1].v, p)
    ext = None
    if p.size_rule:
        q = extent_rank(len(zs), p.size_percent)
        ext = [sorted((aligned[i][c], ids[i]) for i in range(len(zs)))[q][0] for c in (1, 2, 3)]
    out = []
    for i in range(len(zs)):
        m = list(final[i].m)
        if ext is not None:
            m[4:7] = ext
        box, vel = output(m, final[i].v)
        out.append(dict(box=box, vel=vel, state=filtered[i].words(), aligned=aligned[i]))
    return out


# ---- the log ------------------------------------------------------------------------------------------------------------------------
def segments_of(tables, valid, keep, b, p):
    """-> (segments [[(record, gap), ...], ...] of the clips that are filtered, dead records [r, ...], flags) of stream b."""
    frames, records = int(tables["cursor"][b, 0]), int(tables["cursor"][b, 1])
    words = [(int(w[0]), int(w[2]) & 0xffff, (int(w[2]) >> 16) & 1) for w in tables["frame"][b, :frames]]
    segs, dead, flags = [], [], 0
    for clip in U.clips(words):
        recs = [[r for r in range(words[f][0], words[f][0] + words[f][1]) if r < records] for f in clip]
        if len({int(tables["rec_track"][b, r]) for fr in recs for r in fr}) > TRACKS:
            flags |= FLAG_TRACKS
        if flags & FLAG_TRACKS:
            dead += [r for fr in recs for r in fr]
            continue
        last, open_seg = {}, {}
        for f, fr in zip(clip, recs):
            n = int(tables["tag"][b, f, 1])
            seen = set()
            for r in fr:                                   # increasing index: the first eligible record of an id is its member
                tid = int(tables["rec_track"][b, r])
                if not (valid[b, r] > 0 and (keep is None or keep[b, r]) and tid != INT_MIN):
                    continue
                if tid in seen:
                    flags |= FLAG_DUPLICATE
                    continue
                seen.add(tid)
                k = n - last[tid][1] if tid in last else None
                if k is None or k < 1 or k > p.max_gap:
                    open_seg[tid] = [(r, -1)]
                    segs.append(open_seg[tid])
                else:
                    open_seg[tid].append((r, k))
                last[tid] = (r, n)
    return segs, dead, flags


def filter_log(tables, box, valid, keep=None, par=None, poison=False):
    """rtk_result_log_filter_boxes on the tables of a host log with its per-record boxes (box (B,R,8), valid (B,R)): -> dict of box
    (B,R,8), vel (B,R,4), state (B,R,16), aligned (B,R,4) float64, valid (B,R), link (B,R,4), flags (B) int32.  Words at or beyond a
    stream's records cursor hold 0, or the poison."""
    p = par or Par()
    B, R = tables["rec_track"].shape
    fill = POISON if poison else 0
    f64 = lambda w: np.full((B, R, 2 * w), fill, np.int32).view(np.float64).reshape(B, R, w)
    out = dict(box=f64(8), vel=f64(4), state=f64(16), aligned=f64(4), valid=np.full((B, R), fill, np.int32),
               link=np.full((B, R, 4), fill, np.int32), flags=np.zeros(B, np.int32))
    for b in range(B):
        records = int(tables["cursor"][b, 1])
        for name in ("box", "vel", "state", "aligned", "valid"):
            out[name][b, :records] = 0
        out["link"][b, :records] = -1
        segs, _, out["flags"][b] = segments_of(tables, valid, keep, b, p)
        for seg in segs:
            ids = [r for r, _ in seg]
            rows = run_segment([measurement(box[b, r]) for r in ids], [k for _, k in seg], ids, p)
            for i, (r, k) in enumerate(seg):
                for name in ("box", "vel", "state", "aligned"):
                    out[name][b, r] = rows[i][name]
                out["valid"][b, r] = valid[b, r]
                out["link"][b, r] = (ids[i - 1] if i else -1, k, ids[i + 1] if i + 1 < len(ids) else -1, ids[0])
    return out


def track_tables(boxes, frames=None, tid=7):
    """One track of per-frame boxes ((n,8) rows) -> (tables, box (1,R,8), valid (1,R)): a one-stream log with one record per frame
    at frame numbers `frames` (default 0, 1, 2, ...)."""
    n = len(boxes)
    frames = list(range(n)) if frames is None else list(frames)
    log = U.HostLog(1, 1, n, n, n)
    for i in range(n):
        log.append(np.zeros((1, 3, 1), np.float32), np.zeros((1, 1), np.int32), [1], np.array([[tid]], np.int32), np.ones((1, 1), np.float32),
                   [0], [frames[i]], reset=[i == 0])
    return log.tables(), np.asarray(boxes, np.float64).reshape(1, n, 8).copy(), np.ones((1, n), np.int32)


def ids_dims(streams, slack=3):
    """(K, F, R) of the smallest log that holds `streams` with `slack` record slots behind the fullest stream's cursor."""
    return (max([len(ids) for s in streams for _, _, ids in s] + [1]), max(len(s) for s in streams) + 1,
            max(sum(len(ids) for _, _, ids in s) for s in streams) + slack)


def ids_log(streams, poison=False, dims=None):
    """streams[b] = [(frame number, begins a clip, [track id, ...]), ...] -> a HostLog of dims (K, F, R) (default: ids_dims) with these
    frames, every record an object of one point."""
    B = len(streams)
    K, F, R = dims or ids_dims(streams)
    log = U.HostLog(B, K, F, R, R, poison=poison)
    F = max(len(s) for s in streams)
    cols = np.arange(K, dtype=np.int32)
    for t in range(F):
        live = [t < len(s) for s in streams]
        frames = [s[t] if t < len(s) else (0, False, []) for s in streams]
        ids = np.zeros((B, K), np.int32)
        for b, (_, _, row) in enumerate(frames):
            ids[b, :len(row)] = row
        log.append(np.zeros((B, 3, K), np.float32), np.tile(cols, (B, 1)), [len(f[2]) for f in frames], ids, np.full((B, K), 0.5, np.float32),
                   [b for b in range(B)], [f[0] for f in frames], reset=[f[1] for f in frames], active=live)
    return log


def random_boxes(rng, B, R):
    """(B,R,8) rows of the ObjectBoxes layout: l >= w, yaw in [-pi/2, pi/2), area = l w."""
    xy, z = rng.uniform(-60.0, 60.0, size=(B, R, 2)), rng.uniform(-2.0, 2.0, size=(B, R, 1))
    a, c = rng.uniform(0.5, 5.0, size=(B, R, 1)), rng.uniform(0.5, 5.0, size=(B, R, 1))
    l, w = np.maximum(a, c), np.minimum(a, c)
    h, yaw = rng.uniform(0.5, 3.0, size=(B, R, 1)), rng.uniform(-PI / 2.0, PI / 2.0, size=(B, R, 1))
    return np.concatenate([xy, z, l, w, h, yaw, l * w], axis=2)


# ---- the dense restatement ----------------------------------------------------------------------------------------------------------
def dense_track(zs, p, smooth_pass):
    """The ten-state constant-velocity filter over (x, y, z, yaw, l, w, h, vx, vy, vz) in matrices, one frame between measurements, no
    orientation correction: predict x = F x, P = F P F' + Q; update with K = P H' (H P H' + R)^-1 and the Joseph form
    P = (I - K H) P (I - K H)' + K R K'; then the dense Rauch-Tung-Striebel recursion.  -> (n,10) means."""
    Fm = np.eye(10)
    Fm[0, 7] = Fm[1, 8] = Fm[2, 9] = 1.0
    Hm = np.hstack([np.eye(7), np.zeros((7, 3))])
    Q = np.diag([p.q_pos] * 3 + [p.q_yaw] + [p.q_size] * 3 + [p.q_vel] * 3)
    Rm = np.diag([p.r_pos] * 3 + [p.r_yaw] + [p.r_size] * 3)
    x = np.concatenate([np.asarray(zs[0], np.float64), np.zeros(3)])
    P = np.diag([p.p0] * 7 + [p.p0_vel] * 3)
    xs, Ps, xp, Pp = [x], [P], [None], [None]
    I = np.eye(10)
    for z in zs[1:]:
        x, P = Fm @ x, Fm @ P @ Fm.T + Q
        xp.append(x)
        Pp.append(P)
        K = P @ Hm.T @ np.linalg.inv(Hm @ P @ Hm.T + Rm)
        x = x + K @ (np.asarray(z, np.float64) - Hm @ x)
        P = (I - K @ Hm) @ P @ (I - K @ Hm).T + K @ Rm @ K.T
        xs.append(x)
        Ps.append(P)
    if smooth_pass:
        for i in range(len(zs) - 2, -1, -1):
            G = Ps[i] @ Fm.T @ np.linalg.inv(Pp[i + 1])
            xs[i] = xs[i] + G @ (xs[i + 1] - xp[i + 1])
    return np.array(xs)


# ---- the synthetic track of the quality test ----------------------------------------------------------------------------------------
def arc_track(seed, frames=40, size=(4.0, 1.8, 1.5), points=(3, 8), drop=0.2):
    """A box driven along an arc, a few uniform interior points per frame, a fifth of the frames dropped.
    -> [(frame number, points (n,3) fp32, true box (x, y, z, l, w, h, yaw))]."""
    rng = np.random.default_rng(seed)
    l, w, h = size
    radius, speed = rng.uniform(25.0, 60.0), rng.uniform(0.6, 1.4)
    a0, cx, cy = rng.uniform(0.0, 2.0 * PI), rng.uniform(-20.0, 20.0), rng.uniform(-20.0, 20.0)
    out = []
    for t in range(frames):
        a = a0 + speed * t / radius
        x, y, yaw = cx + radius * math.cos(a), cy + radius * math.sin(a), a + PI / 2.0
        n = int(rng.integers(points[0], points[1] + 1))
        u = rng.uniform(-0.5, 0.5, size=(n, 3)) * [l, w, h]
        px = x + u[:, 0] * math.cos(yaw) - u[:, 1] * math.sin(yaw)
        py = y + u[:, 0] * math.sin(yaw) + u[:, 1] * math.cos(yaw)
        keep = t == 0 or rng.uniform() >= drop
        if keep:
            out.append((t, np.column_stack([px, py, 0.75 + u[:, 2]]).astype(np.float32), (x, y, 0.75, l, w, h, yaw)))
    return out
