"""A host statement of the box fitting rule (include/rtk_fused.h, "Oriented boxes"): plain Python floats (float64), one operation per
expression step, every loop in the order the rule names -- no vectorised reduction whose order is unspecified.  The kernels of
csrc/track_boxes.hip are compared with it bit for bit (yaw within the two atan2s' error), and `fit` also returns the runner-up's area so
that a test can assert its own margin."""
import math

import numpy as np

MAX_POINTS = 128
FLAG_AXIS, FLAG_OBJECTS = 1, 2
PI = math.pi
POISON = 0x5a5a5a5a
INF = float("inf")


def extents(xs, ys, dx, dy):
    """(smin, smax, tmin, tmax) of s = dx x + dy y, t = dx y - dy x in point order; a zero extreme is +0."""
    s0 = t0 = INF
    s1 = t1 = -INF
    for x, y in zip(xs, ys):
        s = dx * x + dy * y
        t = dx * y - dy * x
        s0 = s if s < s0 else s0
        s1 = s if s > s1 else s1
        t0 = t if t < t0 else t0
        t1 = t if t > t1 else t1
    return s0 + 0.0, s1 + 0.0, t0 + 0.0, t1 + 0.0


def candidates(xs, ys, axis_only=False):
    """[(c, dx, dy, q, area, extents)] of every candidate that is not skipped, in increasing c."""
    n = len(xs)
    e = extents(xs, ys, 1.0, 0.0)
    out = [(0, 1.0, 0.0, 1.0, ((e[1] - e[0]) * (e[3] - e[2])) / 1.0, e)]
    if axis_only:
        return out
    c = 0
    for i in range(n):
        for j in range(i + 1, n):
            c += 1
            dx, dy = xs[j] - xs[i], ys[j] - ys[i]
            q = dx * dx + dy * dy
            if q == 0.0:
                continue
            e = extents(xs, ys, dx, dy)
            out.append((c, dx, dy, q, ((e[1] - e[0]) * (e[3] - e[2])) / q, e))
    return out


def candidates_side_by_side(xs, ys):
    """`candidates` for a large object: the same operations in the same order for every candidate, the candidates side by side in
    numpy arrays.  Only elementwise operations are vectorised (each is the IEEE operation on its element); the scan over the points is
    the explicit loop in point order.  tests/test_track_boxes_cpu.py holds it to `candidates` bit for bit."""
    x, y = np.asarray(xs, np.float64), np.asarray(ys, np.float64)
    n = len(x)
    i, j = np.triu_indices(n, 1)                      # the pairs i < j in lexicographic order
    dx, dy = np.concatenate(([1.0], x[j] - x[i])), np.concatenate(([0.0], y[j] - y[i]))
    q = dx * dx + dy * dy
    s0, t0 = np.full(len(q), INF), np.full(len(q), INF)
    s1, t1 = np.full(len(q), -INF), np.full(len(q), -INF)
    for k in range(n):
        s = dx * x[k] + dy * y[k]
        t = dx * y[k] - dy * x[k]
        s0, s1 = np.where(s < s0, s, s0), np.where(s > s1, s, s1)
        t0, t1 = np.where(t < t0, t, t0), np.where(t > t1, t, t1)
    s0, s1, t0, t1 = s0 + 0.0, s1 + 0.0, t0 + 0.0, t1 + 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        area = ((s1 - s0) * (t1 - t0)) / q
    return [(int(c), float(dx[c]), float(dy[c]), float(q[c]), float(area[c]), (float(s0[c]), float(s1[c]), float(t0[c]), float(t1[c])))
            for c in np.nonzero(q != 0.0)[0]]


def fit(points, min_extent=0.0):
    """points (n,3) of fp32 values -> (box (8,) float64, cand, valid, runner_up): runner_up is the smallest area among the candidates
    whose area is not the winner's (inf when there is none): the margin a test asserts."""
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    n = len(pts)
    if n == 0:
        return np.zeros(8), -1, 0, INF
    if not np.isfinite(pts).all():
        return np.zeros(8), -1, -1, INF
    xs, ys, zs = pts[:, 0].tolist(), pts[:, 1].tolist(), pts[:, 2].tolist()
    zlo, zhi = INF, -INF
    for z in zs:
        zlo = z if z < zlo else zlo
        zhi = z if z > zhi else zhi
    zlo, zhi = zlo + 0.0, zhi + 0.0
    cands = candidates_side_by_side(xs, ys) if 24 < n <= MAX_POINTS else candidates(xs, ys, axis_only=n > MAX_POINTS)
    win = cands[0]
    for cd in cands[1:]:
        if cd[4] < win[4]:
            win = cd
    others = [cd[4] for cd in cands if cd[4] != win[4]]
    runner_up = min(others) if others else INF
    c, dx, dy, q, area, (s0, s1, t0, t1) = win
    S, T = s1 - s0, t1 - t0
    r = math.sqrt(q)
    len_s, len_t = S / r, T / r
    ms, mt = (s0 + s1) / 2.0, (t0 + t1) / 2.0
    cx = (ms * dx - mt * dy) / q
    cy = (ms * dy + mt * dx) / q
    yaw = math.atan2(dy, dx)
    if len_t > len_s:
        len_s, len_t = len_t, len_s
        yaw = yaw + PI / 2.0
    while yaw >= PI / 2.0:
        yaw = yaw - PI
    while yaw < -(PI / 2.0):
        yaw = yaw + PI
    h = zhi - zlo
    box = np.array([cx, cy, (zlo + zhi) / 2.0, len_s if len_s > min_extent else min_extent, len_t if len_t > min_extent else min_extent,
                    h if h > min_extent else min_extent, yaw, area], dtype=np.float64)
    return box, c, n, runner_up


def log_boxes(tables, keep=None, min_extent=0.0, poison=False):
    """rtk_result_log_boxes on the tables of a host log (_result_log_util.HostLog.tables()): -> box (B,R,8) float64, cand, valid (B,R)
    int32, flags (B) int32, margins [(b, r, area, runner_up)].  Words at or beyond a stream's records cursor hold 0, or the poison."""
    B, R = tables["rec_track"].shape
    fill = POISON if poison else 0
    box = np.full((B, R, 16), fill, np.int32).view(np.float64).reshape(B, R, 8)
    cand, valid = np.full((B, R), fill, np.int32), np.full((B, R), fill, np.int32)
    flags, margins = np.zeros(B, np.int32), []
    for b in range(B):
        for f in range(int(tables["cursor"][b, 0])):
            rec, at, word, _ = (int(v) for v in tables["frame"][b, f])
            for r in range(rec, rec + (word & 0xffff)):
                n = int(tables["rec_size"][b, r])
                if keep is None or keep[b, r]:
                    bx, c, v, runner = fit(tables["points"][b, at:at + n], min_extent)
                    if n > MAX_POINTS and v > 0:
                        flags[b] |= FLAG_AXIS
                    margins.append((b, r, bx[7], runner))
                else:
                    bx, c, v = np.zeros(8), -1, 0
                box[b, r], cand[b, r], valid[b, r] = bx, c, v
                at += n
    return box, cand, valid, flags, margins


def step_boxes(pc1, obj, num_objects, K, active=None, min_extent=0.0):
    """rtk_object_boxes: pc1 (B,3,N) fp32, obj (B,N), num_objects (B) -> box (B,K,8), cand, valid (B,K), flags (B), margins."""
    B, _, N = pc1.shape
    box, cand, valid = np.zeros((B, K, 8)), np.full((B, K), -1, np.int32), np.zeros((B, K), np.int32)
    flags, margins = np.zeros(B, np.int32), []
    for b in range(B):
        if active is not None and not active[b]:
            continue
        num = int(num_objects[b])
        if num < 0 or num > K:
            flags[b] |= FLAG_OBJECTS
            continue
        for j in range(num):
            cols = [p for p in range(N) if obj[b, p] == j]
            bx, c, v, runner = fit(pc1[b][:, cols].T, min_extent)
            if len(cols) > MAX_POINTS and v > 0:
                flags[b] |= FLAG_AXIS
            box[b, j], cand[b, j], valid[b, j] = bx, c, v
            margins.append((b, j, bx[7], runner))
    return box, cand, valid, flags, margins


def margin_ok(area, runner_up, rel=1e-6):
    """The runner-up's area exceeds the winner's by a relative `rel` (of the runner-up; an exact tie inside the winner's class is
    decided by the candidate index and needs no margin)."""
    return runner_up == INF or runner_up - area > rel * runner_up


def kitti_text(tables, box, valid, keep=None, transforms=None, obj_type="Car"):
    """{seq: the text of its KITTI tracking result file} from a host log's tables and the statement's boxes: per kept record with a box
    one line, in (index, record) order."""
    from ratrack_amd import vod_io
    lines = {}
    for b in range(tables["cursor"].shape[0]):
        for f in range(int(tables["cursor"][b, 0])):
            rec, _, word, _ = (int(v) for v in tables["frame"][b, f])
            seq, index = int(tables["tag"][b, f, 0]), int(tables["tag"][b, f, 1])
            for r in range(rec, rec + (word & 0xffff)):
                if (keep is not None and not keep[b, r]) or valid[b, r] <= 0:
                    continue
                tf = None if transforms is None else transforms[(seq, index)]
                fields = vod_io.box_label_fields(box[b, r, :7], tf)
                text = vod_io.format_kitti_track_line(index, int(tables["rec_track"][b, r]), obj_type, fields, float(tables["rec_conf"][b, r]))
                lines.setdefault(seq, []).append((index, r, text))
    return {seq: "".join(t for _, _, t in sorted(rows, key=lambda x: (x[0], x[1]))) for seq, rows in lines.items()}
