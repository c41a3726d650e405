"""Shared by tests/test_track_box_cpu.py and tests/test_track_box_gpu.py: the host statement of the oriented-box IoU on the pair log
(include/rtk_score.h, the last section; ratrack_amd/track_score.py: `TrackScorer(similarity="box")` / `"box_bev"`), in numpy scalars of
one floating-point type -- float64 is the statement, numpy.longdouble the yardstick of its own rounding.

  the similarity  operation by operation as the header states it: the detection's box, the label box read upright, the prefilter, the z
                  overlap, the cut of the detection's footprint by the object's rectangle and Green's theorem, the value
  the producer    the frame's pair list in (i, then j) order, the fit rule, and the packed pair log with its pair_sim
  the reference   `exact_iou`: the same boxes in `fractions.Fraction` -- a Sutherland-Hodgman clip of one rectangle by the other, the
                  shoelace area, headings that are rational points of the circle -- which shares no code with the statement
  the replays     the host statements that exist, with their two similarity functions substituted as `_track_centre_util` does
                  (`patch_similarity`, `pack`, `entries_from_logs`, `with_sims` are its own: a log that carries its similarity)

THE BOUND ON pair_sim.  The device's sincos and sqrt are not correctly rounded and its operation order may differ from numpy's, so
pair_sim is compared within SIM_BOUND = 64 * SIM_D, where SIM_D bounds the largest |s(float64) - s(longdouble)| of this statement over
the tests' own scenarios (`measure_d`; tests/test_track_box_cpu.py measures it again and holds it below SIM_D).  Measured with an
80-bit long double: 3.9e-16 over the producer scenarios (seeds 21, 23, 24), the exact frame, the crowded frame and the rational cases
of the CPU test.  A few ulp of heading error move a corner by ulp x the box's extent; 64 covers that and another summation order, and
2.56e-14 stays eleven orders below the spacing of any level the replays use."""
import fractions
import math

import numpy as np

import _track_centre_util as C

F = fractions.Fraction
MODE_3D, MODE_BEV = 0, 1                   # RTK_SCORE_BOX_3D, RTK_SCORE_BOX_BEV
MODES = {"box": MODE_3D, "box_bev": MODE_BEV}
SIM_D = 4.0e-16                            # the largest float64 - longdouble difference measured (3.9e-16), rounded up
SIM_BOUND = 64 * SIM_D                     # 2.56e-14: what pair_sim may differ by between the device and the float64 statement

patch_similarity, pack, entries_from_logs, with_sims = C.patch_similarity, C.pack, C.entries_from_logs, C.with_sims
common_count, member_columns = C.common_count, C.member_columns


# ---- the similarity ---------------------------------------------------------------------------------------------------------------------
def cut_area(Dx, Dy, lx, ly, wx, wy, a, b, T):
    """The area of the rectangle with centre D and half axes (lx, ly), (-wx, wy) cut by |x| <= a, |y| <= b: Sutherland-Hodgman by the
    four half-planes x <= a, x >= -a, y <= b, y >= -b on a set of directed edges in eight slots -- the rectangle's four, then the edge
    each cut adds along its bound from where the outline leaves to where it comes back -- and Green's theorem over the slots in
    order.  A crossing point is formed once, its cut coordinate set to the bound itself."""
    zero = T(0.0)
    cs = [((Dx + lx) - wx, (Dy + ly) + wy), ((Dx - lx) - wx, (Dy - ly) + wy), ((Dx - lx) + wx, (Dy - ly) - wy), ((Dx + lx) + wx, (Dy + ly) - wy)]
    edges = [[cs[e][0], cs[e][1], cs[(e + 1) & 3][0], cs[(e + 1) & 3][1]] for e in range(4)] + [None] * 4
    for k in range(4):
        lim = a if k < 2 else b
        bound = -lim if k & 1 else lim
        axis = 0 if k < 2 else 1
        out = back = None
        for e in range(4 + k):
            ed = edges[e]
            if ed is None:
                continue
            v0, v1 = ed[axis], ed[2 + axis]
            s0, s1 = (v0 + lim, v1 + lim) if k & 1 else (lim - v0, lim - v1)
            in0, in1 = s0 >= 0, s1 >= 0
            if in0 and in1:
                continue
            if not in0 and not in1:
                edges[e] = None
                continue
            t = s0 / (s0 - s1)
            c = (bound, ed[1] + t * (ed[3] - ed[1])) if axis == 0 else (ed[0] + t * (ed[2] - ed[0]), bound)
            if in0:
                ed[2], ed[3] = c
                out = c
            else:
                ed[0], ed[1] = c
                back = c
        if out is not None and back is not None:
            edges[4 + k] = [out[0], out[1], back[0], back[1]]
    acc = zero
    for ed in edges:
        if ed is not None:
            acc = acc + (ed[0] * ed[3] - ed[2] * ed[1])
    return T(0.5) * acc


def detection(box, valid, mode, T=np.float64):
    """Row (8) of rtk_object_boxes and its valid word -> None (no box: no pairs) or (cx, cy, L, W, c, s, bottom, top, h)."""
    cx, cy, cz, l, w, h, yaw = (T(v) for v in np.asarray(box, np.float64)[:7])
    if not (int(valid) > 0 and all(np.isfinite(v) for v in (cx, cy, cz, l, w, h, yaw)) and l > 0 and w > 0 and (mode == MODE_BEV or h > 0)):
        return None
    half = T(0.5)
    return cx, cy, half * l, half * w, np.cos(yaw), np.sin(yaw), cz - half * h, cz + half * h, h


def upright(row, T=np.float64):
    """Row (16) of the frame-1 box table (centre | R | half-extent | pad) -> None (no pairs) or (gx, gy, hx, hy, a, b, bottom, top)."""
    r = np.asarray(row, np.float64)
    gx, gy, gz, ux, uy, h0, h1, h2 = (T(v) for v in (r[0], r[1], r[2], r[3], r[6], r[12], r[13], r[14]))
    n = np.sqrt(ux * ux + uy * uy)
    if not (all(np.isfinite(v) for v in (gx, gy, gz, ux, uy, h0, h1, h2, n)) and n != 0 and h0 > 0 and h1 > 0 and h2 > 0):
        return None
    return gx, gy, ux / n, uy / n, h0, h1, gz - h2, gz + h2


def prefilter(det, gt, T=np.float64):
    """-> (d2, rr * rr): the pair has s = 0 where d2 > rr * rr."""
    dx, dy = det[0] - gt[0], det[1] - gt[1]
    rr = np.sqrt(det[2] * det[2] + det[3] * det[3]) + np.sqrt(gt[4] * gt[4] + gt[5] * gt[5])
    return dx * dx + dy * dy, rr * rr


def similarity_of(det, gt, mode, T=np.float64):
    """`detection` and `upright` (either may be None) -> s, every operation an operation of T of its own."""
    zero = T(0.0)
    if det is None or gt is None:
        return zero
    dcx, dcy, L, W, c, s, dbot, dtop, h = det
    gx, gy, hx, hy, a, b, gbot, gtop = gt
    d2, rr2 = prefilter(det, gt, T)
    if d2 > rr2:
        return zero
    zo = T(1.0)
    if mode == MODE_3D:
        zo = (dtop if dtop < gtop else gtop) - (dbot if dbot > gbot else gbot)
        if not zo > 0:
            return zero
    dx, dy = dcx - gx, dcy - gy
    Dx, Dy = dx * hx + dy * hy, dy * hx - dx * hy
    ex, ey = c * hx + s * hy, s * hx - c * hy
    I2 = cut_area(Dx, Dy, L * ex, L * ey, W * ey, W * ex, a, b, T)
    two = T(2.0)
    l, w, a2, b2 = two * L, two * W, two * a, two * b
    Ai, Aj = l * w, a2 * b2
    if mode == MODE_BEV:
        v = I2 / ((Ai + Aj) - I2)
    else:
        I3 = I2 * zo
        v = I3 / ((Ai * h + Aj * (gtop - gbot)) - I3)
    return v if v < 1 else (T(1.0) if v >= 1 else v)


def similarity(box, valid, row, mode, T=np.float64):
    """s of one detection row and one label-box row."""
    with np.errstate(all="ignore"):
        return similarity_of(detection(box, valid, mode, T), upright(row, T), mode, T)


# ---- the producer ---------------------------------------------------------------------------------------------------------------------------
def frame_pairs(fr, b, mode, T=np.float64):
    """One stream's frame -> ([(i, j, common)], [s], margins): the pairs with s > 0 (a NaN is none) in (i, then j) order; margins: the
    relative distance |d2 - rr^2| / rr^2 of every pair of boxes from the prefilter's rim."""
    n, P, G = int(fr["n_valid"][b]), int(fr["num"][b]), int(fr["count"][b])
    K = fr["boxes"].shape[1]
    pairs, sims, margins = [], [], []
    with np.errstate(all="ignore"):
        gts = [upright(fr["boxes"][b, fr["slot"][b, j]], T) if 0 <= fr["slot"][b, j] < K else None for j in range(G)]
        mcols = [member_columns(fr["members"][b, j], n) for j in range(G)]
        for i in range(P):
            det = detection(fr["det_box"][b, i], fr["det_valid"][b, i], mode, T)
            if det is None:
                continue
            cols = [p for p in range(n) if fr["obj"][b, p] == i]
            for j in range(G):
                if gts[j] is None:
                    continue
                d2, rr2 = prefilter(det, gts[j], T)
                margins.append(float(abs(d2 - rr2) / rr2))
                s = similarity_of(det, gts[j], mode, T)
                if s > 0:
                    pairs.append((i, j, common_count(fr["pc1"][b], cols, mcols[j])))
                    sims.append(s)
    return pairs, sims, margins


def host_pair_log(frames, B, F, R, Q, mode, T=np.float64):
    """frames: `scenario`'s -> dict(pair_cursor (B), pair_frame (B,F,2), pair_key, pair_common (B,Q) int32, pair_sim (B,Q), frames (B),
    dropped (B), entries, margins) as rtk_track_score_pairs_box leaves them: a frame is logged whole or not at all."""
    a = dict(pair_cursor=np.zeros(B, np.int32), pair_frame=np.zeros((B, F, 2), np.int32), pair_key=np.zeros((B, Q), np.int32),
             pair_common=np.zeros((B, Q), np.int32), pair_sim=np.zeros((B, Q), T), frames=np.zeros(B, np.int64),
             dropped=np.zeros(B, bool), entries=[[] for _ in range(B)], margins=[], all_sims=[])
    rec, lab = np.zeros(B, np.int64), np.zeros(B, np.int64)
    for fr in frames:
        for b in range(B):
            if not fr["active"][b]:
                continue
            P, G = int(fr["num"][b]), int(fr["count"][b])
            pairs, sims, margins = frame_pairs(fr, b, mode, T)
            a["margins"] += margins
            a["all_sims"] += [float(s) for s in sims]
            f, q = int(a["frames"][b]), int(a["pair_cursor"][b])
            if not (f < F and rec[b] + P <= R and lab[b] + G <= R and q + len(pairs) <= Q):
                a["dropped"][b] = True
                continue
            a["pair_frame"][b, f] = (q, len(pairs))
            for k, ((i, j, c), s) in enumerate(zip(pairs, sims)):
                a["pair_key"][b, q + k], a["pair_common"][b, q + k], a["pair_sim"][b, q + k] = (i << 8) | j, c, s
            a["pair_cursor"][b], a["frames"][b] = q + len(pairs), f + 1
            rec[b], lab[b] = rec[b] + P, lab[b] + G
            a["entries"][b].append((pairs, [float(s) for s in sims]))
    return a


def condition_holds(log):
    """What the device comparison rests on, of the host statement alone: no logged pair has 0 < s < 1e-6, and no pair of boxes lies
    within 1e-6 (relative) of the prefilter's rim."""
    return all(s >= 1e-6 for s in log["all_sims"]) and all(m >= 1e-6 for m in log["margins"])


def measure_d(frames, B, mode):
    """The largest |s(float64) - s(longdouble)| over every pair of boxes of `frames` that either precision logs."""
    d = 0.0
    for fr in frames:
        for b in range(B):
            if not fr["active"][b]:
                continue
            lo, hi = ({(i, j): s for (i, j, _), s in zip(*frame_pairs(fr, b, mode, T)[:2])} for T in (np.float64, np.longdouble))
            for k in set(lo) | set(hi):
                d = max(d, abs(float(np.longdouble(lo.get(k, 0.0)) - np.longdouble(hi.get(k, 0.0)))))
    return d


# ---- the reference: exact rational arithmetic -----------------------------------------------------------------------------------------------
def _rect(cx, cy, c, s, L, W):
    """Corners, counter-clockwise, of the 2L x 2W rectangle about (cx, cy) with its length along (c, s); all Fractions."""
    return [(cx + sl * L * c - sw * W * s, cy + sl * L * s + sw * W * c) for sl, sw in ((1, 1), (-1, 1), (-1, -1), (1, -1))]


def _clip_polygon(poly, clip):
    """Sutherland-Hodgman: the convex polygon `poly` cut by every edge of the convex counter-clockwise polygon `clip`."""
    out = list(poly)
    for k in range(len(clip)):
        (ax, ay), (bx, by) = clip[k], clip[(k + 1) % len(clip)]
        side = lambda p: (bx - ax) * (p[1] - ay) - (by - ay) * (p[0] - ax)          # >= 0: inside
        src, out = out, []
        for m in range(len(src)):
            p, q = src[m], src[(m + 1) % len(src)]
            sp, sq = side(p), side(q)
            if sp >= 0:
                out.append(p)
            if (sp > 0 and sq < 0) or (sp < 0 and sq > 0):
                t = sp / (sp - sq)
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
        if not out:
            return []
    return out


def _area(poly):
    return sum(poly[k][0] * poly[(k + 1) % len(poly)][1] - poly[(k + 1) % len(poly)][0] * poly[k][1] for k in range(len(poly))) / 2 if poly else F(0)


def exact_iou(det, gt, mode):
    """det, gt: dict(c=(x, y, z), heading=(cos, sin) a rational point of the circle, size=(l, w, h)), all Fractions -> the exact IoU (a
    Fraction): BEV of the footprints, 3D of the upright boxes."""
    rects = [_rect(F(r["c"][0]), F(r["c"][1]), F(r["heading"][0]), F(r["heading"][1]), F(r["size"][0]) / 2, F(r["size"][1]) / 2) for r in (det, gt)]
    I = _area(_clip_polygon(rects[0], rects[1]))
    A = [F(r["size"][0]) * F(r["size"][1]) for r in (det, gt)]
    if mode == MODE_BEV:
        return I / (A[0] + A[1] - I)
    top = min(F(r["c"][2]) + F(r["size"][2]) / 2 for r in (det, gt))
    bottom = max(F(r["c"][2]) - F(r["size"][2]) / 2 for r in (det, gt))
    zo = max(top - bottom, F(0))
    V = [A[k] * F(r["size"][2]) for k, r in enumerate((det, gt))]
    return I * zo / (V[0] + V[1] - I * zo)


def det_row(r):
    """A rational box -> row (8) of rtk_object_boxes: yaw by atan2 of the heading (the one place trigonometry enters the statement)."""
    l, w, h = (float(v) for v in r["size"])
    return np.array([float(r["c"][0]), float(r["c"][1]), float(r["c"][2]), l, w, h, math.atan2(float(r["heading"][1]), float(r["heading"][0])), l * w])


def gt_row(r, tilt=0.0):
    """A rational box -> row (16) of the frame-1 box table: R = Rz(heading) Ry(tilt), so that a tilt shortens the heading's projection."""
    c, s = float(r["heading"][0]), float(r["heading"][1])
    ct, st = math.cos(tilt), math.sin(tilt)
    R = np.array([[c * ct, -s, c * st], [s * ct, c, s * st], [-st, 0.0, ct]])
    return np.concatenate([[float(v) for v in r["c"]], R.reshape(-1), [float(v) / 2 for v in r["size"]], [0.0]])


# ---- hand-built frames for the producer ------------------------------------------------------------------------------------------------------
def scenario(seed, B=4, N=96, Kobj=16, K=8, frames=3, many=None):
    """Seeded frames for a scorer of B streams: hand-built ground-truth objects (any members), label boxes and detection boxes (any
    boxes: update_raw takes them as given).  Per stream and frame up to Kobj - 4 detections of 1 to 4 columns and up to K objects;
    the label boxes stand 2 to 6 m apart with headings of any angle and a tilt of 0.0094 rad (R's first column is shorter than 1),
    in slots permuted against the kept order; detection i sits on object i % G with an offset of up to its size and a heading within
    0.5 rad of the object's, or anywhere; every fourth is lifted out of the object's z range.  Members share columns with detections
    or not, so pairs with and without a common point are logged.
    Stream 0: detection 1 has valid = 0, detection 2 valid = -1 and a NaN, detection 3 width 0.  Stream 2: object 1 has a half-extent
    0; stream 3: object 0 has no heading (R[0][0] = R[1][0] = 0), object 1 a NaN centre.  Stream 1: n_valid < N.  Frame 1: stream 0 has
    P = 0, stream 1 has G = 0, stream 2 is inactive, stream 3 is reset.  many: stream 1 has that many detections in frame 2 (the
    ordered prefix then crosses a wave).  Every stream is reset in frame 0."""
    rng = np.random.default_rng(seed)
    Wd = (N + 31) // 32
    out = []
    for f in range(frames):
        pc1 = (rng.integers(-160, 160, (B, 3, N)).astype(np.float32) / np.float32(64.0))
        obj, num, ids = np.full((B, N), -1, np.int32), np.zeros(B, np.int32), np.full((B, Kobj), -1, np.int32)
        conf = (rng.integers(1, 256, (B, Kobj)).astype(np.float32) / np.float32(256.0))
        n_valid, count = np.full(B, N, np.int32), np.zeros(B, np.int32)
        members = np.zeros((B, K, Wd), np.uint32)
        slot, label_id, size = np.full((B, K), -1, np.int32), np.full((B, K), -1, np.int32), np.zeros((B, K), np.int32)
        boxes = np.zeros((B, K, 16), np.float64)
        det_box, det_valid = np.zeros((B, Kobj, 8), np.float64), np.zeros((B, Kobj), np.int32)
        active, reset = np.ones(B, np.uint8), np.zeros(B, np.uint8)
        for b in range(B):
            reset[b] = 1 if f == 0 or (b == 3 and f == 1) else 0
            active[b] = 0 if (b == 2 and f == 1) else 1
            n = N if b != 1 else N - 20
            n_valid[b] = n
            P = 0 if (b == 0 and f == 1) else int(rng.integers(5, Kobj - 3))
            if many and b == 1 and f == 2:
                P = many
            G = 0 if (b == 1 and f == 1) else int(rng.integers(3, K + 1))
            perm, at = rng.permutation(n), 0
            for i in range(P):
                m = 1 if P > n // 4 else int(rng.integers(1, 5))
                cols = perm[at:at + m] if at + m <= n else perm[at:at]
                at += len(cols)
                obj[b, cols] = i
                ids[b, i] = 100 + i + 20 * (f % 2)
            num[b] = P
            if b == 1:
                obj[b, n:] = rng.integers(0, max(P, 1), N - n)
            slots = rng.permutation(K)[:G]
            geo = []
            for j in range(G):
                ang, sz = float(rng.uniform(-np.pi, np.pi)), rng.uniform((1.0, 0.6, 1.0), (4.5, 2.2, 2.0))
                c = np.array([3.0 * (j % 3) + rng.uniform(-0.5, 0.5), 4.0 * (j // 3) + rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5)])
                r = dict(c=c, heading=(math.cos(ang), math.sin(ang)), size=sz)
                boxes[b, slots[j]] = gt_row(r, tilt=0.0094)
                geo.append((c, ang, sz))
                cols = rng.choice(n, int(rng.integers(2, 9)), replace=False)
                if P and rng.random() < 0.7:
                    own = [p for p in range(n) if obj[b, p] == int(rng.integers(0, P))]
                    cols = np.unique(np.concatenate([cols, np.array(own[:3], dtype=np.int64)]))
                for p in cols.tolist():
                    members[b, j, p >> 5] |= np.uint32(1 << (p & 31))
                size[b, j], slot[b, j] = len(set(cols.tolist())), slots[j]
            label_id[b, :G] = 10 + rng.permutation(K + 3)[:G]
            count[b] = G
            for i in range(P):
                sz = rng.uniform((0.8, 0.5, 0.8), (4.5, 2.2, 2.0))
                if G and rng.random() < 0.85:
                    c, ang, gsz = geo[i % G]
                    c = c + rng.uniform(-1.0, 1.0, 3) * np.array([gsz[0], gsz[1], 0.3 * gsz[2]]) * 0.6
                    ang = ang + float(rng.uniform(-0.5, 0.5)) + (np.pi / 2 if rng.random() < 0.2 else 0.0)
                    if i % 4 == 3:
                        c[2] += 4.0                       # footprints overlap, the z ranges do not
                else:
                    c, ang = rng.uniform((-2.0, -2.0, -0.5), (8.0, 10.0, 0.5)), float(rng.uniform(-np.pi, np.pi))
                yaw = (ang + np.pi / 2) % np.pi - np.pi / 2                  # rtk_object_boxes' range
                det_box[b, i] = (c[0], c[1], c[2], sz[0], sz[1], sz[2], yaw, sz[0] * sz[1])
                det_valid[b, i] = int((obj[b, :n] == i).sum()) or 1
            if b == 0 and P > 3:
                det_valid[b, 1] = 0
                det_valid[b, 2], det_box[b, 2, 0] = -1, np.nan
                det_box[b, 3, 4] = 0.0
            if b == 2 and G > 1:
                boxes[b, slot[b, 1], 13] = 0.0
            if b == 3 and G > 1:
                boxes[b, slot[b, 0], 3], boxes[b, slot[b, 0], 6] = 0.0, 0.0
                boxes[b, slot[b, 1], 1] = np.nan
        out.append(dict(pc1=pc1, obj=obj, num=num, ids=ids, conf=conf, n_valid=n_valid, count=count, members=members, slot=slot, label_id=label_id,
                        size=size, active=active, reset=reset, boxes=boxes, det_box=det_box, det_valid=det_valid,
                        centre=np.zeros((B, K, 3), np.float64)))
    return out


def exact_frame():
    """One stream, yaw = 0, R = identity, every coordinate dyadic and every extent a power of two, so that every operation of the
    statement is exact but the last division, whatever the clip.  Object j and detection j stand at x = 10 j, far from every other.
      0  identical 2 x 2 x 2 boxes                                     s = 1
      1  a 2 x 2 x 2 detection inside a 4 x 2 x 2 object, three faces shared   s = 1/2
      2  2 x 2 x 2 boxes a metre apart in x                              s = 1/3
      3  2 x 2 x 2 boxes a metre apart in x and in y                     s = 1/7
      4  2 x 2 x 2 boxes touching along an edge (two metres apart in x)  not logged
      5  2 x 2 x 2 boxes touching at a corner                            not logged
      6  identical footprints, z ranges apart                            BEV s = 1; 3D not logged
    -> (frame, N, K, Kobj, {mode: [(i, j, common, s)]})."""
    N, K, Kobj = 64, 8, 8
    P = G = 7
    pc1 = np.zeros((1, 3, N), np.float32)
    pc1[0] = (np.arange(3 * N, dtype=np.float32).reshape(3, N) % 29) + 1.0
    obj = np.full((1, N), -1, np.int32)
    members = np.zeros((1, K, 2), np.uint32)
    for i in range(P):
        obj[0, 2 * i:2 * i + 2] = i
        for p in (2 * i, 2 * i + 1) if i != 2 else (40, 41):          # pair 2 has no common point
            members[0, i, p >> 5] |= np.uint32(1 << (p & 31))
    gts = [((0, 0, 0), (2, 2, 2)), ((10, 0, 0), (4, 2, 2)), ((20, 0, 0), (2, 2, 2)), ((30, 0, 0), (2, 2, 2)), ((40, 0, 0), (2, 2, 2)),
           ((50, 0, 0), (2, 2, 2)), ((60, 0, 0), (2, 2, 2))]
    dets = [((0, 0, 0), (2, 2, 2)), ((11, 0, 0), (2, 2, 2)), ((21, 0, 0), (2, 2, 2)), ((31, 1, 0), (2, 2, 2)), ((42, 0, 0), (2, 2, 2)),
            ((52, 2, 0), (2, 2, 2)), ((60, 0, 4), (2, 2, 2))]
    boxes, det_box = np.zeros((1, K, 16), np.float64), np.zeros((1, Kobj, 8), np.float64)
    for j, (c, sz) in enumerate(gts):
        boxes[0, j] = gt_row(dict(c=c, heading=(1, 0), size=sz))
    for i, (c, sz) in enumerate(dets):
        det_box[0, i] = det_row(dict(c=c, heading=(1, 0), size=sz))
    fr = dict(pc1=pc1, obj=obj, num=np.array([P], np.int32), ids=np.array([[7, 8, 9, 10, 11, 12, 13, -1]], np.int32),
              conf=np.full((1, Kobj), 0.5, np.float32), n_valid=np.array([N], np.int32), count=np.array([G], np.int32), members=members,
              slot=np.array([[0, 1, 2, 3, 4, 5, 6, -1]], np.int32), label_id=np.array([[10, 11, 12, 13, 14, 15, 16, -1]], np.int32),
              size=np.array([[2, 2, 2, 2, 2, 2, 2, 0]], np.int32), active=np.ones(1, np.uint8), reset=np.ones(1, np.uint8), boxes=boxes,
              det_box=det_box, det_valid=np.array([[2, 2, 2, 2, 2, 2, 2, 0]], np.int32), centre=np.zeros((1, K, 3), np.float64))
    want = [(0, 0, 2, 1.0), (1, 1, 2, 0.5), (2, 2, 0, 1.0 / 3.0), (3, 3, 2, 1.0 / 7.0)]
    return fr, N, K, Kobj, {MODE_3D: want, MODE_BEV: want + [(6, 6, 2, 1.0)]}


def crowded_frame():
    """Two streams, Kobj = 64, K = 40.  Stream 0: 64 detections and 40 objects that all overlap -- 2560 valid pairs, more than
    RTK_SCORE_PAIR_EDGES; stream 1: two detections and three objects.  16 track ids x 40 labels: the clip's pairs fit the alignment
    pass.  -> (frame, B, N, Kobj, K)."""
    B, N, Kobj, K = 2, 128, 64, 40
    pc1 = (np.arange(B * 3 * N, dtype=np.float32).reshape(B, 3, N) % 17) / np.float32(64.0)
    obj = np.full((B, N), -1, np.int32)
    obj[0, :] = np.arange(N) % 64
    obj[1, :4] = [0, 0, 1, 1]
    members = np.zeros((B, K, (N + 31) // 32), np.uint32)
    for j in range(K):
        members[:, j, j >> 5] |= np.uint32(1 << (j & 31))
        members[:, j, (j + 64) >> 5] |= np.uint32(1 << ((j + 64) & 31))
    boxes, det_box = np.zeros((B, K, 16), np.float64), np.zeros((B, Kobj, 8), np.float64)
    for j in range(K):
        boxes[:, j] = gt_row(dict(c=(0.125 * (j % 4), 0.0625 * (j // 4), 0), heading=(F(3, 5), F(4, 5)), size=(4, 2, 2)))
    for i in range(Kobj):
        det_box[:, i] = det_row(dict(c=(0.25 - 0.03125 * (i % 8), 0.0625 * (i // 8), 0.25), heading=(F(4, 5), F(3, 5)), size=(3, 2, 1.5)))
    fr = dict(pc1=pc1, obj=obj, num=np.array([64, 2], np.int32), ids=np.tile(np.arange(64, dtype=np.int32) % 16 + 100, (B, 1)),
              conf=np.full((B, Kobj), 0.5, np.float32), n_valid=np.array([N, N], np.int32), count=np.array([K, 3], np.int32), members=members,
              slot=np.tile(np.arange(K, dtype=np.int32), (B, 1)), label_id=np.tile(np.arange(K, dtype=np.int32) + 10, (B, 1)),
              size=np.full((B, K), 2, np.int32), active=np.ones(B, np.uint8), reset=np.ones(B, np.uint8), boxes=boxes, det_box=det_box,
              det_valid=np.full((B, Kobj), 2, np.int32), centre=np.zeros((B, K, 3), np.float64))
    return fr, B, N, Kobj, K
