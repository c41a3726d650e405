"""Shared by tests/test_track_centre_cpu.py and tests/test_track_centre_gpu.py: the host statement of TrackEval's centre-distance
similarity on the pair log (include/rtk_score.h, the last section; ratrack_amd/track_score.py: `TrackScorer(similarity="centre")`), in
float64 numpy and plain Python.

  the producer   centres by np.cumsum in column order, the similarity operation by operation, the frame's pair list in (i, then j)
                 order, the fit rule, and the packed pair log with its pair_sim
  the replays    the host statements that exist -- `_track_optimal_util.replay` / `host_sweep`, `_track_hota_optimal_util.host_hota_optimal`
                 / `dense_hota_optimal` / `host_identity_all` / `dense_identity_all` -- with their two similarity functions (`pair_iou`,
                 `valid_pairs`) substituted by `patch_similarity`: a log entry carries a `sims` list beside `pairs`, and a pair is valid iff
                 it describes its frame, its detection remains and s > 0.  Those statements restate `la_solve`, the device's documented
                 choice, so every counter is compared.

A log entry is `_track_optimal_util`'s (dict(reset, labels, dets, sizes, label_sizes, pairs)) plus sims [s of pair k]."""
import numpy as np

import _track_hota_optimal_util as HO
import _track_optimal_util as O

ZERO_DISTANCE = 2.0


# ---- the producer --------------------------------------------------------------------------------------------------------------------
def centre_of(pc_b, cols):
    """pc_b (3,N) float32, cols ascending -> the float64 centre: three sums from 0.0 in column order, each divided by the count."""
    pts = pc_b[:, cols].astype(np.float64)
    return np.cumsum(pts, axis=1)[:, -1] / np.float64(len(cols))


def similarity(c, g, zero_distance=ZERO_DISTANCE):
    """s = 1 - |c - g| / zero_distance, every operation a float64 operation of its own."""
    dx, dy, dz = np.float64(c[0]) - np.float64(g[0]), np.float64(c[1]) - np.float64(g[1]), np.float64(c[2]) - np.float64(g[2])
    d2 = (dx * dx + dy * dy) + dz * dz
    return np.float64(1.0) - np.sqrt(d2) / np.float64(zero_distance)


def common_count(pc_b, cols, member_cols):
    """rtk_track_score's `common`: the (detection point, object point) pairs closer than 1e-5, float32 differences squared in float64."""
    if not len(cols) or not len(member_cols):
        return 0
    a, o = pc_b[:, cols].astype(np.float32), pc_b[:, member_cols].astype(np.float32)
    d = (a[:, :, None] - o[:, None, :]).astype(np.float64)
    d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    return int((d2 < 1e-5 * 1e-5).sum())


def member_columns(words, n):
    """One object's (W) uint32 member words -> its columns below n, ascending."""
    return [p for p in range(n) if (int(words[p >> 5]) >> (p & 31)) & 1]


def frame_pairs(pc_b, obj_b, n, P, members_b, centre_b, G, zero_distance=ZERO_DISTANCE):
    """One stream's frame -> ([(i, j, common)], [s]) in (i, then j) order: the pairs with s > 0.0 (a NaN is none); a detection without
    a live column has none."""
    pairs, sims = [], []
    mcols = [member_columns(members_b[j], n) for j in range(G)]
    for i in range(P):
        cols = [p for p in range(n) if obj_b[p] == i]
        if not cols:
            continue
        c = centre_of(pc_b, cols)
        for j in range(G):
            s = similarity(c, centre_b[j], zero_distance)
            if s > 0.0:
                pairs.append((i, j, common_count(pc_b, cols, mcols[j])))
                sims.append(float(s))
    return pairs, sims


def host_pair_log(frames, B, F, R, Q, zero_distance=ZERO_DISTANCE):
    """frames: [dict(pc1 (B,3,N), obj (B,N), n_valid (B), num (B), count (B), members (B,K,W) uint32, centre (B,K,3), active (B))] ->
    dict(pair_cursor (B), pair_frame (B,F,2), pair_key, pair_common (B,Q) int32, pair_sim (B,Q) float64, frames (B): the frames each
    stream logged, dropped (B): whether a frame did not fit) as rtk_track_score_pairs_centre leaves them: a frame is logged whole or
    not at all."""
    a = dict(pair_cursor=np.zeros(B, np.int32), pair_frame=np.zeros((B, F, 2), np.int32), pair_key=np.zeros((B, Q), np.int32),
             pair_common=np.zeros((B, Q), np.int32), pair_sim=np.zeros((B, Q), np.float64), frames=np.zeros(B, np.int64),
             dropped=np.zeros(B, bool), entries=[[] for _ in range(B)])
    rec, lab = np.zeros(B, np.int64), np.zeros(B, np.int64)
    for fr in frames:
        for b in range(B):
            if not fr["active"][b]:
                continue
            n, P, G = int(fr["n_valid"][b]), int(fr["num"][b]), int(fr["count"][b])
            pairs, sims = frame_pairs(fr["pc1"][b], fr["obj"][b], n, P, fr["members"][b], fr["centre"][b], G, zero_distance)
            f, q = int(a["frames"][b]), int(a["pair_cursor"][b])
            if not (f < F and rec[b] + P <= R and lab[b] + G <= R and q + len(pairs) <= Q):
                a["dropped"][b] = True
                continue
            a["pair_frame"][b, f] = (q, len(pairs))
            for k, ((i, j, c), s) in enumerate(zip(pairs, sims)):
                a["pair_key"][b, q + k], a["pair_common"][b, q + k], a["pair_sim"][b, q + k] = (i << 8) | j, c, s
            a["pair_cursor"][b], a["frames"][b] = q + len(pairs), f + 1
            rec[b], lab[b] = rec[b] + P, lab[b] + G
            a["entries"][b].append((pairs, sims))
    return a


def dense_similarity(centres, positions, zero_distance=ZERO_DISTANCE):
    """TrackEval's _calculate_euclidean_similarity: (P,3) against (G,3) -> (P,G) max(0, 1 - ||a - b|| / zero_distance)."""
    dist = np.linalg.norm(np.asarray(centres, np.float64)[:, np.newaxis] - np.asarray(positions, np.float64)[np.newaxis, :], axis=2)
    return np.maximum(0, 1 - dist / zero_distance)


# ---- the replays: the existing host statements on the log's own similarity ----------------------------------------------------------------
def _sim_lookup(e):
    return {(i, j): s for (i, j, _), s in zip(e["pairs"], e["sims"])}


def pair_sim(e, i, j, c):
    """In place of `_track_optimal_util.pair_iou`: the log's similarity of the pair, or 0.0 (no candidate at any min_iou > 0) where it
    is not > 0.  The common count and the sizes are not read."""
    s = _sim_lookup(e)[(i, j)]
    return s if s > 0.0 else 0.0


def valid_pairs(e, sc, tau):
    """In place of `_track_hota_optimal_util.valid_pairs`: [(i, j, s)] in pair-log order -- the key describes the frame, the detection
    remains, s > 0.0 (a NaN is not)."""
    P, G = len(e["dets"]), len(e["labels"])
    return [(i, j, s) for (i, j, _), s in zip(e["pairs"], e["sims"]) if 0 <= i < P and 0 <= j < G and not sc[i] < tau and s > 0.0]


def patch_similarity(monkeypatch):
    """Substitutes the two similarity functions of the existing host statements (undone by pytest when the test ends, or by the
    `monkeypatch.context()` it was given)."""
    monkeypatch.setattr(O, "pair_iou", pair_sim)
    monkeypatch.setattr(HO, "valid_pairs", valid_pairs)


def with_sims(logs, seed, zero_some_commons=True):
    """Entries of `_track_optimal_util` -> the same entries with a `sims` list: similarities on the grid k / 20 (ties, and values exactly
    at the alpha levels and at min_iou = 0.25, 0.5) mixed with random ones in (0, 1]; every third pair's common count set to 0, which a
    replay on the similarity must not notice."""
    rng = np.random.default_rng(seed)
    out = []
    for lb in logs:
        nb = []
        for e in lb:
            sims = [float(rng.integers(1, 21)) / 20.0 if rng.random() < 0.6 else float(1.0 - rng.random()) for _ in e["pairs"]]
            pairs = [(i, j, 0 if zero_some_commons and k % 3 == 0 else c) for k, (i, j, c) in enumerate(e["pairs"])]
            nb.append(dict(e, pairs=pairs, sims=sims))
        out.append(nb)
    return out


def pack(logs, F, R, Q):
    """`_track_optimal_util.pack` plus pair_sim (B,Q) float64."""
    a = O.pack(logs, F, R, Q)
    a["pair_sim"] = np.zeros((len(logs), Q), np.float64)
    for b, lb in enumerate(logs):
        q = 0
        for e in lb:
            a["pair_sim"][b, q:q + len(e["sims"])] = e["sims"]
            q += len(e["sims"])
    return a


def entries_from_logs(cursor, frame, label, track, best, conf, iou, pair_frame, pair_key, pair_common, size, label_size, pair_sim):
    """`_track_optimal_util.entries_from_logs` of a centre scorer's tensors, each entry with its sims."""
    logs = O.entries_from_logs(cursor, frame, label, track, best, conf, iou, pair_frame, pair_key, pair_common, size, label_size)
    for b, lb in enumerate(logs):
        for f, e in enumerate(lb):
            q, nq = (int(v) for v in pair_frame[b, f])
            e["sims"] = [float(v) for v in pair_sim[b, q:q + nq]]
    return logs


# ---- hand-built frames for the producer -----------------------------------------------------------------------------------------------------
def scenario(seed, B=4, N=96, Kobj=16, K=8, frames=3, zero_distance=ZERO_DISTANCE):
    """Seeded frames for a scorer of B streams (hand-built ground-truth objects: any members, any centres).  Per stream and frame up to
    Kobj - 4 detections of 1 to 6 columns each and up to K objects; an object's position is a detection's centre plus an offset of 0 to
    1.5 zero_distance (some pairs within reach, some not), its members a random set of columns (common > 0 and the position are
    independent).  Stream 0: coordinates of mixed magnitude within one detection (1e4, 1, 1e-4 interleaved); stream 3's detection 0: 1e7, 1,
    1e-7, -1e7.  Stream 1: n_valid < N,
    the dead columns carry detection indices and coordinates of 1e6.  Stream 2: detection 1 has no live column; inactive in frame 1.
    Stream 3: reset in frame 1.  Frame 1: stream 0 has P = 0, stream 1 has G = 0.  Every stream is reset in frame 0."""
    rng = np.random.default_rng(seed)
    W = (N + 31) // 32
    out = []
    for f in range(frames):
        pc1 = (rng.integers(-160, 160, (B, 3, N)).astype(np.float32) / np.float32(64.0))      # within 2.5: many centres near many objects
        obj, num, ids = np.full((B, N), -1, np.int32), np.zeros(B, np.int32), np.full((B, Kobj), -1, np.int32)
        conf = (rng.integers(1, 256, (B, Kobj)).astype(np.float32) / np.float32(256.0))
        n_valid, count = np.full(B, N, np.int32), np.zeros(B, np.int32)
        members, centre = np.zeros((B, K, W), np.uint32), np.zeros((B, K, 3), np.float64)
        slot, label_id, size = np.full((B, K), -1, np.int32), np.full((B, K), -1, np.int32), np.zeros((B, K), np.int32)
        active, reset = np.ones(B, np.uint8), np.zeros(B, np.uint8)
        for b in range(B):
            reset[b] = 1 if f == 0 or (b == 3 and f == 1) else 0
            active[b] = 0 if (b == 2 and f == 1) else 1
            n = N if b != 1 else N - 36
            n_valid[b] = n
            P = 0 if (b == 0 and f == 1) else int(rng.integers(3, Kobj - 3))
            G = 0 if (b == 1 and f == 1) else int(rng.integers(2, K + 1))
            perm = rng.permutation(n)
            at = 0
            for i in range(P):
                m = int(rng.integers(1, 7))
                cols = perm[at:at + m] if at + m <= n else perm[at:at]
                at += len(cols)
                if b == 2 and i == 1:
                    cols = cols[:0]                # a detection without a live column
                obj[b, cols] = i
                if b == 0:                         # 1e4, 1, 1e-4 interleaved in column order: the summation order shows
                    for k, p in enumerate(sorted(cols.tolist())):
                        pc1[b, :, p] = np.float32((1e4, 1.0, 1e-4)[k % 3]) * (np.float32(1.0) + pc1[b, :, p] / np.float32(64.0))
                if b == 3 and i == 0:              # a wider spread (1e7, 1, 1e-7): float32 values that far apart do not add exactly in float64
                    for k, p in enumerate(sorted(cols.tolist())):
                        pc1[b, :, p] = np.float32((1e7, 1.0, 1e-7, -1e7)[k % 4]) * (np.float32(1.0) + pc1[b, :, p] / np.float32(64.0))
                ids[b, i] = 100 + i + 20 * (f % 2)
            num[b] = P
            if b == 1:                             # dead columns that carry detection indices and large coordinates
                obj[b, n:] = rng.integers(0, max(P, 1), N - n)
                pc1[b, :, n:] = np.float32(1e6)
            centres = [centre_of(pc1[b], [p for p in range(n) if obj[b, p] == i]) if (obj[b, :n] == i).any() else None for i in range(P)]
            live = [c for c in centres if c is not None]
            for j in range(G):
                base = live[j % len(live)] if live else np.zeros(3)
                d = rng.normal(size=3)
                d = d / np.linalg.norm(d) * float(rng.random()) * 1.5 * zero_distance
                centre[b, j] = base + d
                cols = rng.choice(n, int(rng.integers(2, 9)), replace=False)
                if live and rng.random() < 0.7:    # share some columns with a detection
                    own = [p for p in range(n) if obj[b, p] == int(rng.integers(0, P))]
                    cols = np.unique(np.concatenate([cols, np.array(own[:3], dtype=np.int64)]))
                for p in cols.tolist():
                    members[b, j, p >> 5] |= np.uint32(1 << (p & 31))
                size[b, j], slot[b, j] = len(set(cols.tolist())), j
            label_id[b, :G] = 10 + rng.permutation(K + 3)[:G]          # distinct within a frame, persisting over the frames
            count[b] = G
        out.append(dict(pc1=pc1, obj=obj, num=num, ids=ids, conf=conf, n_valid=n_valid, count=count, members=members, centre=centre, slot=slot,
                        label_id=label_id, size=size, active=active, reset=reset))
    return out
