"""Shared by tests/test_track_identity_cpu.py and tests/test_track_identity_gpu.py: the host statement of the identity metrics over
the scorer's log (include/rtk_score.h, ratrack_amd/track_score.py: `TrackScorer.identity`), written from the definitions in two forms
over the log entries of tests/_track_sweep_util.py, the generators of the clips whose optimum a greedy pairing misses, and that greedy
pairing itself.

  fast form    the walk of the header: per (stream, level) the frames in log order, per clip the sparse pair counts n[g,t], and at the
               clip's close the weight of a maximum-weight one-to-one matching by this file's own O(n^3) Hungarian method
  matrix form  as TrackEval's `Identity` computes it: per clip dense potential_matches_count / gt_id_count / tracker_id_count arrays
               over ALL the clip's labels and remaining track ids, the (G+T) x (G+T) fn_mat + fp_mat, one minimum-cost assignment
               (scipy's when `scipy` is asked for, this file's otherwise)

Everything is exact integer arithmetic until the three ratios."""
import math

import numpy as np

from _track_hota_util import clips_of, entries_from_log, plain_scores  # noqa: F401  (entries_from_log: for the tests)

COUNTERS = ("frames", "clips", "gt", "pred", "idtp", "pairs")
BIG = 10 ** 10                                      # TrackEval's 1e10, as an integer


# ---- the assignment --------------------------------------------------------------------------------------------------------------------
def min_assignment(cost):
    """cost: n rows x m columns (n <= m) of Python ints -> the column of every row in a minimum-cost assignment of all rows (the
    Hungarian method with potentials, O(n^2 m), exact)."""
    n, m = len(cost), len(cost[0]) if cost else 0
    assert n <= m
    inf = float("inf")
    u, v, p, way = [0] * (n + 1), [0] * (m + 1), [0] * (m + 1), [0] * (m + 1)
    for i in range(1, n + 1):
        p[0], j0 = i, 0
        minv, used = [inf] * (m + 1), [False] * (m + 1)
        while True:
            used[j0] = True
            i0, delta, j1, row = p[j0], inf, 0, cost[p[j0] - 1]
            for j in range(1, m + 1):
                if not used[j]:
                    cur = row[j - 1] - u[i0] - v[j]
                    if cur < minv[j]:
                        minv[j], way[j] = cur, j0
                    if minv[j] < delta:
                        delta, j1 = minv[j], j
            for j in range(m + 1):
                if used[j]:
                    u[p[j]] += delta
                    v[j] -= delta
                else:
                    minv[j] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    col = [0] * n
    for j in range(1, m + 1):
        if p[j]:
            col[p[j] - 1] = j - 1
    return col


def max_weight(n):
    """n: {(label, track id): weight > 0} -> the weight of a maximum-weight one-to-one matching of labels and track ids."""
    if not n:
        return 0
    gids, tids = sorted({g for g, _ in n}), sorted({t for _, t in n})
    if len(gids) > len(tids):                       # rows are the smaller side
        n, gids, tids = {(t, g): w for (g, t), w in n.items()}, tids, gids
    gi, ti = {g: k for k, g in enumerate(gids)}, {t: k for k, t in enumerate(tids)}
    cost = [[0] * len(tids) for _ in gids]          # a pair that never occurred weighs 0: matched or not, it adds nothing
    for (g, t), w in n.items():
        cost[gi[g]][ti[t]] = -w
    col = min_assignment(cost)
    return -sum(cost[i][j] for i, j in enumerate(col))


def greedy_weight(n):
    """Heaviest pair first (among equals the one that appeared first), each label and each track id once."""
    gs, ts, total = set(), set(), 0
    for (g, t), w in sorted(n.items(), key=lambda kv: -kv[1]):        # sorted is stable: insertion order among equals
        if g not in gs and t not in ts:
            gs.add(g); ts.add(t)
            total += w
    return total


# ---- fast form -------------------------------------------------------------------------------------------------------------------------
def frame_candidates(e, sc, tau, alpha):
    """One frame -> (number of remaining detections, their track ids, the set of (label, track id) of its candidates)."""
    kept, tids, pairs = set(e["labels"]), [], []
    for (tid, _, best, iou), s in zip(e["dets"], sc):
        if s < tau:
            continue
        tids.append(tid)
        if best != -1 and best in kept and iou >= alpha and (best, tid) not in pairs:
            pairs.append((best, tid))
    return len(tids), tids, pairs


def clip_pairs(clip, tau, alpha):
    """-> (n {(label, track id): frames} in order of first appearance, gt, pred) of one clip."""
    n, gt, pred = {}, 0, 0
    for e, sc in clip:
        remaining, _, pairs = frame_candidates(e, sc, tau, alpha)
        gt += len(e["labels"])
        pred += remaining
        for key in pairs:
            n[key] = n.get(key, 0) + 1
    return n, gt, pred


def walk(log_b, scores_b, tau, alpha):
    """-> (counters dict of one stream at one level, [(optimum, greedy weight, pairs)] of its clips)."""
    c, clips = dict.fromkeys(COUNTERS, 0), []
    for clip in clips_of(log_b, scores_b):
        n, gt, pred = clip_pairs(clip, tau, alpha)
        best = max_weight(n)
        clips.append((best, greedy_weight(n), len(n)))
        c["frames"] += len(clip)
        c["clips"] += 1
        c["gt"] += gt
        c["pred"] += pred
        c["idtp"] += best
        c["pairs"] += len(n)
    return c, clips


def _ratio(x, y):
    return x / y if y else float("nan")


def values(counters):
    """The host arithmetic with Python numbers: the streams pooled, per level."""
    out = {k: [] for k in ("idtp", "idfn", "idfp", "gt", "pred", "pairs", "idf1", "idr", "idp")}
    for a in range(counters.shape[0]):
        t = {k: int(counters[a, :, i].sum()) for i, k in enumerate(COUNTERS)}
        row = dict(idtp=t["idtp"], idfn=t["gt"] - t["idtp"], idfp=t["pred"] - t["idtp"], gt=t["gt"], pred=t["pred"], pairs=t["pairs"],
                   idf1=_ratio(2.0 * float(t["idtp"]), float(t["gt"] + t["pred"])), idr=_ratio(float(t["idtp"]), float(t["gt"])),
                   idp=_ratio(float(t["idtp"]), float(t["pred"])))
        for k, v in row.items():
            out[k].append(v)
    return out


def host_identity(logs, scores=None, tau=-math.inf, alphas=(0.5,)):
    """-> dict(counters (A,B,6) int64, clips: per level the list of every clip's (optimum, greedy weight, pairs), and the values of the
    header's host arithmetic: per-level lists idtp, idfn, idfp, gt, pred, pairs, idf1, idr, idp)."""
    B, A = len(logs), len(alphas)
    scores = [plain_scores(lb) for lb in logs] if scores is None else scores
    counters, clips = np.zeros((A, B, len(COUNTERS)), dtype=np.int64), [[] for _ in range(A)]
    for a, alpha in enumerate(alphas):
        for b in range(B):
            c, cl = walk(logs[b], scores[b], tau, alpha)
            counters[a, b] = [c[k] for k in COUNTERS]
            clips[a] += cl
    return dict(counters=counters, clips=clips, alpha=list(alphas), **values(counters))


# ---- matrix form -----------------------------------------------------------------------------------------------------------------------
def matrix_identity(logs, scores=None, tau=-math.inf, alphas=(0.5,), scipy=False):
    """TrackEval's arrangement -> per level a dict(idtp, idfn, idfp), pooled over the streams and their clips."""
    if scipy:
        from scipy.optimize import linear_sum_assignment
    scores = [plain_scores(lb) for lb in logs] if scores is None else scores
    out = []
    for alpha in alphas:
        idtp = idfn = idfp = 0
        for lb, sb in zip(logs, scores):
            for clip in clips_of(lb, sb):
                gids = sorted({lab for e, _ in clip for lab in e["labels"]})
                tids = sorted({t for e, sc in clip for t in frame_candidates(e, sc, tau, alpha)[1]})
                gi, ti = {g: k for k, g in enumerate(gids)}, {t: k for k, t in enumerate(tids)}
                G, T = len(gids), len(tids)
                if G + T == 0:
                    continue
                potential_matches_count = np.zeros((G, T), dtype=np.int64)
                gt_id_count, tracker_id_count = np.zeros(G, dtype=np.int64), np.zeros(T, dtype=np.int64)
                for e, sc in clip:
                    _, remaining, pairs = frame_candidates(e, sc, tau, alpha)
                    for lab in e["labels"]:
                        gt_id_count[gi[lab]] += 1
                    for t in remaining:
                        tracker_id_count[ti[t]] += 1
                    for lab, t in pairs:
                        potential_matches_count[gi[lab], ti[t]] += 1
                fp_mat, fn_mat = np.zeros((G + T, G + T), dtype=np.int64), np.zeros((G + T, G + T), dtype=np.int64)
                fp_mat[G:, :T] = BIG
                fn_mat[:G, T:] = BIG
                for g in range(G):
                    fn_mat[g, :T] = gt_id_count[g]
                    fn_mat[g, T + g] = gt_id_count[g]
                for t in range(T):
                    fp_mat[:G, t] = tracker_id_count[t]
                    fp_mat[t + G, t] = tracker_id_count[t]
                fn_mat[:G, :T] -= potential_matches_count
                fp_mat[:G, :T] -= potential_matches_count
                total = fn_mat + fp_mat
                if scipy:
                    rows, cols = linear_sum_assignment(total)
                else:
                    rows, cols = list(range(G + T)), min_assignment([[int(x) for x in r] for r in total])
                fn, fp = int(fn_mat[rows, cols].sum()), int(fp_mat[rows, cols].sum())
                idfn += fn
                idfp += fp
                idtp += int(gt_id_count.sum()) - fn
        out.append(dict(idtp=idtp, idfn=idfn, idfp=idfp))
    return out


# ---- the clips a greedy pairing gets wrong ---------------------------------------------------------------------------------------------
def _det(tid, best=-1, iou=0.0, conf=0.0):
    return (int(tid), np.float32(conf), int(best), float(iou))


def random_clip(rng, n, frames, ious=(0.9,), first=True, label0=0, track0=100):
    """n labels (all kept in every frame) and n track ids over `frames` frames: every track appears with probability 0.6 and takes a
    uniformly random best label; its IoU is drawn from `ious` and its confidence uniformly."""
    out = []
    for f in range(frames):
        dets = [_det(track0 + t, label0 + int(rng.integers(n)), float(rng.choice(ious)), float(rng.random())) for t in range(n)
                if rng.random() < 0.6]
        out.append(dict(reset=bool(first and f == 0), labels=[label0 + g for g in range(n)], dets=dets))
    return out


RANDOM_SHAPES = ((4, 12), (6, 24), (8, 40))


def dense_clip(seed=11, sticky=False, n=32, frames=256):
    """One clip of n labels and n track ids over `frames` frames: in frame f track t's best label is perm_f[t] of a seeded permutation,
    IoU 0.9 -- every one of the n * n pairs occurs.  sticky: with probability 0.3 the label is t, else with probability 0.4 it is
    (t + 1) mod n, else perm_f[t]: heavy diagonals over a thin background."""
    rng = np.random.default_rng(seed)
    out = []
    for f in range(frames):
        perm = rng.permutation(n)
        dets = []
        for t in range(n):
            g = int(perm[t])
            if sticky:
                x = rng.random()
                g = t if x < 0.3 else (t + 1) % n if x < 0.3 + 0.7 * 0.4 else g
            dets.append(_det(100 + t, g, 0.9))
        out.append(dict(reset=f == 0, labels=list(range(n)), dets=dets))
    return out
