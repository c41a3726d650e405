"""Shared by tests/test_track_hota_optimal_cpu.py and tests/test_track_hota_optimal_gpu.py: the host statements of HOTA under the optimal
matching and of the identity metrics over every pair (include/rtk_score.h, at the end; ratrack_amd/track_score.py:
`TrackScorer.hota(matching="optimal")`, `TrackScorer.identity(pairs="all")`), over the log entries of tests/_track_optimal_util.py
(dict(reset, labels, dets, sizes, label_sizes, pairs)).

  sparse form  the header's definitions, sum by sum in the stated order: per clip the alignment pass over the valid pairs (r, k, q, pmc,
               cg, ct, A), per frame ONE matching by `la_solve` of tests/_track_optimal_util.py over the 28-bit weights, per level the
               threshold on the matched pairs, at the clip's close the (g,t) with n > 0 in order of first appearance among the valid pairs
  dense form   as TrackEval's HOTA.eval_sequence / Identity.eval_sequence compute it: a similarity matrix per frame (kept objects x
               detections), sim_iou = similarity / (row sums + column sums - similarity), an id-indexed potential_matches_count,
               global_alignment_score, score_mat = global_alignment_score[ids] * similarity, matches_counts per level.  Where bits
               matter its additions are np.cumsum in the same order (adding the 0.0 of a pair that is none changes no bit), and the
               frame's assignment is `la_solve` on the nonzero entries of score_mat: the one departure from TrackEval the header
               states.  It takes logs whose track ids and label ids are distinct within a frame, as TrackEval's data are.

Everything is float64 arithmetic on the logged integers."""
import itertools
import math

import numpy as np

import _track_identity_util as I
from _track_hota_util import alpha_levels, clips_of, plain_scores
from _track_optimal_util import frame_from_ious, la_solve, make_frame

COUNTERS = ("frames", "clips", "gt", "pred", "tp", "pairs")
SUMS = ("ass", "ass_re", "ass_pr", "loc")
ONE = 1 << 28
EDGES = 2048
ALIGN_PAIRS = 1024


# ---- one frame -------------------------------------------------------------------------------------------------------------------------
def valid_pairs(e, sc, tau):
    """-> [(i, j, s)] in pair-log order: the logged pairs that describe the frame, with c > 0, a remaining detection and a positive
    denominator; s unclamped."""
    P, G, out = len(e["dets"]), len(e["labels"]), []
    for i, j, c in e["pairs"]:
        if not (0 <= i < P and 0 <= j < G) or c <= 0 or sc[i] < tau:
            continue
        den = e["sizes"][i] + e["label_sizes"][j] - c
        if den > 0:
            out.append((i, j, float(c) / float(den)))
    return out


def score_weight(score):
    """The float64 score A * sbar truncated to 28 bits; a positive overlap never vanishes."""
    return max(1, int(math.floor(min(score, 1.0) * float(ONE))))


def weight(a, sbar):
    return score_weight(a * sbar)


def remaining(e, sc, tau):
    return [i for i in range(len(e["dets"])) if not sc[i] < tau]


# ---- sparse form -----------------------------------------------------------------------------------------------------------------------
def clip_alignment(clip, tau):
    """The alignment pass of one clip -> (A {(g,t): float}, cg, ct, order: the potential (g,t) in order of first appearance)."""
    pmc, cg, ct = {}, {}, {}
    for e, sc in clip:
        vp = valid_pairs(e, sc, tau)
        r, k = {}, {}
        for i, j, s in vp:
            sb = min(s, 1.0)
            r[i] = r.get(i, 0.0) + sb
            k[j] = k.get(j, 0.0) + sb
        for i, j, s in vp:
            sb = min(s, 1.0)
            key = (e["labels"][j], e["dets"][i][0])
            pmc[key] = pmc.get(key, 0.0) + sb / ((r[i] + k[j]) - sb)
        for lab in e["labels"]:
            cg[lab] = cg.get(lab, 0) + 1
        for i in remaining(e, sc, tau):
            ct[e["dets"][i][0]] = ct.get(e["dets"][i][0], 0) + 1
    A = {(g, t): m / (float(cg[g] + ct[t]) - m) for (g, t), m in pmc.items()}
    return A, cg, ct, list(pmc)


def frame_matching(e, sc, tau, A):
    """-> (cp: the detection matched to every kept object or -1, {(i, j): s}, the edges)."""
    vp = valid_pairs(e, sc, tau)
    edges = [(i, j, weight(A[(e["labels"][j], e["dets"][i][0])], min(s, 1.0))) for i, j, s in vp]
    _, cp = la_solve(len(e["dets"]), len(e["labels"]), edges)
    return cp, {(i, j): s for i, j, s in vp}, edges


def walk(log_b, scores_b, tau, A_levels):
    """-> (counters (A,6), sums (A,4), trace) of one stream.  trace: per frame dict(cp, sims, edges, A) for the tests that look inside."""
    levels = alpha_levels(A_levels)
    c = [dict.fromkeys(COUNTERS, 0) for _ in levels]
    s = [dict.fromkeys(SUMS, 0.0) for _ in levels]
    trace = []
    for clip in clips_of(log_b, scores_b):
        A, cg, ct, order = clip_alignment(clip, tau)
        n = [dict() for _ in levels]
        for e, sc in clip:
            cp, sims, edges = frame_matching(e, sc, tau, A)
            trace.append(dict(cp=cp, sims=sims, edges=edges, A=A))
            for a, alpha in enumerate(levels):
                for j, i in enumerate(cp):
                    if i >= 0 and sims[(i, j)] >= alpha:
                        key = (e["labels"][j], e["dets"][i][0])
                        n[a][key] = n[a].get(key, 0) + 1
                        c[a]["tp"] += 1
                        s[a]["loc"] += sims[(i, j)]
        for a in range(len(levels)):
            c[a]["frames"] += len(clip)
            c[a]["clips"] += 1
            c[a]["gt"] += sum(cg.values())
            c[a]["pred"] += sum(ct.values())
            for key in order:
                m = n[a].get(key, 0)
                if m == 0:
                    continue
                g, t = key
                N = float(m * m)
                s[a]["ass"] += N / float(cg[g] + ct[t] - m)
                s[a]["ass_re"] += N / float(cg[g])
                s[a]["ass_pr"] += N / float(ct[t])
                c[a]["pairs"] += 1
    return c, s, trace


def host_hota_optimal(logs, scores=None, tau=-math.inf, A=19):
    """-> dict(counters (A,B,6) int64, sums (A,B,4) float64, trace: per stream the frames' matchings)."""
    B = len(logs)
    scores = [plain_scores(lb) for lb in logs] if scores is None else scores
    counters, sums = np.zeros((A, B, len(COUNTERS)), dtype=np.int64), np.zeros((A, B, len(SUMS)), dtype=np.float64)
    traces = []
    for b in range(B):
        c, s, trace = walk(logs[b], scores[b], tau, A)
        traces.append(trace)
        for a in range(A):
            counters[a, b] = [c[a][k] for k in COUNTERS]
            sums[a, b] = [s[a][k] for k in SUMS]
    return dict(counters=counters, sums=sums, trace=traces)


# ---- dense form ------------------------------------------------------------------------------------------------------------------------
def _ordered_sum(a, axis):
    """The sums along `axis`, one addition after the other from 0.0 (np.sum adds pairwise)."""
    if a.shape[axis] == 0:
        return np.zeros(np.delete(a.shape, axis))
    return np.take(np.cumsum(a, axis=axis), -1, axis=axis)


def frame_similarity(e, sc, tau):
    """-> (similarity (G, P) float64, 0 where there is no valid pair; the remaining detection indices)."""
    sim = np.zeros((len(e["labels"]), len(e["dets"])), dtype=np.float64)
    for i, j, s in valid_pairs(e, sc, tau):
        sim[j, i] = s
    return sim, remaining(e, sc, tau)


def dense_hota_optimal(logs, scores=None, tau=-math.inf, A=19):
    """TrackEval's arrangement -> dict(counters (A,B,6), sums (A,B,4))."""
    B = len(logs)
    scores = [plain_scores(lb) for lb in logs] if scores is None else scores
    levels = alpha_levels(A)
    counters, sums = np.zeros((A, B, len(COUNTERS)), dtype=np.int64), np.zeros((A, B, len(SUMS)), dtype=np.float64)
    for b in range(B):
        ass, loc = np.zeros((A, 3)), [0.0] * A
        for clip in clips_of(logs[b], scores[b]):
            gids = sorted({g for e, _ in clip for g in e["labels"]})
            tids = sorted({e["dets"][i][0] for e, sc in clip for i in remaining(e, sc, tau)})
            gi, ti = {g: k for k, g in enumerate(gids)}, {t: k for k, t in enumerate(tids)}
            potential_matches_count = np.zeros((len(gids), len(tids)), dtype=np.float64)
            gt_id_count, tracker_id_count = np.zeros((len(gids), 1)), np.zeros((1, len(tids)))
            first, frames = {}, []
            for e, sc in clip:
                similarity, rem = frame_similarity(e, sc, tau)
                assert len(set(e["labels"])) == len(e["labels"]) and len({d[0] for d in e["dets"]}) == len(e["dets"])
                sbar = np.minimum(similarity, 1.0)
                denom = (_ordered_sum(sbar, 0)[np.newaxis, :] + _ordered_sum(sbar, 1)[:, np.newaxis]) - sbar
                sim_iou = np.zeros_like(sbar)
                mask = sbar > 0.0
                sim_iou[mask] = sbar[mask] / denom[mask]
                gt_ids_t = np.array([gi[g] for g in e["labels"]], dtype=np.int64)
                tracker_ids_t = np.array([ti.get(d[0], -1) for d in e["dets"]], dtype=np.int64)       # -1: removed, its column is all 0
                keep = tracker_ids_t >= 0
                potential_matches_count[gt_ids_t[:, np.newaxis], tracker_ids_t[np.newaxis, keep]] += sim_iou[:, keep]
                gt_id_count[gt_ids_t] += 1
                tracker_id_count[0, tracker_ids_t[[i for i in rem]]] += 1
                for i in range(similarity.shape[1]):                                                   # pair-log order: (i, then j)
                    for j in range(similarity.shape[0]):
                        if similarity[j, i] > 0.0:
                            first.setdefault((int(gt_ids_t[j]), int(tracker_ids_t[i])), len(first))
                frames.append((similarity, sbar, gt_ids_t, tracker_ids_t))
            with np.errstate(divide="ignore", invalid="ignore"):
                global_alignment_score = potential_matches_count / ((gt_id_count + tracker_id_count) - potential_matches_count)
            matches_counts = [np.zeros((len(gids), len(tids)), dtype=np.int64) for _ in levels]
            for similarity, sbar, gt_ids_t, tracker_ids_t in frames:
                score_mat = np.zeros_like(sbar)
                if len(tids):                                                                          # (a removed detection's column is all 0)
                    score_mat = global_alignment_score[gt_ids_t[:, np.newaxis], np.maximum(tracker_ids_t, 0)[np.newaxis, :]] * sbar
                edges = [(i, j, score_weight(float(score_mat[j, i]))) for i in range(similarity.shape[1]) for j in range(similarity.shape[0])
                         if similarity[j, i] > 0.0]
                _, cp = la_solve(similarity.shape[1], similarity.shape[0], edges)
                match_rows = np.array([j for j, i in enumerate(cp) if i >= 0], dtype=np.int64)
                match_cols = np.array([i for i in cp if i >= 0], dtype=np.int64)
                for a, alpha in enumerate(levels):
                    sims = similarity[match_rows, match_cols] if len(match_rows) else np.zeros(0)
                    actually_matched_mask = sims >= alpha
                    alpha_match_rows, alpha_match_cols = match_rows[actually_matched_mask], match_cols[actually_matched_mask]
                    counters[a, b, COUNTERS.index("tp")] += len(alpha_match_rows)
                    if len(alpha_match_rows):
                        loc[a] = float(np.cumsum(np.concatenate([[loc[a]], sims[actually_matched_mask]]))[-1])
                        matches_counts[a][gt_ids_t[alpha_match_rows], tracker_ids_t[alpha_match_cols]] += 1
            order = sorted(first, key=first.get)
            for a in range(A):
                mc = np.array([matches_counts[a][g, t] for g, t in order], dtype=np.int64)
                gc = np.array([gt_id_count[g, 0] for g, t in order], dtype=np.int64)
                tc = np.array([tracker_id_count[0, t] for g, t in order], dtype=np.int64)
                hit = mc > 0
                N = (mc[hit] * mc[hit]).astype(np.float64)
                for k, den in enumerate((gc[hit] + tc[hit] - mc[hit], gc[hit], tc[hit])):
                    ass[a, k] = np.cumsum(np.concatenate([[ass[a, k]], N / den.astype(np.float64)]))[-1]
                counters[a, b, COUNTERS.index("pairs")] += int(hit.sum())
                counters[a, b, COUNTERS.index("frames")] += len(clip)
                counters[a, b, COUNTERS.index("clips")] += 1
                counters[a, b, COUNTERS.index("gt")] += int(gt_id_count.sum())
                counters[a, b, COUNTERS.index("pred")] += int(tracker_id_count.sum())
        for a in range(A):
            sums[a, b] = [ass[a, 0], ass[a, 1], ass[a, 2], loc[a]]
    return dict(counters=counters, sums=sums)


# ---- the quantisation ------------------------------------------------------------------------------------------------------------------
def float_optimum(scores):
    """scores (P, G) float64 >= 0 -> the largest sum a one-to-one matching can have: scipy's linear_sum_assignment, or all permutations."""
    P, G = scores.shape
    if min(P, G) == 0:
        return 0.0
    try:
        from scipy.optimize import linear_sum_assignment
        rows, cols = linear_sum_assignment(-scores)
        return float(scores[rows, cols].sum())
    except ImportError:
        small, big = (scores, G) if P <= G else (scores.T, P)
        return max(float(sum(small[r, c] for r, c in enumerate(perm))) for perm in itertools.permutations(range(big), small.shape[0]))


# ---- identity over every pair ------------------------------------------------------------------------------------------------------------
def clip_pairs_all(clip, tau, alpha):
    """-> (n {(label, track id): frames} in order of first appearance, gt, pred) of one clip: a frame counts for a pair when some
    remaining detection of the track has a valid pair with the label's object and s >= alpha."""
    n, gt, pred = {}, 0, 0
    for e, sc in clip:
        gt += len(e["labels"])
        pred += len(remaining(e, sc, tau))
        seen = []
        for i, j, s in valid_pairs(e, sc, tau):
            key = (e["labels"][j], e["dets"][i][0])
            if s >= alpha and key not in seen:
                seen.append(key)
                n[key] = n.get(key, 0) + 1
    return n, gt, pred


def host_identity_all(logs, scores=None, tau=-math.inf, alphas=(0.5,)):
    """-> dict(counters (A,B,6) int64 in IDENTITY_COUNTERS order, and the values of the header's host arithmetic)."""
    B, A = len(logs), len(alphas)
    scores = [plain_scores(lb) for lb in logs] if scores is None else scores
    counters = np.zeros((A, B, len(I.COUNTERS)), dtype=np.int64)
    for a, alpha in enumerate(alphas):
        for b in range(B):
            for clip in clips_of(logs[b], scores[b]):
                n, gt, pred = clip_pairs_all(clip, tau, alpha)
                counters[a, b] += (len(clip), 1, gt, pred, I.max_weight(n), len(n))
    return dict(counters=counters, alpha=list(alphas), **I.values(counters))


def dense_identity_all(logs, scores=None, tau=-math.inf, alphas=(0.5,)):
    """TrackEval's Identity.eval_sequence -> per level dict(idtp, idfn, idfp): potential_matches_count from the similarity matrices
    (every entry >= alpha), the (G+T) x (G+T) fn_mat + fp_mat, one minimum-cost assignment."""
    scores = [plain_scores(lb) for lb in logs] if scores is None else scores
    out = []
    for alpha in alphas:
        idtp = idfn = idfp = 0
        for lb, sb in zip(logs, scores):
            for clip in clips_of(lb, sb):
                gids = sorted({g for e, _ in clip for g in e["labels"]})
                tids = sorted({e["dets"][i][0] for e, sc in clip for i in remaining(e, sc, tau)})
                gi, ti = {g: k for k, g in enumerate(gids)}, {t: k for k, t in enumerate(tids)}
                G, T = len(gids), len(tids)
                if G + T == 0:
                    continue
                potential_matches_count = np.zeros((G, T), dtype=np.int64)
                gt_id_count, tracker_id_count = np.zeros(G, dtype=np.int64), np.zeros(T, dtype=np.int64)
                for e, sc in clip:
                    similarity, rem = frame_similarity(e, sc, tau)
                    matches_mask = similarity >= alpha
                    match_idx_gt, match_idx_tracker = np.nonzero(matches_mask)
                    gt_ids_t = np.array([gi[g] for g in e["labels"]], dtype=np.int64)
                    tracker_ids_t = np.array([ti.get(d[0], -1) for d in e["dets"]], dtype=np.int64)
                    potential_matches_count[gt_ids_t[match_idx_gt], tracker_ids_t[match_idx_tracker]] += 1
                    gt_id_count[gt_ids_t] += 1
                    tracker_id_count[tracker_ids_t[rem]] += 1
                fp_mat, fn_mat = np.zeros((G + T, G + T), dtype=np.int64), np.zeros((G + T, G + T), dtype=np.int64)
                fp_mat[G:, :T] = I.BIG
                fn_mat[:G, T:] = I.BIG
                for g in range(G):
                    fn_mat[g, :T] = gt_id_count[g]
                    fn_mat[g, T + g] = gt_id_count[g]
                for t in range(T):
                    fp_mat[:G, t] = tracker_id_count[t]
                    fp_mat[t + G, t] = tracker_id_count[t]
                fn_mat[:G, :T] -= potential_matches_count
                fp_mat[:G, :T] -= potential_matches_count
                total = fn_mat + fp_mat
                rows, cols = list(range(G + T)), I.min_assignment([[int(x) for x in r] for r in total])
                fn, fp = int(fn_mat[rows, cols].sum()), int(fp_mat[rows, cols].sum())
                idfn += fn
                idfp += fp
                idtp += int(gt_id_count.sum()) - fn
        out.append(dict(idtp=idtp, idfn=idfn, idfp=idfp))
    return out


# ---- the constructed cases ---------------------------------------------------------------------------------------------------------------
# Detections and objects of 20 points: c common points give the IoU c / (40 - c) -- 10: 1/3, 12: 3/7, 15: 3/5, 16: 2/3, 20: 1.
def alignment_case():
    """One clip of 4 frames: object 5 is followed by track 1 with IoU 3/5 in every frame; in frame 2 track 2, seen only there, has IoU
    2/3 with it.  An IoU-only matching of frame 2 takes track 2; the alignment score keeps track 1, whose 3/5 is below alpha = 13/20."""
    one = lambda reset=False: frame_from_ious([5], [(1, 0.5)], {(0, 0): 15}, reset)
    return [one(True), one(), frame_from_ious([5], [(1, 0.5), (2, 0.5)], {(0, 0): 15, (1, 0): 16}), one()]


def leak_case():
    """The alignment case, then a reset and its frame 2 alone: within that one-frame clip track 2 scores higher, so it is taken -- unless
    the first clip's alignment scores leak into the second."""
    return alignment_case() + [frame_from_ious([5], [(1, 0.5), (2, 0.5)], {(0, 0): 15, (1, 0): 16}, True)]


def identity_case():
    """One clip, one track: in frames 0 and 1 its detection overlaps object 1 with 2/3 (its best) and object 2 with 3/5; in frame 2 only
    object 2, with 3/5.  Best objects only: n = {(1,t): 2, (2,t): 1}, idtp 2.  Every pair above 0.5: n[(2,t)] = 3, idtp 3."""
    both = lambda reset=False: frame_from_ious([1, 2], [(7, 0.5)], {(0, 0): 16, (0, 1): 15}, reset)
    return [both(True), both(), frame_from_ious([1, 2], [(7, 0.5)], {(0, 1): 15})]


def threshold_case():
    """Two frames; detection 0 (track 10, confidence 1/8) overlaps objects 1 and 2, detection 1 (track 11, confidence 7/8) object 1.  A
    threshold of 0.5 removes track 10, which changes k of object 1 and with it q, pmc and A of (1, 11)."""
    fr = lambda reset: make_frame([1, 2], [20, 10], [(10, 0.125, 20), (11, 0.875, 11)], [(0, 0, 15), (0, 1, 10), (1, 0, 11)], reset)
    return [fr(True), fr(False), make_frame([1, 2], [20, 10], [(11, 0.875, 11)], [(0, 0, 11)])]


def clamp_case():
    """Coincident points: detection 0 and object 0 of 4 points with 6 common pairs, IoU 6 / 2 = 3, clamped to 1 in r, k, q and the weight
    and unclamped in the alpha test and LocA; detection 1 overlaps the same object with 1/7."""
    fr = lambda reset: make_frame([3], [4], [(1, 0.5, 4), (2, 0.5, 20)], [(0, 0, 6), (1, 0, 3)], reset)
    return [fr(True), fr(False)]


def tie_case():
    """One frame, one detection of 4 points against two objects of 4 points: 4 common pairs (IoU 1) with object 0 and 6 (IoU 3, clamped to
    1) with object 1.  Both edges weigh the same; the solver's rule gives the smaller column, object 0, and LocA gains 1 and not 3."""
    return [make_frame([8, 9], [4, 4], [(1, 0.5, 4)], [(0, 0, 4), (0, 1, 6)], True)]


def empty_sides_case():
    """A frame without detections, a frame without kept objects, then an ordinary one."""
    return [make_frame([7, 8], [9, 9], [], [], True), make_frame([], [], [(1, 0.5, 9), (2, 0.5, 9)], []), frame_from_ious([7], [(1, 0.5)], {(0, 0): 16})]


def constructed_logs():
    """The streams of the constructed cases, by name (dicts keep their order)."""
    return dict(alignment=alignment_case(), leak=leak_case(), identity=identity_case(), threshold=threshold_case(), clamp=clamp_case(),
                tie=tie_case(), empty_sides=empty_sides_case(), empty=[])


def edge_overflow_frame():
    """65 detections (16 track ids, each repeated) x 32 objects: 64 full rows and one pair more, EDGES + 1 valid pairs in one frame and
    16 * 32 potential pairs in its clip."""
    pairs = [(i, j, 20) for i in range(64) for j in range(32)] + [(64, 0, 20)]
    return make_frame(range(32), [40] * 32, [(100 + i % 16, 0.5, 40) for i in range(65)], pairs, True)


def pair_overflow_frame():
    """64 detections of distinct track ids x 17 objects, every pair present: 1088 potential pairs in one clip, and no more than EDGES
    valid pairs in the frame."""
    return make_frame(range(17), [40] * 17, [(100 + i, 0.5, 40) for i in range(64)], [(i, j, 20) for i in range(64) for j in range(17)], True)
