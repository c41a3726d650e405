"""Shared by tests/test_track_hota_cpu.py and tests/test_track_hota_gpu.py: the host statement of HOTA over the scorer's log
(include/rtk_score.h, ratrack_amd/track_score.py: `TrackScorer.hota`), written from the definitions in two forms over the log
entries of tests/_track_sweep_util.py (`sequence_log`, `track_scores`), and a converter from downloaded `log_*` tensors to such entries.

  fast form    the walk of the header: per (stream, alpha) the frames in log order, candidates in detection order, per clip the
               label counts, the track counts and the pairs in order of first appearance; Python floats in the device's sum orders
  matrix form  as TrackEval computes it: per clip dense matches_count / gt_id_count / tracker_id_count arrays,
               ass_a = m / max(1, g + t - m), AssA = sum m * ass_a / TP -- another order of the sums, so compared at relative 1e-12

Every float is float64 arithmetic on integers and on the log's IoUs."""
import math

import numpy as np

COUNTERS = ("frames", "clips", "gt", "pred", "tp", "pairs")
SUMS = ("ass", "ass_re", "ass_pr", "loc")


def alpha_levels(A):
    return [a / (A + 1) for a in range(1, A + 1)]


def plain_scores(log_b):
    """Scores that no threshold removes (for tau = -inf the scores do not matter)."""
    return [[0.0] * len(e["dets"]) for e in log_b]


def clips_of(log_b, scores_b):
    """-> the stream's clips, each a list of (entry, scores): a clip closes at a reset frame or at the end of the log."""
    clips = []
    for f, (e, sc) in enumerate(zip(log_b, scores_b)):
        if f == 0 or e["reset"]:
            clips.append([])
        clips[-1].append((e, sc))
    return clips


def frame_matches(e, sc, tau, alpha):
    """One frame under the rule -> (remaining detection indices, [(index, label, track id, iou)] true positives in detection order).
    alpha None: no level (the sweep's replay)."""
    remaining, taken, tps = [], set(), []
    for i, ((tid, _, best, iou), s) in enumerate(zip(e["dets"], sc)):
        if s < tau:
            continue
        remaining.append(i)
        if best == -1 or (alpha is not None and not iou >= alpha):
            continue                                    # no candidate: takes nothing, the object stays free
        if best in taken:
            continue
        taken.add(best)
        tps.append((i, best, tid, iou))
    return remaining, tps


# ---- fast form ---------------------------------------------------------------------------------------------------------------------
def walk(log_b, scores_b, tau, alpha):
    """-> (counters dict, sums dict, freed) of one stream at one level.  freed: the true positives that the rule without a level
    leaves unmatched -- a later detection won an object whose first taker fell below alpha."""
    c, s, freed = dict.fromkeys(COUNTERS, 0), dict.fromkeys(SUMS, 0.0), 0
    for clip in clips_of(log_b, scores_b):
        cg, ct, n = {}, {}, {}                          # dicts keep insertion order: n's is the order of first appearance
        for e, sc in clip:
            remaining, tps = frame_matches(e, sc, tau, alpha)
            plain = {t[0] for t in frame_matches(e, sc, tau, None)[1]}
            for lab in e["labels"]:
                cg[lab] = cg.get(lab, 0) + 1
            for i in remaining:
                tid = e["dets"][i][0]
                ct[tid] = ct.get(tid, 0) + 1
            for i, lab, tid, iou in tps:
                n[(lab, tid)] = n.get((lab, tid), 0) + 1
                s["loc"] += iou
                freed += int(i not in plain)
            c["frames"] += 1
        c["clips"] += 1
        c["gt"] += sum(cg.values())
        c["pred"] += sum(ct.values())
        c["tp"] += sum(n.values())
        c["pairs"] += len(n)
        for (lab, tid), m in n.items():
            N = float(m * m)
            s["ass"] += N / float(cg[lab] + ct[tid] - m)
            s["ass_re"] += N / float(cg[lab])
            s["ass_pr"] += N / float(ct[tid])
    return c, s, freed


def host_hota(logs, scores=None, tau=-math.inf, A=19):
    """-> dict(counters (A,B,6) int64, sums (A,B,4) float64, freed (A), and the values of the header's host arithmetic: per-level
    lists tp, fn, fp, gt, pred, pairs, deta, detre, detpr, assa, assre, asspr, loca, hota_alpha and the means hota, deta_mean, ...)."""
    B = len(logs)
    scores = [plain_scores(lb) for lb in logs] if scores is None else scores
    counters, sums = np.zeros((A, B, len(COUNTERS)), dtype=np.int64), np.zeros((A, B, len(SUMS)), dtype=np.float64)
    freed = [0] * A
    for a, alpha in enumerate(alpha_levels(A)):
        for b in range(B):
            c, s, fr = walk(logs[b], scores[b], tau, alpha)
            counters[a, b] = [c[k] for k in COUNTERS]
            sums[a, b] = [s[k] for k in SUMS]
            freed[a] += fr
    out = dict(counters=counters, sums=sums, freed=freed, **values(counters, sums))
    return out


def _ratio(x, y):
    return x / y if y else float("nan")


def values(counters, sums):
    """The host arithmetic with Python floats: the streams pooled in stream order, per level, then the means."""
    A, B = counters.shape[:2]
    names = ("deta", "detre", "detpr", "assa", "assre", "asspr", "loca", "hota_alpha")
    out = {k: [] for k in ("tp", "fn", "fp", "gt", "pred", "pairs") + names}
    for a in range(A):
        t = {k: int(counters[a, :, i].sum()) for i, k in enumerate(COUNTERS)}
        q = [0.0] * len(SUMS)
        for b in range(B):
            for i in range(len(SUMS)):
                q[i] += float(sums[a, b, i])
        tp, fn, fp = t["tp"], t["gt"] - t["tp"], t["pred"] - t["tp"]
        row = dict(tp=tp, fn=fn, fp=fp, gt=t["gt"], pred=t["pred"], pairs=t["pairs"], deta=_ratio(float(tp), float(tp + fn + fp)),
                   detre=_ratio(float(tp), float(tp + fn)), detpr=_ratio(float(tp), float(tp + fp)), assa=_ratio(q[0], float(tp)),
                   assre=_ratio(q[1], float(tp)), asspr=_ratio(q[2], float(tp)), loca=_ratio(q[3], float(tp)))
        row["hota_alpha"] = math.sqrt(row["deta"] * row["assa"]) if not (math.isnan(row["deta"]) or math.isnan(row["assa"])) else float("nan")
        for k, v in row.items():
            out[k].append(v)
    for k in names:
        acc = 0.0
        for v in out[k]:
            if not math.isnan(v):
                acc += v
        out["hota" if k == "hota_alpha" else k + "_mean"] = acc / A
    return out


# ---- matrix form -------------------------------------------------------------------------------------------------------------------
def matrix_hota(logs, scores=None, tau=-math.inf, A=19):
    """TrackEval's arrangement -> per level a dict(tp, fn, fp, assa, assre, asspr, loca, deta, hota_alpha), pooled over the streams
    and their clips."""
    scores = [plain_scores(lb) for lb in logs] if scores is None else scores
    out = []
    for alpha in alpha_levels(A):
        tp = gt = pred = 0
        ass = ass_re = ass_pr = loc = 0.0
        for lb, sb in zip(logs, scores):
            for clip in clips_of(lb, sb):
                gids = sorted({lab for e, _ in clip for lab in e["labels"]})
                tids = sorted({e["dets"][i][0] for e, sc in clip for i in frame_matches(e, sc, tau, alpha)[0]})
                gi, ti = {g: k for k, g in enumerate(gids)}, {t: k for k, t in enumerate(tids)}
                matches_count = np.zeros((len(gids), len(tids)), dtype=np.float64)
                gt_id_count, tracker_id_count = np.zeros((len(gids), 1)), np.zeros((1, len(tids)))
                for e, sc in clip:
                    remaining, tps = frame_matches(e, sc, tau, alpha)
                    for lab in e["labels"]:
                        gt_id_count[gi[lab], 0] += 1
                    for i in remaining:
                        tracker_id_count[0, ti[e["dets"][i][0]]] += 1
                    for _, lab, tid, iou in tps:
                        matches_count[gi[lab], ti[tid]] += 1
                        loc += iou
                ass_a = matches_count / np.maximum(1, gt_id_count + tracker_id_count - matches_count)
                ass += float((matches_count * ass_a).sum())
                ass_re += float((matches_count * (matches_count / np.maximum(1, gt_id_count))).sum())
                ass_pr += float((matches_count * (matches_count / np.maximum(1, tracker_id_count))).sum())
                tp += int(matches_count.sum())
                gt += int(gt_id_count.sum())
                pred += int(tracker_id_count.sum())
        fn, fp = gt - tp, pred - tp
        deta, assa = _ratio(tp, tp + fn + fp), _ratio(ass, tp)
        out.append(dict(tp=tp, fn=fn, fp=fp, assa=assa, assre=_ratio(ass_re, tp), asspr=_ratio(ass_pr, tp), loca=_ratio(loc, tp), deta=deta,
                        hota_alpha=math.sqrt(deta * assa) if tp else float("nan")))
    return out


# ---- the device's log, as entries ------------------------------------------------------------------------------------------------------
def entries_from_log(cursor, frame, label, track, best, conf, iou):
    """Downloaded log_cursor (B,4), log_frame (B,F,4), log_label, log_track, log_best, log_conf, log_iou (B,R) arrays -> per stream
    the list of its frames' entries: dict(reset, labels, dets [(track id, conf, best label, iou)]) as `sequence_log` builds them."""
    logs = []
    for b in range(cursor.shape[0]):
        lb = []
        for f in range(int(cursor[b, 0])):
            r, l, pw, G = (int(v) for v in frame[b, f])
            P = pw & 0xffff
            dets = [(int(track[b, r + i]), np.float32(conf[b, r + i]), int(best[b, r + i]), float(iou[b, r + i])) for i in range(P)]
            lb.append(dict(reset=bool((pw >> 16) & 1), labels=[int(v) for v in label[b, l:l + G]], dets=dets))
        logs.append(lb)
    return logs
