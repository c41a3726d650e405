"""Shared by tests/test_track_sweep_cpu.py and tests/test_track_sweep_gpu.py: the host statement of the confidence sweep
(include/rtk_score.h, ratrack_amd/track_score.py: sAMOTA / AMOTA / AMOTP), written from the definitions in two forms, and the
confidence plan that turns the seeded sequence of tests/_track_score_util.py into one that exercises it.

  fast form             a replay over per-detection pre-greedy best objects (vod_gt.iou_points against every kept object)
  full-definition form  for a threshold, the filtered detections are deleted from the `objects` dict and the rest goes through
                        `host_match` + `HostScorer`: the code the per-frame score is pinned against

Every float is float64 Python arithmetic on integers and on IoU sums added in stream, frame and detection order."""
import functools

import numpy as np

import _track_score_util as S
from ratrack_amd import vod_gt

COUNTERS = S.COUNTERS
SHAPE = dict(B=16, N=256, K=32, frames=12)      # the case both test files use


# ---- the confidence plan -----------------------------------------------------------------------------------------------------------
def confidence_plan(seq):
    """-> per frame a (B,K) float32 array, laid out like `ids`: a track's first detection in a clip 0 (as the tracker reports a new
    track), later ones base + ((5 f + tid) % 7 - 3) / 256 with base = ((37 tid + 11 b) % 29 + 2) / 32 for planned tracks and
    ((tid + b) % 4 + 1) / 32 for the spurious clusters (tid >= 9000).  Multiples of 1/256 below 1: their float64 sums are exact."""
    B, K = seq["B"], seq["K"]
    seen = [set() for _ in range(B)]
    out = []
    for f, fr in enumerate(seq["frames"]):
        conf = np.zeros((B, K), dtype=np.float32)
        for b in range(B):
            if not fr["active"][b]:
                continue
            if fr["reset"][b]:
                seen[b] = set()
            for i in range(int(fr["num"][b])):
                tid = int(fr["ids"][b, i])
                if tid in seen[b]:
                    base = ((37 * tid + 11 * b) % 29 + 2) / 32 if tid < 9000 else ((tid + b) % 4 + 1) / 32
                    conf[b, i] = base + ((5 * f + tid) % 7 - 3) / 256
                seen[b].add(tid)
        out.append(conf)
    return out


def raw_confidences(seq, seed=7):
    """Seeded fp32 confidences in [0, 1) that are NOT quantised and spread over 40 binades (the float64 sum of a few fp32 numbers of
    one magnitude would still be exact): the order of a track's float64 sum shows in its last bits."""
    rng = np.random.default_rng(seed)
    shape = (seq["B"], seq["K"])
    return [(rng.random(shape, dtype=np.float32) * np.exp2(-rng.integers(0, 40, shape)).astype(np.float32)).astype(np.float32)
            for _ in seq["frames"]]


# ---- the log, as the host sees it ------------------------------------------------------------------------------------------------------
def frame_entry(r, objects, confs, reset):
    """One logged frame: r the host_gt_objects tuple, objects {track id: (1,6,n)} in detection order, confs per detection."""
    dets = []
    for (tid, pts), c in zip(objects.items(), confs):
        best, bi = -1, 0
        for lab, g in r[7].items():
            v = vod_gt.iou_points(pts[0].numpy().T, g[0].numpy().T)
            if v > bi:
                bi, best = v, lab
        dets.append((int(tid), np.float32(c), int(best), float(bi)))
    return dict(reset=bool(reset), labels=[int(k) for k in r[7].keys()], dets=dets, r=r, objects=objects)


def sequence_log(seq, confs):
    """-> per stream the list of its active frames' entries (log order)."""
    logs = [[] for _ in range(seq["B"])]
    for fr, conf in zip(seq["frames"], confs):
        for b in range(seq["B"]):
            if not fr["active"][b]:
                continue
            n = int(fr["n_valid"][b])
            r = S.host_gt_objects(fr["per_stream"][b], fr["pc1"][b], n)
            objects = S.objects_dict(fr["pc1"][b], fr["obj"][b, :n], fr["ids"][b], int(fr["num"][b]))
            logs[b].append(frame_entry(r, objects, conf[b, :len(objects)], fr["reset"][b]))
    return logs


def track_scores(log_b):
    """-> per frame, per detection: the score of its (clip, track id): float64 sum of the fp32 confidences in log order / count.
    Also the {(clip, tid): score} table."""
    acc, clip = {}, 0
    for e in log_b:
        clip += int(e["reset"])
        for tid, c, _, _ in e["dets"]:
            s = acc.setdefault((clip, tid), [0.0, 0])
            s[0] += float(c)
            s[1] += 1
    table = {k: s[0] / s[1] for k, s in acc.items()}
    per, clip = [], 0
    for e in log_b:
        clip += int(e["reset"])
        per.append([table[(clip, tid)] for tid, _, _, _ in e["dets"]])
    return per, table


# ---- replay, fast form -------------------------------------------------------------------------------------------------------------
def _close(c, table):
    for k, v in zip(("tracks", "mt", "pt", "ml"), S.HostScorer.classify(list(table.values()))):
        c[k] += v
    table.clear()


def replay(log_b, scores_b, tau):
    """-> (counters dict, iou_sum, per frame the indices of the true positives)."""
    c, iou_sum, table, tps = dict.fromkeys(COUNTERS, 0), 0.0, {}, []
    for e, sc in zip(log_b, scores_b):
        if e["reset"]:
            _close(c, table)
        taken, pred, tp = {}, 0, []
        for i, ((tid, _, best, iou), s) in enumerate(zip(e["dets"], sc)):
            if s < tau:
                continue
            pred += 1
            if best == -1 or best in taken:
                continue
            taken[best] = tid
            iou_sum += iou
            tp.append(i)
        M = len(taken)
        c["frames"] += 1
        c["gt"] += len(e["labels"])
        c["pred"] += pred
        c["tp"] += M
        c["fp"] += pred - M
        c["fn"] += len(e["labels"]) - M
        for lab in e["labels"]:
            ent = table.setdefault(lab, [None, 0, 0])
            ent[1] += 1
            if lab in taken:
                if ent[0] is not None and ent[0] != taken[lab]:
                    c["idsw"] += 1
                ent[0] = taken[lab]
                ent[2] += 1
        tps.append(tp)
    _close(c, table)
    return c, iou_sum, tps


# ---- replay, full-definition form ----------------------------------------------------------------------------------------------------
def replay_full(log_b, scores_b, tau):
    """The same through vod_gt.map_gt_objects (`host_match`) and `HostScorer` on the objects that remain."""
    hs = S.HostScorer()
    for e, sc in zip(log_b, scores_b):
        objects = {tid: pts for (tid, pts), s in zip(e["objects"].items(), sc) if not s < tau}
        mapping, gt_id, iou = S.host_match(e["r"], objects)
        hs.frame(e["labels"], list(objects.keys()), gt_id, iou, mapping, e["reset"])
    return hs.final(), hs.iou_sum


# ---- thresholds and values -----------------------------------------------------------------------------------------------------------
def thresholds_walk(sorted_scores, G, L):
    """The KITTI walk -> every threshold it appends (the first, recall 0, included)."""
    s, n, cur, out = sorted_scores, len(sorted_scores), 0.0, []
    for i in range(n):
        l = (i + 1) / G
        r = (i + 2) / G if i < n - 1 else l
        if (r - cur) < (cur - l) and i < n - 1:
            continue
        out.append(s[i])
        cur += 1 / L
    return out


def host_sweep(logs, L=40, full=None):
    """-> dict(thresholds (L+1: -inf, the levels' thresholds, +inf past `reached`), reached, counters (L+1,B,11) int64, iou_sums
    (L+1,B), pooled per-level lists, amota, samota, amotp, best, scores, tp0).  full: an iterable of indices that are ALSO replayed in
    the full-definition form and compared (counters equal, IoU sums bit-equal)."""
    B = len(logs)
    scored = [track_scores(lb) for lb in logs]
    scores = [p for p, _ in scored]
    first = [replay(logs[b], scores[b], -np.inf) for b in range(B)]
    pool = sorted((scores[b][f][i] for b in range(B) for f, tp in enumerate(first[b][2]) for i in tp), reverse=True)
    G = sum(c["gt"] for c, _, _ in first)
    walked = thresholds_walk(pool, G, L)
    assert len(walked) <= L + 1, len(walked)
    reached = max(len(walked) - 1, 0)
    thr = np.array([-np.inf] + walked[1:] + [np.inf] * (L - reached), dtype=np.float64)
    counters, iou_sums = np.zeros((L + 1, B, len(COUNTERS)), dtype=np.int64), np.zeros((L + 1, B), dtype=np.float64)
    for k in range(reached + 1):
        for b in range(B):
            c, q, _ = replay(logs[b], scores[b], thr[k]) if k else first[b]
            counters[k, b] = [c[n] for n in COUNTERS]
            iou_sums[k, b] = q
            if full is not None and k in full:
                cf, qf = replay_full(logs[b], scores[b], thr[k])
                assert cf == c and qf == q, (k, b, cf, c, qf, q)
    idx = {n: i for i, n in enumerate(COUNTERS)}
    mota, smota, motp = [None], [None], [None]
    amota = samota = amotp = 0.0
    for k in range(1, reached + 1):
        t = [int(v) for v in counters[k].sum(axis=0)]
        err, Gk, rk = t[idx["fp"]] + t[idx["fn"]] + t[idx["idsw"]], t[idx["gt"]], k / L
        q = 0.0
        for b in range(B):
            q += float(iou_sums[k, b])
        mota.append(1 - err / Gk)
        smota.append(max(0.0, 1 - (err - (1 - rk) * Gk) / (rk * Gk)))
        motp.append(q / t[idx["tp"]] if t[idx["tp"]] else float("nan"))
        amota += mota[k]
        samota += smota[k]
        if t[idx["tp"]]:
            amotp += motp[k]
    best = None
    for k in range(1, reached + 1):
        if best is None or mota[k] > mota[best]:
            best = k
    return dict(thresholds=thr, reached=reached, counters=counters, iou_sums=iou_sums, mota=mota, smota=smota, motp=motp,
                amota=amota / L, samota=samota / L, amotp=amotp / L, best=best, scores=scores, tables=[t for _, t in scored],
                tp0=[f[2] for f in first], walked=walked)


@functools.lru_cache(maxsize=2)
def planned(raw=False):
    """The shared case, computed once: -> (seq, confs, logs, host_sweep(logs))."""
    seq = S.synthetic_sequence(**SHAPE)
    confs = raw_confidences(seq) if raw else confidence_plan(seq)
    logs = sequence_log(seq, confs)
    return seq, confs, logs, host_sweep(logs)


def census(logs, sw):
    """The situations the sweep has to meet on this log."""
    B, L = len(logs), len(sw["thresholds"]) - 1
    freed = 0
    for k in range(1, sw["reached"] + 1):
        for b in range(B):
            _, _, tps = replay(logs[b], sw["scores"][b], sw["thresholds"][k])
            freed += sum(len(set(tp) - set(tp0)) for tp, tp0 in zip(tps, sw["tp0"][b]))
    pooled = sw["counters"][1:sw["reached"] + 1].sum(axis=1)
    col = lambda n: pooled[:, COUNTERS.index(n)].tolist()
    every = [v for t in sw["tables"] for v in t.values()]
    shared = sum(1 for v in every if every.count(v) > 1 and v != 0.0)
    return dict(freed_matches=freed, idsw_values=len(set(col("idsw"))), mt_values=len(set(col("mt"))), ml_values=len(set(col("ml"))),
                tracks_sharing_a_score=shared, tracks=len(every))
