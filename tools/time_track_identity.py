"""The identity metrics over the scorer's log (ratrack_amd/track_score.py `TrackScorer.identity`, csrc/track_identity.hip,
csrc/lds_assignment.h): the launch, the whole call and the host statement, with HOTA over the same log as the yardstick, and the
solver at its limit.

    python tools/time_track_identity.py [--streams 64] [--points 256] [--boxes 32] [--max-objects 128] [--iters 50] [--warmup 5]
                                        [--rounds 3] [--frames 300] [--alphas 19] [--out profiles/track_identity_timing.json]

The log of tools/time_track_hota.py (--streams x --frames frames of the batch of tools/time_track_score.py; seeded confidences; track
ids that change now and then; a reset every 100 frames).  Measured on the machine it runs on, device time between events around the
entry point, medians of --iters after --warmup, --rounds rounds with the variants alternating inside every round:

  identity           `rtk_score_identity` at the single level 0.5, nothing removed (one launch, grid streams x 1)
  identity_levels    the same at HOTA's --alphas levels (grid streams x alphas)
  hota               `rtk_score_hota` at --alphas levels over the same log: the yardstick, one walk of the same kind per workgroup
  identity_no_candidates   `rtk_score_identity` at --alphas levels on a copy of the log whose detections have no best label: the walk
                     without pairs, so that the difference to identity_levels is the pair list and the solver
  dense, dense_sticky      one stream, one clip of 256 frames, 32 labels x 32 track ids, every pair present (1024 edges) / heavy
                     diagonals over a thin background (tests/_track_identity_util.py `dense_clip`, restated): the solver at
                     RTK_SCORE_ID_PAIRS, one level
  dense_no_candidates      the dense log without best labels: its walk alone

and, wall clock, `identity()` and `hota()` end to end (each call ends in its download) and the host statement -- the header's
definitions as Python loops with an O(n^3) Hungarian method, over the downloaded log and over the dense clips -- with host and
device compared for equality.

Writes one JSON object to --out and prints it.  Not part of bench.py."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ratrack_amd import _lib, abi, gt_device as G, synth, track_score as TS  # noqa: E402
from time_track_score import make_streams  # noqa: E402
from time_track_sweep import block_us, host_log, summary  # noqa: E402


# ---- the host statement over a downloaded log (include/rtk_score.h) ---------------------------------------------------------------------
def max_weight(n):
    """{(label, track id): weight} -> the weight of a maximum-weight one-to-one matching (the Hungarian method on -weight, exact)."""
    if not n:
        return 0
    rows, cols = sorted({g for g, _ in n}), sorted({t for _, t in n})
    if len(rows) > len(cols):
        n, rows, cols = {(t, g): w for (g, t), w in n.items()}, cols, rows
    ri, ci = {g: k for k, g in enumerate(rows)}, {t: k for k, t in enumerate(cols)}
    R, C = len(rows), len(cols)
    cost = [[0] * C for _ in range(R)]
    for (g, t), w in n.items():
        cost[ri[g]][ci[t]] = -w
    inf = float("inf")
    u, v, p, way = [0] * (R + 1), [0] * (C + 1), [0] * (C + 1), [0] * (C + 1)
    for i in range(1, R + 1):
        p[0], j0 = i, 0
        minv, used = [inf] * (C + 1), [False] * (C + 1)
        while True:
            used[j0] = True
            i0, delta, j1, row = p[j0], inf, 0, cost[p[j0] - 1]
            for j in range(1, C + 1):
                if not used[j]:
                    cur = row[j - 1] - u[i0] - v[j]
                    if cur < minv[j]:
                        minv[j], way[j] = cur, j0
                    if minv[j] < delta:
                        delta, j1 = minv[j], j
            for j in range(C + 1):
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
    return -sum(cost[p[j] - 1][j - 1] for j in range(1, C + 1) if p[j])


def host_walk(lb, alpha):
    """One stream at one level, nothing removed -> 6 counters."""
    c, n = [0] * 6, {}

    def close():
        c[1] += 1; c[4] += max_weight(n); c[5] += len(n)
        n.clear()

    for f, (reset, labels, tracks, _, bests, ious) in enumerate(lb):
        if reset and f > 0:
            close()
        kept, seen = set(labels), set()
        for tid, best, v in zip(tracks, bests, ious):
            if best != -1 and best in kept and v >= alpha and (best, tid) not in seen:
                seen.add((best, tid))
                n[(best, tid)] = n.get((best, tid), 0) + 1
        c[0] += 1; c[2] += len(labels); c[3] += len(tracks)
    if lb:
        close()
    return c


def host_identity(logs, alphas):
    counters = np.zeros((len(alphas), len(logs), 6), dtype=np.int64)
    for a, alpha in enumerate(alphas):
        for b, lb in enumerate(logs):
            counters[a, b] = host_walk(lb, alpha)
    return counters


# ---- the dense clip (tests/_track_identity_util.py, dense_clip) -----------------------------------------------------------------------------
def dense_scorer(sticky, dev, n=32, frames=256, seed=11):
    """A one-stream scorer whose log holds the clip, written as rtk_track_score_logged packs it."""
    rng = np.random.default_rng(seed)
    sc = TS.TrackScorer(streams=1, max_objects=8, max_boxes=8, max_gt_tracks=1024, sweep_frames=frames, sweep_records=frames * n, device=dev)
    frame = np.zeros((1, frames, 4), np.int32)
    label, track, best = (np.zeros((1, frames * n), np.int32) for _ in range(3))
    for f in range(frames):
        perm = rng.permutation(n)
        frame[0, f] = (f * n, f * n, n + 65536 * int(f == 0), n)
        label[0, f * n:(f + 1) * n] = np.arange(n)
        for t in range(n):
            g = int(perm[t])
            if sticky:
                x = rng.random()
                g = t if x < 0.3 else (t + 1) % n if x < 0.3 + 0.7 * 0.4 else g
            track[0, f * n + t], best[0, f * n + t] = 100 + t, g
    sc.log_cursor.copy_(torch.tensor([[frames, frames * n, frames * n, 0]], dtype=torch.int32))
    sc.log_frame.copy_(torch.from_numpy(frame))
    sc.log_label.copy_(torch.from_numpy(label))
    sc.log_track.copy_(torch.from_numpy(track))
    sc.log_best.copy_(torch.from_numpy(best))
    sc.log_iou.fill_(0.9)
    return sc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--boxes", type=int, default=32)
    ap.add_argument("--max-objects", type=int, default=128)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--alphas", type=int, default=19)
    ap.add_argument("--out", default=os.path.join("profiles", "track_identity_timing.json"))
    a = ap.parse_args()
    dev = "cuda"
    B, N, K, KO, A = a.streams, a.points, a.boxes, a.max_objects, a.alphas
    d = synth.make_frame_pairs(B, N, case_id=1000)
    t = {k: torch.from_numpy(v).to(dev) for k, v in d.items()}
    per_stream = make_streams(d, B, N, K)
    bb = G.pack_boxes(per_stream, K, dev)
    types_d = TS.pack_box_types(per_stream, K, dev)
    idx = G.ground_truth(t["pc1"], t["pc2"], bb).box_index.cpu().numpy()
    obj, num, ids = np.full((B, N), -1, dtype=np.int32), np.zeros(B, dtype=np.int32), np.full((B, KO), -1, dtype=np.int32)
    for b in range(B):
        slots = sorted(set(idx[b][idx[b] >= 0].tolist()))
        for i, s in enumerate(slots):
            obj[b, idx[b] == s] = i
        num[b] = len(slots)
        ids[b, :len(slots)] = 100 + np.array(slots)
    obj_d, num_d, ids_d = (torch.from_numpy(x).to(dev) for x in (obj, num, ids))
    gobj = TS.gt_objects(t["pc1"], bb, types_d, min_obj_points=2)
    gobj.check()

    # ---- the log: time_track_hota.py's ----
    F, R = a.frames, a.frames * int(num.max())
    sc = TS.TrackScorer(streams=B, max_objects=KO, max_boxes=K, max_gt_tracks=1024, sweep_frames=F, sweep_records=R)
    gen = torch.Generator(dev).manual_seed(2)
    ids_f = ids_d.clone()
    for f in range(F):
        if f % 7 == 6:                                      # now and then some tracks change their id
            ids_f = torch.where((torch.rand(B, KO, device=dev, generator=gen) < 0.1) & (ids_f >= 0), ids_f + 1000, ids_f)
        reset = torch.full((B,), int(f % 100 == 0), dtype=torch.uint8, device=dev)
        drop = torch.rand(B, device=dev, generator=gen) < 0.2                       # a fifth of the frames lose their last detection
        sc.update_raw(t["pc1"], obj_d, torch.where(drop, (num_d - 1).clamp(min=0), num_d), ids_f, gobj, reset=reset,
                      object_conf=torch.rand(B, KO, device=dev, generator=gen))
    sc.check()
    levels = [k / (A + 1) for k in range(1, A + 1)]
    one = sc.identity()                                     # warm-up: the code object
    idn = sc.identity(alphas=levels)
    sc.hota(A)
    dense, sticky = dense_scorer(False, dev), dense_scorer(True, dev)
    d_one, s_one = dense.identity(), sticky.identity()

    # ---- the launches ----
    st = abi.stream()
    lg, no_cand = sc._log_block(), sc._log_block()
    best_off = torch.full_like(sc.log_best, -1)
    no_cand.rec_best = best_off.data_ptr()
    dlg, slg, dno = dense._log_block(), sticky._log_block(), dense._log_block()
    dbest_off = torch.full_like(dense.log_best, -1)
    dno.rec_best = dbest_off.data_ptr()
    flags = torch.zeros(B, dtype=torch.int32, device=dev)
    half = torch.full((1,), 0.5, dtype=torch.float64, device=dev)
    lv = torch.tensor(levels, dtype=torch.float64, device=dev)
    ic = torch.empty(A, B, 6, dtype=torch.int64, device=dev)
    hc = torch.empty(A, B, 6, dtype=torch.int64, device=dev)
    hq = torch.empty(A, B, 4, dtype=torch.float64, device=dev)
    id_fn, hota_fn = _lib._fn("rtk_score_identity"), _lib._fn("rtk_score_hota")
    ident = lambda streams, block, al, count: (lambda: id_fn(streams, sc.T, ctypes.addressof(block), None, None, al.data_ptr(), count, ic.data_ptr(),
                                                                flags.data_ptr(), st))
    variants = {
        "identity": ident(B, lg, half, 1),
        "identity_levels": ident(B, lg, lv, A),
        "hota": lambda: hota_fn(B, sc.T, ctypes.addressof(lg), None, None, A, hc.data_ptr(), hq.data_ptr(), flags.data_ptr(), st),
        "identity_no_candidates": ident(B, no_cand, lv, A),
        "dense": ident(1, dlg, half, 1),
        "dense_sticky": ident(1, slg, half, 1),
        "dense_no_candidates": ident(1, dno, half, 1),
    }
    runs = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            runs[k].append(block_us(fn, a.iters, a.warmup))
    assert int(flags.sum()) == 0, flags.tolist()
    s = summary(runs)

    # ---- the calls and the host statement ----
    walls = {"identity": [], "identity_levels": [], "hota": []}
    for _ in range(5):
        for k, fn in (("identity", lambda: sc.identity()), ("identity_levels", lambda: sc.identity(alphas=levels)), ("hota", lambda: sc.hota(A))):
            h0 = time.perf_counter()
            fn()
            walls[k].append(1e3 * (time.perf_counter() - h0))
    h0 = time.perf_counter()
    logs = host_log(sc)
    host = host_identity(logs, [0.5])
    host_ms = 1e3 * (time.perf_counter() - h0)
    host_all = host_identity(logs, levels)
    dense_host = {}
    for name, scorer, res in (("dense", dense, d_one), ("dense_sticky", sticky, s_one)):
        h0 = time.perf_counter()
        hcnt = host_identity(host_log(scorer), [0.5])
        dense_host[name] = dict(host_statement_ms=round(1e3 * (time.perf_counter() - h0), 1), pairs=int(res.pairs[0]), idtp=int(res.idtp[0]),
                                host_and_device_agree_exactly=bool(np.array_equal(res.counters, hcnt)),
                                solver_us=round(s[name]["median_us"] - s["dense_no_candidates"]["median_us"], 3))
    med = lambda k: statistics.median(walls[k])
    res = {"what": "the identity metrics over the scorer's log: the launch, the call, the host statement; HOTA over the same log as the yardstick; "
                   "the solver on a clip of 1024 pairs",
           "streams": B, "points": N, "boxes": K, "max_objects": KO, "iters": a.iters, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "frames_per_stream": F, "alphas": A, "logged_records": int(sc.log_cursor[:, 1].sum()),
           "lds_bytes": _lib._fn("rtk_score_identity_lds_bytes")(sc.T),
           "launches": s,
           "ratio_identity_levels_over_hota": round(s["identity_levels"]["median_us"] / s["hota"]["median_us"], 3),
           "pairs_and_solver_us_at_all_levels": round(s["identity_levels"]["median_us"] - s["identity_no_candidates"]["median_us"], 3),
           "call_ms_wall_median": {k: round(med(k), 3) for k in walls}, "call_ms_wall_runs": {k: [round(x, 3) for x in v] for k, v in walls.items()},
           "ratio_identity_levels_call_over_hota_call": round(med("identity_levels") / med("hota"), 3),
           "host_statement_ms": round(host_ms, 1), "ratio_host_over_identity_call": round(host_ms / med("identity"), 1),
           "host_and_device_agree_exactly": bool(np.array_equal(one.counters, host)),
           "host_and_device_agree_exactly_at_all_levels": bool(np.array_equal(idn.counters, host_all)),
           "dense_clips": dense_host,
           "idf1": float(one.idf1[0]), "idr": float(one.idr[0]), "idp": float(one.idp[0]), "idtp": idn.idtp.tolist(), "pairs": idn.pairs.tolist(),
           "clips": int(one.counters[0, :, 1].sum())}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
