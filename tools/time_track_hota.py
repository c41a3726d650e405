"""HOTA over the scorer's log (ratrack_amd/track_score.py `TrackScorer.hota`, csrc/track_hota.hip): the launch, the whole call and
the host statement, with the sweep's replay over the same log for scale.

    python tools/time_track_hota.py [--streams 64] [--points 256] [--boxes 32] [--max-objects 128] [--iters 50] [--warmup 5]
                                    [--rounds 3] [--frames 300] [--alphas 19] [--levels 40] [--out profiles/track_hota_timing.json]

The log of tools/time_track_sweep.py, part (c): --streams x --frames frames of the batch of tools/time_track_score.py (seeded
confidences; track ids that change now and then; a reset every 100 frames).  Measured on the machine it runs on, device time between
events around the entry point, medians of --iters after --warmup, --rounds rounds with the variants alternating inside every round:

  hota               `rtk_score_hota`, --alphas levels, nothing removed (one launch, grid streams x alphas)
  hota_threshold     the same with the track scores and the sweep's best threshold (the scores computed outside the timed block)
  replay             `rtk_score_replay` over the --levels + 1 thresholds of the sweep on the same log, every index replayed: the
                     scale HOTA is expected to be of, since --alphas workgroups per stream do the same walk plus a pair table
  hota_no_candidates `rtk_score_hota` on a copy of the log whose detections have no best label: the walk and the track table,
                     without the greedy matches, the pair list and the association sums
  hota_no_detections on a copy whose frames hold no detection: the walk and the label table alone

and, wall clock, `hota()` end to end (the call ends in its download) and the host statement -- the header's definitions as Python
loops over the downloaded log -- with the two compared for equality.

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
from time_track_sweep import block_us, host_log, host_scores, summary  # noqa: E402


# ---- the host statement over a downloaded log (include/rtk_score.h) ---------------------------------------------------------------------
def host_walk(lb, scores, tau, alpha):
    """One stream at one level -> (6 counters, 4 sums)."""
    c, s = [0] * 6, [0.0] * 4
    cg, ct, n = {}, {}, {}

    def close():
        c[1] += 1; c[5] += len(n)
        for (lab, tid), m in n.items():                     # insertion order: the order of first appearance
            N = float(m * m)
            s[0] += N / float(cg[lab] + ct[tid] - m)
            s[1] += N / float(cg[lab])
            s[2] += N / float(ct[tid])
        cg.clear(); ct.clear(); n.clear()

    for f, ((reset, labels, tracks, _, bests, ious), sc) in enumerate(zip(lb, scores)):
        if reset and f > 0:
            close()
        taken = set()
        for lab in labels:
            cg[lab] = cg.get(lab, 0) + 1
        for tid, best, v, x in zip(tracks, bests, ious, sc):
            if x < tau:
                continue
            ct[tid] = ct.get(tid, 0) + 1
            c[3] += 1
            if best == -1 or not v >= alpha or best in taken:
                continue
            taken.add(best)
            n[(best, tid)] = n.get((best, tid), 0) + 1
            s[3] += v
            c[4] += 1
        c[0] += 1; c[2] += len(labels)
    if lb:
        close()
    return c, s


def host_hota(logs, scores, tau, A):
    B = len(logs)
    counters, sums = np.zeros((A, B, 6), dtype=np.int64), np.zeros((A, B, 4))
    for a in range(A):
        alpha = (a + 1) / (A + 1)
        for b in range(B):
            counters[a, b], sums[a, b] = host_walk(logs[b], scores[b], tau, alpha)
    return TS.hota_values(counters, sums)


def agree(ho, host):
    means = ("hota", "deta_mean", "assa_mean", "detre_mean", "detpr_mean", "assre_mean", "asspr_mean", "loca_mean")
    return bool(np.array_equal(ho.counters, host["counters"]) and np.array_equal(ho.sums.view(np.int64), host["sums"].view(np.int64)) and
                all(getattr(ho, k) == host[k] for k in means))


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
    ap.add_argument("--levels", type=int, default=40)
    ap.add_argument("--out", default=os.path.join("profiles", "track_hota_timing.json"))
    a = ap.parse_args()
    dev = "cuda"
    B, N, K, KO, A, L = a.streams, a.points, a.boxes, a.max_objects, a.alphas, a.levels
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

    # ---- the log: time_track_sweep.py's part (c) ----
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
    sw = sc.sweep(L)
    ho = sc.hota(A)                                         # warm-up: the code object
    tau = sw.best["threshold"] if sw.best is not None else float("-inf")
    ho_t = sc.hota(A, threshold=tau)

    # ---- the launches ----
    st = abi.stream()
    lg = sc._log_block()
    score = torch.zeros(B, sc.R, dtype=torch.float64, device=dev)
    flags = torch.zeros(B, dtype=torch.int32, device=dev)
    _lib.call("rtk_score_track_means", B, ctypes.addressof(lg), score.data_ptr(), flags.data_ptr(), st)
    thr_one = torch.full((1,), tau, dtype=torch.float64, device=dev)
    thr_all = torch.from_numpy(sw.thresholds.copy()).to(dev)
    hc = torch.empty(A, B, 6, dtype=torch.int64, device=dev)
    hq = torch.empty(A, B, 4, dtype=torch.float64, device=dev)
    rc = torch.empty(L + 1, B, len(TS.COUNTERS), dtype=torch.int64, device=dev)
    rq = torch.empty(L + 1, B, dtype=torch.float64, device=dev)
    # copies of the log with a phase switched off through the inputs
    no_cand, no_det = sc._log_block(), sc._log_block()
    best_off = torch.full_like(sc.log_best, -1)
    frame_off = sc.log_frame.clone()
    frame_off[:, :, 2] &= 65536                             # P = 0 in every frame, the clip marks stay
    no_cand.rec_best, no_det.frame = best_off.data_ptr(), frame_off.data_ptr()
    hota_fn, replay_fn = _lib._fn("rtk_score_hota"), _lib._fn("rtk_score_replay")
    hota_on = lambda block, s, th: (lambda: hota_fn(B, sc.T, ctypes.addressof(block), s, th, A, hc.data_ptr(), hq.data_ptr(), flags.data_ptr(), st))
    variants = {
        "hota": hota_on(lg, None, None),
        "hota_threshold": hota_on(lg, score.data_ptr(), thr_one.data_ptr()),
        "replay": lambda: replay_fn(B, sc.T, ctypes.addressof(lg), score.data_ptr(), thr_all.data_ptr(), None, L + 1, rc.data_ptr(), rq.data_ptr(),
                                    None, st),
        "hota_no_candidates": hota_on(no_cand, None, None),
        "hota_no_detections": hota_on(no_det, None, None),
    }
    runs = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            runs[k].append(block_us(fn, a.iters, a.warmup))
    assert int(flags.sum()) == 0, flags.tolist()
    s = summary(runs)

    # ---- the call and the host statement ----
    walls = []
    for _ in range(5):
        h0 = time.perf_counter()
        ho = sc.hota(A)
        walls.append(1e3 * (time.perf_counter() - h0))
    h0 = time.perf_counter()
    logs = host_log(sc)
    plain = [[[0.0] * len(fr[2]) for fr in lb] for lb in logs]
    host = host_hota(logs, plain, -np.inf, A)
    host_ms = 1e3 * (time.perf_counter() - h0)
    host_t = host_hota(logs, [host_scores(lb) for lb in logs], tau, A)
    res = {"what": "HOTA over the scorer's log: the launch, the call, the host statement; the sweep's replay over the same log for scale",
           "streams": B, "points": N, "boxes": K, "max_objects": KO, "iters": a.iters, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "frames_per_stream": F, "alphas": A, "levels": L, "levels_reached": sw.reached,
           "logged_records": int(sc.log_cursor[:, 1].sum()), "threshold": tau,
           "launches": s,
           "ratio_hota_over_replay": round(s["hota"]["median_us"] / s["replay"]["median_us"], 3),
           "ratio_per_workgroup_hota_over_replay": round(s["hota"]["median_us"] / A / (s["replay"]["median_us"] / (L + 1)), 3),
           "hota_call_ms_wall_median": round(statistics.median(walls), 3), "hota_call_ms_wall_runs": [round(x, 3) for x in walls],
           "host_statement_ms": round(host_ms, 1), "ratio_host_over_hota_call": round(host_ms / statistics.median(walls), 1),
           "host_and_device_agree_exactly": agree(ho, host), "host_and_device_agree_exactly_at_threshold": agree(ho_t, host_t),
           "hota": ho.hota, "deta": ho.deta_mean, "assa": ho.assa_mean, "loca": ho.loca_mean, "tp": ho.tp.tolist(), "pairs": ho.pairs.tolist(),
           "hota_at_threshold": ho_t.hota, "assa_at_threshold": ho_t.assa_mean}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
