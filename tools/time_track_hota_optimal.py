"""HOTA under the optimal matching and the identity metrics over every pair (ratrack_amd/track_score.py
`TrackScorer.hota(matching="optimal")`, `TrackScorer.identity(pairs="all")`; csrc/track_hota_optimal.hip, csrc/track_identity_pairs.hip)
against the greedy calls they stand beside and against their host statements.

    python tools/time_track_hota_optimal.py [--streams 64] [--points 256] [--boxes 32] [--max-objects 128] [--iters 50] [--warmup 5]
                                            [--rounds 3] [--frames 300] [--alphas 19] [--host-streams 8]
                                            [--out profiles/hota_optimal_timing.json]

The log of tools/time_track_hota.py (--streams x --frames frames of the batch of tools/time_track_score.py; seeded confidences; track
ids that change now and then; a reset every 100 frames), written with `sweep_pairs` on.  Measured on the machine it runs on, device
time between events around the entry points, medians of --iters after --warmup, --rounds rounds with the variants alternating inside
every round:

  hota                 `rtk_score_hota`, --alphas levels, nothing removed (the greedy rule; grid streams x alphas)
  alignment            `rtk_score_alignment` (grid streams: one wave per stream)
  hota_optimal_match   `rtk_score_hota_optimal` on the alignment's tables (grid streams x alphas: every level solves every frame)
  hota_optimal_one     the same launch with ONE level: one solve per frame and stream -- what the levels would share
  hota_optimal         the two launches of `hota(matching="optimal")`, back to back
  identity             `rtk_score_identity` at the single level 0.5
  identity_pairs       `rtk_score_identity_pairs` at the single level 0.5

and, wall clock, the four calls end to end (each ends in its download) and the two host statements -- the header's definitions as Python
loops over the downloaded logs of the first --host-streams streams, compared with the device's numbers of those streams for equality.

Writes one JSON object to --out and prints it.  Not part of bench.py."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ratrack_amd import _lib, abi, gt_device as G, synth, track_score as TS  # noqa: E402
from time_track_identity import max_weight  # noqa: E402
from time_track_score import make_streams  # noqa: E402
from time_track_sweep import block_us, summary  # noqa: E402

INF = 0x7fffffff
ONE = float(1 << 28)


# ---- the host statements over the downloaded logs (include/rtk_score.h, at the end) ----------------------------------------------------
def host_logs(scorer, streams):
    """-> per stream the frames: (reset, labels, tracks, [(i, j, s)] valid pairs in pair-log order; nothing is removed)."""
    get = lambda n: getattr(scorer, n)[:streams].cpu().numpy()
    cursor, frame, label, track, pframe, pkey, pcommon, size, lsize = (get(n) for n in (
        "log_cursor", "log_frame", "log_label", "log_track", "pair_frame", "pair_key", "pair_common", "log_size", "log_label_size"))
    logs = []
    for b in range(streams):
        lb = []
        for f in range(int(cursor[b, 0])):
            r, l, pz, g = (int(v) for v in frame[b, f])
            P, (q, nq) = pz & 0xffff, (int(v) for v in pframe[b, f])
            pairs = []
            for key, c in zip(pkey[b, q:q + nq].tolist(), pcommon[b, q:q + nq].tolist()):
                i, j = key >> 8, key & 255
                den = int(size[b, r + i]) + int(lsize[b, l + j]) - c if key >= 0 and i < P and j < g else 0
                if c > 0 and den > 0:
                    pairs.append((i, j, float(c) / float(den)))
            lb.append((bool(pz >> 16), label[b, l:l + g].tolist(), track[b, r:r + P].tolist(), pairs))
        logs.append(lb)
    return logs


def la_solve(R, C, edges):
    """csrc/lds_assignment.h restated: rows enter in order, the nearest column wins, ties go to the smaller index -> cp."""
    adj = [[] for _ in range(R)]
    for r, c, w in edges:
        adj[r].append((c, w))
    u, v, cp, way = [0] * R, [0] * C, [-1] * C, [-1] * C
    for r in range(R):
        if not adj[r]:
            continue
        u[r] = -max([0] + [w + v[c] for c, w in adj[r]])
        dist, done = [INF] * C, [False] * C
        i, base, jin, dd, jdd, D, jend = r, 0, -1, INF, -1, 0, -1
        for _ in range(C + 1):
            ui = u[i]
            if base - ui < dd:
                dd, jdd = base - ui, jin
            for c, w in adj[i]:
                if not done[c] and base + (-w - ui - v[c]) < dist[c]:
                    dist[c], way[c] = base + (-w - ui - v[c]), jin
            d, j = min(((dist[k], k) for k in range(C) if not done[k] and dist[k] != INF), default=(INF, -1))
            if d == INF or dd <= d:
                D, jend = dd, jdd
                break
            owner, done[j] = cp[j], True
            if owner < 0:
                D, jend = d, j
                break
            i, base, jin = owner, d, j
        for j in range(C):
            if done[j]:
                v[j] -= D - dist[j]
                if cp[j] >= 0:
                    u[cp[j]] += D - dist[j]
        u[r] += D
        j, step = jend, 0
        while step < C and j >= 0:
            cp[j] = r if way[j] < 0 else cp[way[j]]
            j, step = way[j], step + 1
    return cp


def clips_of(lb):
    clips = []
    for f, fr in enumerate(lb):
        if f == 0 or fr[0]:
            clips.append([])
        clips[-1].append(fr)
    return clips


def host_hota_optimal(logs, A):
    """-> counters (A,B,6), sums (A,B,4)."""
    B = len(logs)
    counters, sums = np.zeros((A, B, 6), dtype=np.int64), np.zeros((A, B, 4))
    levels = [(a + 1) / (A + 1) for a in range(A)]
    for b, lb in enumerate(logs):
        c, s = [[0] * 6 for _ in levels], [[0.0] * 4 for _ in levels]
        for clip in clips_of(lb):
            pmc, cg, ct = {}, {}, {}
            for _, labels, tracks, pairs in clip:
                r, k = {}, {}
                for i, j, v in pairs:
                    r[i] = r.get(i, 0.0) + min(v, 1.0)
                    k[j] = k.get(j, 0.0) + min(v, 1.0)
                for i, j, v in pairs:
                    sb = min(v, 1.0)
                    pmc[(labels[j], tracks[i])] = pmc.get((labels[j], tracks[i]), 0.0) + sb / ((r[i] + k[j]) - sb)
                for g in labels:
                    cg[g] = cg.get(g, 0) + 1
                for t in tracks:
                    ct[t] = ct.get(t, 0) + 1
            al = {(g, t): m / (float(cg[g] + ct[t]) - m) for (g, t), m in pmc.items()}
            n = [dict() for _ in levels]
            for _, labels, tracks, pairs in clip:
                edges = [(i, j, max(1, int(math.floor(min(al[(labels[j], tracks[i])] * min(v, 1.0), 1.0) * ONE)))) for i, j, v in pairs]
                cp, sim = la_solve(len(tracks), len(labels), edges), {(i, j): v for i, j, v in pairs}
                for a, alpha in enumerate(levels):
                    for j, i in enumerate(cp):
                        if i >= 0 and sim[(i, j)] >= alpha:
                            n[a][(labels[j], tracks[i])] = n[a].get((labels[j], tracks[i]), 0) + 1
                            c[a][4] += 1
                            s[a][3] += sim[(i, j)]
            for a in range(A):
                c[a][0] += len(clip); c[a][1] += 1; c[a][2] += sum(cg.values()); c[a][3] += sum(ct.values())
                for (g, t) in pmc:                           # insertion order: first appearance among the valid pairs
                    m = n[a].get((g, t), 0)
                    if m:
                        N = float(m * m)
                        s[a][0] += N / float(cg[g] + ct[t] - m)
                        s[a][1] += N / float(cg[g])
                        s[a][2] += N / float(ct[t])
                        c[a][5] += 1
        for a in range(A):
            counters[a, b], sums[a, b] = c[a], s[a]
    return counters, sums


def host_identity_pairs(logs, alpha):
    counters = np.zeros((1, len(logs), 6), dtype=np.int64)
    for b, lb in enumerate(logs):
        for clip in clips_of(lb):
            n = {}
            for _, labels, tracks, pairs in clip:
                for key in dict.fromkeys((labels[j], tracks[i]) for i, j, v in pairs if v >= alpha):
                    n[key] = n.get(key, 0) + 1
            counters[0, b] += (len(clip), 1, sum(len(fr[1]) for fr in clip), sum(len(fr[2]) for fr in clip), max_weight(n), len(n))
    return counters


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
    ap.add_argument("--host-streams", type=int, default=8)
    ap.add_argument("--out", default=os.path.join("profiles", "hota_optimal_timing.json"))
    a = ap.parse_args()
    dev = "cuda"
    B, N, K, KO, A = a.streams, a.points, a.boxes, a.max_objects, a.alphas
    HB = min(a.host_streams, B)
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

    # ---- the two logs: time_track_hota.py's, with the pairs ----
    F, R = a.frames, a.frames * int(num.max())
    Q = 4 * R
    sc = TS.TrackScorer(streams=B, max_objects=KO, max_boxes=K, max_gt_tracks=1024, sweep_frames=F, sweep_records=R, sweep_pairs=Q)
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
    calls = {"hota": lambda: sc.hota(A), "hota_optimal": lambda: sc.hota(A, matching="optimal"), "identity": lambda: sc.identity(),
             "identity_pairs": lambda: sc.identity(pairs="all")}
    first = {k: fn() for k, fn in calls.items()}            # warm-up: the code objects

    # ---- the launches ----
    st, ad = abi.stream(), ctypes.addressof
    lg, pr = sc._log_block(), sc._pair_block()
    flags = torch.zeros(B, dtype=torch.int32, device=dev)
    hc = torch.empty(A, B, 6, dtype=torch.int64, device=dev)
    hq = torch.empty(A, B, 4, dtype=torch.float64, device=dev)
    ic = torch.empty(1, B, 6, dtype=torch.int64, device=dev)
    half = torch.full((1,), 0.5, dtype=torch.float64, device=dev)
    pair_a = torch.empty(B, sc.Q, dtype=torch.float64, device=dev)
    pair_index, clip_cg, clip_ct = (torch.empty(B, sc.Q, dtype=torch.int32, device=dev) for _ in range(3))
    hota_fn, align_fn, match_fn = _lib._fn("rtk_score_hota"), _lib._fn("rtk_score_alignment"), _lib._fn("rtk_score_hota_optimal")
    id_fn, idp_fn = _lib._fn("rtk_score_identity"), _lib._fn("rtk_score_identity_pairs")
    align = lambda: align_fn(B, sc.T, ad(lg), ad(pr), None, None, pair_a.data_ptr(), pair_index.data_ptr(), clip_cg.data_ptr(), clip_ct.data_ptr(),
                             flags.data_ptr(), st)
    match = lambda levels: (lambda: match_fn(B, ad(lg), ad(pr), None, None, levels, pair_a.data_ptr(), pair_index.data_ptr(), clip_cg.data_ptr(),
                                             clip_ct.data_ptr(), hc.data_ptr(), hq.data_ptr(), flags.data_ptr(), st))
    align()
    variants = {
        "hota": lambda: hota_fn(B, sc.T, ad(lg), None, None, A, hc.data_ptr(), hq.data_ptr(), flags.data_ptr(), st),
        "alignment": align,
        "hota_optimal_match": match(A),
        "hota_optimal_one": match(1),
        "hota_optimal": lambda: (align(), match(A)()),
        "identity": lambda: id_fn(B, sc.T, ad(lg), None, None, half.data_ptr(), 1, ic.data_ptr(), flags.data_ptr(), st),
        "identity_pairs": lambda: idp_fn(B, sc.T, ad(lg), ad(pr), None, None, half.data_ptr(), 1, ic.data_ptr(), flags.data_ptr(), st),
    }
    runs = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            runs[k].append(block_us(fn, a.iters, a.warmup))
    assert int(flags.sum()) == 0, flags.tolist()
    s = summary(runs)
    med = lambda k: s[k]["median_us"]

    # ---- the calls and the host statements ----
    walls = {k: [] for k in calls}
    for _ in range(5):
        for k, fn in calls.items():
            h0 = time.perf_counter()
            fn()
            walls[k].append(1e3 * (time.perf_counter() - h0))
    wall = {k: round(statistics.median(v), 3) for k, v in walls.items()}
    h0 = time.perf_counter()
    logs = host_logs(sc, HB)
    log_ms = 1e3 * (time.perf_counter() - h0)
    h0 = time.perf_counter()
    hcn, hsm = host_hota_optimal(logs, A)
    hota_host_ms = 1e3 * (time.perf_counter() - h0)
    h0 = time.perf_counter()
    icn = host_identity_pairs(logs, 0.5)
    id_host_ms = 1e3 * (time.perf_counter() - h0)
    ho, idp = first["hota_optimal"], first["identity_pairs"]
    scale = B / HB
    res = {"what": "HOTA under the optimal matching and the identity metrics over every pair: the launches, the calls and the host statements, "
                   "beside the greedy calls over the same log",
           "streams": B, "points": N, "boxes": K, "max_objects": KO, "iters": a.iters, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "frames_per_stream": F, "alphas": A, "logged_records": int(sc.log_cursor[:, 1].sum()), "logged_pairs": int(sc.pair_cursor.sum()),
           "pairs_per_frame": round(float(sc.pair_cursor.sum()) / float(sc.log_cursor[:, 0].sum()), 2),
           "lds_bytes": {"alignment": _lib._fn("rtk_score_alignment_lds_bytes")(sc.T), "identity_pairs": _lib._fn("rtk_score_identity_pairs_lds_bytes")(sc.T)},
           "launches": s,
           "ratio_hota_optimal_over_hota": round(med("hota_optimal") / med("hota"), 3),
           "ratio_identity_pairs_over_identity": round(med("identity_pairs") / med("identity"), 3),
           "alignment_share_of_hota_optimal": round(med("alignment") / med("hota_optimal"), 3),
           "ratio_match_all_levels_over_one_level": round(med("hota_optimal_match") / med("hota_optimal_one"), 3),
           "call_ms_wall_median": wall, "call_ms_wall_runs": {k: [round(x, 3) for x in v] for k, v in walls.items()},
           "host_statement_streams": HB, "host_log_decode_ms": round(log_ms, 1),
           "host_statement_ms": {"hota_optimal": round(hota_host_ms, 1), "identity_pairs": round(id_host_ms, 1)},
           "host_statement_ms_scaled_to_all_streams": {"hota_optimal": round(hota_host_ms * scale, 1), "identity_pairs": round(id_host_ms * scale, 1)},
           "ratio_host_over_call": {"hota_optimal": round(hota_host_ms * scale / wall["hota_optimal"], 1),
                                    "identity_pairs": round(id_host_ms * scale / wall["identity_pairs"], 1)},
           "host_and_device_agree_exactly": {
               "hota_optimal": bool(np.array_equal(ho.counters[:, :HB], hcn) and np.array_equal(ho.sums[:, :HB].view(np.int64), hsm.view(np.int64))),
               "identity_pairs": bool(np.array_equal(idp.counters[:, :HB], icn))},
           "hota": {"greedy": first["hota"].hota, "optimal": ho.hota}, "assa": {"greedy": first["hota"].assa_mean, "optimal": ho.assa_mean},
           "deta": {"greedy": first["hota"].deta_mean, "optimal": ho.deta_mean}, "loca": {"greedy": first["hota"].loca_mean, "optimal": ho.loca_mean},
           "tp": {"greedy": first["hota"].tp.tolist(), "optimal": ho.tp.tolist()},
           "idf1": {"best": float(first["identity"].idf1[0]), "all": float(idp.idf1[0])},
           "idtp": {"best": int(first["identity"].idtp[0]), "all": int(idp.idtp[0])}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
