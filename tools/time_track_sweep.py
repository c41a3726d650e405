"""The per-frame log and the confidence sweep (ratrack_amd/track_score.py `TrackScorer.sweep`, csrc/track_sweep.hip): what the log
costs the scoring launch, and the sweep against its host statement.

    python tools/time_track_sweep.py [--streams 64] [--points 256] [--boxes 32] [--max-objects 128] [--iters 200] [--warmup 20]
                                     [--rounds 3] [--frames 300] [--levels 40] [--parent-lib PATH/librtk_hip.so]
                                     [--out profiles/track_sweep_timing.json]

The batch of tools/time_track_score.py (B synthetic frames, K boxes per frame on the clouds' own points, detections made from the
boxes' point sets).  Measured on the machine it runs on, device time between events around the entry point, medians of --iters after
--warmup, --rounds rounds with the variants alternating inside every round:

  (a) `rtk_track_score` of this tree against the same entry point of --parent-lib, a librtk_hip.so built from the parent commit
      (both fed the same argument blocks); without --parent-lib this part is reported as not measured;
  (b) `rtk_track_score_logged` against `rtk_track_score` (the log's cursors are set back before every timed block: no frame is
      refused for lack of room);
  (c) a log of --streams x --frames frames (the batch every frame; seeded confidences; track ids that change now and then; a reset
      every 100 frames), then `sweep(--levels)`: per launch (`_lib.TIMING`), the whole call with its download (wall clock around a
      call that ends in the download), and the host statement -- the definitions as Python loops over the downloaded log -- with
      the two compared for equality.

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


def block_us(fn, iters, warmup):
    """Median microseconds between events around fn."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    return round(1e3 * statistics.median(e0.elapsed_time(e1) for e0, e1 in pairs), 3)


def summary(runs):
    return {k: dict(rounds_us=v, median_us=round(statistics.median(v), 3), spread_us=round(max(v) - min(v), 3)) for k, v in runs.items()}


# ---- the host statement over a downloaded log (include/rtk_score.h) ---------------------------------------------------------------------
def host_log(scorer):
    get = lambda n: getattr(scorer, "log_" + n).cpu().numpy()
    cursor, frame, label, track, best, conf, iou = (get(n) for n in ("cursor", "frame", "label", "track", "best", "conf", "iou"))
    logs = []
    for b in range(scorer.B):
        lb = []
        for f in range(int(cursor[b, 0])):
            r, l, pz, g = (int(v) for v in frame[b, f])
            P = pz & 0xffff
            lb.append((bool(pz >> 16), label[b, l:l + g].tolist(), track[b, r:r + P].tolist(), conf[b, r:r + P].astype(np.float64).tolist(),
                       best[b, r:r + P].tolist(), iou[b, r:r + P].tolist()))
        logs.append(lb)
    return logs


def host_scores(lb):
    acc, clip = {}, 0
    for reset, _, tracks, confs, _, _ in lb:
        clip += int(reset)
        for tid, c in zip(tracks, confs):
            s = acc.setdefault((clip, tid), [0.0, 0])
            s[0] += c
            s[1] += 1
    per, clip = [], 0
    for reset, _, tracks, _, _, _ in lb:
        clip += int(reset)
        per.append([acc[(clip, tid)][0] / acc[(clip, tid)][1] for tid in tracks])
    return per


def _close(c, table):
    for _, seen, matched in table.values():
        r = matched / seen
        c[7] += 1
        c[8 if r > 0.8 else (10 if r < 0.2 else 9)] += 1
    table.clear()


def host_replay(lb, scores, tau, tp_scores=None):
    c, q, table = [0] * 11, 0.0, {}
    for (reset, labels, tracks, _, bests, ious), sc in zip(lb, scores):
        if reset:
            _close(c, table)
        taken, pred = {}, 0
        for tid, best, v, s in zip(tracks, bests, ious, sc):
            if s < tau:
                continue
            pred += 1
            if best == -1 or best in taken:
                continue
            taken[best] = tid
            q += v
            if tp_scores is not None:
                tp_scores.append(s)
        M = len(taken)
        c[0] += 1; c[1] += len(labels); c[2] += pred; c[3] += M; c[4] += pred - M; c[5] += len(labels) - M
        for lab in labels:
            e = table.setdefault(lab, [None, 0, 0])
            e[1] += 1
            if lab in taken:
                if e[0] is not None and e[0] != taken[lab]:
                    c[6] += 1
                e[0] = taken[lab]
                e[2] += 1
    _close(c, table)
    return c, q


def host_sweep(logs, L):
    B = len(logs)
    scores = [host_scores(lb) for lb in logs]
    pool, first = [], []
    for b in range(B):
        first.append(host_replay(logs[b], scores[b], -np.inf, pool))
    pool.sort(reverse=True)
    Gt, n, cur, walked = sum(c[1] for c, _ in first), len(pool), 0.0, []
    for i in range(n):
        l = (i + 1) / Gt
        r = (i + 2) / Gt if i < n - 1 else l
        if (r - cur) < (cur - l) and i < n - 1:
            continue
        walked.append(pool[i])
        cur += 1 / L
    reached = max(len(walked) - 1, 0)
    thr = np.array([-np.inf] + walked[1:] + [np.inf] * (L - reached))
    counters, sums = np.zeros((L + 1, B, 11), dtype=np.int64), np.zeros((L + 1, B))
    for k in range(reached + 1):
        for b in range(B):
            counters[k, b], sums[k, b] = host_replay(logs[b], scores[b], thr[k]) if k else first[b]
    return TS.sweep_values(counters, sums, thr, reached, L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--boxes", type=int, default=32)
    ap.add_argument("--max-objects", type=int, default=128)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--levels", type=int, default=40)
    ap.add_argument("--parent-lib", default=None, help="librtk_hip.so built from the parent commit, for (a)")
    ap.add_argument("--out", default=os.path.join("profiles", "track_sweep_timing.json"))
    a = ap.parse_args()
    dev = "cuda"
    B, N, K, KO = a.streams, a.points, a.boxes, a.max_objects
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
    conf_d = torch.rand(B, KO, device=dev, generator=torch.Generator(dev).manual_seed(1))
    res = {"what": "the scorer's per-frame log and the confidence sweep: cost of the log, sweep vs its host statement",
           "streams": B, "points": N, "boxes": K, "max_objects": KO, "iters": a.iters, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "gt_objects_kept": int(gobj.count.sum()), "detections": int(num.sum())}

    # ---- (a) + (b): the scoring launch -- this tree, the parent's library, the logged variant ----
    plain = TS.TrackScorer(streams=B, max_objects=KO, max_boxes=K, max_gt_tracks=1024)
    room = a.iters + a.warmup
    logged = TS.TrackScorer(streams=B, max_objects=KO, max_boxes=K, max_gt_tracks=1024, sweep_frames=room, sweep_records=room * int(num.max()))
    # the argument blocks of one unlogged call, built once and handed to both libraries (the tensors they point into stay alive)
    i32 = lambda *sh: torch.empty(*sh, dtype=torch.int32, device=dev)
    outs = [i32(B, KO), i32(B, KO), i32(B, K), torch.empty(B, KO, dtype=torch.float64, device=dev), torch.empty(B, KO, KO, device=dev),
            torch.empty(B, dtype=torch.uint8, device=dev)]
    blk_in = abi.ScoreIn(B, N, KO, K, plain.T, abi.view(t["pc1"]), obj_d.data_ptr(), num_d.data_ptr(), ids_d.data_ptr(), None,
                         gobj.slot.data_ptr(), gobj.label_id.data_ptr(), gobj.count.data_ptr(), gobj.size.data_ptr(), gobj.members.data_ptr(),
                         None, None)
    blk_st = abi.ScoreState(*[getattr(plain, n).data_ptr() for n, _ in abi.ScoreState._fields_])
    blk_out = abi.ScoreOut(*[x.data_ptr() for x in outs])
    args = (ctypes.addressof(blk_in), ctypes.addressof(blk_st), ctypes.addressof(blk_out), abi.stream())
    this_fn = _lib._fn("rtk_track_score")
    variants = {"this_tree": lambda: this_fn(*args)}
    if a.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        parent.rtk_track_score.argtypes, parent.rtk_track_score.restype = [ctypes.c_void_p] * 4, ctypes.c_int
        assert not hasattr(parent, "rtk_track_score_logged"), "--parent-lib exports the logged entry point: not the parent's library"
        variants["parent"] = lambda: parent.rtk_track_score(*args)

    def logged_call():
        logged.update_raw(t["pc1"], obj_d, num_d, ids_d, gobj, object_conf=conf_d)

    def logged_block():                                     # one timed block never runs out of room
        logged.log_cursor.zero_()
        return logged_call
    runs = {k: [] for k in list(variants) + ["update_raw_unlogged", "update_raw_logged"]}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            runs[k].append(block_us(fn, a.iters, a.warmup))
        runs["update_raw_unlogged"].append(block_us(lambda: plain.update_raw(t["pc1"], obj_d, num_d, ids_d, gobj), a.iters, a.warmup))
        runs["update_raw_logged"].append(block_us(logged_block(), a.iters, a.warmup))
    logged.check()
    s = summary(runs)
    res["a_rtk_track_score_entry_point"] = {k: s[k] for k in variants}
    if a.parent_lib:
        diff = round(s["this_tree"]["median_us"] - s["parent"]["median_us"], 3)
        res["a_this_minus_parent_us"] = diff
        res["a_within_parent_spread"] = bool(diff <= s["parent"]["spread_us"])
    else:
        res["a_this_minus_parent_us"] = "not measured (no --parent-lib)"
    res["b_update_raw_call"] = {k: s[k] for k in ("update_raw_unlogged", "update_raw_logged")}
    res["b_log_cost_us"] = round(s["update_raw_logged"]["median_us"] - s["update_raw_unlogged"]["median_us"], 3)

    # ---- (c) the sweep over --frames frames of every stream ----
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
    sw = sc.sweep(a.levels)                                 # warm-up: code objects, the sort's workspace
    torch.cuda.synchronize()
    walls = []
    for _ in range(5):
        h0 = time.perf_counter()
        sw = sc.sweep(a.levels)
        walls.append(1e3 * (time.perf_counter() - h0))
    _lib.TIMING = []
    sc.sweep(a.levels)
    torch.cuda.synchronize()
    launches = [(name, round(1e3 * e0.elapsed_time(e1), 1)) for name, e0, e1 in _lib.TIMING]
    _lib.TIMING = None
    h0 = time.perf_counter()
    logs = host_log(sc)
    host = host_sweep(logs, a.levels)
    host_ms = 1e3 * (time.perf_counter() - h0)
    agree = bool(np.array_equal(sw.counters, host["counters"]) and np.array_equal(sw.iou_sums.view(np.int64), host["iou_sums"].view(np.int64)) and
                 np.array_equal(sw.thresholds.view(np.int64), host["thresholds"].view(np.int64)) and sw.reached == host["reached"] and
                 sw.amota == host["amota"] and sw.samota == host["samota"] and sw.amotp == host["amotp"])
    res.update({"c_frames_per_stream": F, "c_levels": a.levels, "c_logged_records": int(sc.log_cursor[:, 1].sum()),
                "c_true_positives_unfiltered": sw.unfiltered["tp"], "c_levels_reached": sw.reached,
                "c_amota": sw.amota, "c_samota": sw.samota, "c_amotp": sw.amotp,
                "c_sweep_launches_us_in_call_order": launches, "c_sweep_launches_us_sum": round(sum(v for _, v in launches), 1),
                "c_sweep_call_ms_wall_median": round(statistics.median(walls), 3), "c_sweep_call_ms_wall_runs": [round(x, 3) for x in walls],
                "c_host_statement_ms": round(host_ms, 1), "c_ratio_host_over_sweep_call": round(host_ms / statistics.median(walls), 1),
                "c_host_and_device_agree_exactly": agree})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
