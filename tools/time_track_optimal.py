"""The pair log and the replay under the per-frame optimal matching (ratrack_amd/track_score.py `TrackScorer(sweep_pairs=...)`,
`sweep(matching="optimal")`; csrc/track_score.hip, csrc/track_optimal.hip): what logging the pairs costs per frame, and what the
optimal replay costs against the greedy one.

    python tools/time_track_optimal.py [--streams 64] [--points 256] [--boxes 32] [--max-objects 128] [--iters 50] [--warmup 5]
                                       [--rounds 3] [--frames 300] [--levels 40] [--min-iou 0.25] [--parent-lib PATH]
                                       [--out profiles/track_optimal_timing.json]

The log of tools/time_track_sweep.py, part (c): --streams x --frames frames of the batch of tools/time_track_score.py (seeded
confidences; track ids that change now and then; a reset every 100 frames), here with the pair log beside it.  Measured on the machine
it runs on, device time between events around the entry point, medians of --iters after --warmup, --rounds rounds with the variants
alternating inside every round:

  (a) per frame, on the same argument blocks, the cursors set back to 0 before every block so that every call logs its frame:
      score_logged          `rtk_track_score_logged`
      score_pairs           `rtk_track_score_pairs`: the same launch that also appends the frame's pairs
      score_logged_parent   `rtk_track_score_logged` of the library given as --parent-lib (the parent commit's build), when given
  (b) over the --levels + 1 thresholds of the sweep, every index replayed:
      replay                `rtk_score_replay` (the greedy rule)
      replay_optimal        `rtk_score_replay_optimal` at --min-iou
      replay_optimal_walk   the same with min_iou = 2, which no pair reaches: the walk, the pair reads and the track table, without edges
                            -- the difference to replay_optimal is the assignment (building the edges, the solve, reading it back)

Writes one JSON object to --out and prints it.  Not part of bench.py."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ratrack_amd import _lib, abi, gt_device as G, synth, track_score as TS  # noqa: E402
from time_track_score import make_streams  # noqa: E402
from time_track_sweep import block_us, summary  # noqa: E402


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
    ap.add_argument("--levels", type=int, default=40)
    ap.add_argument("--min-iou", type=float, default=0.25)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join("profiles", "track_optimal_timing.json"))
    a = ap.parse_args()
    dev = "cuda"
    B, N, K, KO, L = a.streams, a.points, a.boxes, a.max_objects, a.levels
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

    # ---- the two logs: time_track_sweep.py's part (c), with the pairs ----
    F, R = a.frames, a.frames * int(num.max())
    Q = 4 * R
    sc = TS.TrackScorer(streams=B, max_objects=KO, max_boxes=K, max_gt_tracks=1024, sweep_frames=F, sweep_records=R, sweep_pairs=Q)
    plain = TS.TrackScorer(streams=B, max_objects=KO, max_boxes=K, max_gt_tracks=1024, sweep_frames=F, sweep_records=R)
    gen = torch.Generator(dev).manual_seed(2)
    ids_f = ids_d.clone()
    for f in range(F):
        if f % 7 == 6:                                      # now and then some tracks change their id
            ids_f = torch.where((torch.rand(B, KO, device=dev, generator=gen) < 0.1) & (ids_f >= 0), ids_f + 1000, ids_f)
        reset = torch.full((B,), int(f % 100 == 0), dtype=torch.uint8, device=dev)
        drop = torch.rand(B, device=dev, generator=gen) < 0.2                       # a fifth of the frames lose their last detection
        conf = torch.rand(B, KO, device=dev, generator=gen)
        for s in (sc, plain):
            s.update_raw(t["pc1"], obj_d, torch.where(drop, (num_d - 1).clamp(min=0), num_d), ids_f, gobj, reset=reset, object_conf=conf)
    sc.check()
    same_log = all(torch.equal(getattr(sc, k), getattr(plain, k)) for k in ("counters", "log_cursor", "log_frame", "log_label", "log_track",
                                                                           "log_best", "log_conf", "log_iou"))
    sw_g = sc.sweep(L)
    sw_o = sc.sweep(L, matching="optimal", min_iou=a.min_iou)

    # ---- (a) the scoring launch, with and without the pairs ----
    st = abi.stream()
    tm = TS.TrackScorer(streams=B, max_objects=KO, max_boxes=K, max_gt_tracks=1024, sweep_frames=F, sweep_records=R, sweep_pairs=Q)
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    outs = (i32(B, KO), i32(B, KO), i32(B, K), torch.empty(B, KO, dtype=torch.float64, device=dev), torch.empty(B, KO, KO, device=dev),
            torch.empty(B, dtype=torch.uint8, device=dev))
    conf = torch.rand(B, KO, device=dev, generator=gen)
    blk_in = abi.ScoreIn(B, N, KO, K, tm.T, abi.view(t["pc1"]), obj_d.data_ptr(), num_d.data_ptr(), ids_d.data_ptr(), None, gobj.slot.data_ptr(),
                         gobj.label_id.data_ptr(), gobj.count.data_ptr(), gobj.size.data_ptr(), gobj.members.data_ptr(), None, None)
    blk_st = abi.ScoreState(*(getattr(tm, k).data_ptr() for k in ("counters", "iou_sum", "table_key", "table_last", "table_seen", "table_matched",
                                                                  "table_used", "prev_gt_id", "prev_count", "prev_gt", "flags")))
    blk_out = abi.ScoreOut(*(x.data_ptr() for x in outs))
    blk_lg, blk_pr = tm._log_block(conf.data_ptr()), tm._pair_block()
    ad = ctypes.addressof
    assert a.iters + a.warmup <= F, "every timed call must find room in the log"

    def per_frame(fn, *tail):
        def run():
            return fn(ad(blk_in), ad(blk_st), ad(blk_out), ad(blk_lg), *tail, st)

        def block():
            tm.log_cursor.zero_()
            tm.pair_cursor.zero_()
            return block_us(run, a.iters, a.warmup)
        return block
    frame_variants = {"score_logged": per_frame(_lib._fn("rtk_track_score_logged")),
                      "score_pairs": per_frame(_lib._fn("rtk_track_score_pairs"), None, ad(blk_pr))}
    if a.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        pfn = parent.rtk_track_score_logged
        pfn.argtypes, pfn.restype = abi.SIGNATURES["rtk_track_score_logged"], ctypes.c_int
        frame_variants["score_logged_parent"] = per_frame(pfn)

    # ---- (b) the replays over the sweep's thresholds ----
    lg, pr = sc._log_block(), sc._pair_block()
    score = torch.zeros(B, sc.R, dtype=torch.float64, device=dev)
    flags = torch.zeros(B, dtype=torch.int32, device=dev)
    _lib.call("rtk_score_track_means", B, ad(lg), score.data_ptr(), flags.data_ptr(), st)
    thr_g = torch.from_numpy(sw_g.thresholds.copy()).to(dev)
    thr_o = torch.from_numpy(sw_o.thresholds.copy()).to(dev)
    rc = torch.empty(L + 1, B, len(TS.COUNTERS), dtype=torch.int64, device=dev)
    oc = torch.empty(L + 1, B, len(TS.OPTIMAL_COUNTERS), dtype=torch.int64, device=dev)
    oq = torch.empty(L + 1, B, dtype=torch.int64, device=dev)
    rq = torch.empty(L + 1, B, dtype=torch.float64, device=dev)
    replay_fn, optimal_fn = _lib._fn("rtk_score_replay"), _lib._fn("rtk_score_replay_optimal")
    optimal_on = lambda m: (lambda: optimal_fn(B, sc.T, ad(lg), ad(pr), score.data_ptr(), thr_o.data_ptr(), None, L + 1, m, oc.data_ptr(),
                                                oq.data_ptr(), rq.data_ptr(), None, flags.data_ptr(), st))
    replay_variants = {
        "replay": lambda: block_us(lambda: replay_fn(B, sc.T, ad(lg), score.data_ptr(), thr_g.data_ptr(), None, L + 1, rc.data_ptr(), rq.data_ptr(),
                                                     None, st), a.iters, a.warmup),
        "replay_optimal": lambda: block_us(optimal_on(a.min_iou), a.iters, a.warmup),
        "replay_optimal_walk": lambda: block_us(optimal_on(2.0), a.iters, a.warmup),
    }
    variants = dict(frame_variants, **replay_variants)
    runs = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, block in variants.items():
            runs[k].append(block())
    assert int(flags.sum()) == 0 and int(tm.flags.sum()) == 0, (flags.tolist(), tm.flags.tolist())
    s = summary(runs)
    med = lambda k: s[k]["median_us"]
    res = {"what": "the pair log per frame against rtk_track_score_logged, and the replay under the per-frame optimal matching against the greedy replay",
           "streams": B, "points": N, "boxes": K, "max_objects": KO, "iters": a.iters, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "frames_per_stream": F, "levels": L, "min_iou": a.min_iou, "logged_records": int(sc.log_cursor[:, 1].sum()),
           "logged_pairs": int(sc.pair_cursor.sum()), "pairs_per_frame": round(float(sc.pair_cursor.sum()) / float(sc.log_cursor[:, 0].sum()), 2),
           "main_log_and_counters_equal_without_the_pair_log": bool(same_log),
           "launches": s,
           "ratio_pairs_over_logged": round(med("score_pairs") / med("score_logged"), 3),
           "pairs_extra_us_per_frame": round(med("score_pairs") - med("score_logged"), 3),
           "ratio_logged_over_parent": round(med("score_logged") / med("score_logged_parent"), 3) if a.parent_lib else None,
           "ratio_optimal_over_replay": round(med("replay_optimal") / med("replay"), 3),
           "assignment_share_of_optimal": round(1.0 - med("replay_optimal_walk") / med("replay_optimal"), 3),
           "levels_reached": {"greedy": sw_g.reached, "optimal": sw_o.reached},
           "greedy": {"amota": sw_g.amota, "samota": sw_g.samota, "amotp": sw_g.amotp, "tp": int(sw_g.tp[0]), "fp": int(sw_g.fp[0]),
                      "fn": int(sw_g.fn[0]), "idsw": int(sw_g.idsw[0])},
           "optimal": {"amota": sw_o.amota, "samota": sw_o.samota, "amotp": sw_o.amotp, "tp": int(sw_o.tp[0]), "fp": int(sw_o.fp[0]),
                       "fn": int(sw_o.fn[0]), "idsw": int(sw_o.idsw[0]), "frag": int(sw_o.frag[0])}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
