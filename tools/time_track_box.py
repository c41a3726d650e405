"""The pair log under the oriented-box IoU (ratrack_amd/track_score.py `TrackScorer(similarity="box")` / `"box_bev"`;
csrc/track_score.hip): what the box launch costs per frame against `rtk_track_score_pairs_centre` and `rtk_track_score_pairs`, and
how many pairs each similarity logs.

    python tools/time_track_box.py [--streams 64] [--points 256] [--boxes 32] [--max-objects 128] [--iters 200] [--warmup 5] [--rounds 3]
                                   [--min-extent 0.2] [--out profiles/box_iou_timing.json]

The batch of tools/time_track_centre.py: one synthetic frame per stream, the detections the ground-truth clusters themselves, their boxes
fitted by `rtk_object_boxes` with --min-extent.  Measured on the machine it runs on, in one process, device time between events around
the entry point, medians of --iters after --warmup, --rounds rounds with the variants alternating inside every round, on the same
argument blocks, the cursors set back to 0 before every block so that every call logs its frame:

      score_pairs           `rtk_track_score_pairs`
      score_pairs_centre    `rtk_track_score_pairs_centre`
      score_pairs_box       `rtk_track_score_pairs_box`, RTK_SCORE_BOX_3D
      score_pairs_box_bev   `rtk_track_score_pairs_box`, RTK_SCORE_BOX_BEV

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

from ratrack_amd import _lib, abi, boxes as BX, gt_device as G, synth, track_score as TS  # noqa: E402
from time_track_score import make_streams  # noqa: E402
from time_track_sweep import block_us, summary  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--boxes", type=int, default=32)
    ap.add_argument("--max-objects", type=int, default=128)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-extent", type=float, default=0.2)
    ap.add_argument("--out", default=os.path.join("profiles", "box_iou_timing.json"))
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
    bx = BX.object_boxes_raw(t["pc1"], obj_d, num_d, KO, min_extent=a.min_extent)
    bx.check()

    F = a.iters + a.warmup
    R, Q = F * int(num.max()), F * int(num.max()) * int(gobj.count.max())
    mk = lambda **kw: TS.TrackScorer(streams=B, max_objects=KO, max_boxes=K, max_gt_tracks=1024, sweep_frames=F, sweep_records=R, sweep_pairs=Q, **kw)
    # how many pairs a frame logs under each similarity
    conf = torch.rand(B, KO, device=dev, generator=torch.Generator(dev).manual_seed(2))
    pairs = {}
    for name in TS.SIMILARITIES:
        sc = mk(similarity=name)
        sc.update_raw(t["pc1"], obj_d, num_d, ids_d, gobj, object_conf=conf, det_boxes=bx.box, det_box_valid=bx.valid)
        sc.check()
        pairs[name] = round(float(sc.pair_cursor.sum()) / B, 2)

    st, ad = abi.stream(), ctypes.addressof
    tm = mk(similarity="box")          # its blocks serve every launch: the plain one ignores pair_sim
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    outs = (i32(B, KO), i32(B, KO), i32(B, K), torch.empty(B, KO, dtype=torch.float64, device=dev), torch.empty(B, KO, KO, device=dev),
            torch.empty(B, dtype=torch.uint8, device=dev))
    blk_in = abi.ScoreIn(B, N, KO, K, tm.T, abi.view(t["pc1"]), obj_d.data_ptr(), num_d.data_ptr(), ids_d.data_ptr(), None, gobj.slot.data_ptr(),
                         gobj.label_id.data_ptr(), gobj.count.data_ptr(), gobj.size.data_ptr(), gobj.members.data_ptr(), None, None)
    blk_st = abi.ScoreState(*(getattr(tm, k).data_ptr() for k in ("counters", "iou_sum", "table_key", "table_last", "table_seen", "table_matched",
                                                                  "table_used", "prev_gt_id", "prev_count", "prev_gt", "flags")))
    blk_out = abi.ScoreOut(*(x.data_ptr() for x in outs))
    blk_lg, blk_pr = tm._log_block(conf.data_ptr()), tm._pair_block()
    centre_d, boxes_d = gobj.centre.contiguous(), gobj.boxes.contiguous()

    def per_frame(fn, *tail):
        def run():
            return fn(ad(blk_in), ad(blk_st), ad(blk_out), ad(blk_lg), None, ad(blk_pr), *tail, st)

        def block():
            tm.log_cursor.zero_()
            tm.pair_cursor.zero_()
            return block_us(run, a.iters, a.warmup)
        return block
    box_tail = (tm.pair_sim.data_ptr(), bx.box.data_ptr(), bx.valid.data_ptr(), boxes_d.data_ptr())
    variants = {"score_pairs": per_frame(_lib._fn("rtk_track_score_pairs")),
                "score_pairs_centre": per_frame(_lib._fn("rtk_track_score_pairs_centre"), tm.pair_sim.data_ptr(), centre_d.data_ptr(), 2.0),
                "score_pairs_box": per_frame(_lib._fn("rtk_track_score_pairs_box"), *box_tail, TS.BOX_MODES["box"]),
                "score_pairs_box_bev": per_frame(_lib._fn("rtk_track_score_pairs_box"), *box_tail, TS.BOX_MODES["box_bev"])}
    runs = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, block in variants.items():
            runs[k].append(block())
    assert int(tm.flags.sum()) == 0, tm.flags.tolist()
    s = summary(runs)
    med = lambda k: s[k]["median_us"]
    res = {"what": "rtk_track_score_pairs_box per launch against rtk_track_score_pairs_centre and rtk_track_score_pairs, on the same frame",
           "streams": B, "points": N, "boxes": K, "max_objects": KO, "iters": a.iters, "rounds": a.rounds, "min_extent": a.min_extent,
           "device": torch.cuda.get_device_name(0),
           "detections_per_frame": round(float(num.sum()) / B, 2), "kept_objects_per_frame": round(float(gobj.count.sum()) / B, 2),
           "detections_with_a_box_per_frame": round(float(((bx.valid > 0) & (bx.box[:, :, 4] > 0)).sum()) / B, 2),
           "pairs_per_frame": pairs,
           "launches": s,
           "ratio_box_over_centre": round(med("score_pairs_box") / med("score_pairs_centre"), 3),
           "ratio_box_bev_over_centre": round(med("score_pairs_box_bev") / med("score_pairs_centre"), 3),
           "ratio_box_over_pairs": round(med("score_pairs_box") / med("score_pairs"), 3),
           "box_extra_us_over_centre": round(med("score_pairs_box") - med("score_pairs_centre"), 3)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
