"""The pair log under TrackEval's centre-distance similarity (ratrack_amd/track_score.py `TrackScorer(similarity="centre")`;
csrc/track_score.hip and the replays' files): what the centre launch costs per frame against `rtk_track_score_pairs`, what the
four replays cost on a centre log against an IoU log of the same frames, and how many pairs each similarity logs.

    python tools/time_track_centre.py [--streams 64] [--points 256] [--boxes 32] [--max-objects 128] [--iters 200] [--replay-iters 50]
                                      [--warmup 5] [--rounds 3] [--frames 300] [--levels 40] [--min-iou 0.25] [--zero-distance 2.0] [--parent-lib PATH]
                                      [--out profiles/track_centre_timing.json]

The batch and the log of tools/time_track_optimal.py (--streams x --frames frames; seeded confidences; track ids that change now and
then; a reset every 100 frames), fed to an "iou" scorer and to a "centre" scorer.  Measured on the machine it runs on, in one process,
device time between events around the entry point, medians of --iters (the replays: --replay-iters) after --warmup, --rounds rounds with the variants alternating
inside every round:

  (a) per frame, on the same argument blocks, the cursors set back to 0 before every block so that every call logs its frame:
      score_pairs           `rtk_track_score_pairs`
      score_pairs_centre    `rtk_track_score_pairs_centre`
      score_pairs_parent    `rtk_track_score_pairs` of the library given as --parent-lib (the parent commit's build), when given
  (b) the four replays, each on the IoU log (`iou/...`) and on the centre log (`centre/...`, the *_sim entry points):
      replay_optimal        over the --levels + 1 thresholds of that log's sweep, at --min-iou
      alignment             the alignment pass
      hota_optimal          19 levels
      identity_pairs        the level 0.5

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
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--replay-iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--levels", type=int, default=40)
    ap.add_argument("--min-iou", type=float, default=0.25)
    ap.add_argument("--zero-distance", type=float, default=2.0)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join("profiles", "track_centre_timing.json"))
    a = ap.parse_args()
    dev = "cuda"
    B, N, K, KO, L, A = a.streams, a.points, a.boxes, a.max_objects, a.levels, 19
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

    # ---- the logs of the same frames under either similarity ----
    F, R = a.frames, a.frames * int(num.max())
    Q = a.frames * int(num.max()) * int(gobj.count.max())          # every (detection, object) pair of every frame would fit
    mk = lambda **kw: TS.TrackScorer(streams=B, max_objects=KO, max_boxes=K, max_gt_tracks=1024, sweep_frames=F, sweep_records=R, sweep_pairs=Q, **kw)
    scorers = {"iou": mk(), "centre": mk(similarity="centre", zero_distance=a.zero_distance)}
    gen = torch.Generator(dev).manual_seed(2)
    ids_f = ids_d.clone()
    for f in range(F):
        if f % 7 == 6:                                      # now and then some tracks change their id
            ids_f = torch.where((torch.rand(B, KO, device=dev, generator=gen) < 0.1) & (ids_f >= 0), ids_f + 1000, ids_f)
        reset = torch.full((B,), int(f % 100 == 0), dtype=torch.uint8, device=dev)
        drop = torch.rand(B, device=dev, generator=gen) < 0.2                       # a fifth of the frames lose their last detection
        conf = torch.rand(B, KO, device=dev, generator=gen)
        for s in scorers.values():
            s.update_raw(t["pc1"], obj_d, torch.where(drop, (num_d - 1).clamp(min=0), num_d), ids_f, gobj, reset=reset, object_conf=conf)
    for s in scorers.values():
        s.check()
    same = all(torch.equal(getattr(scorers["iou"], k), getattr(scorers["centre"], k))
               for k in ("counters", "iou_sum", "log_cursor", "log_frame", "log_label", "log_track", "log_best", "log_conf", "log_iou", "log_size",
                         "log_label_size"))
    sweeps = {k: s.sweep(L, matching="optimal", min_iou=a.min_iou) for k, s in scorers.items()}
    hotas = {k: s.hota(alphas=A, matching="optimal") for k, s in scorers.items()}
    idents = {k: s.identity(alphas=(0.5,), pairs="all") for k, s in scorers.items()}

    # ---- (a) the scoring launch under either similarity ----
    st, ad = abi.stream(), ctypes.addressof
    tm = mk(similarity="centre", zero_distance=a.zero_distance)          # its blocks serve both launches: the plain one ignores pair_sim
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
    centre_d = gobj.centre.contiguous()
    assert a.iters + a.warmup <= F, "every timed call must find room in the log"

    def per_frame(fn, *tail):
        def run():
            return fn(ad(blk_in), ad(blk_st), ad(blk_out), ad(blk_lg), None, ad(blk_pr), *tail, st)

        def block():
            tm.log_cursor.zero_()
            tm.pair_cursor.zero_()
            return block_us(run, a.iters, a.warmup)
        return block
    variants = {"score_pairs": per_frame(_lib._fn("rtk_track_score_pairs")),
                "score_pairs_centre": per_frame(_lib._fn("rtk_track_score_pairs_centre"), tm.pair_sim.data_ptr(), centre_d.data_ptr(), a.zero_distance)}
    if a.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        pfn = parent.rtk_track_score_pairs
        pfn.argtypes, pfn.restype = abi.SIGNATURES["rtk_track_score_pairs"], ctypes.c_int
        variants["score_pairs_parent"] = per_frame(pfn)

    # ---- (b) the four replays on either log ----
    flags = torch.zeros(B, dtype=torch.int32, device=dev)
    keep = []
    for name, sc in scorers.items():
        lg, pr = sc._log_block(), sc._pair_block()
        sim = (sc.pair_sim.data_ptr(),) if sc.centre else ()
        end = "_sim" if sc.centre else ""
        score = torch.zeros(B, sc.R, dtype=torch.float64, device=dev)
        _lib.call("rtk_score_track_means", B, ad(lg), score.data_ptr(), flags.data_ptr(), st)
        thr = torch.from_numpy(sweeps[name].thresholds.copy()).to(dev)
        oc = torch.empty(L + 1, B, len(TS.OPTIMAL_COUNTERS), dtype=torch.int64, device=dev)
        oq, rq = torch.empty(L + 1, B, dtype=torch.int64, device=dev), torch.empty(L + 1, B, dtype=torch.float64, device=dev)
        pair_a = torch.empty(B, sc.Q, dtype=torch.float64, device=dev)
        pidx, cg, ct = (torch.empty(B, sc.Q, dtype=torch.int32, device=dev) for _ in range(3))
        hc = torch.empty(A, B, len(TS.HOTA_COUNTERS), dtype=torch.int64, device=dev)
        hq = torch.empty(A, B, len(TS.HOTA_SUMS), dtype=torch.float64, device=dev)
        half = torch.full((1,), 0.5, dtype=torch.float64, device=dev)
        ic = torch.empty(1, B, len(TS.IDENTITY_COUNTERS), dtype=torch.int64, device=dev)
        keep.append((lg, pr, score, thr, oc, oq, rq, pair_a, pidx, cg, ct, hc, hq, half, ic))
        fo, fa, fh, fi = (_lib._fn(n + end) for n in ("rtk_score_replay_optimal", "rtk_score_alignment", "rtk_score_hota_optimal", "rtk_score_identity_pairs"))
        calls = {
            "replay_optimal": lambda fo=fo, lg=lg, pr=pr, sim=sim, score=score, thr=thr, oc=oc, oq=oq, rq=rq, T=sc.T: fo(
                B, T, ad(lg), ad(pr), *sim, score.data_ptr(), thr.data_ptr(), None, L + 1, a.min_iou, oc.data_ptr(), oq.data_ptr(), rq.data_ptr(), None,
                flags.data_ptr(), st),
            "alignment": lambda fa=fa, lg=lg, pr=pr, sim=sim, pair_a=pair_a, pidx=pidx, cg=cg, ct=ct, T=sc.T: fa(
                B, T, ad(lg), ad(pr), *sim, None, None, pair_a.data_ptr(), pidx.data_ptr(), cg.data_ptr(), ct.data_ptr(), flags.data_ptr(), st),
            "hota_optimal": lambda fh=fh, lg=lg, pr=pr, sim=sim, pair_a=pair_a, pidx=pidx, cg=cg, ct=ct, hc=hc, hq=hq: fh(
                B, ad(lg), ad(pr), *sim, None, None, A, pair_a.data_ptr(), pidx.data_ptr(), cg.data_ptr(), ct.data_ptr(), hc.data_ptr(), hq.data_ptr(),
                flags.data_ptr(), st),
            "identity_pairs": lambda fi=fi, lg=lg, pr=pr, sim=sim, half=half, ic=ic, T=sc.T: fi(
                B, T, ad(lg), ad(pr), *sim, None, None, half.data_ptr(), 1, ic.data_ptr(), flags.data_ptr(), st),
        }
        for k, call in calls.items():          # (alignment comes before hota_optimal in every round: its tables are written by then)
            variants["%s/%s" % (name, k)] = lambda call=call: block_us(call, a.replay_iters, a.warmup)
    runs = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, block in variants.items():
            runs[k].append(block())
    assert int(flags.sum()) == 0 and int(tm.flags.sum()) == 0, (flags.tolist(), tm.flags.tolist())
    s = summary(runs)
    med = lambda k: s[k]["median_us"]
    frames_logged = {k: int(sc.log_cursor[:, 0].sum()) for k, sc in scorers.items()}
    res = {"what": "rtk_track_score_pairs_centre against rtk_track_score_pairs per frame, and the four replays on a centre log against an IoU log of the same frames",
           "streams": B, "points": N, "boxes": K, "max_objects": KO, "iters": a.iters, "replay_iters": a.replay_iters, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "frames_per_stream": F, "levels": L, "alphas": A, "min_iou": a.min_iou, "zero_distance": a.zero_distance,
           "detections_per_frame": round(float(scorers["iou"].log_cursor[:, 1].sum()) / frames_logged["iou"], 2),
           "kept_objects_per_frame": round(float(scorers["iou"].log_cursor[:, 2].sum()) / frames_logged["iou"], 2),
           "pairs_per_frame": {k: round(float(sc.pair_cursor.sum()) / frames_logged[k], 2) for k, sc in scorers.items()},
           "everything_but_the_pair_log_equal": bool(same),
           "launches": s,
           "ratio_centre_over_pairs": round(med("score_pairs_centre") / med("score_pairs"), 3),
           "centre_extra_us_per_frame": round(med("score_pairs_centre") - med("score_pairs"), 3),
           "ratio_pairs_over_parent": round(med("score_pairs") / med("score_pairs_parent"), 3) if a.parent_lib else None,
           "ratio_centre_over_iou": {k: round(med("centre/" + k) / med("iou/" + k), 3) for k in ("replay_optimal", "alignment", "hota_optimal", "identity_pairs")},
           "levels_reached": {k: sw.reached for k, sw in sweeps.items()},
           "numbers": {k: {"amota": sweeps[k].amota, "amotp": sweeps[k].amotp, "tp": int(sweeps[k].tp[0]), "idsw": int(sweeps[k].idsw[0]),
                           "hota": hotas[k].hota, "loca_mean": hotas[k].loca_mean, "idf1": float(idents[k].idf1[0])} for k in scorers}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
