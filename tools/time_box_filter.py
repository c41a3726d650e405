"""The track box filter (ResultLog.filter_boxes) next to the per-frame fit it follows (ResultLog.boxes), on one log.

    python tools/time_box_filter.py [--streams 64] [--points 256] [--max-objects 128] [--frames 64] [--rounds 7] [--iters 20]
                                    [--warmup 5] [--moving-bias 4.0] [--out profiles/box_filter_timing.json]

The log is the one tools/time_track_boxes.py builds: B streams of synthetic frames through a `BatchedTracker(graph=True)` with
synthetic weights, --frames frames appended.  In one process, device time between events: every round times rtk_result_log_boxes and
then rtk_result_log_filter_boxes in each of its four smooth x size_rule modes (default parameters otherwise, `into=` buffers, so nothing
is allocated), the median of --iters launches each; the figure reported is the median over the rounds, so that a drift of the clocks
touches every launch alike.  Writes one JSON object to --out and prints it.  Not part of bench.py."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from ratrack_amd import boxes as BX, result_log as RL, synth, tracker as T  # noqa: E402
from ratrack_amd.track4d import Args, Track4D  # noqa: E402
from time_track_boxes import BATCHES, events  # noqa: E402

MODES = [("filter", 0, 0), ("filter_extent", 0, 1), ("smooth", 1, 0), ("smooth_extent", 1, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--max-objects", type=int, default=128)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--moving-bias", type=float, default=4.0)
    ap.add_argument("--out", default=os.path.join("profiles", "box_filter_timing.json"))
    a = ap.parse_args()
    dev = "cuda"
    B, N, K, F = a.streams, a.points, a.max_objects, a.frames
    batches = []
    for i in range(BATCHES):
        d = synth.make_frame_pairs(B, N, case_id=2000 + i)
        batches.append(tuple(torch.from_numpy(d[k]).to(dev) for k in ("pc1", "pc2", "feature1", "feature2")))
    net = Track4D(Args()).to(dev).eval()
    sd = net.state_dict()
    synth.fill_state_dict(sd)
    sd["fd_layer.cp.linear.bias"].add_(a.moving_bias)
    net.invalidate_fused()
    res = {"what": "rtk_result_log_filter_boxes in its four modes next to rtk_result_log_boxes on one log: events, medians of rounds",
           "streams": B, "points": N, "max_objects": K, "frames": F, "rounds": a.rounds, "iters": a.iters,
           "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        trk = T.BatchedTracker(net, streams=B, max_objects=K, graph=True)
        log = RL.ResultLog(B, K, F, F * K, F * N, device=dev)
        for t in range(F):
            log.append(trk.step(*batches[t % BATCHES]), seq=list(range(B)), index=t, reset=[t == 0] * B)
        trk.check()
        log.check()
        fitted = BX.ObjectBoxes.empty(B, log.R, dev)
        log.boxes(into=fitted)
        outs = {name: BX.FilteredBoxes.empty(B, log.R, dev) for name, _, _ in MODES}
        filters = {name: BX.BoxFilter(smooth=sm, size_rule=sz) for name, sm, sz in MODES}
        rounds = {name: [] for name in ["boxes"] + [m[0] for m in MODES]}
        for _ in range(a.rounds):
            rounds["boxes"].append(events(lambda: log.boxes(into=fitted), a.iters, a.warmup))
            for name, _, _ in MODES:
                rounds[name].append(events(lambda: log.filter_boxes(fitted, filter=filters[name], into=outs[name]), a.iters, a.warmup))
        res["log_boxes_ms"] = round(statistics.median(rounds["boxes"]), 4)
        for name, _, _ in MODES:
            res[name + "_ms"] = round(statistics.median(rounds[name]), 4)
            res[name + "_over_boxes"] = round(res[name + "_ms"] / res["log_boxes_ms"], 4)
        res["spread_ms"] = {name: [round(min(v), 4), round(max(v), 4)] for name, v in rounds.items()}
        out = outs["smooth_extent"]
        torch.cuda.synchronize()
        live = torch.arange(log.R, device=dev)[None, :] < log.cursor[:, 1:2]
        member = live & (out.valid > 0)
        starts = member & (out.link[..., 0] < 0)
        res["log_records"] = int(log.cursor[:, 1].sum())
        res["members"] = int(member.sum())
        res["segments"] = int(starts.sum())
        res["mean_segment"] = round(res["members"] / max(res["segments"], 1), 2)
        first = (out.link[..., 3].long() + torch.arange(B, device=dev)[:, None] * log.R)[member]
        res["longest_segment"] = int(torch.bincount(first).max()) if first.numel() else 0
        res["flags"] = sorted(set(out.flags.tolist()))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
