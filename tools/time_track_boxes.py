"""Oriented boxes (ratrack_amd/boxes.py) next to the tracked step they follow.

    python tools/time_track_boxes.py [--streams 64] [--points 256] [--max-objects 128] [--frames 64] [--iters 200] [--warmup 20]
                                     [--moving-bias 4.0] [--out profiles/track_boxes_timing.json]

B streams of synthetic frames (synth.make_frame_pairs, a few distinct batches cycled), synthetic weights with the segmentation head's
bias raised so that every stream has objects.  In one process, device time between events, the median of --iters after --warmup:

  * the tracked step of a `BatchedTracker(graph=True)` without boxes, and of one with `boxes=True` (the launch inside the graph);
  * rtk_object_boxes alone on a step's outputs (`object_boxes(out, into=...)`);
  * rtk_result_log_boxes alone on that tracker's log of --frames frames (`ResultLog.boxes(into=...)`), and with a `keep` mask.

Writes one JSON object to --out and prints it.  Not part of bench.py."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from ratrack_amd import boxes as BX, result_log as RL, synth, tracker as T  # noqa: E402
from ratrack_amd.track4d import Args, Track4D  # noqa: E402

BATCHES = 8


def events(fn, iters, warmup):
    """-> the median ms between events around fn."""
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
    return statistics.median(e0.elapsed_time(e1) for e0, e1 in pairs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--max-objects", type=int, default=128)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--moving-bias", type=float, default=4.0)
    ap.add_argument("--out", default=os.path.join("profiles", "track_boxes_timing.json"))
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
    res = {"what": "oriented boxes: rtk_object_boxes and rtk_result_log_boxes next to the tracked step (graph=True), events, medians",
           "streams": B, "points": N, "max_objects": K, "frames": F, "iters": a.iters, "device": torch.cuda.get_device_name(0)}
    count = [0]
    with torch.no_grad():
        step_ms = {}
        for name, kw in (("step_ms", {}), ("step_with_boxes_ms", dict(boxes=True))):
            trk = T.BatchedTracker(net, streams=B, max_objects=K, graph=True, **kw)

            def step():
                count[0] += 1
                return trk.step(*batches[count[0] % BATCHES])
            step_ms[name] = events(step, a.iters, a.warmup)
            trk.check()
        res.update({k: round(v, 4) for k, v in step_ms.items()})
        # the launch alone, on the outputs of the last step of the tracker with boxes
        out = trk.last
        into = BX.ObjectBoxes.empty(B, K, dev)
        res["object_boxes_ms"] = round(events(lambda: BX.object_boxes(out, into=into), a.iters, a.warmup), 4)
        assert torch.equal(into.box.view(torch.int64), out.object_boxes.view(torch.int64))
        valid = into.valid[into.valid > 0]
        res["step_objects"] = int(valid.numel())
        res["step_object_points"] = int(valid.sum())
        res["step_largest_object"] = int(valid.max()) if valid.numel() else 0
        res["step_candidates"] = int((1 + valid.long() * (valid.long() - 1) // 2)[valid <= BX.MAX_POINTS].sum())
        # the log of F frames of that tracker
        log = RL.ResultLog(B, K, F, F * K, F * N, device=dev)
        for t in range(F):
            log.append(step(), seq=list(range(B)), index=t, reset=[t == 0] * B)
        log.check()
        rows = BX.ObjectBoxes.empty(B, log.R, dev)
        res["log_boxes_ms"] = round(events(lambda: log.boxes(into=rows), a.iters, a.warmup), 4)
        sel = log.select(min_track_frames=2, check=False)
        res["log_boxes_keep_ms"] = round(events(lambda: log.boxes(keep=sel, into=rows), a.iters, a.warmup), 4)
        res["log_records"] = int(log.cursor[:, 1].sum())
        res["log_points"] = int(log.cursor[:, 2].sum())
        res["log_kept_records"] = int(sel.keep.sum())
        res["log_flags"] = sorted(set(rows.flags.tolist()))
    res["object_boxes_over_step"] = round(res["object_boxes_ms"] / res["step_ms"], 4)
    res["log_boxes_per_frame_over_step"] = round(res["log_boxes_ms"] / F / res["step_ms"], 5)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
