"""Throughput of the batched tracker (ratrack_amd/tracker.py) against the B = 1 Track4D.forward loop on the same frames.

    python tools/time_tracker.py [--streams 64] [--points 256] [--steps 20] [--warmup 3] [--b1-pairs 64]
                                 [--static-state] [--graph] [--groups G] [--repeats 1]

--static-state: the tracker that advances its state in place (and the state-advance launch timed alone); --graph: the captured
step; --groups G (with --graph): G independent groups of --streams sequences each through `TrackerPipeline`, pairs/s over all
groups.  --repeats R: the timed loop R times, every run reported (the spread) and the median taken.

Synthetic clouds (synth.make_frame_pairs) and synthetic weights with the cls-bias shift of the golden forward case (+0.09 on
fd_layer.cp.linear.bias), so that every frame has moving points to cluster and associate.  Prints one JSON line: tracked
frame-pairs/s of BatchedTracker.step at B = --streams, and of the B = 1 forward() loop; the objects per frame for context.
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/time_tracker.py --steps 5`."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from ratrack_amd import synth, tracker as T  # noqa: E402
from ratrack_amd.track4d import Args, Track4D  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--b1-pairs", type=int, default=64, help="frame-pairs timed through the B = 1 forward() loop (0: skip)")
    ap.add_argument("--static-state", action="store_true")
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--groups", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=1)
    a = ap.parse_args()
    dev = "cuda"
    B, N = a.streams, a.points
    net = Track4D(Args()).to(dev).eval()
    synth.fill_state_dict(net.state_dict())
    with torch.no_grad():
        net.fd_layer.cp.linear.bias += 0.09
    net.invalidate_fused()
    frames = []
    for s in range(4):          # four distinct batches, cycled
        d = synth.make_frame_pairs(B, N, case_id=100 + s)
        frames.append([torch.from_numpy(d[k]).to(dev) for k in ("pc1", "pc2", "feature1", "feature2")])
    if a.groups > 1 and not a.graph:
        ap.error("--groups needs --graph (a pipeline group is a captured tracker)")
    G = a.groups
    pipe = T.TrackerPipeline(net, groups=G, streams=B) if G > 1 else None
    trk = pipe.trackers[0] if pipe else T.BatchedTracker(net, streams=B, static_state=a.static_state, graph=a.graph)

    def one(i):
        if pipe is None:
            return [trk.step(*frames[i % 4])]
        return [pipe.submit(g, *frames[(i + g) % 4]) for g in range(G)]
    with torch.no_grad():
        for i in range(a.warmup + (3 if a.graph else 0)):      # the captured tracker's own eager warm-up and its capture
            one(i)
        if pipe:
            pipe.drain()
        torch.cuda.synchronize()
        runs, objs = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            for i in range(a.steps):
                outs = one(i)
                if pipe is None and not a.graph:
                    objs.append(outs[0].num_objects)
            if pipe:
                pipe.drain()
            torch.cuda.synchronize()
            runs.append(time.perf_counter() - t0)
        dt = statistics.median(runs)
        for t_ in (pipe.trackers if pipe else [trk]):
            t_.check()
        if not objs:                 # a captured step's outputs are overwritten in place: the last step stands for the run
            objs = [o.num_objects for o in outs]
        mean_objects = float(torch.stack(objs).float().mean())
        advance_us = None
        if trk.static_state:         # the state advance alone: the launch `associate` begins with
            from ratrack_amd.fused import copy_multi
            jobs = [(trk.desc[1].clone(), trk.desc[0]), (trk.ids[1].clone(), trk.ids[0]), (trk.count[1].clone(), trk.count[0])]
            ev = []
            for _ in range(60):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                copy_multi(jobs)
                e1.record()
                ev.append((e0, e1))
            torch.cuda.synchronize()
            advance_us = round(1e3 * statistics.median(e0.elapsed_time(e1) for e0, e1 in ev[10:]), 2)
        # the same frames through the B = 1 forward() loop (stream b of batch i as one sequence)
        pairs = a.b1_pairs
        dt1 = None
        net.max_id = 0
        h, prev = torch.zeros(5, 1, 128, device=dev), dict()
        fr = lambda j: [t[j % B:j % B + 1] for t in frames[(j // B) % 4]]
        if pairs > 0:
            for j in range(a.warmup):
                h, *_, objects, _, _ = net(*fr(j), h, prev)
                prev = objects
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for j in range(pairs):
                h, _, _, _, _, _, _, objects, _, _ = net(*fr(j), h, prev)
                prev = objects
            torch.cuda.synchronize()
            dt1 = time.perf_counter() - t1
    print(json.dumps({"metric": "tracked_frame_pairs_per_s", "streams": B, "points": N, "steps": a.steps,
                      "mode": ("graph" if a.graph else "eager") + ("+static_state" if trk.static_state and not a.graph else ""), "groups": G,
                      "batched_pairs_per_s": round(G * B * a.steps / dt, 1), "batched_ms_per_step": round(1e3 * dt / a.steps, 3),
                      "ms_per_step_runs": [round(1e3 * r / a.steps, 3) for r in runs], "state_advance_us": advance_us,
                      "b1_forward_pairs_per_s": None if dt1 is None else round(pairs / dt1, 1),
                      "b1_ms_per_pair": None if dt1 is None else round(1e3 * dt1 / pairs, 3),
                      "mean_objects_per_frame": round(mean_objects, 2),
                      "device": torch.cuda.get_device_name(0)}))

if __name__ == "__main__":
    main()
