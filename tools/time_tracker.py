"""Throughput of the batched tracker (ratrack_amd/tracker.py) against the B = 1 Track4D.forward loop on the same frames.

    python tools/time_tracker.py [--streams 64] [--points 256] [--steps 20] [--warmup 3] [--b1-pairs 64]

Synthetic clouds (synth.make_frame_pairs) and synthetic weights with the cls-bias shift of the golden forward case (+0.09 on
fd_layer.cp.linear.bias), so that every frame has moving points to cluster and associate.  Prints one JSON line: tracked
frame-pairs/s of BatchedTracker.step at B = --streams, and of the B = 1 forward() loop; the objects per frame for context.
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/time_tracker.py --steps 5`."""
import argparse
import json
import os
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
    ap.add_argument("--b1-pairs", type=int, default=64, help="frame-pairs timed through the B = 1 forward() loop")
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
    trk = T.BatchedTracker(net, streams=B)
    with torch.no_grad():
        for i in range(a.warmup):
            trk.step(*frames[i % 4])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        objs = []
        for i in range(a.steps):
            out = trk.step(*frames[i % 4])
            objs.append(out.num_objects)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        trk.check()
        mean_objects = float(torch.stack(objs).float().mean())
        # the same frames through the B = 1 forward() loop (stream b of batch i as one sequence)
        pairs = a.b1_pairs
        net.max_id = 0
        h, prev = torch.zeros(5, 1, 128, device=dev), dict()
        fr = lambda j: [t[j % B:j % B + 1] for t in frames[(j // B) % 4]]
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
                      "batched_pairs_per_s": round(B * a.steps / dt, 1), "batched_ms_per_step": round(1e3 * dt / a.steps, 3),
                      "b1_forward_pairs_per_s": round(pairs / dt1, 1), "b1_ms_per_pair": round(1e3 * dt1 / pairs, 3),
                      "mean_objects_per_frame": round(mean_objects, 2),
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
