"""The filter inside the tracked step (rtk_track_box_filter_step, BatchedTracker(box_filter=...)): the launch alone and what it adds to
the captured step.

    python tools/time_box_filter_step.py [--streams 64] [--points 256] [--max-objects 128] [--rounds 7] [--iters 50] [--warmup 10]
                                         [--moving-bias 4.0] [--out profiles/box_filter_step_timing.json]

In one process, device time between events (tools/time_track_boxes.py's `events`: the median of --iters calls); every figure is the
median over --rounds rounds, with the smallest and largest round beside it.
  launch    rtk_track_box_filter_step alone on full tables: --streams streams of --max-objects rows, every row a track that is measured
            and continues (the previous table a permutation of the new one), `into=` buffers, so nothing is allocated.
  step      two `BatchedTracker(graph=True, boxes=True)` on the same net and the same frames, one of them with box_filter.  Without
            the option a tracker issues exactly the launches it issued before the option existed: that one is the baseline.  Every
            round times the baseline, then the filtered tracker, then the baseline again; the difference of a round is the filtered
            step minus the mean of its two baselines, and the two baselines of a round against each other are the run-to-run spread.
Writes one JSON object to --out and prints it.  Not part of bench.py."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from ratrack_amd import boxes as BX, synth, tracker as T  # noqa: E402
from ratrack_amd.track4d import Args, Track4D  # noqa: E402
from time_track_boxes import BATCHES, events  # noqa: E402


def full_tables(B, K, dev, seed=0):
    """Full tables in which every row continues a track: ids_new a permutation of ids_prev per stream, random boxes."""
    g = torch.Generator().manual_seed(seed)
    perm = lambda: torch.stack([torch.randperm(K, generator=g) for _ in range(B)]).to(torch.int32).to(dev)
    count = torch.full((B,), K, dtype=torch.int32, device=dev)
    u = torch.rand(B, K, 8, generator=g, dtype=torch.float64)
    box = torch.stack([u[..., 0] * 100 - 50, u[..., 1] * 100 - 50, u[..., 2] * 4 - 2, 2 + 3 * u[..., 3], 0.5 + 1.5 * u[..., 4], 0.5 + 2 * u[..., 5],
                       (u[..., 6] - 0.5) * 3.14, (2 + 3 * u[..., 3]) * (0.5 + 1.5 * u[..., 4])], dim=2).contiguous().to(dev)
    return perm(), perm(), count, box, torch.ones(B, K, dtype=torch.int32, device=dev)


def spread(v):
    return [round(min(v), 4), round(max(v), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--max-objects", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--moving-bias", type=float, default=4.0)
    ap.add_argument("--out", default=os.path.join("profiles", "box_filter_step_timing.json"))
    a = ap.parse_args()
    dev = "cuda"
    B, N, K = a.streams, a.points, a.max_objects
    res = {"what": "rtk_track_box_filter_step alone on full tables, and the captured tracked step (graph=True, boxes=True) with and "
                   "without box_filter: events, medians of rounds, [min, max] of the rounds beside them",
           "streams": B, "points": N, "max_objects": K, "rounds": a.rounds, "iters": a.iters, "device": torch.cuda.get_device_name(0)}
    flt = BX.BoxFilter()
    # ---- the launch alone ----
    ids_prev, ids_new, count, box, valid = full_tables(B, K, dev)
    state = torch.zeros(B, K, 16, dtype=torch.float64, device=dev)
    since = torch.full((B, K), -1, dtype=torch.int32, device=dev)
    into = BX.StepBoxes.empty(B, K, dev)
    ones, zeros = torch.ones(B, dtype=torch.uint8, device=dev), torch.zeros(B, dtype=torch.uint8, device=dev)
    launch = lambda: BX.filter_step_raw(ids_prev, count, ids_new, count, count, box, valid, state, since, filter=flt, active=ones, reset=zeros, into=into)
    launch()                                   # every row starts; from here on every row continues
    rounds = [events(launch, a.iters, a.warmup) for _ in range(a.rounds)]
    torch.cuda.synchronize()
    res["launch_ms"] = round(statistics.median(rounds), 4)
    res["launch_spread_ms"] = spread(rounds)
    res["launch_rows_continuing"] = int((into.gap == 1).sum())
    # ---- the captured step ----
    batches = []
    for i in range(BATCHES):
        d = synth.make_frame_pairs(B, N, case_id=2000 + i)
        batches.append(tuple(torch.from_numpy(d[k]).to(dev) for k in ("pc1", "pc2", "feature1", "feature2")))
    net = Track4D(Args()).to(dev).eval()
    sd = net.state_dict()
    synth.fill_state_dict(sd)
    sd["fd_layer.cp.linear.bias"].add_(a.moving_bias)
    net.invalidate_fused()
    with torch.no_grad():
        base = T.BatchedTracker(net, streams=B, max_objects=K, graph=True, boxes=True)
        filt = T.BatchedTracker(net, streams=B, max_objects=K, graph=True, boxes=True, box_filter=flt)
        count_steps = {id(base): 0, id(filt): 0}

        def step(trk):
            count_steps[id(trk)] += 1
            return trk.step(*batches[count_steps[id(trk)] % BATCHES])
        for trk in (base, filt):
            for _ in range(a.warmup + 3):
                step(trk)
            assert trk.captured
        first, with_filter, second = [], [], []
        for _ in range(a.rounds):
            first.append(events(lambda: step(base), a.iters, a.warmup))
            with_filter.append(events(lambda: step(filt), a.iters, a.warmup))
            second.append(events(lambda: step(base), a.iters, a.warmup))
        base.check()
        filt.check()
        out = filt.last
        torch.cuda.synchronize()
        res["step_objects"] = int(out.num_objects.sum())
        res["step_rows_with_a_filter"] = int((out.filtered_since >= 0).sum())
        res["step_rows_continuing"] = int((out.filtered_gap > 0).sum())
    baseline = [(x + y) / 2 for x, y in zip(first, second)]
    diff = [f - m for f, m in zip(with_filter, baseline)]
    again = [abs(x - y) for x, y in zip(first, second)]
    res["step_baseline_ms"] = round(statistics.median(baseline), 4)
    res["step_baseline_spread_ms"] = spread(first + second)
    res["step_with_filter_ms"] = round(statistics.median(with_filter), 4)
    res["step_with_filter_spread_ms"] = spread(with_filter)
    res["step_difference_ms"] = round(statistics.median(diff), 4)
    res["step_difference_spread_ms"] = spread(diff)
    res["baseline_run_to_run_ms"] = round(statistics.median(again), 4)
    res["baseline_run_to_run_max_ms"] = round(max(again), 4)
    res["difference_over_step"] = round(res["step_difference_ms"] / res["step_baseline_ms"], 5)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
