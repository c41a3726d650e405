"""What the tracking term adds to a train step (ratrack_amd/track_train.py) at B = 64, N = 256 with the reference weights.

    python tools/time_track_train.py [--streams 64] [--points 256] [--boxes 32] [--max-objects 128] [--iters 100] [--warmup 10]
                                     [--out profiles/track_train_timing.json] [--graph] [--repeats 1]

One batch of B synthetic frame pairs (synth.make_frame_pairs) with K boxes per frame laid on the clouds' own points, the reference
state dict with the segmentation head's bias raised by 0.09 so that every frame has moving points (tests/test_tracker_gpu.py), the
learning rate 0 so that the timed steps all see the same weights.  Measured on the machine it runs on, device time between events,
median of --iters after --warmup:

  (a) `SequenceTrainer.step` (eager; with --graph also captured in a hipGraph, `SequenceTrainer(graph=True)`, on a second net with
      the same weights; --repeats R measures each of the two R times in turn and reports every median: the spread);
  (b) `Trainer.step` on the same batch (eager, and captured in a hipGraph);
  (c) `BatchedTracker.associate` + `TrackScorer.update` on the same batch, and their launches (`_lib.TIMING`);
  (d) the three new entry points alone on that frame's `StepResult` / `MatchResult`, per entry point.

Writes one JSON object to --out and prints it.  Not part of bench.py."""
import argparse
import json
import os
import statistics
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ratrack_amd import _lib, gt_device as G, synth, track_score as TS, tracker as T, track_train as TT, vod_gt  # noqa: E402
from ratrack_amd.track4d import Args, Track4D  # noqa: E402
from ratrack_amd.train import Trainer  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY_TF = types.SimpleNamespace(t_radar_camera=np.eye(4), t_radar_lidar=np.eye(4))
NEW = ("rtk_affinity_train", "rtk_affinity_wgrad", "rtk_object_descriptors_bwd")
ASSOC = ("rtk_dbscan_batched", "rtk_object_descriptors", "rtk_affinity_pairs", "rtk_associate_batched", "rtk_track_score")


def reference_net(dev):
    with open(os.path.join(ROOT, "tests", "golden", "state_dict_spec.json")) as f:
        spec = json.load(f)["entries"]
    sd = {}
    for k, (shape, dtype) in spec.items():
        a = synth.tensor_for_key(k, tuple(shape), dtype_is_int=(dtype == "int64"))
        sd[k] = torch.from_numpy(np.ascontiguousarray(a)).reshape(shape).to(dev)
    sd["fd_layer.cp.linear.bias"] = sd["fd_layer.cp.linear.bias"] + 0.09
    net = Track4D(Args()).to(dev)
    net.load_state_dict(sd, strict=True)
    return net.train()


def make_streams(d, B, N, K, seed=1):
    rng = np.random.default_rng(seed)
    per_stream = []
    for b in range(B):
        labels = {}
        for k in range(K):
            c = d["pc1"][b, :, (k * 7) % N].astype(np.float64)
            l, w, h, ry = rng.uniform(2, 6), rng.uniform(1.5, 4), rng.uniform(1.5, 3), rng.uniform(-3, 3)
            labels[k] = vod_gt.Label("rider" if k % 4 == 1 else "Car", k, 0, 0, 0, 0, 0, 0, float(h), float(w), float(l), float(c[0]),
                                     float(c[1]), float(c[2]), float(ry))
        per_stream.append((labels, IDENTITY_TF, labels, IDENTITY_TF))
    return per_stream


def timed(fn, iters, warmup, per_launch=False):
    """-> (median ms between events around fn, {entry point: median ms of the sum of its calls in one fn})."""
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
    total = statistics.median(e0.elapsed_time(e1) for e0, e1 in pairs)
    per = {}
    if per_launch:
        runs = []
        for _ in range(iters):
            _lib.TIMING = []
            fn()
            runs.append(_lib.TIMING)
        _lib.TIMING = None
        torch.cuda.synchronize()
        for run in runs:
            once = {}
            for name, e0, e1 in run:
                once[name] = once.get(name, 0.0) + e0.elapsed_time(e1)
            for name, ms in once.items():
                per.setdefault(name, []).append(ms)
        per = {k: round(statistics.median(v), 4) for k, v in per.items()}
    return round(total, 4), per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--boxes", type=int, default=32)
    ap.add_argument("--max-objects", type=int, default=128)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join("profiles", "track_train_timing.json"))
    ap.add_argument("--graph", action="store_true", help="also time the captured sequence step")
    ap.add_argument("--repeats", type=int, default=1)
    a = ap.parse_args()
    dev = "cuda"
    B, N, K, KO = a.streams, a.points, a.boxes, a.max_objects
    d = synth.make_frame_pairs(B, N, case_id=1000)
    t = {k: torch.from_numpy(v).to(dev) for k, v in d.items()}
    per_stream = make_streams(d, B, N, K)
    bb = G.pack_boxes(per_stream, K, dev)
    types_d = TS.pack_box_types(per_stream, K, dev)
    pc1, pc2, f1, f2 = t["pc1"], t["pc2"], t["feature1"], t["feature2"]
    gt = G.ground_truth(pc1, pc2, bb)
    net = reference_net(dev)
    gobj = TS.gt_objects(pc1, bb, types_d, min_obj_points=net.min_obj_points)
    h0 = torch.zeros(5, B, 128, device=dev)

    # ---- (a) the sequence step ----
    tr = TT.SequenceTrainer(net, streams=B, max_objects=KO, max_boxes=K, lr=0.0)
    state = {}

    def seq_step():
        state["items"], _, state["out"], state["match"] = tr.step(pc1, pc2, f1, f2, gt.gt_warp, gt.gt_cls, gobj, h0)
    tr.step(pc1, pc2, f1, f2, gt.gt_warp, gt.gt_cls, gobj, h0, reset=torch.ones(B, dtype=torch.bool))
    a_ms, a_launch = timed(seq_step, a.iters, a.warmup, per_launch=True)
    tr.check()
    a_runs, g_runs, g_loss = [a_ms], [], None
    if a.graph:
        trg = TT.SequenceTrainer(reference_net(dev), streams=B, max_objects=KO, max_boxes=K, lr=0.0, graph=True)
        gstate = {}

        def graph_step():
            gstate["items"] = trg.step(pc1, pc2, f1, f2, gt.gt_warp, gt.gt_cls, gobj, h0)[0]
        trg.step(pc1, pc2, f1, f2, gt.gt_warp, gt.gt_cls, gobj, h0, reset=torch.ones(B, dtype=torch.bool))
        g_runs.append(timed(graph_step, a.iters, a.warmup + 5)[0])
        assert trg.captured
        for _ in range(a.repeats - 1):          # alternating: eager, captured, eager, ...
            a_runs.append(timed(seq_step, a.iters, 2)[0])
            g_runs.append(timed(graph_step, a.iters, 2)[0])
        trg.check()
        g_loss = float(gstate["items"]["TrackingLoss"])
    out, match = state["out"], state["match"]
    pairs = int((out.num_prev.long() * out.num_objects.long() * match.aff_defined.long()).sum())

    # ---- (c) associate + scorer.update, (d) the three new entry points, on that frame ----
    with torch.no_grad():
        flow, _, cls, _, _, _, prop = net.backbone(pc1, pc2, f1, f2, h0)
    flow, cls, prop = flow.detach(), cls.detach(), prop.detach()
    reset, active = torch.zeros(B, dtype=torch.uint8, device=dev), torch.ones(B, dtype=torch.uint8, device=dev)

    def assoc():
        o = tr.tracker.associate(pc1, f1, flow, cls, prop, None, reset, active)
        return o, tr.scorer.update(o, gobj, reset=reset, active=active)
    c_ms, c_launch = timed(assoc, a.iters, a.warmup, per_launch=True)
    out, match = assoc()
    weights, weights_bwd = T.pack_affinity(net.affinity), TT.pack_affinity_bwd(net.affinity)
    scale = torch.full((B,), 0.5 / B, device=dev)

    def new_launches():
        _, d_desc, _, _ = TT.affinity_backward(weights, weights_bwd, out.desc_prev, out.num_prev, out.descriptors, out.num_objects,
                                               match.aff_target, match.aff_defined, scale, None, out.active, tr.max_pairs)
        TT.descriptors_backward(out, d_desc)
    d_ms, d_launch = timed(new_launches, a.iters, a.warmup, per_launch=True)
    d_pairs = int((out.num_prev.long() * out.num_objects.long() * match.aff_defined.long()).sum())

    # ---- (b) the backbone-only step on the same batch ----
    b_ms = {}
    for graph in (False, True):
        base = Trainer(reference_net(dev), lr=0.0, graph=graph)
        step = lambda: base.step(pc1, pc2, f1, f2, gt.gt_warp, gt.gt_cls, h0)
        b_ms["graph" if graph else "eager"] = timed(step, a.iters, a.warmup + 5)[0]

    res = {"what": "the tracking term of B sequences: the sequence step against the backbone-only step, the tracker + scorer launches "
                   "and the three new entry points alone",
           "streams": B, "points": N, "boxes": K, "max_objects": KO, "max_pairs": tr.max_pairs, "iters": a.iters,
           "device": torch.cuda.get_device_name(0),
           "detected_objects": int(out.num_objects.sum()), "live_pairs_in_the_timed_step": pairs, "live_pairs_in_d": d_pairs,
           "tracking_loss": float(state["items"]["TrackingLoss"]),
           "a_sequence_step_ms": a_ms, "a_sequence_step_ms_runs": a_runs,
           "a_sequence_step_graph_ms": statistics.median(g_runs) if g_runs else None, "a_sequence_step_graph_ms_runs": g_runs,
           "tracking_loss_of_the_captured_step": g_loss, "a_new_entry_points_ms_inside_the_step": {k: a_launch.get(k) for k in NEW},
           "a_tracker_scorer_launches_ms_inside_the_step": {k: a_launch.get(k) for k in ASSOC},
           "b_trainer_step_eager_ms": b_ms["eager"], "b_trainer_step_graph_ms": b_ms["graph"],
           "c_associate_plus_update_ms": c_ms, "c_launch_ms": {k: c_launch.get(k) for k in ASSOC},
           "d_three_entry_points_ms": d_ms, "d_launch_ms": {k: d_launch.get(k) for k in NEW},
           "step_minus_eager_trainer_step_ms": round(a_ms - b_ms["eager"], 4),
           "step_minus_eager_trainer_step_minus_c_ms": round(a_ms - b_ms["eager"] - c_ms, 4)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
