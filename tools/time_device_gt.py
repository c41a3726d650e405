"""Device ground truth + scoring (ratrack_amd/gt_device.py) against the host path it stands in for and against the train step.

    python tools/time_device_gt.py [--streams 64] [--points 256] [--boxes 32] [--iters 200] [--warmup 20] [--train-steps 20]
                                   [--out profiles/device_gt_timing.json]

One batch of B synthetic frame pairs (synth.make_frame_pairs) with K boxes per frame laid on the clouds' own points, so that
boxes hold points, overlap, and have partners in the other frame.  Measured on the machine it runs on:

  (a) `ground_truth` + `frame_metrics` for the batch -- device time between events around the two calls and, per launch, around
      each entry point (`_lib.TIMING`), median of --iters after --warmup;
  (b) the host path for the same batch on tensors already in memory (no file parsing): per stream `vod_gt.filter_object_points`
      on both frames, `vod_io.compensate_ego_motion`, `vod_gt.gt_scene_flow`, then `metrics.eval_scene_flow` and
      `metrics.eval_motion_seg`; wall clock, median of 5 passes over the batch;
  (c) one `Trainer.step` at the same B and N as bench.py --mode train runs it (one captured graph, synthetic weights), wall clock
      per step over --train-steps after the warm-up and capture.

Writes one JSON object to --out and prints it.  Not part of bench.py."""
import argparse
import json
import os
import statistics
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ratrack_amd import _lib, gt_device as G, metrics as M, synth, vod_gt, vod_io  # noqa: E402
from ratrack_amd.track4d import Args, Track4D  # noqa: E402

IDENTITY_TF = types.SimpleNamespace(t_radar_camera=np.eye(4), t_radar_lidar=np.eye(4))


def make_streams(d, B, N, K, seed=1):
    """K labels per frame and stream: frame-1 boxes centred on points of pc1, their partners shifted a little (a few without a
    partner, a few far away from every point), and an ego motion per stream."""
    rng = np.random.default_rng(seed)
    L = lambda i, c, l, w, h, ry: vod_gt.Label("Car", i, 0, 0, 0, 0, 0, 0, float(h), float(w), float(l), float(c[0]), float(c[1]), float(c[2]), float(ry))
    per_stream, egos = [], []
    for b in range(B):
        labels1, labels2 = {}, {}
        for k in range(K):
            c = d["pc1"][b, :, (k * 7) % N].astype(np.float64)
            l, w, h, ry = rng.uniform(2, 6), rng.uniform(1.5, 4), rng.uniform(1.5, 3), rng.uniform(-3, 3)
            labels1[k] = L(k, c, l, w, h, ry)
            if k % 8 == 7:
                continue
            c2 = c + rng.uniform(-0.5, 0.5, 3) if k % 8 != 6 else c + 1000.0
            labels2[k] = L(k, c2, l, w, h, ry + rng.uniform(-0.1, 0.1))
        ego = np.eye(4)
        ego[:3, :3] = vod_gt.rot_z(rng.uniform(-0.05, 0.05))
        ego[:3, 3] = rng.uniform(-1, 1, 3)
        per_stream.append((labels1, IDENTITY_TF, labels2, IDENTITY_TF, ego))
        egos.append(ego)
    return per_stream, egos


def host_pass(per_stream, egos, t, warp, cls):
    """The host path of one batch: GT per stream, then the two metric functions per stream (the reference's per-frame loop)."""
    out = []
    for b, (labels1, tf1, labels2, tf2, ego) in enumerate(per_stream):
        pc1, pc2 = t["pc1"][b:b + 1], t["pc2"][b:b + 1]
        r1 = vod_gt.filter_object_points(2, labels1, pc1, tf1)
        r2 = vod_gt.filter_object_points(2, labels2, pc2, tf2)
        comp = vod_io.compensate_ego_motion(pc1[0].numpy().T, ego)
        pc1_comp = torch.from_numpy(np.ascontiguousarray(comp[:, :3].T.astype(np.float32))).unsqueeze(0)
        gt = vod_gt.gt_scene_flow(r2[4], r1[1], r1[5], pc1, pc1_comp, r1[6], r2[6])
        sf = M.eval_scene_flow(pc1, warp[b:b + 1], gt, 1.0 - r1[1].float().unsqueeze(0))
        seg = M.eval_motion_seg((cls[b:b + 1] > 0.5).float(), r1[1].float().unsqueeze(0))
        out.append((sf, seg))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--boxes", type=int, default=32)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--train-steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "device_gt_timing.json"))
    a = ap.parse_args()
    dev = "cuda"
    B, N, K = a.streams, a.points, a.boxes
    d = synth.make_frame_pairs(B, N, case_id=1000)
    host = {k: torch.from_numpy(v) for k, v in d.items()}
    t = {k: v.to(dev) for k, v in host.items()}
    per_stream, egos = make_streams(d, B, N, K)
    g = torch.Generator().manual_seed(0)
    warp_h = host["gt_warp"] + 0.1 * torch.randn(B, 3, N, generator=g)
    cls_h = torch.rand(B, N, generator=g)
    warp, cls = warp_h.to(dev), cls_h.to(dev)

    # ---- (a) the device path ----
    t0 = time.perf_counter()
    bb = G.pack_boxes(per_stream, K, dev)
    torch.cuda.synchronize()
    pack_ms = 1e3 * (time.perf_counter() - t0)

    def device_pass():
        gt = G.ground_truth(t["pc1"], t["pc2"], bb)
        fm = G.frame_metrics(t["pc1"], warp, gt.gt_warp, 1.0 - gt.gt_cls.float(), cls, gt.gt_cls)
        return gt, fm
    for _ in range(a.warmup):
        gt, fm = device_pass()
    gt.check()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        device_pass()
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    calls_ms = [e0.elapsed_time(e1) for e0, e1 in pairs]
    _lib.TIMING = []
    for _ in range(a.iters):
        device_pass()
    torch.cuda.synchronize()
    per_launch = {}
    for name, e0, e1 in _lib.TIMING:
        per_launch.setdefault(name, []).append(e0.elapsed_time(e1))
    _lib.TIMING = None
    torch.cuda.synchronize()
    w0 = time.perf_counter()
    for _ in range(a.iters):
        device_pass()
    torch.cuda.synchronize()
    wall_ms = 1e3 * (time.perf_counter() - w0) / a.iters
    launch_ms = {k: statistics.median(v) for k, v in per_launch.items()}

    # ---- (b) the host path, same batch ----
    host_pass(per_stream, egos, host, warp_h, cls_h)
    host_ms = []
    for _ in range(5):
        h0 = time.perf_counter()
        host_out = host_pass(per_stream, egos, host, warp_h, cls_h)
        host_ms.append(1e3 * (time.perf_counter() - h0))
    # the two paths score the same thing
    vals = fm.values.cpu().numpy()
    agree = max(abs(vals[b][G.KEYS.index(k)] - v) / max(1.0, abs(v)) for b, (sf, seg) in enumerate(host_out) for k, v in {**sf, **seg}.items()
                if not np.isnan(v))

    # ---- (c) the train step ----
    from ratrack_amd.train import Trainer
    net = Track4D(Args()).to(dev).eval()
    synth.fill_state_dict(net.state_dict())
    net.invalidate_fused()
    tr = Trainer(net, graph=True)
    h = torch.zeros(5, B, 128, device=dev)
    step = lambda: tr.step(t["pc1"], t["pc2"], t["feature1"], t["feature2"], t["gt_warp"], t["gt_cls"], h)
    for _ in range(6):
        step()
    torch.cuda.synchronize()
    s0 = time.perf_counter()
    for _ in range(a.train_steps):
        step()
    torch.cuda.synchronize()
    train_ms = 1e3 * (time.perf_counter() - s0) / a.train_steps

    a_ms = statistics.median(calls_ms)
    res = {"what": "ground truth + metrics of one batch: device path vs host path vs one train step",
           "streams": B, "points": N, "boxes": K, "iters": a.iters, "device": torch.cuda.get_device_name(0),
           "a_device_calls_ms_median": round(a_ms, 4), "a_device_calls_ms_p10_p90": [round(float(np.quantile(calls_ms, q)), 4) for q in (0.1, 0.9)],
           "a_device_launch_ms_median": {k: round(v, 4) for k, v in launch_ms.items()},
           "a_device_wall_ms_per_batch": round(wall_ms, 4), "pack_boxes_and_upload_ms": round(pack_ms, 3),
           "b_host_ms_per_batch_median": round(statistics.median(host_ms), 2), "b_host_ms_runs": [round(x, 2) for x in host_ms],
           "c_train_step_ms": round(train_ms, 3), "c_train_step": "Trainer(graph=True).step, %d steps after capture" % a.train_steps,
           "ratio_host_over_device": round(statistics.median(host_ms) / a_ms, 1), "ratio_device_over_train_step": round(a_ms / train_ms, 4),
           "host_device_max_rel_diff": float(agree), "labelled_points": int(gt.gt_cls.sum())}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
