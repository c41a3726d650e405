"""Ground-truth objects + matching + tracking score on the device (ratrack_amd/track_score.py) against the host path they stand in
for and against the tracker step they follow.

    python tools/time_track_score.py [--streams 64] [--points 256] [--boxes 32] [--max-objects 128] [--iters 200] [--warmup 20]
                                     [--moving-bias 4.0] [--out profiles/track_score_timing.json]

One batch of B synthetic frames (synth.make_frame_pairs) with K boxes per frame laid on the clouds' own points (every fourth a
rider), detections made from the boxes' point sets (the last box of each point, so overlapping boxes give partial detections).
Measured on the machine it runs on:

  (a) `gt_objects` + `TrackScorer.update_raw` for the batch: device time between events around the two calls and, per launch, around
      each entry point (`_lib.TIMING`), median of --iters after --warmup; the same for ablated inputs that switch phases off
      (no rider among the types: no merge loop; boxes of negative extent: the membership tests run but nothing is inside, so no
      centre walk and nothing after it; no box at all: what is left is the launch, the loads and the duplicate scan; no detection:
      no pair count; no kept object: no pair count and no table update);
  (b) the host path for the same batch on tensors already in memory: per stream `vod_gt.filter_object_points`, the objects dict,
      `vod_gt.map_gt_objects`, the target list of `loss.affinity_loss` and the counting; wall clock, median of 5 passes;
  (c) one `BatchedTracker.step` at the same B and N and its four association launches (`_lib.TIMING`), twice: with synthetic
      weights as they are (no point is called moving, so the four launches find nothing to do: their floor) and with the
      segmentation head's bias raised (--moving-bias) so that there are objects to cluster and associate.

Writes one JSON object to --out and prints it.  Not part of bench.py."""
import argparse
import json
import os
import random
import statistics
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ratrack_amd import _lib, gt_device as G, synth, track_score as TS, tracker as T, vod_gt  # noqa: E402
from ratrack_amd.track4d import Args, Track4D  # noqa: E402

IDENTITY_TF = types.SimpleNamespace(t_radar_camera=np.eye(4), t_radar_lidar=np.eye(4))
ASSOC = ("rtk_dbscan_batched", "rtk_object_descriptors", "rtk_affinity_pairs", "rtk_associate_batched")


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


def timed(fn, iters, warmup):
    """-> (median ms between events around fn, {entry point: median ms})."""
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
    total = [e0.elapsed_time(e1) for e0, e1 in pairs]
    _lib.TIMING = []
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    per = {}
    for name, e0, e1 in _lib.TIMING:
        per.setdefault(name, []).append(e0.elapsed_time(e1))
    _lib.TIMING = None
    return statistics.median(total), {k: round(statistics.median(v), 4) for k, v in per.items()}


def host_pass(per_stream, pc1, obj, num, ids, prev, counters):
    out = []
    for b, item in enumerate(per_stream):
        r = vod_gt.filter_object_points(2, item[0], pc1[b:b + 1], item[1])
        objects = {}
        for i in range(int(num[b])):
            xyz = pc1[b][:, obj[b] == i]
            objects[int(ids[b, i])] = torch.cat((xyz, xyz), dim=0).unsqueeze(0)
        mapping, _ = vod_gt.map_gt_objects(r[9], r[7], objects, rng=random)
        if prev[b] and mapping:
            keys_p, keys_c = list(prev[b].keys()), list(mapping.keys())
            torch.tensor([1.0 if m == n else 0.0 for m in keys_p for n in keys_c])
        matched = sum(1 for k in mapping if k >= 0)
        counters[b] += np.array([1, len(r[7]), len(objects), matched, len(objects) - matched, len(r[7]) - matched])
        out.append(mapping)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--boxes", type=int, default=32)
    ap.add_argument("--max-objects", type=int, default=128)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--moving-bias", type=float, default=4.0, help="added to the segmentation head's bias for (c)")
    ap.add_argument("--out", default=os.path.join("profiles", "track_score_timing.json"))
    a = ap.parse_args()
    dev = "cuda"
    B, N, K, KO = a.streams, a.points, a.boxes, a.max_objects
    d = synth.make_frame_pairs(B, N, case_id=1000)
    host = {k: torch.from_numpy(v) for k, v in d.items()}
    t = {k: v.to(dev) for k, v in host.items()}
    per_stream = make_streams(d, B, N, K)
    bb = G.pack_boxes(per_stream, K, dev)
    types_d = TS.pack_box_types(per_stream, K, dev)
    gt = G.ground_truth(t["pc1"], t["pc2"], bb)
    # detections: every box that is some point's last box, numbered in slot order
    idx = gt.box_index.cpu().numpy()
    obj = np.full((B, N), -1, dtype=np.int32)
    num = np.zeros(B, dtype=np.int32)
    ids = np.full((B, KO), -1, dtype=np.int32)
    for b in range(B):
        slots = sorted(set(idx[b][idx[b] >= 0].tolist()))
        for i, s in enumerate(slots):
            obj[b, idx[b] == s] = i
        num[b] = len(slots)
        ids[b, :len(slots)] = 100 + np.array(slots)
    obj_d, num_d, ids_d = torch.from_numpy(obj).to(dev), torch.from_numpy(num).to(dev), torch.from_numpy(ids).to(dev)
    scorer = TS.TrackScorer(streams=B, max_objects=KO, max_boxes=K, max_gt_tracks=1024)

    hollow = types.SimpleNamespace(B=B, K=K, boxes=bb.boxes.clone(), box_id=bb.box_id, count=bb.count)
    hollow.boxes[..., 12:15] = -1.0
    nobox = types.SimpleNamespace(B=B, K=K, boxes=bb.boxes, box_id=bb.box_id, count=torch.zeros_like(bb.count))

    def device_pass(types_=types_d, num_=num_d, min_pts=2, boxes=bb):
        gobj = TS.gt_objects(t["pc1"], boxes, types_, min_obj_points=min_pts)
        return gobj, scorer.update_raw(t["pc1"], obj_d, num_, ids_d, gobj)
    gobj, m = device_pass()
    gobj.check()
    scorer.check()
    a_ms, a_launch = timed(device_pass, a.iters, a.warmup)
    no_rider = timed(lambda: device_pass(types_=torch.zeros_like(types_d)), a.iters, a.warmup)[1]
    no_pred = timed(lambda: device_pass(num_=torch.zeros_like(num_d)), a.iters, a.warmup)[1]
    hollow_ms = timed(lambda: device_pass(boxes=hollow), a.iters, a.warmup)[1]
    nobox_ms = timed(lambda: device_pass(boxes=nobox), a.iters, a.warmup)[1]
    no_gt = timed(lambda: device_pass(min_pts=1 << 20), a.iters, a.warmup)[1]

    # ---- (b) the host path ----
    counters = np.zeros((B, 6), dtype=np.int64)
    prev = host_pass(per_stream, host["pc1"], obj, num, ids, [None] * B, counters)
    host_ms = []
    for _ in range(5):
        h0 = time.perf_counter()
        prev = host_pass(per_stream, host["pc1"], obj, num, ids, prev, counters)
        host_ms.append(1e3 * (time.perf_counter() - h0))
    # the two paths match the same detections to the same objects
    dev_ids = m.pred_gt_id.cpu().numpy()
    agree = all([k if k >= 0 else -1 for k in prev[b].keys()] == dev_ids[b, :num[b]].tolist() for b in range(B) if prev[b])

    # ---- (c) the tracker step: with the synthetic weights as they are (no point is called moving: the floor of the four launches)
    #      and with the segmentation head's bias raised (objects in every stream) ----
    steps = {}
    for name, bias in (("c_idle", 0.0), ("c", a.moving_bias)):
        net = Track4D(Args()).to(dev).eval()
        sd = net.state_dict()
        synth.fill_state_dict(sd)
        sd["fd_layer.cp.linear.bias"].add_(bias)
        net.invalidate_fused()
        trk = T.BatchedTracker(net, streams=B, max_objects=KO)
        step = lambda: trk.step(t["pc1"], t["pc2"], t["feature1"], t["feature2"])
        ms, launch = timed(step, max(20, a.iters // 4), 10)
        trk.check()
        steps[name] = dict(step_ms=round(ms, 4), detected_objects=int(trk.last.num_objects.sum()),
                           association_launch_ms_median={k: launch.get(k) for k in ASSOC},
                           four_association_launches_ms=round(sum(launch.get(k, 0.0) for k in ASSOC), 4))
    assoc_ms, idle_ms = steps["c"]["four_association_launches_ms"], steps["c_idle"]["four_association_launches_ms"]

    both = a_launch["rtk_gt_objects"] + a_launch["rtk_track_score"]
    res = {"what": "ground-truth objects + matching + score of one batch: device path vs host path vs one tracker step",
           "streams": B, "points": N, "boxes": K, "max_objects": KO, "iters": a.iters, "device": torch.cuda.get_device_name(0),
           "gt_objects_kept": int(gobj.count.sum()), "detections": int(num.sum()), "matches": int((dev_ids >= 0).sum()),
           "a_device_calls_ms_median": round(a_ms, 4), "a_device_launch_ms_median": a_launch, "a_two_launches_ms": round(both, 4),
           "a_launch_ms_no_rider": no_rider, "a_launch_ms_hollow_boxes": hollow_ms, "a_launch_ms_no_box": nobox_ms,
           "a_launch_ms_no_detection": no_pred, "a_launch_ms_no_kept_object": no_gt,
           "b_host_ms_per_batch_median": round(statistics.median(host_ms), 2), "b_host_ms_runs": [round(x, 2) for x in host_ms],
           "c_tracker_step": steps["c"], "c_idle_tracker_step": steps["c_idle"],
           "ratio_host_over_device": round(statistics.median(host_ms) / a_ms, 1),
           "ratio_two_launches_over_four_association_launches": round(both / assoc_ms, 3),
           "ratio_two_launches_over_four_idle_association_launches": round(both / idle_ms, 3),
           "host_device_matches_agree": bool(agree)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
