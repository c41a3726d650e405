"""What training the re-acquisition costs: rtk_track_score_memory against rtk_track_score, and the captured sequence train step with
reacquire=None and reacquire=2, next to a checkout of the parent commit on the same machine.

    python tools/time_track_memory_train.py [--parent DIR] [--rounds 3] [--streams 64] [--points 256] [--boxes 32] [--max-objects 128]
                                            [--iters 100] [--warmup 10] [--max-pairs 131072]
                                            [--out profiles/track_memory_train_timing.json]

Every measurement is a process of its own (this one starts them and never touches the GPU itself); the processes of one round run one
after the other, this tree and the parent's (--parent: a checkout of the parent commit with its library built) alternating, and who
goes first alternates too, so that a drift of the machine lands on both.  A process works through four synthetic batches of --streams
clouds of --points points in rotation (synth.make_frame_pairs; --boxes boxes per frame laid on the clouds' own points), so that tracks
are lost and found, and reports the median device time between events over --iters steps:

  score   a BatchedTracker(max_age=2) with synthetic weights (the segmentation head's bias raised, as tools/time_track_memory.py does)
          is stepped eagerly and a plain TrackScorer scores every step, the update between events: (a) rtk_track_score here against
          the parent's.  score/both: a TrackScorer(track_memory=True) scores the same StepResult and GtObjects as well, each update
          between events of its own, the two taking turns to go first: (b) the new entry point against rtk_track_score on the same
          argument blocks (the second of two scorers finds its inputs in the cache: compare within score/both only).
  step    SequenceTrainer(graph=True, lr=0).step with the reference weights (tools/time_track_train.py), captured: (a) reacquire=None
          here against the parent's trainer, (c) reacquire=2, with the live pairs and the coasted rows of the last step next to it -- at
          the default max_pairs, where streams beyond the cap are left out of the term and `check` says so, and at --max-pairs.

Per configuration the JSON holds the median and the spread (min, max) over the rounds.  What executes no new code -- rtk_track_score
and the reacquire=None step -- must sit inside the parent's own run-to-run spread.  Not part of bench.py."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import types

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _batches(a, dev, net_min_points):
    """Four batches in rotation: (pc1, pc2, f1, f2, gt_warp, gt_cls, gobj)."""
    import numpy as np
    import torch
    from ratrack_amd import gt_device as G, synth, track_score as TS, vod_gt
    tf = types.SimpleNamespace(t_radar_camera=np.eye(4), t_radar_lidar=np.eye(4))
    B, N, K = a.streams, a.points, a.boxes
    rng = np.random.default_rng(1)
    out = []
    for i in range(4):
        d = synth.make_frame_pairs(B, N, case_id=1000 + i)
        per_stream = []
        for b in range(B):
            labels = {}
            for k in range(K):
                c = d["pc1"][b, :, (k * 7) % N].astype(np.float64)
                l, w, h, ry = rng.uniform(2, 6), rng.uniform(1.5, 4), rng.uniform(1.5, 3), rng.uniform(-3, 3)
                labels[k] = vod_gt.Label("rider" if k % 4 == 1 else "Car", k, 0, 0, 0, 0, 0, 0, float(h), float(w), float(l), float(c[0]),
                                         float(c[1]), float(c[2]), float(ry))
            per_stream.append((labels, tf, labels, tf))
        t = {k: torch.from_numpy(v).to(dev) for k, v in d.items()}
        bb = G.pack_boxes(per_stream, K, dev)
        gt = G.ground_truth(t["pc1"], t["pc2"], bb)
        gobj = TS.gt_objects(t["pc1"], bb, TS.pack_box_types(per_stream, K, dev), min_obj_points=net_min_points)
        out.append((t["pc1"], t["pc2"], t["feature1"], t["feature2"], gt.gt_warp, gt.gt_cls, gobj))
    return out


def _median_ms(pairs):
    return round(statistics.median(e0.elapsed_time(e1) for e0, e1 in pairs), 4)


def measure_score(a):
    import torch
    from ratrack_amd import synth, track_score as TS, tracker as T
    from ratrack_amd.track4d import Args, Track4D
    dev = "cuda"
    net = Track4D(Args()).to(dev).eval()
    sd = net.state_dict()
    synth.fill_state_dict(sd)
    sd["fd_layer.cp.linear.bias"].add_(a.moving_bias)
    net.invalidate_fused()
    batches = _batches(a, dev, net.min_obj_points)
    trk = T.BatchedTracker(net, streams=a.streams, max_objects=a.max_objects, max_age=2)
    kw = dict(streams=a.streams, max_objects=a.max_objects, max_boxes=a.boxes)
    scorers = {"rtk_track_score": TS.TrackScorer(**kw)}
    if a.memory:
        scorers["rtk_track_score_memory"] = TS.TrackScorer(track_memory=True, **kw)
    times = {k: [] for k in scorers}
    with torch.no_grad():
        for i in range(a.warmup + a.iters):
            pc1, pc2, f1, f2, _, _, gobj = batches[i % 4]
            out = trk.step(pc1, pc2, f1, f2)
            order = list(scorers.items()) if i % 2 == 0 else list(scorers.items())[::-1]
            for name, sc in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                m = sc.update(out, gobj)
                e1.record()
                if i >= a.warmup:
                    times[name].append((e0, e1))
        torch.cuda.synchronize()
    res = {k + "_ms": _median_ms(v) for k, v in times.items()}
    res.update(detected_objects=int(out.num_objects.sum()), previous_rows=int(out.num_prev.sum()), coasted_rows=int(out.num_coasted.sum()),
               target_ones=int(m.aff_target.sum()), device=torch.cuda.get_device_name(0))
    print("RESULT " + json.dumps(res), flush=True)


def measure_step(a):
    import numpy as np
    import torch
    from ratrack_amd import synth, track_train as TT
    from ratrack_amd.track4d import Args, Track4D
    dev = "cuda"
    with open(os.path.join(os.path.abspath(a.root), "tests", "golden", "state_dict_spec.json")) as f:
        spec = json.load(f)["entries"]
    sd = {}
    for k, (shape, dtype) in spec.items():
        v = synth.tensor_for_key(k, tuple(shape), dtype_is_int=(dtype == "int64"))
        sd[k] = torch.from_numpy(np.ascontiguousarray(v)).reshape(shape).to(dev)
    sd["fd_layer.cp.linear.bias"] = sd["fd_layer.cp.linear.bias"] + 0.09
    net = Track4D(Args()).to(dev)
    net.load_state_dict(sd, strict=True)
    net.train()
    batches = _batches(a, dev, net.min_obj_points)
    kw = {} if a.reacquire == "none" else dict(reacquire=int(a.reacquire))
    if a.one_max_pairs:
        kw["max_pairs"] = a.one_max_pairs
    tr = TT.SequenceTrainer(net, streams=a.streams, max_objects=a.max_objects, max_boxes=a.boxes, lr=0.0, graph=True, **kw)
    h0 = torch.zeros(5, a.streams, 128, device=dev)
    tr.step(*batches[0], h0, reset=torch.ones(a.streams, dtype=torch.bool))
    pairs = []
    for i in range(1, a.warmup + 5 + a.iters + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        items, _, out, match = tr.step(*batches[i % 4], h0)
        e1.record()
        if i > a.warmup + 5:
            pairs.append((e0, e1))
    torch.cuda.synchronize()
    assert tr.captured
    res = dict(step_ms=_median_ms(pairs), live_pairs=int((out.num_prev.long() * out.num_objects.long() * match.aff_defined.long()).sum()),
               detected_objects=int(out.num_objects.sum()), previous_rows=int(out.num_prev.sum()), target_ones=int(match.aff_target.sum()),
               tracking_loss=float(items["TrackingLoss"]), device=torch.cuda.get_device_name(0))
    if kw:
        res["coasted_rows"] = int(out.num_coasted.sum())
    try:
        tr.check()
    except RuntimeError as e:                   # (a taller table may pass max_pairs: reported, the time stands for what ran)
        res["check"] = str(e)
    print("RESULT " + json.dumps(res), flush=True)


def child(a, root, what, **opt):
    cmd = [sys.executable, os.path.abspath(__file__), "--one", what, "--root", root, "--streams", str(a.streams), "--points", str(a.points),
           "--boxes", str(a.boxes), "--max-objects", str(a.max_objects), "--iters", str(a.iters), "--warmup", str(a.warmup),
           "--moving-bias", str(a.moving_bias)]
    for k, v in opt.items():
        cmd += ["--" + ("one-max-pairs" if k == "max-pairs" else k)] + ([] if v is True else [str(v)])
    out = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.timeout, check=True).stdout.decode()
    return json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, its library built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--boxes", type=int, default=32)
    ap.add_argument("--max-objects", type=int, default=128)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--moving-bias", type=float, default=4.0, help="score: added to the segmentation head's bias")
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds a measuring process may take")
    ap.add_argument("--out", default=os.path.join("profiles", "track_memory_train_timing.json"))
    ap.add_argument("--one", default=None, choices=("score", "step"), help="(internal) measure one configuration in this process")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--memory", action="store_true", help="(internal) score: the memory scorer too")
    ap.add_argument("--one-max-pairs", type=int, default=0, help="(internal) step: max_pairs of the trainer (0: its default)")
    ap.add_argument("--reacquire", default="none")
    ap.add_argument("--max-pairs", type=int, default=1 << 17, help="step: the cap of the second reacquire=2 configuration (the first "
                    "keeps the default, 32768, beyond which streams are left out of the term and flagged)")
    a = ap.parse_args()
    if a.one:
        sys.path.insert(0, os.path.abspath(a.root))
        return measure_score(a) if a.one == "score" else measure_step(a)
    configs = [("this/score", HERE, "score", {}), ("this/score/both", HERE, "score", dict(memory=True)),
               ("this/step/reacquire=none", HERE, "step", {}), ("this/step/reacquire=2", HERE, "step", dict(reacquire=2)),
               ("this/step/reacquire=2/max_pairs=%d" % a.max_pairs, HERE, "step", {"reacquire": 2, "max-pairs": a.max_pairs})]
    if a.parent:
        configs += [("parent/score", a.parent, "score", {}), ("parent/step/reacquire=none", a.parent, "step", {})]
    runs = {}
    for r in range(a.rounds):
        for what in ("score", "step"):
            order = [c for c in configs if c[2] == what]
            for key, root, _, opt in (order if r % 2 == 0 else order[::-1]):      # the trees alternate, and who goes first alternates too
                runs.setdefault(key, []).append(child(a, root, what, **opt))
                print(key, runs[key][-1], flush=True)
    res = {"what": "device ms between events, median of --iters per process; per configuration the median, min and max over the rounds "
                   "(one process each, the trees alternating).  score: one TrackScorer.update behind an eager BatchedTracker(max_age=2); "
                   "step: the captured SequenceTrainer.step",
           "streams": a.streams, "points": a.points, "boxes": a.boxes, "max_objects": a.max_objects, "iters": a.iters, "rounds": a.rounds,
           "device": next(iter(runs.values()))[0]["device"], "configurations": {}}
    for key, rs in runs.items():
        c = {}
        for k in ("rtk_track_score_ms", "rtk_track_score_memory_ms", "step_ms"):
            if k in rs[0]:
                ms = [x[k] for x in rs]
                c.update({k + "_median": round(statistics.median(ms), 4), k + "_min": min(ms), k + "_max": max(ms), k + "_runs": ms})
        for k in ("live_pairs", "detected_objects", "previous_rows", "coasted_rows", "target_ones", "tracking_loss", "check"):
            if k in rs[0]:
                c[k] = rs[-1][k]
        res["configurations"][key] = c
    if a.parent:
        cf = res["configurations"]
        for name, key, k in (("rtk_track_score", "score", "rtk_track_score_ms"), ("step_reacquire_none", "step/reacquire=none", "step_ms")):
            p, t = cf["parent/" + key], cf["this/" + key]
            res[name + "_inside_parent_spread"] = bool(p[k + "_min"] <= t[k + "_median"] <= p[k + "_max"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
