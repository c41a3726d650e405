"""The result log (ratrack_amd/result_log.py) against the tracked step it follows and against the per-step writer it replaces.

    python tools/time_result_log.py [--streams 64] [--points 256] [--max-objects 128] [--frames 100] [--iters 100] [--warmup 10]
                                    [--moving-bias 4.0] [--out profiles/result_log_timing.json]

B streams of synthetic frames (synth.make_frame_pairs, a few distinct batches cycled), synthetic weights with the segmentation head's
bias raised so that every stream has objects to cluster and associate.  Measured on the machine it runs on:

  (a) the eager tracker: device time between events around `step` and around `step` + `append`, median of --iters after --warmup, and
      per launch (`_lib.TIMING`) the four association launches next to rtk_result_log_append;
  (b) the captured tracker (`graph=True`): the same two, by events and by wall clock per step (the host's share of an append: its
      argument checks and, with `seq` / `index` as host values, one small host-to-device copy; with device tensors none);
  (c) `select` on the finished log (one launch), and `write` split into download / format (paths checked, texts rendered) / file I/O;
  (d) the job end to end on the captured tracker, wall clock: --frames steps with per-step `write_results`, against the same steps
      with `append` and one `write` at the end; the two directory trees are compared byte for byte.

Writes one JSON object to --out and prints it.  Not part of bench.py."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from ratrack_amd import _lib, result_log as RL, synth, tracker as T  # noqa: E402
from ratrack_amd.track4d import Args, Track4D  # noqa: E402

ASSOC = ("rtk_dbscan_batched", "rtk_object_descriptors", "rtk_affinity_pairs", "rtk_associate_batched")
BATCHES = 8


def events(fn, iters, warmup):
    """-> (median ms between events around fn, median wall ms per call with one synchronisation at the end of the run)."""
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
    h0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    wall = 1e3 * (time.perf_counter() - h0) / iters
    return statistics.median(e0.elapsed_time(e1) for e0, e1 in pairs), wall


def per_launch(fn, iters):
    _lib.TIMING = []
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    per = {}
    for name, e0, e1 in _lib.TIMING:
        per.setdefault(name, []).append(e0.elapsed_time(e1))
    _lib.TIMING = None
    return {k: round(statistics.median(v), 4) for k, v in per.items()}


def tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for n in files:
            p = os.path.join(d, n)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--max-objects", type=int, default=128)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--moving-bias", type=float, default=4.0)
    ap.add_argument("--out", default=os.path.join("profiles", "result_log_timing.json"))
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
    names = ["seq%02d" % b for b in range(B)]
    seq_host = list(range(B))
    seq_dev = torch.arange(B, dtype=torch.int32, device=dev)
    index_dev = torch.zeros(B, dtype=torch.int32, device=dev)
    new_log = lambda frames: RL.ResultLog(B, K, frames, frames * K, frames * N, device=dev)
    res = {"what": "result log: append next to the tracked step, select, write; the job against per-step write_results",
           "streams": B, "points": N, "max_objects": K, "frames": F, "iters": a.iters, "device": torch.cuda.get_device_name(0)}

    # ---- (a), (b): step and step + append ----
    for name, kw in (("a_eager", {}), ("b_graph", dict(graph=True))):
        trk = T.BatchedTracker(net, streams=B, max_objects=K, **kw)
        log = new_log(4 * (a.iters + a.warmup) + 8)
        count = [0]

        def step():
            count[0] += 1
            return trk.step(*batches[count[0] % BATCHES])

        def step_append_host():
            log.append(step(), seq=seq_host, index=count[0])

        def step_append_device():
            log.append(step(), seq=seq_dev, index=index_dev)
        with torch.no_grad():
            step_ms, step_wall = events(step, a.iters, a.warmup)
            trk.check()
            log.clear()
            host_ms, host_wall = events(step_append_host, a.iters, a.warmup)
            log.check()
            log.clear()
            dev_ms, dev_wall = events(step_append_device, a.iters, a.warmup)
            log.check()
            r = dict(step_ms=round(step_ms, 4), step_append_ms=round(dev_ms, 4), step_append_host_words_ms=round(host_ms, 4),
                     step_wall_ms=round(step_wall, 4), step_append_wall_ms=round(dev_wall, 4), step_append_host_words_wall_ms=round(host_wall, 4),
                     detected_objects_last_step=int(trk.last.num_objects.sum()), object_points_last_step=int((trk.last.obj >= 0).sum()))
            if not kw:
                log.clear()
                launch = per_launch(step_append_device, max(20, a.iters // 4))
                r["launch_ms_median"] = {k: launch.get(k) for k in ASSOC + ("rtk_result_log_append",)}
                r["cheapest_association_launch_ms"] = min(launch[k] for k in ASSOC)
        res[name] = r

    # ---- (d) the job, twice, on fresh captured trackers; (c) on the second one's log ----
    def job(write_per_step, root, frames=F):
        trk = T.BatchedTracker(net, streams=B, max_objects=K, graph=True)
        log = new_log(frames)
        with torch.no_grad():
            for i in range(a.warmup):
                trk.step(*batches[i % BATCHES])
            torch.cuda.synchronize()
            h0 = time.perf_counter()
            for t in range(frames):
                out = trk.step(*batches[t % BATCHES], reset=[t == 0] * B)
                if write_per_step:
                    trk.write_results(root, names, [t] * B, out)
                else:
                    log.append(out, seq=seq_host, index=t, reset=[t == 0] * B)
            torch.cuda.synchronize()
            steps_s = time.perf_counter() - h0
        return trk, log, steps_s

    with tempfile.TemporaryDirectory() as tmp:
        root_a, root_b = os.path.join(tmp, "per_step"), os.path.join(tmp, "log")
        job(True, os.path.join(tmp, "warm"), 5)                 # first touch of every code path and of the file system
        _, _, per_step_s = job(True, root_a)
        _, log, loop_s = job(False, root_b)
        h0 = time.perf_counter()
        host, keep, flags = log.download()
        h1 = time.perf_counter()
        RL.raise_on_flags(flags.tolist(), K)
        where = RL.check_paths(root_b, names, host)
        texts = RL.render_frames(host)
        h2 = time.perf_counter()
        for b, f, path in where:
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "w+") as fh:
                fh.write(texts[(b, f)])
        h3 = time.perf_counter()
        ta, tb = tree(root_a), tree(root_b)
        h4 = time.perf_counter()
        log.write(os.path.join(tmp, "again"), names)
        whole_write_s = time.perf_counter() - h4
        records, points = int(host["cursor"][:, 1].sum()), int(host["cursor"][:, 2].sum())
        res["d_job"] = dict(per_step_write_results_s=round(per_step_s, 4), append_loop_s=round(loop_s, 4), download_s=round(h1 - h0, 4),
                            format_s=round(h2 - h1, 4), file_io_s=round(h3 - h2, 4), append_and_one_write_s=round(loop_s + (h3 - h0), 4),
                            write_call_s=round(whole_write_s, 4), files=len(tb), bytes=sum(len(v) for v in tb.values()),
                            records=records, points=points, files_identical=bool(ta == tb and len(ta) == B * F),
                            speedup=round(per_step_s / (loop_s + (h3 - h0)), 2))
        # the operating point: the median score of the tracks of two frames or more, handed over as a 0-dim device tensor (the
        # batches carry no motion from one to the next, so most objects start a track and a track rarely lasts)
        live = torch.arange(log.R, device=dev)[None, :] < log.cursor[:, 1:2]
        plain = log.select(check=False)
        lengths = plain.track_frames[live]
        lasting = live & (plain.track_frames >= 2)
        thr = plain.track_score[lasting].median() if bool(lasting.any()) else torch.zeros((), dtype=torch.float64, device=dev)
        sel_ms, _ = events(lambda: log.select(threshold=thr, min_track_frames=2, check=False), max(20, a.iters // 4), 5)
        h0 = time.perf_counter()
        log.write(os.path.join(tmp, "filtered"), names, threshold=thr, min_track_frames=2)
        res["c_select"] = dict(select_ms=round(sel_ms, 4), filtered_write_call_s=round(time.perf_counter() - h0, 4), threshold=float(thr),
                               min_track_frames=2, kept_records=int(log.select(threshold=thr, min_track_frames=2).keep.sum()), records=records,
                               records_by_track_frames={"1": int((lengths == 1).sum()), "2": int((lengths == 2).sum()),
                                                        "3_or_more": int((lengths >= 3).sum())})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
