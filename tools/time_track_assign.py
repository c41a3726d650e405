"""The batched tracker's two association modes side by side (ratrack_amd/tracker.py `BatchedTracker(assign=...)`;
csrc/track_batched.hip rtk_associate_batched, csrc/track_assign.hip rtk_associate_optimal): what the exact assignment costs against the
500 log-Sinkhorn iterations it replaces, per launch and per tracked step, and what its worst cases cost.

    python tools/time_track_assign.py [--streams 64] [--points 256] [--max-objects 128] [--iters 50] [--warmup 5] [--rounds 3]
                                      [--steps 20] [--repeats 3] [--worst-k 197] [--worst-iters 10]
                                      [--out profiles/track_assign_timing.json]

The operating point is tools/time_tracker.py's: its synthetic clouds and weights, --streams sequences of --points points.  Measured on
the machine it runs on, in one process:

  (a) per launch, device time between events around the entry point, medians of --iters after --warmup, --rounds rounds with the two
      entry points alternating inside every round, both on the SAME inputs -- the aff, counts, obj and previous IDs that a tracked step
      of the Sinkhorn tracker handed its association launch (the last of a few steps):
      associate_batched     `rtk_associate_batched`, iters = 500, alpha = 0.9
      associate_optimal     `rtk_associate_optimal`, min_affinity = 0.01
      and, from their outputs, how often the two decisions agree and what the Sinkhorn decision's matching weighs on the exact
      assignment's scale;
  (b) tracked frame-pairs/s of the whole `step()` in both modes, eager and captured (`graph=True`), as tools/time_tracker.py times
      them: a host clock around --steps steps ending in a synchronise, --repeats runs, the modes alternating;
  (c) the exact solve's worst cases at K = --worst-k, every stream holding the same full block: dense random, and the product matrix
      aff[i][j] ~ (i + 1)(j + 1); beside each time the search rounds of la_solve_dense counted on the host statement
      (tests/_track_assign_util.device_method), and the Sinkhorn launch on the same block for scale.

Writes one JSON object to --out and prints it.  Not part of bench.py."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _track_assign_util as U  # noqa: E402
from ratrack_amd import _lib, abi, synth, tracker as T  # noqa: E402
from ratrack_amd.track4d import Args, Track4D  # noqa: E402
from time_track_sweep import block_us, summary  # noqa: E402

DEV = "cuda"


class Launch:
    """One set of association inputs and the two entry points on it, each with output buffers of its own."""

    def __init__(self, aff, num, prev_count, prev_ids, obj):
        self.B, self.K = aff.shape[0], aff.shape[1]
        self.N = obj.shape[1]
        self.aff, self.num, self.prev_count, self.prev_ids, self.obj = aff, num, prev_count, prev_ids, obj
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=DEV)
        B, K, N = self.B, self.K, self.N
        self.out = {k: dict(counter=i32(B), ids=i32(B, K), count=i32(B), object_ids=i32(B, K), object_conf=torch.zeros(B, K, device=DEV),
                            indices1=i32(B, K), num_prev=i32(B), point_track_id=i32(B, N)) for k in ("batched", "optimal")}
        self.total = torch.zeros(B, dtype=torch.int64, device=DEV)
        self.st = abi.stream()

    def _head(self):
        return (self.B, self.N, self.K, None, None, self.aff.data_ptr(), self.num.data_ptr(), self.obj.data_ptr(), self.prev_ids.data_ptr(),
                self.prev_count.data_ptr())

    def _tail(self, o):
        return tuple(o[k].data_ptr() for k in ("counter", "ids", "count", "object_ids", "object_conf", "indices1", "num_prev", "point_track_id"))

    def batched(self):
        _lib.call("rtk_associate_batched", *self._head(), 0.9, 500, *self._tail(self.out["batched"]), None, self.st)

    def optimal(self):
        _lib.call("rtk_associate_optimal", *self._head(), 0.01, *self._tail(self.out["optimal"]), self.total.data_ptr(), self.st)

    def decisions(self):
        """How the two decisions compare on this launch's inputs."""
        self.batched()
        self.optimal()
        torch.cuda.synchronize()
        aff, num, m = self.aff.cpu().numpy(), self.num.tolist(), self.prev_count.tolist()
        ib, cb = self.out["batched"]["indices1"].tolist(), self.out["batched"]["object_conf"].tolist()
        io, total = self.out["optimal"]["indices1"].tolist(), self.total.tolist()
        same = solved = weight_b = weight_o = matched_b = matched_o = 0
        for b in range(self.B):
            if not (m[b] and num[b]):
                continue
            solved += 1
            w = U.quantise(aff[b, :m[b], :num[b]])
            kept = [i if cb[b][j] != 0.0 else -1 for j, i in enumerate(ib[b][:num[b]])]      # an ID is inherited only with conf != 0
            same += kept == io[b][:num[b]]
            weight_b += U.check_matching(w, kept)
            weight_o += total[b]
            matched_b += sum(1 for i in kept if i >= 0)
            matched_o += sum(1 for i in io[b][:num[b]] if i >= 0)
        return dict(streams_associated=solved, streams_with_the_same_decision=same, matched_pairs_sinkhorn=matched_b,
                    matched_pairs_optimal=matched_o, weight_sinkhorn=weight_b, weight_optimal=weight_o,
                    weight_ratio=round(weight_b / weight_o, 6) if weight_o else None)


def full_block(block, B, K):
    """Every stream holds `block` (K x K): the inputs of a launch with nothing but full streams."""
    aff = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(block, (B, K, K)))).to(DEV)
    full = torch.full((B,), K, dtype=torch.int32, device=DEV)
    ids = torch.arange(K, dtype=torch.int32, device=DEV).repeat(B, 1).contiguous()
    obj = torch.full((B, 64), -1, dtype=torch.int32, device=DEV)
    return Launch(aff, full, full.clone(), ids, obj)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--max-objects", type=int, default=128)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--worst-k", type=int, default=197)
    ap.add_argument("--worst-iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join("profiles", "track_assign_timing.json"))
    a = ap.parse_args()
    B, N, K = a.streams, a.points, a.max_objects
    net = Track4D(Args()).to(DEV).eval()
    synth.fill_state_dict(net.state_dict())
    with torch.no_grad():
        net.fd_layer.cp.linear.bias += 0.09
    net.invalidate_fused()
    frames = []
    for s in range(4):
        d = synth.make_frame_pairs(B, N, case_id=100 + s)
        frames.append([torch.from_numpy(d[k]).to(DEV) for k in ("pc1", "pc2", "feature1", "feature2")])

    # ---- (a) the two launches on what a tracked step hands its association ----
    trk = T.BatchedTracker(net, streams=B, max_objects=K)
    with torch.no_grad():
        for i in range(4):
            prev_ids, prev_count = trk.ids[1 - trk.cur].clone(), trk.count[1 - trk.cur].clone()
            out = trk.step(*frames[i % 4])
    trk.check()
    op = Launch(out.aff.clone(), out.num_objects.clone(), prev_count, prev_ids, out.obj.clone())
    decisions = op.decisions()
    variants = {"associate_batched": lambda: block_us(op.batched, a.iters, a.warmup),
                "associate_optimal": lambda: block_us(op.optimal, a.iters, a.warmup)}
    runs = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, block in variants.items():
            runs[k].append(block())
    launches = summary(runs)
    rounds_op = [U.device_method(U.quantise(op.aff[b, :int(op.prev_count[b]), :int(op.num[b])].cpu().numpy()))[2] for b in range(B)]

    # ---- (b) the whole step in both modes ----
    def stepper(**kw):
        t = T.BatchedTracker(net, streams=B, max_objects=K, **kw)
        with torch.no_grad():
            for i in range(a.warmup + (3 if kw.get("graph") else 0)):
                t.step(*frames[i % 4])
        torch.cuda.synchronize()
        return t
    modes = {"eager_sinkhorn": stepper(), "eager_optimal": stepper(assign="optimal"), "graph_sinkhorn": stepper(graph=True),
             "graph_optimal": stepper(graph=True, assign="optimal")}
    step_runs = {k: [] for k in modes}
    with torch.no_grad():
        for _ in range(a.repeats):
            for k, t in modes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(a.steps):
                    t.step(*frames[i % 4])
                torch.cuda.synchronize()
                step_runs[k].append(time.perf_counter() - t0)
    for t in modes.values():
        t.check()
    steps = {k: dict(ms_per_step_runs=[round(1e3 * r / a.steps, 3) for r in v], ms_per_step=round(1e3 * statistics.median(v) / a.steps, 3),
                     pairs_per_s=round(B * a.steps / statistics.median(v), 1)) for k, v in step_runs.items()}

    # ---- (c) the worst cases of the exact solve ----
    KW = a.worst_k
    rng = np.random.default_rng(7)
    blocks = {"dense_random": (0.02 + 0.97 * rng.random((KW, KW))).astype(np.float32), "product_matrix": U.product_matrix(KW, KW)}
    worst = {}
    for name, block in blocks.items():
        lw = full_block(block, B, KW)
        w = U.quantise(block)
        host_total, _, host_rounds = U.device_method(w)
        us = {"associate_optimal": [], "associate_batched": []}
        for _ in range(a.rounds):
            us["associate_optimal"].append(block_us(lw.optimal, a.worst_iters, 2))
            us["associate_batched"].append(block_us(lw.batched, a.worst_iters, 2))
        torch.cuda.synchronize()
        assert set(lw.total.tolist()) == {host_total}, (name, host_total, lw.total.tolist()[:4])
        worst[name] = dict(search_rounds=host_rounds, total=host_total, launches=summary(us),
                           ns_per_round=round(1e3 * statistics.median(us["associate_optimal"]) / host_rounds, 1))

    med = lambda k: launches[k]["median_us"]
    res = {"what": "rtk_associate_optimal (an exact assignment) against rtk_associate_batched (500 log-Sinkhorn iterations, mutual best) on the "
                   "same inputs, the tracked step in both modes, and the exact solve's worst cases",
           "streams": B, "points": N, "max_objects": K, "iters": a.iters, "warmup": a.warmup, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0),
           "operating_point": {"mean_objects": round(float(op.num.float().mean()), 2), "mean_previous": round(float(op.prev_count.float().mean()), 2),
                               "max_objects_in_a_stream": int(op.num.max()), "search_rounds_mean": round(float(np.mean(rounds_op)), 1),
                               "search_rounds_max": int(max(rounds_op)), "lds_bytes_optimal": _lib._fn("rtk_associate_optimal_lds_bytes")(K)},
           "launches": launches,
           "ratio_optimal_over_batched": round(med("associate_optimal") / med("associate_batched"), 4),
           "decisions": decisions,
           "steps": steps,
           "step_ratio_optimal_over_sinkhorn": {m: round(steps[m + "_optimal"]["ms_per_step"] / steps[m + "_sinkhorn"]["ms_per_step"], 4)
                                                for m in ("eager", "graph")},
           "worst_k": KW, "worst_iters": a.worst_iters, "worst_cases": worst,
           "not_measured": "tracking quality on real sequences: the tree holds three example frames and no checkpoint"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
