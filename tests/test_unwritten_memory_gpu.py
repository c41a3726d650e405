"""GPU: nothing in the training, tracking and scoring paths depends on memory nobody wrote.

The package takes uninitialised device memory at some 135 sites (torch.empty / empty_like), many of them written in part by design:
workgroup partials, inverse index tables without their padding and duplicate positions, saved activations and sign masks, the
per-pair workspace of the tracking term.  A test that repeats one step on one batch cannot see a stray read of such a buffer: the
caching allocator hands the step the blocks its predecessor used, and they hold last step's -- correct -- values.  Here every case
runs under the `poison` allocator of tools/hazard_harness.py, which fills what torch.empty and its kin hand out before the caller
sees it (eager execution only, never inside a graph capture).

The rule for a deterministic case (built once): two clean runs agree bit for bit; the runs under the poisons (NaN, 1), (1e30, 3) and
(-7.5, 2) -- float fill, integer fill -- equal the first clean run bit for bit in every recorded tensor, compared as integer views
(NaN-safe): outputs, loss items, every parameter gradient, every BatchNorm running statistic, every state tensor kept between
frames, and after an optimizer step the parameters and the Adam moments.  Where a contract leaves part of a tensor undefined (the
padding columns of a padded batch's outputs, the rows of the tracker's (B, K) tables past a stream's object count), the recorded
tensor is that part zeroed on the device.

The integer fill is a valid value of whatever it could be read as -- an index below every indexed extent, never negative -- so that
a stray read changes a result instead of faulting: every poisoned case has points per cloud, n_valid, distinct points (= unique
centroids per level) and the CAPACITIES of its object, box, ground-truth track and pair tables at 4 or more, asserted by the case
builders (assert_extents) -- the capacity is what an index is in range of.  The live counts are asserted from the first clean run
where the case is about them (live_counts): objects per clustered stream, kept ground-truth objects and live pairs of the tracker
and sequence cases.  The fixtures of the ground-truth and scorer cases keep their streams without boxes or detections.

The default path (train_ops.DETERMINISTIC = False: float atomics, bits differ from run to run) runs under (NaN, 1) and (NaN, 3):
every recorded tensor finite, the four loss items within 1e-5 max(|x|, 1) of the clean run
(tests/test_varn_train_gpu.py::test_padded_batch_equals_unpadded_batch's bound for loss items).  A case whose clean runs differ
although it was meant to be deterministic stands under this rule too (the module path, see DEFAULT_PATH_CASES).
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ratrack_amd import synth
from ratrack_amd.track4d import Args, Track4D

from _util import REAL_CASES, inputs_of, load_case, reference_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
POISONS = [(NAN, 1), (1e30, 3), (-7.5, 2)]
DEFAULT_PATH_POISONS = [(NAN, 1), (NAN, 3)]
LOSS_KEYS = ("Loss", "SceneFlowLoss", "TrackingLoss", "SegLoss")
OUTPUTS = ("flow", "h", "cls", "cor", "pc1_features", "pc2_features", "prop")
CLS_SHIFT = 0.09          # moving points in every frame (tests/test_tracker_gpu.py)


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def _poison(float_fill, int_fill):
    from hazard_harness import poison
    return poison(float_fill, int_fill)


def _bits(t):
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32)
    if t.dtype == torch.float64:
        return t.contiguous().view(torch.int64)
    return t.to(torch.uint8) if t.dtype == torch.bool else t


def differing(ref, cur):
    """Names of the recorded tensors of `cur` that are not bit for bit those of `ref`."""
    assert list(ref) == list(cur), sorted(set(ref) ^ set(cur))
    return [k for k in ref if ref[k].shape != cur[k].shape or ref[k].dtype != cur[k].dtype or not torch.equal(_bits(ref[k]), _bits(cur[k]))]


def _record(d):
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in d.items()}


def evaluate(run, poisons=POISONS):
    """-> (names that differ between two clean runs, {poison: names that differ from the first clean run})."""
    ref = run()
    clean = differing(ref, run())
    out = {}
    for p in poisons:
        with _poison(*p) as active:
            cur = run()
        assert active.fills > 0, "the case took no uninitialised device memory through the patched allocators"
        out[p] = differing(ref, cur)
    return clean, out


def check_deterministic(name, run, poisons=POISONS):
    clean, bad = evaluate(run, poisons)
    assert not clean, "%s: two clean runs differ in %d tensors: %s" % (name, len(clean), clean[:8])
    for p, names in bad.items():
        assert not names, "%s under poison %s: %d recorded tensors depend on unwritten memory: %s" % (name, p, len(names), names[:8])


def evaluate_default_path(run, poisons=DEFAULT_PATH_POISONS):
    """-> [(poison or None for the clean run, non-finite tensors, loss items off by more than 1e-5 max(|x|, 1))]."""
    rows, ref = [], None
    for p in [None] + list(poisons):
        if p is None:
            cur = ref = run()
        else:
            with _poison(*p) as active:
                cur = run()
            assert active.fills > 0, "the case took no uninitialised device memory through the patched allocators"
        nonfinite = [k for k, v in cur.items() if v.is_floating_point() and not bool(torch.isfinite(v).all())]
        off = []
        for k in LOSS_KEYS:
            a, b = float(cur["loss/" + k]), float(ref["loss/" + k])
            if not abs(a - b) <= 1e-5 * max(abs(b), 1.0):
                off.append((k, a, b))
        rows.append((p, nonfinite, off))
    return rows


def check_default_path(name, run):
    for p, nonfinite, off in evaluate_default_path(run):
        assert not nonfinite, "%s under poison %s: non-finite %s" % (name, p, nonfinite[:8])
        assert not off, "%s under poison %s: loss items moved: %s" % (name, p, off)


# ---- extents ----------------------------------------------------------------------------------------------------------------------
def assert_extents(**extents):
    """Every indexed extent of a poisoned case is at least 4: the integer fills 1, 2, 3 are valid indices wherever they are read."""
    for k, v in extents.items():
        lo = int(min(np.asarray(v).reshape(-1).tolist()))
        assert lo >= 4, "%s = %d: an integer poison of up to 3 would be out of range" % (k, lo)


def live_counts(what, counts, allow_zero=False):
    """Live extents read off a clean run: every count at 4 or more (allow_zero: or 0 -- a stream that sits the frame out)."""
    v = [int(c) for c in torch.as_tensor(counts).reshape(-1).tolist()]
    assert all(c >= 4 or (allow_zero and c == 0) for c in v), "%s = %s: live extents below 4" % (what, v)


def distinct_points(pc, n_valid=None):
    """Smallest number of distinct points among the clouds of pc (B, 3, N) (their first n_valid[b] columns): FPS picks every distinct
    point before it repeats one, so this is also the number of unique centroids of every level (npoint = 512 >= N here, or N > 512)."""
    a = pc.detach().cpu().numpy()
    counts = []
    for b in range(a.shape[0]):
        n = a.shape[2] if n_valid is None else int(n_valid[b])
        counts.append(len(np.unique(a[b, :, :n].T, axis=0)))
    return min(counts)


def _rows(t, counts):
    """t (B, K, ...) with the rows from counts[b] on zeroed."""
    keep = torch.arange(t.shape[1], device=t.device)[None, :] < counts.long()[:, None]
    return torch.where(keep.view(keep.shape + (1,) * (t.dim() - 2)), t, torch.zeros_like(t))


def _cols(t, counts):
    """t (B, ..., N) with the columns from counts[b] on zeroed."""
    keep = torch.arange(t.shape[-1], device=t.device)[None, :] < counts.long()[:, None]
    return torch.where(keep.view((t.shape[0],) + (1,) * (t.dim() - 2) + (t.shape[-1],)), t, torch.zeros_like(t))


# ---- nets and batches -------------------------------------------------------------------------------------------------------------
def make_net(cls_shift=0.0):
    sd = reference_state_dict(DEV)
    if cls_shift:
        sd["fd_layer.cp.linear.bias"] = sd["fd_layer.cp.linear.bias"] + cls_shift
    net = Track4D(Args()).to(DEV)
    net.load_state_dict(sd, strict=True)
    return net


def snapshot(net):
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def synth_batch(B, N, case_id, duplicates=0):
    d = synth.make_frame_pairs(B, N, case_id)
    if duplicates:                                                 # exact duplicates: FPS runs out of points, dead and redirected rows
        for k in ("pc1", "pc2", "feature1", "feature2"):
            d[k][:, :, N - duplicates:] = d[k][:, :, :duplicates]
    return {k: torch.from_numpy(v).to(DEV) for k, v in d.items()}


def real_pair(name):
    case = load_case(name)
    pc1, pc2, f1, f2 = inputs_of(case, DEV)
    return dict(pc1=pc1, pc2=pc2, feature1=f1, feature2=f2, gt_warp=torch.from_numpy(case["in_gt_warp"]).to(DEV),
                gt_cls=torch.from_numpy(case["in_gt_cls"]).to(DEV))


def padded_real_batch(width=384):
    """The three shipped pairs (322/352, 352/242, 242/322 points) as one batch of `width` columns, padded with copies of column 0."""
    pairs = [real_pair(n) for n in REAL_CASES]
    pad = lambda t: torch.cat([t, t[..., :1].expand(*t.shape[:-1], width - t.shape[-1])], dim=-1)
    t = {k: torch.cat([pad(p[k]) for p in pairs], 0).contiguous() for k in pairs[0]}
    t["n_valid"] = torch.tensor([[p["pc1"].shape[2] for p in pairs], [p["pc2"].shape[2] for p in pairs]], dtype=torch.int32, device=DEV)
    assert t["n_valid"][0].tolist() == [322, 352, 242] and t["pc1"].shape[2] == width
    return t


# ---- case 1: the backbone's train step ------------------------------------------------------------------------------------------------
def backbone_case(t, deterministic=True, dedup=True, cv_split=None):
    """-> run(): forward, fused backbone_loss, backward of one Track4D from the reference weights; records the seven outputs (a padded
    batch: their valid columns), the four loss items, every parameter gradient and every BatchNorm buffer."""
    from ratrack_amd import train_ops
    net = make_net().train()
    sd0 = snapshot(net)
    nv = t.get("n_valid")
    assert_extents(points=[t["pc1"].shape[2], t["pc2"].shape[2]], n_valid=[4] if nv is None else nv.cpu().numpy(),
                   distinct=[distinct_points(t["pc1"], None if nv is None else nv[0]), distinct_points(t["pc2"], None if nv is None else nv[1])])

    def run():
        net.load_state_dict(sd0, strict=True)
        net.train()
        net._dedup_train = dedup
        net.zero_grad(set_to_none=True)
        prev = train_ops.set_deterministic(deterministic)
        prev_split = train_ops.CV_SPLIT
        if cv_split is not None:
            train_ops.CV_SPLIT = cv_split
        try:
            kw = {} if nv is None else {"n_valid": nv}
            out = net.backbone(t["pc1"], t["pc2"], t["feature1"], t["feature2"], None, **kw)
            total, items = train_ops.backbone_loss(t["pc1"], out[0], out[2], t["gt_warp"], t["gt_cls"], pretrain=False,
                                                   n_valid=None if nv is None else nv[0].contiguous())
            total.backward()
        finally:
            train_ops.set_deterministic(prev)
            train_ops.CV_SPLIT = prev_split
            net._dedup_train = True
        rec = {}
        for k, v in zip(OUTPUTS, out):
            if nv is not None and k != "h":
                v = _cols(v, nv[1] if k == "pc2_features" else nv[0])
            rec["out/" + k] = v
        rec.update({"loss/" + k: items[k].reshape(1) for k in LOSS_KEYS})
        grads = {"grad/" + k: p.grad for k, p in net.named_parameters() if p.grad is not None}
        assert len(grads) > 150
        rec.update(grads)
        rec.update({"stat/" + k: v for k, v in net.state_dict().items() if "running_" in k or "num_batches" in k})
        return _record(rec)
    return run


BACKBONE_CASES = {
    "b2_n256": lambda: backbone_case(synth_batch(2, 256, 2031)),
    "b3_n77": lambda: backbone_case(synth_batch(3, 77, 2032)),                       # partial last tile, U = N < npoint
    "b2_n256_duplicates": lambda: backbone_case(synth_batch(2, 256, 9, duplicates=56)),      # nuniq < U: redirected and dead rows
    "b1_n1024": lambda: backbone_case(synth_batch(1, 1024, 2033)),                   # FPS down-samples, fp1 interpolates through its table
    "real_549_1047": lambda: backbone_case(real_pair("real_549_1047")),              # N1 != N2: padded inside the backbone
    "padded_real_batch": lambda: backbone_case(padded_real_batch()),                 # live / row0, masked kNN, point weights, device counts
    "b2_n256_fp32_cost_volume": lambda: backbone_case(synth_batch(2, 256, 2031), cv_split=False),
}
DEFAULT_PATH_CASES = {
    "b2_n256": lambda: backbone_case(synth_batch(2, 256, 2031), deterministic=False),
    "padded_real_batch": lambda: backbone_case(padded_real_batch(), deterministic=False),
    "b1_n2304": lambda: backbone_case(synth_batch(1, 2304, 5), deterministic=False),       # above the inverse-table limit: the fallbacks
    # The module path (net._dedup_train = False: the framework's layers, the scattering backwards of grouping_operation and
    # three_interpolate with float atomics) is not reproducible even with DETERMINISTIC set: two clean runs differ in 129 of the
    # recorded tensors, the parameter gradients from pn_head.sa1 on (measured on an MI355X).  It therefore stands under this rule.
    "b2_n256_module_path": lambda: backbone_case(synth_batch(2, 256, 2031), dedup=False),
}


@pytest.mark.parametrize("name", list(BACKBONE_CASES))
def test_backbone_train_step_reads_no_unwritten_memory(name):
    check_deterministic("backbone train step " + name, BACKBONE_CASES[name]())


@pytest.mark.parametrize("name", list(DEFAULT_PATH_CASES))
def test_default_path_train_step_stays_finite_under_poison(name):
    check_default_path("default-path train step " + name, DEFAULT_PATH_CASES[name]())


# ---- case 2: two optimizer steps ----------------------------------------------------------------------------------------------------
def optimizer_state(opt):
    return {"opt/%s/%s" % (i, k): v for i, st in opt.state_dict()["state"].items() for k, v in st.items() if torch.is_tensor(v)}


def trainer_case(B=2, N=256):
    from ratrack_amd.train import Trainer
    net = make_net()
    sd0 = snapshot(net)
    batches = [synth_batch(B, N, 40 + i) for i in range(2)]
    assert_extents(points=[N], distinct=[distinct_points(t[k]) for t in batches for k in ("pc1", "pc2")])

    def run():
        net.load_state_dict(sd0, strict=True)
        net.zero_grad(set_to_none=True)
        tr = Trainer(net, graph=False, lr=1e-3, deterministic=True)
        h = torch.zeros(5, B, 128, device=DEV)
        rec = {}
        for i, t in enumerate(batches):
            items, h = tr.step(t["pc1"], t["pc2"], t["feature1"], t["feature2"], t["gt_warp"], t["gt_cls"], h)
            rec.update({"step%d/loss/%s" % (i, k): items[k].reshape(1).clone() for k in LOSS_KEYS})
            rec["step%d/h" % i] = h.clone()
        rec.update({"state/" + k: v for k, v in net.state_dict().items()})
        rec.update({"grad/" + k: p.grad for k, p in net.named_parameters() if p.grad is not None})
        opt = optimizer_state(tr.opt)
        assert len(opt) > 300
        rec.update(opt)
        return _record(rec)
    return run


def test_two_trainer_steps_read_no_unwritten_memory():
    """FusedAdam, the zero arena and the deferred weight gradients: Trainer(deterministic=True, graph=False), two steps."""
    check_deterministic("two Trainer steps", trainer_case())


# ---- case 6: the fused engine's eval forward --------------------------------------------------------------------------------------
def eval_case(inputs, h, n_valid=None):
    net = make_net().eval()
    assert_extents(points=[inputs[0].shape[2]], n_valid=[4] if n_valid is None else n_valid.cpu().numpy(),
                   distinct=[distinct_points(inputs[i], None if n_valid is None else n_valid[i]) for i in (0, 1)])

    def run():
        net.invalidate_fused()                                     # the engine folds and packs its images again: under poison too
        with torch.no_grad():
            out = net.backbone(*inputs, h) if n_valid is None else net.backbone(*inputs, h, n_valid=n_valid)
        return _record({"out/" + k: v for k, v in zip(OUTPUTS, out)})
    return run


def test_eval_forward_reads_no_unwritten_memory():
    """tools/experiments/dbg_uninit2.py as a test: the golden case with duplicate points, and the padded batch of the shipped frames."""
    import hazard_harness as H
    from ratrack_amd import vod_gt
    check_deterministic("eval forward eval_b1_n256_dups", eval_case(inputs_of(load_case("eval_b1_n256_dups"), DEV), None))
    pc1, pc2, f1, f2, nv = vod_gt.pad_frame_pairs(H.real_pairs(), device=DEV)
    h3 = torch.randn(5, 3, 128, device=DEV, generator=torch.Generator(DEV).manual_seed(17)) * 0.1
    check_deterministic("eval forward padded real batch", eval_case((pc1, pc2, f1, f2), h3, nv))


# ---- case 4: the batched tracker --------------------------------------------------------------------------------------------------
def step_result_record(out, prefix):
    """What a StepResult defines: the (B, K) tables up to each stream's object count, the affinities of its live block."""
    n, m = out.num_objects, out.num_prev
    rec = {k: getattr(out, k) for k in ("flow", "cls", "h", "point_track_id", "num_objects", "num_prev", "flags", "obj")}
    rec.update(object_ids=_rows(out.object_ids, n), object_conf=_rows(out.object_conf, n), indices1=_rows(out.indices1(), n),
               aff=_rows(_rows(out.aff, m).transpose(1, 2), n).transpose(1, 2))
    return {prefix + k: v.clone() for k, v in rec.items()}


def tracker_state(trk, prefix):
    return {prefix + k: getattr(trk, k).clone() for k in ("h", "desc", "ids", "count", "counter")}


def tracker_case():
    from ratrack_amd import tracker as T, vod_gt
    net = make_net(CLS_SHIFT).eval()
    B, FRAMES, sizes = 4, 3, [256, 200, 131, 97]
    seqs = []
    for s, n in enumerate(sizes):
        d = synth.make_frame_pairs(FRAMES, n, case_id=60 + s)
        t = {k: torch.from_numpy(v) for k, v in d.items()}
        if s == 3:                                                 # points hundreds of clustering radii apart: a stream without clusters
            t["pc1"], t["pc2"] = t["pc1"] * 1000.0, t["pc2"] * 1000.0
        seqs.append([(t["pc1"][i:i + 1], t["pc2"][i:i + 1], t["feature1"][i:i + 1], t["feature2"][i:i + 1]) for i in range(FRAMES)])
    frames = [vod_gt.pad_frame_pairs([seqs[s][f] for s in range(B)], device=DEV) for f in range(FRAMES)]
    assert_extents(points=[frames[0][0].shape[2]], n_valid=[fr[4].cpu().numpy() for fr in frames], objects=[128],
                   distinct=[distinct_points(fr[i], fr[4][i]) for fr in frames for i in (0, 1)])

    def run():
        net.invalidate_fused()
        trk = T.BatchedTracker(net, streams=B)
        rec = {}
        for f, (pc1, pc2, f1, f2, nv) in enumerate(frames):
            out = trk.step(pc1, pc2, f1, f2, n_valid=nv)
            rec.update(step_result_record(out, "frame%d/" % f))
            rec.update(tracker_state(trk, "frame%d/state/" % f))
        trk.check()
        return _record(rec)
    return run


def test_batched_tracker_reads_no_unwritten_memory():
    """BatchedTracker.step over three frames of four streams of 256, 200, 131 and 97 points, the last without a cluster."""
    run = tracker_case()
    first = run()
    num = torch.stack([first["frame%d/num_objects" % f] for f in range(3)])
    assert bool((num[:, 3] == 0).all()), num.tolist()
    live_counts("objects of the clustered streams", num[:, :3])
    check_deterministic("BatchedTracker three frames", run)


# ---- case 5: ground truth, metrics, the tracking score --------------------------------------------------------------------------------
GOBJ = ("slot", "label_id", "count", "size", "members", "centre", "flags")
MATCH = ("pred_gt_slot", "pred_gt_id", "gt_pred", "iou", "aff_target", "aff_defined")
SCORER_STATE = ("counters", "iou_sum", "table_key", "table_last", "table_seen", "table_matched", "table_used", "prev_gt", "flags",
                "prev_gt_id", "prev_count")


def ground_truth_case():
    import _gt_util as U
    from ratrack_amd import gt_device as G
    B, N, K = 8, 256, 32
    d = U.synthetic_batch(B, N, K, seed=77)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    pc1, pc2, nv = dev(d["pc1"]), dev(d["pc2"]), dev(d["n_valid"])
    g = torch.Generator().manual_seed(3)
    noise, cls = (0.05 * torch.randn(B, 3, N, generator=g)).to(DEV), torch.rand(B, N, generator=g).to(DEV)
    assert_extents(points=[N], n_valid=d["n_valid"], boxes=[K])

    def run():
        bb = G.pack_boxes(d["per_stream"], K, DEV)
        gt = G.ground_truth(pc1, pc2, bb, n_valid=nv)
        fm = G.frame_metrics(pc1, gt.gt_warp + noise, gt.gt_warp, 1.0 - gt.gt_cls.float(), cls, gt.gt_cls, n_valid=nv)
        acc = G.MetricAccumulator(B, device=DEV)
        acc.update(fm)
        rec = {"gt/" + k: getattr(gt, k) for k in ("gt_cls", "box_index", "obj_id", "gt_warp", "pc1_comp", "counts1", "counts2", "flags")}
        rec.update({"metrics/values": fm.values, "metrics/sums": fm.sums, "acc/value_sum": acc.value_sum, "acc/raw_sum": acc.raw_sum})
        return _record(rec)
    return run


def track_score_case():
    import _track_score_util as S
    from ratrack_amd import gt_device as G, track_score as TS
    B, N, K = 8, 128, 8
    seq = S.synthetic_sequence(B, N, K, 3)
    frames = seq["frames"][:2]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    assert_extents(points=[N], n_valid=[fr["n_valid"] for fr in frames], boxes=[K], objects=[K], gt_tracks=[16])

    def run():
        scorer = TS.TrackScorer(streams=B, max_objects=K, max_boxes=K, max_gt_tracks=16)
        rec = {}
        for f, fr in enumerate(frames):
            pc1, nv = dev(fr["pc1"]), dev(fr["n_valid"])
            bb = G.pack_boxes(fr["per_stream"], K, DEV)
            gobj = TS.gt_objects(pc1, bb, TS.pack_box_types(fr["per_stream"], K, DEV), n_valid=nv, min_obj_points=S.MIN_PTS)
            m = scorer.update_raw(pc1, dev(fr["obj"]), dev(fr["num"]), dev(fr["ids"]), gobj, nv, dev(fr["reset"]), dev(fr["active"]))
            rec.update({"frame%d/gobj/%s" % (f, k): getattr(gobj, k) for k in GOBJ})
            rec.update({"frame%d/match/%s" % (f, k): getattr(m, k) for k in MATCH})
            rec.update({"frame%d/scorer/%s" % (f, k): getattr(scorer, k).clone() for k in SCORER_STATE})
        scorer.check()
        return _record(rec)
    return run


def test_ground_truth_and_metrics_read_no_unwritten_memory():
    check_deterministic("ground_truth + frame_metrics", ground_truth_case())


def test_track_scorer_reads_no_unwritten_memory():
    check_deterministic("gt_objects + TrackScorer two frames", track_score_case())


# ---- case 3: the sequence trainer ---------------------------------------------------------------------------------------------------
def sequence_case(B=2, FRAMES=3):
    """SequenceTrainer.step with the tracking term: the same labelled batch three times; frame 0 resets every stream, stream 1 sits
    frame 1 out, stream 0 is reset in frame 2.  The per-pair workspace keeps its default size; it is a module-level cache
    (track_train._WORKSPACE) that lives as long as the process, so every run drops it and takes a new one -- under poison through the
    patched torch.empty: a cached one would hold the previous run's rows and partials, which are the right ones.
    (tests/_track_train_util.py's builders, blob_frame and pair_case, make the inputs of the kernel pins, not of SequenceTrainer.step:
    the labelled batch is built here, as tests/test_track_train_gpu.py::batch builds it.)"""
    import _gt_util as GU
    from ratrack_amd import gt_device as G, track_score as TS, track_train as TT, vod_gt
    net = make_net(CLS_SHIFT).train()
    sd0 = snapshot(net)
    t = {k: torch.from_numpy(v) for k, v in synth.make_frame_pairs(B, 256, case_id=50).items()}
    pairs = [(t["pc1"][i:i + 1], t["pc2"][i:i + 1], t["feature1"][i:i + 1], t["feature2"][i:i + 1]) for i in range(B)]
    per_stream = []
    for b in range(B):
        p = t["pc1"][b].numpy()
        mk = lambda k: vod_gt.Label("rider" if k == 2 else "Car", k, 0, 0, 0, 0, 0, 0, 3.0, 4.0, 6.0, float(p[0, 10 * k]), float(p[1, 10 * k]),
                                    float(p[2, 10 * k]), 0.3 * k)
        labels = {k: mk(k) for k in range(6)}
        per_stream.append((labels, GU.IDENTITY_TF, labels, GU.IDENTITY_TF))
    pc1, pc2, f1, f2, nv = vod_gt.pad_frame_pairs(pairs, device=DEV)
    bb = G.pack_boxes(per_stream, 8, DEV)
    gt = G.ground_truth(pc1, pc2, bb, n_valid=nv)
    gobj = TS.gt_objects(pc1, bb, TS.pack_box_types(per_stream, 8, DEV), n_valid=nv, min_obj_points=net.min_obj_points)
    data = (pc1, pc2, f1, f2, gt.gt_warp, gt.gt_cls, gobj)
    resets = [[1] * B, [0] * B, [1] + [0] * (B - 1)]
    actives = [[1] * B, [1, 0] + [1] * (B - 2), [1] * B]
    assert_extents(points=[pc1.shape[2]], n_valid=nv.cpu().numpy(), distinct=[distinct_points(pc1, nv[0]), distinct_points(pc2, nv[1])],
                   objects=[128], boxes=[8], gt_tracks=[32], pairs=[TT.default_max_pairs(B, 128)])

    live_counts("kept ground-truth objects", gobj.count)

    def run():
        TT._WORKSPACE.clear()
        net.load_state_dict(sd0, strict=True)
        net.zero_grad(set_to_none=True)
        tr = TT.SequenceTrainer(net, streams=B, max_boxes=8, max_gt_tracks=32, deterministic=True)
        h, rec = None, {}
        for f in range(FRAMES):
            items, h, out, match = tr.step(*data, h, n_valid=nv, reset=torch.tensor(resets[f], dtype=torch.bool),
                                           active=torch.tensor(actives[f], dtype=torch.bool))
            p = "frame%d/" % f
            rec.update({p + "loss/" + k: items[k].reshape(1).clone() for k in LOSS_KEYS})
            rec[p + "h_out"] = h.clone()
            rec.update(step_result_record(out, p + "out/"))
            rec.update({p + "match/" + k: getattr(match, k).clone() for k in MATCH})
            rec.update(tracker_state(tr.tracker, p + "tracker/"))
            rec.update({p + "scorer/" + k: getattr(tr.scorer, k).clone() for k in SCORER_STATE})
        tr.check()
        rec.update({"state/" + k: v for k, v in net.state_dict().items()})
        rec.update({"grad/" + k: q.grad for k, q in net.named_parameters() if q.grad is not None})
        rec.update(optimizer_state(tr.opt))
        return _record(rec)
    return run


def test_sequence_trainer_reads_no_unwritten_memory():
    run = sequence_case()
    first = run()
    assert float(first["frame1/loss/TrackingLoss"]) > 0 and float(first["frame0/loss/TrackingLoss"]) == 0, "the tracking term never ran"
    for f in range(3):
        n, m = first["frame%d/out/num_objects" % f], first["frame%d/out/num_prev" % f]
        live_counts("objects in frame %d" % f, n, allow_zero=True)
        live_counts("live pairs in frame %d" % f, n * m, allow_zero=True)
    assert int((first["frame1/out/num_objects"] * first["frame1/out/num_prev"]).sum()) >= 4
    check_deterministic("SequenceTrainer three frames", run)
