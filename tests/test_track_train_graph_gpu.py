"""GPU: the sequence train step replayed from a hipGraph (track_train.SequenceTrainer(graph=True)) against the same step run eagerly.

Both trainers are deterministic (`Trainer(deterministic=True)`: a step is reproducible bit for bit), start from the same weights and
see the same batches, and a replay launches the kernels the eager step launches: every output and, after the run, every parameter
must be bit-equal."""
import numpy as np
import pytest
import torch

import _gt_util as GU
from _util import reference_state_dict
from ratrack_amd import gt_device as G, synth, track_score as TS, track_train as TT, vod_gt
from ratrack_amd.track4d import Args, Track4D

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 4
STEPS = 7
RESET, INACTIVE = (1, 5), (2, 6)          # (stream, step)
ITEMS = ("Loss", "SceneFlowLoss", "SegLoss", "TrackingLoss")


def ref_net():
    sd = reference_state_dict(DEV)
    sd["fd_layer.cp.linear.bias"] = sd["fd_layer.cp.linear.bias"] + 0.09      # moving points in every frame (tests/test_tracker_gpu.py)
    net = Track4D(Args()).to(DEV)
    net.load_state_dict(sd, strict=True)
    return net.train()


def batch():
    """The recipe of tests/test_track_train_gpu.py: synthetic pairs, six labelled boxes per stream."""
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
    types = TS.pack_box_types(per_stream, 8, DEV)
    gt = G.ground_truth(pc1, pc2, bb, n_valid=nv)
    gobj = TS.gt_objects(pc1, bb, types, n_valid=nv, min_obj_points=2)
    return (pc1, pc2, f1, f2, gt.gt_warp, gt.gt_cls, gobj), nv


def record(res):
    items, h, out, match = res
    rec = {k: items[k].clone() for k in ITEMS}
    rec.update(h=h.clone(), point_track_id=out.point_track_id.clone(), object_ids=out.object_ids.clone(),
               aff_target=match.aff_target.clone(), pred_gt_id=match.pred_gt_id.clone())
    return rec


def test_the_captured_sequence_step_equals_the_eager_one():
    data, nv = batch()
    nets = [ref_net(), ref_net()]
    assert all(torch.equal(a, b) for a, b in zip(nets[0].state_dict().values(), nets[1].state_dict().values()))
    kw = dict(streams=B, max_boxes=8, max_gt_tracks=32, deterministic=True)
    eager = TT.SequenceTrainer(nets[0], **kw)
    graph = TT.SequenceTrainer(nets[1], graph=True, graph_warmup=2, **kw)
    aff = lambda net: [p.detach().clone() for p in net.affinity.parameters()]
    hs = [None, None]
    captured, replayed_term, moved = [], [], []
    for t in range(STEPS + 1):
        mk = dict(n_valid=nv)
        if t == 0:
            mk["reset"] = torch.ones(B, dtype=torch.bool)
        if t == RESET[1]:
            mk["reset"] = [s == RESET[0] for s in range(B)]
        if t == INACTIVE[1]:
            mk["active"] = [s != INACTIVE[0] for s in range(B)]
        if t == STEPS:                      # one more step with pretrain: a new key, hence an eager warm-up step of the captured trainer
            mk["pretrain"] = True
        before = aff(nets[1])
        recs = []
        for i, tr in enumerate((eager, graph)):
            res = tr.step(*data, hs[i], **mk)
            recs.append(record(res))
            hs[i] = res[1]
        captured.append(graph.captured)
        for k in recs[0]:
            assert torch.equal(recs[0][k], recs[1][k]), (t, k)
        if graph.captured:
            replayed_term.append(float(recs[1]["TrackingLoss"]))
            moved.append(all(not torch.equal(a, b) for a, b in zip(before, aff(nets[1]))))
    print("   captured", captured, "TrackingLoss on the replayed steps", replayed_term, "Affinity moved", moved)
    # step 0 has h=None (its own key), steps 1 and 2 warm the key with h up, step 3 captures and replays
    assert captured == [False, False, False, True, True, True, True, False]
    assert captured[RESET[1]] and captured[INACTIVE[1]]
    assert max(replayed_term) > 0 and any(moved)
    for (name, a), (_, b) in zip(nets[0].state_dict().items(), nets[1].state_dict().items()):
        assert torch.equal(a, b), name
    ra, rb = eager.scorer.result(), graph.scorer.result()
    np.testing.assert_equal(ra, rb)
    assert ra["overall"]["frames"] > 0
    eager.check()
    graph.check()
