"""GPU: the tracker's in-place state, the captured step and the pipeline of captured groups (ratrack_amd/tracker.py).

The bar is bit equality with the default eager `BatchedTracker`: the same kernels run on the same inputs -- the state advance is a
copy, a replay launches what the capture recorded -- and the forward's outputs do not depend on what else shares the device."""
import os

import pytest
import torch

from _util import reference_state_dict
from ratrack_amd import synth, tracker as T, vod_gt
from ratrack_amd.track4d import Args, Track4D

pytestmark = pytest.mark.gpu
DEV = "cuda"
CLS_SHIFT = 0.09          # tests/test_tracker_gpu.py: moving points in every frame
SIZES = [256, 200, 160, 97]
STEPS = 6
RESET, INACTIVE = (1, 3), (2, 4)          # (stream, step); stream 2 is active again at step 5
TENSORS = ("flow", "cls", "h", "labels", "obj", "point_track_id", "num_objects", "num_prev", "object_ids", "object_conf", "flags")


def new_net(sd=None):
    if sd is None:
        sd = reference_state_dict(DEV)
        sd["fd_layer.cp.linear.bias"] = sd["fd_layer.cp.linear.bias"] + CLS_SHIFT
    net = Track4D(Args()).to(DEV)
    net.load_state_dict(sd, strict=True)
    return net.eval()


def synth_pairs(count, n, case_id):
    d = synth.make_frame_pairs(count, n, case_id=case_id)
    t = {k: torch.from_numpy(v) for k, v in d.items()}
    return [(t["pc1"][i:i + 1], t["pc2"][i:i + 1], t["feature1"][i:i + 1], t["feature2"][i:i + 1]) for i in range(count)]


def frames(sizes, steps, first_case):
    """[(pc1, pc2, feature1, feature2, n_valid)] per step, the streams padded to one N."""
    seqs = [synth_pairs(steps, n, first_case + s) for s, n in enumerate(sizes)]
    return [vod_gt.pad_frame_pairs([seq[t] for seq in seqs], device=DEV) for t in range(steps)]


def masks(t, B):
    reset = torch.tensor([s == RESET[0] and t == RESET[1] for s in range(B)])
    active = torch.tensor([not (s == INACTIVE[0] and t == INACTIVE[1]) for s in range(B)])
    return reset, active


def snapshot(out, trk):
    """Clones of everything the comparison reads (the next step may overwrite the tensors in place)."""
    snap = {k: getattr(out, k).clone() for k in TENSORS}
    snap["indices1"] = out.indices1().clone()
    snap["counter"] = trk.counter.clone()
    m, n = out.num_prev.tolist(), out.num_objects.tolist()
    snap["aff_live"] = [out.aff[b, :m[b], :n[b]].clone() for b in range(trk.B)]
    snap["desc_live"] = [out.descriptors[b, :n[b]].clone() for b in range(trk.B)]
    return snap


def assert_same(got, want, where):
    for k in TENSORS + ("indices1", "counter"):
        assert torch.equal(got[k], want[k]), (where, k)
    for k in ("aff_live", "desc_live"):
        for b, (x, y) in enumerate(zip(got[k], want[k])):
            assert x.shape == y.shape and torch.equal(x, y), (where, k, b)


def host_objects(out, B):
    res = []
    for b in range(B):
        objects, confs = out.objects(b)
        res.append(([(k, v.clone()) for k, v in objects.items()], [float(c) for c in confs]))
    return res


def result_files(trk, root, t, out):
    paths = trk.write_results(str(root), ["seq%d" % s for s in range(trk.B)], [t] * trk.B, out)
    return {os.path.relpath(p, str(root)): open(p, "rb").read() for p in paths}


@pytest.fixture(scope="module")
def eager(tmp_path_factory):
    """The default tracker (references swapped, every step eager) on the sequence, computed once: per step the cloned tensors, the
    host-side objects of every stream and the result files."""
    B = len(SIZES)
    net = new_net()
    seq = frames(SIZES, STEPS, 40)
    trk = T.BatchedTracker(net, streams=B)
    root = tmp_path_factory.mktemp("eager")
    steps = []
    with torch.no_grad():
        for t, (pc1, pc2, f1, f2, nv) in enumerate(seq):
            reset, active = masks(t, B)
            out = trk.step(pc1, pc2, f1, f2, n_valid=nv, reset=reset, active=active)
            trk.check()
            steps.append(dict(snap=snapshot(out, trk), objects=host_objects(out, B), files=result_files(trk, root, t, out)))
    return dict(sd={k: v.clone() for k, v in net.state_dict().items()}, seq=seq, steps=steps, B=B)


def test_static_state_equals_the_reference_swap(eager):
    B = eager["B"]
    trk = T.BatchedTracker(new_net(eager["sd"]), streams=B, static_state=True)
    with torch.no_grad():
        for t, (pc1, pc2, f1, f2, nv) in enumerate(eager["seq"]):
            reset, active = masks(t, B)
            out = trk.step(pc1, pc2, f1, f2, n_valid=nv, reset=reset, active=active)
            assert_same(snapshot(out, trk), eager["steps"][t]["snap"], t)
            assert trk.cur == 0 and not trk.captured


def test_replay_equals_eager(eager, tmp_path):
    B = eager["B"]
    trk = T.BatchedTracker(new_net(eager["sd"]), streams=B, graph=True, graph_warmup=2)
    captured, inherited, fresh_with_prev, total = [], 0, 0, 0
    with torch.no_grad():
        for t, (pc1, pc2, f1, f2, nv) in enumerate(eager["seq"]):
            reset, active = masks(t, B)
            out = trk.step(pc1, pc2, f1, f2, n_valid=nv, reset=reset, active=active)
            captured.append(trk.captured)
            want = eager["steps"][t]
            assert_same(snapshot(out, trk), want["snap"], t)
            trk.check()
            # the host-side accessors: a cache left over from an earlier replay would answer with that step's sizes
            for b, ((objs, confs), (wobjs, wconfs)) in enumerate(zip(host_objects(out, B), want["objects"])):
                assert [k for k, _ in objs] == [k for k, _ in wobjs], (t, b)
                assert all(torch.equal(x, y) for (_, x), (_, y) in zip(objs, wobjs)), (t, b)
                assert confs == wconfs, (t, b)
            assert result_files(trk, tmp_path, t, out) == want["files"], t
            m, n = out.num_prev.tolist(), out.num_objects.tolist()
            for b in range(B):
                conf = out.object_conf[b, :n[b]]
                inherited += int((conf > 0).sum())
                fresh_with_prev += int((conf == 0).sum()) if m[b] > 0 else 0
                total += n[b]
    print("   captured", captured, "inherited ids", inherited, "fresh ids beside previous objects", fresh_with_prev, "objects", total)
    assert captured == [False, False] + [True] * (STEPS - 2)
    assert captured[RESET[1]] and captured[INACTIVE[1]]
    assert inherited > 0 and fresh_with_prev > 0 and total > 0


def test_pipeline_groups_equal_their_eager_trackers(eager):
    G, B, STEPS_G = 2, 2, 5
    net = new_net(eager["sd"])
    seqs = [frames([256, 200], STEPS_G, 60), frames([256, 97], STEPS_G, 70)]
    want = []
    with torch.no_grad():
        for g in range(G):
            ref = T.BatchedTracker(net, streams=B)
            want.append([snapshot(ref.step(*fr[:4], n_valid=fr[4]), ref) for fr in seqs[g]])
        pipe = T.TrackerPipeline(net, groups=G, streams=B)
        got = [[] for _ in range(G)]
        replays = 0
        for t in range(STEPS_G):
            outs = [pipe.submit(g, *seqs[g][t][:4], n_valid=seqs[g][t][4]) for g in range(G)]      # both groups in flight
            for g in range(G):
                replays += pipe.trackers[g].captured
                with torch.cuda.stream(pipe.streams[g]):
                    got[g].append(snapshot(outs[g], pipe.trackers[g]))
        pipe.drain()
        torch.cuda.synchronize()
    assert replays == G * (STEPS_G - 2)
    for g in range(G):
        for t in range(STEPS_G):
            assert_same(got[g][t], want[g][t], (g, t))
    assert sum(int(s["num_objects"].sum()) for s in want[0] + want[1]) > 0
    with pytest.raises(ValueError, match="groups=5"):
        T.TrackerPipeline(net, groups=5, streams=B)
