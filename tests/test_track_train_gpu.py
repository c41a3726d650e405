"""GPU: the tracking term of B sequences (ratrack_amd/track_train.py, csrc/track_train.hip).

The arbiter is a float64 restatement of the reference formulation on the CPU with autograd (tests/_track_train_util.py); the yardstick
for every gradient tensor is the same formulation in float32 torch, the reference's own arithmetic: the HIP result must stay within
4x float32 torch's distance from float64, or within 1e-6 (_track_train_util.bound).

Measured on an MI355X (max|g - g64| / max|g64|; ours / float32 torch): see DESIGN.md section 4.10."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import _gt_util as GU
import _track_train_util as U
from _util import reference_state_dict
from ratrack_amd import _lib, gt_device as G, synth, tracker as T, track_score as TS, track_train as TT, train_ops, vod_gt
from ratrack_amd.track4d import Args, Track4D

pytestmark = pytest.mark.gpu
DEV = "cuda"
PARAMS = ["%d.%s" % (i, k) for i in (0, 2, 4, 6, 8) for k in ("weight", "bias")]


def ref_net():
    sd = reference_state_dict(DEV)
    sd["fd_layer.cp.linear.bias"] = sd["fd_layer.cp.linear.bias"] + 0.09      # moving points in every frame (tests/test_tracker_gpu.py)
    net = Track4D(Args()).to(DEV)
    net.load_state_dict(sd, strict=True)
    return net.train()


@pytest.fixture(scope="module")
def net():
    return ref_net()


def u8(v):
    return torch.tensor(v, dtype=torch.uint8, device=DEV)


# ---- 1, 2, 4, 5: the affinity backward ---------------------------------------------------------------------------------------------
def run_pairs(net, case, defined, max_pairs=None):
    d = case["dev"]
    return TT.affinity_backward(T.pack_affinity(net.affinity).to(DEV), TT.pack_affinity_bwd(net.affinity), d["prev"], d["prev_count"], d["curr"],
                                d["num_objects"], d["target"], u8(defined), d["scale"], reset=d["reset"], max_pairs=max_pairs)


def pairs_output(net, case):
    d = case["dev"]
    aff = torch.zeros(case["B"], case["K"], case["K"], device=DEV)
    _lib.call("rtk_affinity_pairs", case["B"], case["K"], T.pack_affinity(net.affinity).to(DEV).data_ptr(), d["prev"].data_ptr(),
              d["prev_count"].data_ptr(), d["reset"].data_ptr(), d["curr"].data_ptr(), d["num_objects"].data_ptr(), aff.data_ptr(),
              torch.cuda.current_stream().cuda_stream)
    return aff


_ARBITER = {}


def arbiter(net, defined, dtype):
    """(losses, d_desc, the ten parameter gradients) of the torch formulation on the CPU; computed once per configuration."""
    key = (defined, dtype)
    if key not in _ARBITER:
        case = U.pair_case("cpu")
        mlp = U.mlp_copy(net.affinity, dtype)
        desc = case["curr"].to(dtype).requires_grad_(True)
        total, losses = U.desc_term(mlp, desc, case["prev"].to(dtype), case["m"], case["num_objects"], case["target"], defined, case["scale"])
        total.backward()
        _ARBITER[key] = ([float(l) for l in losses], desc.grad.clone(), [p.grad.clone() for p in mlp.parameters()])
    return _ARBITER[key]


def expected_losses(aff, case, defined):
    out = []
    for b in range(case["B"]):
        m, n = case["m"][b], case["num_objects"][b]
        on = defined[b] and m * n > 0
        out.append(F.binary_cross_entropy(aff[b, :m, :n].reshape(-1), case["dev"]["target"][b, :m, :n].reshape(-1)).item() if on else 0.0)
    return out


@pytest.mark.parametrize("defined", [(1, 1, 1, 1), (0, 1, 1, 1)])
def test_affinity_backward_matches_the_float64_arbiter(net, defined):
    case = U.pair_case(DEV)
    loss, d_desc, d_w, flags = run_pairs(net, case, defined)
    assert flags.tolist() == [0, 0, 0, 0]
    # the loss: the cross entropy of rtk_affinity_pairs' own output (the project's descriptor tolerance: the summation order only)
    aff = pairs_output(net, case)
    want = expected_losses(aff, case, defined)
    only, _ = TT.affinity_loss_only(aff, case["dev"]["target"], u8(defined), case["dev"]["prev_count"], case["dev"]["num_objects"],
                                    reset=case["dev"]["reset"])
    print("   losses", loss.tolist(), "expected", want)
    for b in range(case["B"]):
        assert abs(loss[b].item() - want[b]) <= 1e-5 * abs(want[b]), (b, loss[b].item(), want[b])
        assert abs(only[b].item() - want[b]) <= 1e-5 * abs(want[b]), (b, only[b].item(), want[b])
    assert want[3] == 0.0 and (defined[0] or want[0] == 0.0) and want[1] > 0 and want[2] > 0
    # gradients against the arbiter
    _, dd64, g64 = arbiter(net, defined, torch.float64)
    _, dd32, g32 = arbiter(net, defined, torch.float32)
    U.check_grad("d_desc", d_desc, dd32, dd64)
    for name, ours, a32, a64 in zip(PARAMS, TT.unpack_affinity_grad(d_w), g32, g64):
        U.check_grad(name, ours, a32, a64)
    # everything past the live blocks, and the whole of a stream that sits the term out, is zero
    for b in range(case["B"]):
        n = case["num_objects"][b] if (defined[b] and case["m"][b]) else 0
        assert (d_desc[b, n:] == 0).all(), b
        if n:
            assert (d_desc[b, :n] != 0).any(), b


def test_saturated_affinities_keep_loss_and_gradients_finite(net):
    case = U.pair_case(DEV, diff_scale=1e4)
    defined = (1, 1, 1, 1)
    aff = pairs_output(net, case)
    m, n = case["m"][1], case["num_objects"][1]
    a = aff[1, :m, :n].reshape(-1)
    sat0, sat1 = int((a == 0).sum()), int((a == 1).sum())
    print("   stream 1: %d of %d affinities are exactly 0, %d exactly 1" % (sat0, a.numel(), sat1))
    assert sat0 + sat1 > 0
    loss, d_desc, d_w, _ = run_pairs(net, case, defined)
    want = expected_losses(aff, case, defined)
    for b in range(case["B"]):
        assert abs(loss[b].item() - want[b]) <= 1e-5 * abs(want[b]), (b, loss[b].item(), want[b])
    assert torch.isfinite(loss).all() and torch.isfinite(d_desc).all() and torch.isfinite(d_w).all()
    # the gradient of the pre-sigmoid, read off the workspace rows (stream 1 starts behind stream 0's 40 pairs), against torch's
    # binary_cross_entropy and sigmoid backward on the same affinities: the -100 and 1e-12 clamps
    rows = TT.workspace(torch.device(DEV, torch.cuda.current_device()), TT.default_max_pairs(case["B"], case["K"]))
    first = case["m"][0] * case["num_objects"][0]
    dz = rows[:(first + m * n) * TT.ROW].view(-1, TT.ROW)[first:, 2043]
    leaf = a.clone().requires_grad_(True)
    (case["scale"][1] * F.binary_cross_entropy(leaf, case["dev"]["target"][1, :m, :n].reshape(-1))).backward()
    ref = leaf.grad * (1 - a) * a
    assert torch.isfinite(ref).all()
    assert torch.allclose(dz, ref, rtol=1e-5, atol=1e-20), (dz - ref).abs().max().item()


def test_streams_beyond_the_pair_cap_are_flagged_and_the_others_untouched(net):
    case = U.pair_case(DEV)
    defined = (1, 1, 1, 1)
    full = run_pairs(net, case, defined)
    loss, d_desc, d_w, flags = run_pairs(net, case, defined, max_pairs=448)       # 40 + 408 fit exactly, stream 2's 49 do not
    assert flags.tolist() == [0, 0, 1, 0]
    with pytest.raises(RuntimeError, match=r"stream 2 fell beyond max_pairs=448"):
        TT.check(T.StepResult(pair_flags=flags, max_pairs=448))
    assert torch.equal(loss[:2], full[0][:2]) and torch.equal(d_desc[:2], full[1][:2])
    assert loss[2] == 0 and (d_desc[2] == 0).all() and torch.isfinite(d_w).all()
    _, _, _, flags = run_pairs(net, case, defined, max_pairs=447)
    assert flags.tolist() == [0, 1, 1, 0]
    with pytest.raises(RuntimeError, match=r"streams 1, 2 fell beyond max_pairs=447"):
        TT.check(T.StepResult(pair_flags=flags, max_pairs=447))
    TT.check(T.StepResult(pair_flags=full[3], max_pairs=1 << 15))


# ---- 3: the descriptor backward ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def descriptor_case():
    n_valid = [256, 140, 200]
    B, N, K = 3, 256, 64
    pc1, flow, f1, prop, cls = U.blob_frame(B, N, n_valid, movers=[0.8, 0.9, 0.5], seed=11, device=DEV)
    nv = torch.tensor(n_valid, dtype=torch.int32, device=DEV)
    act = torch.ones(B, dtype=torch.uint8, device=DEV)
    fr = T.TrackFrame(B, N, T._view(pc1), T._view(flow), T._view(f1), T._view(prop), T._view(cls), nv.data_ptr(), act.data_ptr())
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=DEV)
    labels, obj, num, flags = i32(B, N), i32(B, N), i32(B), i32(B)
    _lib.call("rtk_dbscan_batched", ctypes.addressof(fr), 0.5, 1.5, 2, K, labels.data_ptr(), obj.data_ptr(), num.data_ptr(),
              flags.data_ptr(), None, 0, torch.cuda.current_stream().cuda_stream)
    objh, numh = obj.cpu(), num.cpu().tolist()
    assert flags.tolist() == [0, 0, 0] and min(numh) > 0
    # the constructed tie, in stream 0: the object with the most members; its last two members share the largest value of three
    # channels, and one channel is 0 for every member (prop channels from 1 on do not enter the clustering)
    sizes = torch.bincount(objh[0][objh[0] >= 0])
    k = int(sizes.argmax())
    members = torch.nonzero(objh[0] == k).reshape(-1).tolist()
    assert len(members) >= 3
    pa, pb = members[-2], members[-1]
    for c in (10, 11, 12):
        prop[0, c, pa] = prop[0, c, pb] = 7.0
    prop[0, 20, members] = 0.0
    g = torch.Generator().manual_seed(5)
    d_desc = torch.randn(B, K, 141, generator=g).to(DEV)
    active = [1, 1, 0]                                      # stream 2 sits out although it has objects: all zeros
    out = T.StepResult(aff=torch.empty(B, K, K, device=DEV), obj=obj, num_objects=num, pc1=pc1, flow=flow, feature1=f1, prop=prop, cls=cls,
                       active=u8(active))
    return dict(B=B, N=N, K=K, out=out, d_desc=d_desc, obj=objh, num=numh, active=active, tie=(k, members, pa, pb), n_valid=n_valid)


def descriptor_arbiter(dtype):
    c = descriptor_case()
    o = c["out"]
    flow, prop = o.flow.cpu().to(dtype).requires_grad_(True), o.prop.cpu().to(dtype).requires_grad_(True)
    descs = U.descriptors_of(o.pc1.cpu().to(dtype), flow, o.feature1.cpu().to(dtype), prop, c["obj"], c["num"], c["active"])
    total = sum((d * c["d_desc"][b, :d.shape[0]].cpu().to(dtype)).sum() for b, d in enumerate(descs) if d is not None)
    total.backward()
    return flow.grad, prop.grad


def test_descriptor_backward_matches_the_arbiter_with_ties_to_the_lowest_index():
    c = descriptor_case()
    d_flow, d_prop = TT.descriptors_backward(c["out"], c["d_desc"])
    f64, p64 = descriptor_arbiter(torch.float64)
    f32, p32 = descriptor_arbiter(torch.float32)
    U.check_grad("d_flow", d_flow, f32, f64)
    U.check_grad("d_prop", d_prop, p32, p64)
    assert torch.equal(d_prop.cpu().double(), p64)          # copies of d_desc: exact
    k, members, pa, pb = c["tie"]
    for ch in (10, 11, 12):
        assert d_prop[0, ch, pa] == c["d_desc"][0, k, 6 + ch] and d_prop[0, ch, pb] == 0, ch
    assert d_prop[0, 20, members[0]] == c["d_desc"][0, k, 26] and (d_prop[0, 20, members[1:]] == 0).all()
    for b in range(c["B"]):
        off = (c["obj"][b] < 0).to(DEV)
        assert (d_flow[b][:, off] == 0).all() and (d_prop[b][:, off] == 0).all(), b      # non-object points and padding columns
        assert bool(off[c["n_valid"][b]:].all())
    assert (d_flow[2] == 0).all() and (d_prop[2] == 0).all() and (d_flow[0] != 0).any() and (d_prop[1] != 0).any()


# ---- 5: the same bits on a second run ----------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(net):
    case = U.pair_case(DEV)
    a, b = run_pairs(net, case, (1, 1, 1, 1)), run_pairs(net, case, (1, 1, 1, 1))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    c = descriptor_case()
    x, y = TT.descriptors_backward(c["out"], c["d_desc"]), TT.descriptors_backward(c["out"], c["d_desc"])
    assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])


# ---- 6 .. 9: the sequence step -----------------------------------------------------------------------------------------------------
def batch(B=4):
    """The inputs of test_track_score_gpu.py's `tracked` fixture: synthetic pairs, six labelled boxes per stream."""
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
    net = ref_net()
    gt = G.ground_truth(pc1, pc2, bb, n_valid=nv)
    gobj = TS.gt_objects(pc1, bb, types, n_valid=nv, min_obj_points=net.min_obj_points)
    return net, (pc1, pc2, f1, f2, gt.gt_warp, gt.gt_cls, gobj), nv


def aff_params(net):
    return [p for _, p in net.affinity.named_parameters()]


def stream_losses(out, match):
    return TT.affinity_loss_only(out.aff, match.aff_target, match.aff_defined, out.num_prev, out.num_objects, active=out.active)[0]


@pytest.fixture(scope="module")
def sequence():
    """Four frames through one SequenceTrainer(deterministic=True): 0 every stream reset, 1 pretrain, 2 a plain step, 3 forward and
    backward alone (no optimizer step) for the gradient comparison."""
    B = 4
    net, data, nv = batch(B)
    tr = TT.SequenceTrainer(net, streams=B, max_boxes=8, max_gt_tracks=32, deterministic=True)
    snap = lambda: [p.detach().clone() for p in aff_params(net)]
    rec = dict(net=net, tr=tr, data=data, nv=nv, B=B)
    p0 = snap()
    items, h, out, match = tr.step(*data, None, n_valid=nv, reset=torch.ones(B, dtype=torch.bool))
    rec["first"] = dict(items={k: float(v) for k, v in items.items()}, grads=[None if p.grad is None else p.grad.clone() for p in aff_params(net)],
                        before=p0, after=snap(), defined=match.aff_defined.tolist())
    tr.check()
    p1 = snap()
    items, h, out, match = tr.step(*data, h, pretrain=True, n_valid=nv)
    rec["pretrain"] = dict(items={k: float(v) for k, v in items.items()}, before=p1, after=snap(), losses=stream_losses(out, match).clone(),
                           defined=match.aff_defined.tolist())
    p2 = snap()
    items, h, out, match = tr.step(*data, h, n_valid=nv)
    rec["plain"] = dict(items={k: float(v) for k, v in items.items()}, before=p2, after=snap(), defined=match.aff_defined.tolist())
    tr.check()
    reset, active = torch.zeros(B, dtype=torch.uint8, device=DEV), torch.ones(B, dtype=torch.uint8, device=DEV)
    items, _, out, match = tr._forward_backward(*data, h, nv, False, reset, active)
    rec["fb"] = dict(items={k: float(v) for k, v in items.items()}, out=out, match=match, h=h,
                     grads={n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None},
                     desc_prev=out.desc_prev.clone(), defined=match.aff_defined.tolist())
    return rec


def test_affinity_term_runs_without_host_synchronisation(sequence):
    out, match, net = sequence["fb"]["out"], sequence["fb"]["match"], sequence["net"]
    flow, prop = out.flow.clone().requires_grad_(True), out.prop.clone().requires_grad_(True)
    ones = torch.ones(sequence["B"], device=DEV)
    for p in aff_params(net):
        p.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = TT.affinity_term(net.affinity, out, match, flow, prop)
        loss.backward(ones)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert flow.grad is not None and prop.grad is not None and all(p.grad is not None for p in aff_params(net))
    assert torch.isfinite(loss).all() and float(loss.sum()) > 0


def test_whole_step_gradients_match_backbone_loss_plus_the_torch_term(sequence):
    rec, fb = sequence, sequence["fb"]
    net, data, nv, B = rec["net"], rec["data"], rec["nv"], rec["B"]
    pc1, pc2, f1, f2, gt_warp, gt_cls, _ = data
    out, match = fb["out"], fb["match"]
    assert any(fb["defined"]) and fb["items"]["TrackingLoss"] > 0, (fb["defined"], fb["items"])
    obj, num, num_prev = out.obj.cpu(), out.num_objects.tolist(), out.num_prev.tolist()
    target = match.aff_target
    # the composite on the same weights and batch: train-mode backbone + backbone_loss + 0.5 x the float32 torch term, by autograd
    prev = train_ops.set_deterministic(True)
    try:
        net.zero_grad(set_to_none=True)
        flow, _, cls, _, _, _, prop = net.backbone(pc1, pc2, f1, f2, fb["h"], n_valid=nv)
        total, _ = train_ops.backbone_loss(pc1, flow, cls, gt_warp, gt_cls, n_valid=nv[0].contiguous())
        term, _ = U.frame_term(net.affinity.affinity, pc1, flow, f1, prop, obj.to(DEV), num, fb["desc_prev"], num_prev, target, fb["defined"])
        (total + 0.5 * term).backward()
    finally:
        train_ops.set_deterministic(prev)
    ref = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
    assert set(ref) == set(fb["grads"]), set(ref) ^ set(fb["grads"])
    print("   TrackingLoss %.7f, the torch formulation %.7f" % (fb["items"]["TrackingLoss"], float(term)))
    assert abs(float(term) - fb["items"]["TrackingLoss"]) <= 1e-3 * float(term)      # (a sanity check; the gradients below are the test)
    # the Affinity parameters: float64 arbiter of the term on the CPU (they receive nothing from the other two losses)
    mlp64 = U.mlp_copy(net.affinity, torch.float64)
    c = lambda t: t.detach().cpu().double()
    t64, _ = U.frame_term(mlp64, c(pc1), c(flow), c(f1), c(prop), obj, num, c(fb["desc_prev"]), num_prev, c(target), fb["defined"])
    (0.5 * t64).backward()
    for name, p64 in zip(PARAMS, mlp64.parameters()):
        U.check_grad("affinity." + name, fb["grads"]["affinity.affinity." + name], ref["affinity.affinity." + name], p64.grad)
    # the backbone: the project's full-size bound per tensor (tests/test_fullsize_oracle_gpu.py: 1e-3 of the tensor's largest element
    # for every tensor, median 2e-4; a tensor whose exact gradient is zero is measured against 1e-4 of the model's largest, _util.grad_report)
    gmax = max(float(g.abs().max()) for g in ref.values())
    errs = []
    for n, g in ref.items():
        if n.startswith("affinity."):
            continue
        scale = max(float(g.abs().max()), 1e-4 * gmax)
        errs.append((float((fb["grads"][n] - g).abs().max()) / scale, n))
    errs.sort()
    print("   %d backbone tensors: median %.1e, max %.1e (%s)" % (len(errs), errs[len(errs) // 2][0], errs[-1][0], errs[-1][1]))
    assert errs[-1][0] <= 1e-3 and errs[len(errs) // 2][0] <= 2e-4, errs[-3:]


def test_live_set_and_pretrain_behaviour(sequence):
    first, pre, plain = sequence["first"], sequence["pretrain"], sequence["plain"]
    # every stream reset: the term is 0 and the Affinity gradients are zero tensors, not None (a constant live-parameter set)
    assert first["items"]["TrackingLoss"] == 0.0 and not any(first["defined"])
    assert all(g is not None and g.shape == p.shape and not g.any() for g, p in zip(first["grads"], first["before"]))
    # pretrain: reported, weight 0
    assert any(pre["defined"]) and pre["items"]["TrackingLoss"] > 0
    assert all(torch.equal(a, b) for a, b in zip(pre["before"], pre["after"]))
    # a plain step trains the Affinity MLP
    assert any(plain["defined"]) and plain["items"]["TrackingLoss"] > 0
    assert all(not torch.equal(a, b) for a, b in zip(plain["before"], plain["after"]))
    sf, seg = plain["items"]["SceneFlowLoss"], plain["items"]["SegLoss"]
    assert abs(plain["items"]["Loss"] - (0.5 * sf + seg + 0.5 * plain["items"]["TrackingLoss"])) <= 1e-5 * abs(plain["items"]["Loss"])
    assert abs(pre["items"]["Loss"] - pre["items"]["SegLoss"]) <= 1e-6 * abs(pre["items"]["Loss"])


def test_an_inactive_stream_keeps_its_state_and_adds_nothing(sequence):
    """The fixture's frames 0 and 1 again on a second trainer, stream 1 sitting frame 1 out."""
    B = sequence["B"]
    net, data, nv = batch(B)
    tr = TT.SequenceTrainer(net, streams=B, max_boxes=8, max_gt_tracks=32, deterministic=True)
    _, h, _, _ = tr.step(*data, None, n_valid=nv, reset=torch.ones(B, dtype=torch.bool))
    trk, sc = tr.tracker, tr.scorer
    prev = 1 - trk.cur
    state = lambda: [trk.desc[prev][1].clone(), trk.ids[prev][1].clone(), trk.count[prev][1].clone(), trk.counter[1].clone(),
                     sc.counters[1].clone(), sc.iou_sum[1].clone(), sc.prev_gt_id[1].clone(), sc.prev_count[1].clone(), sc.prev_gt[1].clone(),
                     sc.table_key[1].clone(), sc.table_seen[1].clone(), sc.table_matched[1].clone(), sc.table_used[1].clone()]
    before = state()
    n_before = int(trk.count[prev][1])
    _, h2, out, match = tr.step(*data, h, pretrain=True, n_valid=nv, active=[1, 0, 1, 1])
    prev = 1 - trk.cur                                       # the buffers swapped: the carried-over state is the new "previous"
    after = state()
    assert n_before > 0
    assert torch.equal(before[0][:n_before], after[0][:n_before]) and torch.equal(before[1][:n_before], after[1][:n_before])
    assert all(torch.equal(a, b) for a, b in zip(before[2:], after[2:]))
    assert torch.equal(h2[:, 1], h[:, 1])
    losses = stream_losses(out, match)
    want = sequence["pretrain"]["losses"]
    assert losses[1] == 0 and want[1] > 0
    assert torch.equal(losses[[0, 2, 3]], want[[0, 2, 3]]), (losses.tolist(), want.tolist())
