"""GPU: the association-stage kernels -- rtk_log_sinkhorn, rtk_associate_batched (plan and decisions), rtk_object_descriptors,
rtk_affinity_pairs, rtk_dbscan and rtk_dbscan_batched -- against the float64 statements of tests/_assoc_f64.py at the edges of their
tiles, passes and LDS limits.  Values: within `_track_train_util.bound` of float64 (each line printed: ours, torch fp32, the bound);
integers, max-prop channels and copied words: exact.  Every buffer a kernel writes is prefilled, and what lies outside the live part is
checked to be untouched; every launch is followed by a synchronize.  tests/test_assoc_f64_cpu.py holds the ground this stands on."""
import ctypes

import numpy as np
import pytest
import torch

from ratrack_amd import _lib, association as A, tracker as T
from ratrack_amd.abi import stream

import _assoc_f64 as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -77


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def u8(v):
    return torch.tensor(v, dtype=torch.uint8, device=DEV)


def filled(shape, value, dtype=torch.float32):
    return torch.full(shape, value, dtype=dtype, device=DEV)


def sync():
    torch.cuda.synchronize()          # raises if the launch before it failed


def same_bits(a, b):
    return torch.equal(F.bits(a.cpu()), F.bits(b.cpu()))


# ------------------------------------------------------------------------------------------------
# rtk_log_sinkhorn
# ------------------------------------------------------------------------------------------------
def test_kmax_is_what_the_tables_were_written_for():
    assert T.max_objects_limit() == F.KMAX == F.max_objects()


@pytest.mark.parametrize("name", F.names(F.B1_PLAN_CASES))
def test_log_sinkhorn(name):
    d = F.plan_data(name)
    m, n = d.case.m, d.case.n
    scores = d.aff.to(DEV).contiguous()
    buf = filled(((m + 1) * (n + 1) + 64,), float("nan"))
    _lib.call("rtk_log_sinkhorn", m, n, scores.data_ptr(), float(d.case.alpha), d.case.iters, buf.data_ptr(), stream())
    sync()
    out = buf[:(m + 1) * (n + 1)].reshape(m + 1, n + 1)
    assert torch.isnan(buf[(m + 1) * (n + 1):]).all() and not torch.isnan(out).any()
    F.check_grad("log_sinkhorn " + name, out, d.p32, d.p64)


def test_log_sinkhorn_refuses_one_step_over_and_the_framework_path_takes_it(monkeypatch):
    for m, n in F.B1_EXCEED:
        scores, out = filled((m, n), 0.5), filled((m + 1, n + 1), 0.0)
        with pytest.raises(_lib.RtkError, match="exceed"):
            _lib.call("rtk_log_sinkhorn", m, n, scores.data_ptr(), F.ALPHA, F.ITERS, out.data_ptr(), stream())
        sync()

    def refuse(*a):
        raise AssertionError("the HIP Sinkhorn was asked for a table it does not admit")
    monkeypatch.setattr(A, "_log_optimal_transport_hip", refuse)
    d = F.plan_data("diag_126_127")
    got = A.sinkhorn_assignment(d.aff.to(DEV).unsqueeze(0))[0].tolist()
    sync()
    assert got == F.decide_f64(d.p64, d.aff, F.prev_ids_of("diag_126_127", d.case.m), 3).indices1


# ------------------------------------------------------------------------------------------------
# rtk_associate_batched
# ------------------------------------------------------------------------------------------------
def run_associate(streams, K, N, alpha, iters, counters):
    """One launch: `streams` as in _assoc_f64.PLAN_GROUPS.  aff outside each live block and `scores` are NaN beforehand, every other
    output holds SENTINEL.  -> (specs, inputs, outputs) on the CPU."""
    B = len(streams)
    specs = [F.stream_spec(s) for s in streams]
    aff = torch.full((B, K, K), float("nan"))
    prev_ids = torch.full((B, K), -1, dtype=torch.int32)
    obj = torch.empty(B, N, dtype=torch.int32)
    for b, (s, (mode, name, m, n)) in enumerate(zip(streams, specs)):
        if name is not None:
            aff[b, :m, :n] = F.plan_data(name).aff
        prev_ids[b, :m] = torch.tensor(F.prev_ids_of(s, m), dtype=torch.int32)
        obj[b] = F.point_objects(s, n, N)
    inp = dict(aff=aff, prev_ids=prev_ids, obj=obj, counter=list(counters))
    act, rst = u8([mode != "inactive" for mode, _, _, _ in specs]), u8([mode == "reset" for mode, _, _, _ in specs])
    num, pc = i32([n for _, _, _, n in specs]), i32([m for _, _, m, _ in specs])
    aff_d, prev_d, obj_d, counter = aff.to(DEV), prev_ids.to(DEV), obj.to(DEV), i32(list(counters))
    new = lambda *s: filled(s, SENTINEL, torch.int32)
    ids, count, oid, idx, nprev, pid = new(B, K), new(B), new(B, K), new(B, K), new(B), new(B, N)
    conf = filled((B, K), float(SENTINEL))
    scores = filled((B, K + 1, K + 1), float("nan"))
    _lib.call("rtk_associate_batched", B, N, K, act.data_ptr(), rst.data_ptr(), aff_d.data_ptr(), num.data_ptr(), obj_d.data_ptr(),
              prev_d.data_ptr(), pc.data_ptr(), float(alpha), int(iters), counter.data_ptr(), ids.data_ptr(), count.data_ptr(), oid.data_ptr(),
              conf.data_ptr(), idx.data_ptr(), nprev.data_ptr(), pid.data_ptr(), scores.data_ptr(), stream())
    sync()
    out = dict(ids=ids, count=count, object_ids=oid, indices1=idx, num_prev=nprev, point_track_id=pid, conf=conf, scores=scores, counter=counter)
    return specs, inp, {k: v.cpu() for k, v in out.items()}


def check_scores(label, specs, out):
    """The plan of every associated stream against float64; nothing outside (m_b + 1, n_b + 1) changed, no NaN inside."""
    for b, (mode, name, m, n) in enumerate(specs):
        sc = out["scores"][b]
        if mode != "live" or m == 0 or n == 0:
            assert torch.isnan(sc).all(), (label, b)
            continue
        inside = sc[:m + 1, :n + 1]
        assert not torch.isnan(inside).any(), (label, b)
        assert torch.isnan(sc[m + 1:]).all() and torch.isnan(sc[:, n + 1:]).all(), (label, b)
        d = F.plan_data(name)
        F.check_grad("%s[%d] %s" % (label, b, name), inside, d.p32, d.p64)


def check_structure(label, specs, inp, out, K):
    """What holds whatever the plan decides: counts, the rows past num_objects, inactive streams, point_track_id = ids[obj]."""
    for b, (mode, name, m, n) in enumerate(specs):
        where = (label, b)
        oid, conf, idx = out["object_ids"][b], out["conf"][b], out["indices1"][b]
        if mode == "inactive":
            assert torch.equal(out["ids"][b], inp["prev_ids"][b]) and int(out["count"][b]) == m and int(out["num_prev"][b]) == 0, where
            assert (oid == -1).all() and (conf == 0).all() and (idx == -1).all() and (out["point_track_id"][b] == -1).all(), where
            assert int(out["counter"][b]) == inp["counter"][b], where
            continue
        assert int(out["count"][b]) == n and int(out["num_prev"][b]) == (0 if mode == "reset" else m), where
        assert (oid[n:] == -1).all() and (conf[n:] == 0).all() and (idx[n:] == -1).all(), where          # -1 / 0 / -1 past num_objects
        assert torch.equal(out["ids"][b, :n], oid[:n]), where
        o = inp["obj"][b].long()
        live = (o >= 0) & (o < n)
        want = torch.where(live, oid[o.clamp(0, max(n - 1, 0))] if n else torch.full_like(o, -1, dtype=torch.int32), -1)
        assert torch.equal(out["point_track_id"][b], want.to(torch.int32)), where
        assert int(out["counter"][b]) - inp["counter"][b] == int((conf[:n] == 0).sum()), where          # one fresh ID per conf of 0


@pytest.mark.parametrize("name", F.names(F.PLAN_GROUPS))
def test_associate_batched_plan(name):
    g = next(k for k in F.PLAN_GROUPS if k.name == name)
    specs, inp, out = run_associate(g.streams, g.K, 300, g.alpha, g.iters, [10 * b for b in range(len(g.streams))])
    check_scores("associate " + name, specs, out)
    check_structure("associate " + name, specs, inp, out, g.K)
    for b, (mode, pname, m, n) in enumerate(specs):          # the shared header: the same words as rtk_log_sinkhorn wherever it admits the table
        if mode == "live" and m and n and F.sinkhorn_b1_fits(m, n):
            block = F.plan_data(pname).aff.to(DEV).contiguous()
            ref = filled((m + 1, n + 1), float("nan"))
            _lib.call("rtk_log_sinkhorn", m, n, block.data_ptr(), float(g.alpha), g.iters, ref.data_ptr(), stream())
            sync()
            assert same_bits(out["scores"][b, :m + 1, :n + 1], ref), (name, b, pname)


@pytest.mark.parametrize("name", F.names(F.DECISION_GROUPS))
def test_associate_batched_decisions(name):
    g = next(k for k in F.DECISION_GROUPS if k.name == name)
    specs, inp, out = run_associate(g.streams, g.K, g.N, F.ALPHA, F.ITERS, g.counters)
    check_scores("decisions " + name, specs, out)
    check_structure("decisions " + name, specs, inp, out, g.K)
    for b, (s, (mode, pname, m, n)) in enumerate(zip(g.streams, specs)):
        if mode == "inactive":
            continue
        where = (name, b, s)
        live = mode == "live" and m > 0 and n > 0
        d = F.plan_data(pname) if pname is not None else None
        aff = d.aff if live else torch.zeros(0, n)
        prev_ids = F.prev_ids_of(s, m)
        dec = F.decide_f64(d.p64 if live else None, aff, prev_ids if live else [], g.counters[b])
        assert out["indices1"][b, :n].tolist() == dec.indices1, where
        assert out["object_ids"][b, :n].tolist() == dec.ids, where
        assert int(out["counter"][b]) == dec.counter, where
        assert same_bits(out["conf"][b, :n], torch.tensor(np.array(dec.conf, dtype=np.float32))), where          # the aff word itself
        if live and max(m, n) <= 40 and pname not in F.TIES:          # the shipped Python bookkeeping, as tests/test_tracker_gpu.py holds it
            ids, confs, idx, max_id = F.associator_decision(d.aff, prev_ids, g.counters[b], DEV)
            sync()
            assert out["object_ids"][b, :n].tolist() == ids and int(out["counter"][b]) == max_id, where
            assert out["conf"][b, :n].tolist() == confs and out["indices1"][b, :n].tolist() == idx, where
    by = {s: b for b, s in enumerate(g.streams)}
    if "tie_17_33" in by:          # the exact tie: equal words in the kernel's own plan, the lowest index keeps the match
        b = by["tie_17_33"]
        assert same_bits(out["scores"][b, :18, 3], out["scores"][b, :18, 20])
        assert out["indices1"][b, 3] == 5 and out["indices1"][b, 20] == -1
    if "threshold_at" in by:
        at, above = by["threshold_at"], by["threshold_above"]
        assert out["conf"][at, 1] == 0 and out["object_ids"][at, 1] == g.counters[at] and out["indices1"][at, 1] == 1
        assert out["conf"][above, 1] > 0 and out["object_ids"][above, 1] == F.prev_ids_of("threshold_above", 3)[1]


# ------------------------------------------------------------------------------------------------
# rtk_object_descriptors
# ------------------------------------------------------------------------------------------------
def permuted(t):
    """(B,C,N) values held in a (B,N,C) buffer."""
    return t.permute(0, 2, 1).contiguous().to(DEV).permute(0, 2, 1)


def sliced(t):
    """(B,C,N) or (B,N) values held inside a wider buffer."""
    if t.dim() == 2:
        buf = filled((t.shape[0], t.shape[1] + 9), float("nan"))
        buf[:, 4:4 + t.shape[1]] = t.to(DEV)
        return buf[:, 4:4 + t.shape[1]]
    buf = filled((t.shape[0], t.shape[1] + 3, t.shape[2] + 9), float("nan"))
    buf[:, 1:1 + t.shape[1], 4:4 + t.shape[2]] = t.to(DEV)
    return buf[:, 1:1 + t.shape[1], 4:4 + t.shape[2]]


def track_frame(pc1, flow, f1, prop, cls, n_valid, active):
    B, N = cls.shape
    return T.TrackFrame(B, N, T._view(pc1), T._view(flow), T._view(f1), T._view(prop), T._view(cls), n_valid.data_ptr(),
                        None if active is None else active.data_ptr())


@pytest.mark.parametrize("name", F.names(F.DESC_CASES))
def test_object_descriptors(name):
    d = F.desc_data(name)
    k = d.case
    if k.layout == "views":
        pc1, flow, f1, prop, cls = permuted(d.pc1), sliced(d.flow), sliced(d.feature1), permuted(d.prop), sliced(d.cls)
        assert not any(t.is_contiguous() for t in (pc1, flow, f1, prop, cls))
    else:
        pc1, flow, f1, prop, cls = [t.to(DEV) for t in (d.pc1, d.flow, d.feature1, d.prop, d.cls)]
    nv = i32(list(k.n_valid))
    act = None if k.active is None else u8(list(k.active))
    fr = track_frame(pc1, flow, f1, prop, cls, nv, act)
    obj, num, pc = d.obj.to(DEV), i32(list(d.num_objects)), i32(list(k.prev_count))
    prev = torch.randn(k.B, k.K, F.DESC, generator=F._gen("desc_prev", name))
    prev_d = prev.to(DEV)
    desc = filled((k.B, k.K, F.DESC), -7.5)
    _lib.call("rtk_object_descriptors", ctypes.addressof(fr), k.K, obj.data_ptr(), num.data_ptr(), pc.data_ptr(), prev_d.data_ptr(),
              desc.data_ptr(), stream())
    sync()
    got = desc.cpu()
    prefill = torch.full((F.DESC,), -7.5)
    for b in range(k.B):
        if k.active is not None and not k.active[b]:          # carried over: desc_prev's words in the first clamp(prev_count) rows
            mp = min(max(k.prev_count[b], 0), k.K)
            assert same_bits(got[b, :mp], prev[b, :mp]), (name, b)
            assert same_bits(got[b, mp:], prefill.expand(k.K - mp, -1)), (name, b)
            continue
        n = k.counts[b]
        assert same_bits(got[b, n:], prefill.expand(k.K - n, -1)), (name, b)          # rows >= num_objects are not written
        assert not torch.isnan(got[b, :n]).any(), (name, b)
        assert same_bits(got[b, :n, F.DESC_PROP], d.d32[b, :n, F.DESC_PROP]), (name, b)          # a maximum moves bits
        for group, sl in F.DESC_GROUPS:
            F.check_grad("descriptors %s[%d] %s" % (name, b, group), got[b, :n, sl], d.d32[b, :n, sl], d.d64[b, :n, sl])
    one = F.desc_data("n_valid")
    if name == "n_valid":          # one member: the variance is exactly 0
        assert (got[0, 0, 3:6] == 0).all() and (got[0, 0, 139:141] == 0).all()
        assert int((one.obj[4] == 1).sum()) == 1 and (got[4, 1, 3:6] == 0).all() and (got[4, 1, 139:141] == 0).all()


# ------------------------------------------------------------------------------------------------
# rtk_affinity_pairs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.names(F.AFF_CASES))
def test_affinity_pairs(name):
    d = F.aff_data(name)
    k = d.case
    W = T.pack_affinity(F.affinity_net(k.weights)).to(DEV)
    prev, curr = d.prev.to(DEV), d.curr.to(DEV)
    pc, num, rst = i32(list(k.prev_count)), i32(list(k.num_objects)), u8(list(k.reset))
    aff = filled((k.B, k.K, k.K), -7.0)
    _lib.call("rtk_affinity_pairs", k.B, k.K, W.data_ptr(), prev.data_ptr(), pc.data_ptr(), rst.data_ptr(), curr.data_ptr(), num.data_ptr(),
              aff.data_ptr(), stream())
    sync()
    got = aff.cpu()
    untouched = torch.ones(k.B, k.K, k.K, dtype=torch.bool)
    live = sorted(d.a64)
    for b in live:
        untouched[b, :d.m[b], :d.n[b]] = False
    flat = lambda blocks: torch.cat([v.reshape(-1) for v in blocks])
    ours = flat(got[b, :d.m[b], :d.n[b]] for b in live)
    assert not torch.isnan(ours).any()
    # the case's live pairs as one tensor: affinities share one scale, and the rule is stated per case
    F.check_grad("affinity %s (%d pairs)" % (name, ours.numel()), ours, flat(d.a32[b] for b in live), flat(d.a64[b] for b in live))
    assert (got[untouched] == -7.0).all(), "%s: an element outside the live blocks was written" % name
    assert len(d.a64) == sum(1 for m, n in zip(d.m, d.n) if m * n)


# ------------------------------------------------------------------------------------------------
# rtk_dbscan and rtk_dbscan_batched
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.names(F.DBSCAN_CASES))
def test_dbscan(name):
    d = F.db_data(name)
    k = d.case
    B, N = len(k.n_valid), k.N
    x = d.x.to(DEV)                                                     # (B, N, 8): xyz, flow, v_r, prop[0]
    pc1, flow = x[:, :, 0:3].permute(0, 2, 1).contiguous(), x[:, :, 3:6].permute(0, 2, 1).contiguous()
    f1 = filled((B, 2, N), 0.25)
    f1[:, 1] = x[:, :, 6]
    prop = filled((B, 128, N), 0.5)
    prop[:, 0] = x[:, :, 7]
    cls = d.cls.to(DEV)
    nv = i32(list(k.n_valid))
    fr = track_frame(pc1, flow, f1, prop, cls, nv, None)
    new = lambda *s: filled(s, SENTINEL, torch.int32)
    labels, obj, num, flags = new(B, N), new(B, N), new(B), new(B)
    need = B * N * T.DBSCAN_POINT_BYTES if k.work else 0
    work = torch.empty(need, dtype=torch.uint8, device=DEV) if k.work else None
    _lib.call("rtk_dbscan_batched", ctypes.addressof(fr), 0.5, F.EPS, k.min_samples, F.KMAX, labels.data_ptr(), obj.data_ptr(), num.data_ptr(),
              flags.data_ptr(), None if work is None else work.data_ptr(), need, stream())
    sync()
    assert np.array_equal(labels.cpu().numpy(), d.labels), name
    assert np.array_equal(obj.cpu().numpy(), d.obj), name
    assert num.cpu().tolist() == d.num_objects and flags.cpu().tolist() == [0] * B, name
    chan = i32(list(range(8)))
    for b in range(B):          # the B = 1 entry point on each stream's own columns
        n = k.n_valid[b]
        feat, score = x[b, :n].t().contiguous(), cls[b, :n].contiguous()
        lab1 = new(n)
        _lib.call("rtk_dbscan", n, feat.data_ptr(), n, chan.data_ptr(), score.data_ptr(), 0.5, F.EPS, k.min_samples, lab1.data_ptr(), stream())
        sync()
        assert np.array_equal(lab1.cpu().numpy(), d.labels[b, :n]), (name, b)
