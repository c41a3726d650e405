"""GPU: the batched tracker (ratrack_amd/tracker.py, csrc/track_batched.hip) -- B sequences in lockstep, every stream equal to its
own B = 1 Track4D.forward loop; the four kernels pinned against their B = 1 counterparts."""
import ctypes
import os

import numpy as np
import pytest
import torch

from _util import GOLDEN, load_case, reference_state_dict
from ratrack_amd import _lib, association as A, synth, tracker as T, vod_gt, vod_io
from ratrack_amd.track4d import Args, Track4D

pytestmark = pytest.mark.gpu
DEV = "cuda"
CLS_SHIFT = 0.09          # tools/make_golden.py FORWARD_CLS_BIAS_SHIFT: moving points in every frame


def ref_net():
    sd = reference_state_dict(DEV)
    sd["fd_layer.cp.linear.bias"] = sd["fd_layer.cp.linear.bias"] + CLS_SHIFT
    net = Track4D(Args()).to(DEV)
    net.load_state_dict(sd, strict=True)
    return net.eval()


def synth_net():
    net = Track4D(Args()).to(DEV).eval()
    synth.fill_state_dict(net.state_dict())
    with torch.no_grad():
        net.fd_layer.cp.linear.bias += CLS_SHIFT
    net.invalidate_fused()
    return net


def synth_pairs(count, n, case_id):
    d = synth.make_frame_pairs(count, n, case_id=case_id)
    t = {k: torch.from_numpy(v) for k, v in d.items()}
    return [(t["pc1"][i:i + 1], t["pc2"][i:i + 1], t["feature1"][i:i + 1], t["feature2"][i:i + 1]) for i in range(count)]


def radar_pairs():
    ex = os.path.join(GOLDEN, "vod_example")
    scans = [vod_io.load_radar_bin(os.path.join(ex, "radar_%s.bin" % f)) for f in ("00549", "01047", "01201")]
    return [vod_io.frame_pair_tensors(scans[i], scans[(i + 1) % 3]) for i in range(3)]


def reference_order(labels):
    """The numpy ordering of association.cluster_objects_device: object index of every point (by first member point)."""
    out = np.full(labels.shape, -1, dtype=np.int64)
    pts = np.nonzero(labels >= 0)[0]
    if pts.size == 0:
        return out
    ids, first = np.unique(labels[pts], return_index=True)
    rank = np.empty(int(ids.max()) + 1, dtype=np.int64)
    rank[ids[np.argsort(first, kind="stable")]] = np.arange(ids.size)
    out[pts] = rank[labels[pts]]
    return out


def expected_track_ids(objects, obj_row):
    keys = list(objects.keys())
    return np.array([keys[k] if k >= 0 else -1 for k in obj_row], dtype=np.int64)


# ---- 1. reference anchor ------------------------------------------------------------------------------
def test_reference_anchor_is_stream_two_of_four():
    case = load_case("forward_b1_n256")
    net = ref_net()
    trk = T.BatchedTracker(net, streams=4)
    others = {0: synth_pairs(2, 200, 31), 1: synth_pairs(2, 131, 32), 3: synth_pairs(2, 256, 33)}
    with torch.no_grad():
        for fi in range(2):
            g = lambda k: torch.from_numpy(case["f%d_in_%s" % (fi, k)])
            gold = (g("pc1"), g("pc2"), g("feature1"), g("feature2"))
            pairs = [others[b][fi] if b != 2 else gold for b in range(4)]
            pc1, pc2, f1, f2, nv = vod_gt.pad_frame_pairs(pairs, device=DEV)
            out = trk.step(pc1, pc2, f1, f2, n_valid=nv)
            objects, confs = out.objects(2)
            p = "f%d_" % fi
            assert [o.shape[2] for o in objects.values()] == case[p + "object_sizes_curr"].tolist()
            assert list(objects.keys()) == case[p + "object_ids"].tolist()
            if case[p + "aff_mat"].size:
                assert np.abs(out.aff_mat(2).cpu().numpy() - case[p + "aff_mat"]).max() < 1e-4
                assert np.array_equal(out.indices1(2).cpu().numpy(), case[p + "indices1"])
            assert np.allclose([float(c) for c in confs], case[p + "confs"], atol=1e-4)
            assert int(trk.counter[2]) == int(case[p + "max_id"])


# ---- 2. equivalence to B = 1 ---------------------------------------------------------------------------
def test_every_stream_equals_its_own_b1_forward_loop(tmp_path):
    B, STEPS = 8, 5
    RESET, INACTIVE = (3, 2), (6, 3)          # (stream, step)
    net = synth_net()
    synth_sizes = [256, 200, 160, 256, 97]
    seqs = [synth_pairs(STEPS, n, 40 + s) for s, n in enumerate(synth_sizes)]
    rp = radar_pairs()
    seqs += [[rp[(r + t) % 3] for t in range(STEPS)] for r in range(3)]
    trk = T.BatchedTracker(net, streams=B)
    state = [dict(h=torch.zeros(5, 1, 128, device=DEV), prev=dict(), max_id=0) for _ in range(B)]
    total_objects = 0
    with torch.no_grad():
        for t in range(STEPS):
            reset = [s == RESET[0] and t == RESET[1] for s in range(B)]
            active = [not (s == INACTIVE[0] and t == INACTIVE[1]) for s in range(B)]
            pairs = [seqs[s][t] for s in range(B)]
            pc1, pc2, f1, f2, nv = vod_gt.pad_frame_pairs(pairs, device=DEV)
            out = trk.step(pc1, pc2, f1, f2, n_valid=nv, reset=torch.tensor(reset), active=torch.tensor(active))
            trk.check()
            pid = out.point_track_id.cpu().numpy()
            obj = out.obj.cpu().numpy()
            for s in range(B):
                st = state[s]
                if not active[s]:
                    assert out.objects(s) == (dict(), [])
                    assert (pid[s] == -1).all()
                    continue
                if reset[s]:
                    st["h"], st["prev"] = torch.zeros(5, 1, 128, device=DEV), dict()
                net.max_id = st["max_id"]
                x = [v.to(DEV) for v in pairs[s]]
                h, _, cls, _, aff_mat, indices1, confs, objects, _, _ = net(x[0], x[1], x[2], x[3], st["h"], st["prev"])
                st.update(h=h, prev=objects, max_id=net.max_id)
                n1 = x[0].shape[2]
                assert (out.cls[s, :n1] - cls[0]).abs().max().item() < 1e-5, (s, t)
                got, got_confs = out.objects(s)
                assert list(got.keys()) == list(objects.keys()), (s, t)
                for k in objects:
                    assert got[k].shape == objects[k].shape, (s, t, k)
                    assert torch.equal(got[k][:, 3:6], objects[k][:, 3:6]), (s, t, k)
                    assert torch.allclose(got[k], objects[k], rtol=1e-4, atol=1e-4), (s, t, k)
                assert np.allclose([float(c) for c in got_confs], [float(c) for c in confs], atol=1e-5, rtol=0), (s, t)
                assert out.aff_mat(s).shape == aff_mat.shape
                if aff_mat.numel():
                    assert (out.aff_mat(s) - aff_mat).abs().max().item() < 1e-5, (s, t)
                if indices1 is None:
                    assert out.indices1(s) is None
                else:
                    assert torch.equal(out.indices1(s), indices1), (s, t)
                assert int(trk.counter[s]) == net.max_id, (s, t)
                assert np.array_equal(pid[s], expected_track_ids(objects, obj[s])), (s, t)
                assert (pid[s, n1:] == -1).all()
                total_objects += len(objects)
            # result files: byte-identical to vod_io.write_track_results on objects(b), and readable
            paths = trk.write_results(str(tmp_path / "batched"), ["seq%d" % s for s in range(B)], [t] * B, out)
            assert len(paths) == sum(active)
            for s in range(B):
                if not active[s]:
                    continue
                ref = vod_io.write_track_results(str(tmp_path / "ref"), "seq%d" % s, t, *out.objects(s))
                mine = os.path.join(str(tmp_path / "batched"), "seq%d" % s, str(t).zfill(5) + ".txt")
                assert open(mine, "rb").read() == open(ref, "rb").read(), (s, t)
                back = vod_io.read_track_results(mine)
                objs, confs = out.objects(s)
                assert [r[0] for r in back] == list(objs.keys())
                assert [r[2].shape[0] for r in back] == [o.shape[2] for o in objs.values()]
                assert np.allclose([r[1] for r in back], [float(c) for c in confs], rtol=0, atol=0)
    assert total_objects > 0


# ---- 3. kernel pins ------------------------------------------------------------------------------------
def blob_frame(B, N, n_valid, movers, seed):
    """Clustered synthetic frame: (pc1, flow, feature1, prop, cls) (B,C,N) with blobs in the 8 clustering channels."""
    g = torch.Generator().manual_seed(seed)
    pc1 = torch.zeros(B, 3, N); flow = torch.zeros(B, 3, N); f1 = torch.zeros(B, 2, N); prop = torch.zeros(B, 128, N)
    cls = torch.zeros(B, N)
    for b in range(B):
        n = n_valid[b]
        centres = torch.rand(min(max(n // 6, 1), 60), 8, generator=g) * 30.0      # <= 60 clusters: within K
        which = torch.randint(0, centres.shape[0], (n,), generator=g)
        x = centres[which] + torch.randn(n, 8, generator=g) * 0.45
        pc1[b, :, :n], flow[b, :, :n] = x[:, 0:3].t(), x[:, 3:6].t()
        f1[b, 0, :n], f1[b, 1, :n] = torch.randn(n, generator=g), x[:, 6]
        prop[b, 0, :n] = x[:, 7]
        prop[b, 1:, :n] = torch.rand(127, n, generator=g)
        cls[b, :n] = (torch.rand(n, generator=g) < movers[b]).float() * 0.98 + 0.01
        # padding columns: copies of column 0, movers -- they would cluster with it if they took part
        for t_ in (pc1, flow, f1, prop):
            t_[b, :, n:] = t_[b, :, :1]
        cls[b, n:] = 0.99
    return [t.to(DEV) for t in (pc1, flow, f1, prop, cls)]


def run_dbscan_batched(frame, n_valid, K, min_samples):
    pc1, flow, f1, prop, cls = frame
    B, N = cls.shape
    nv = torch.tensor(n_valid, dtype=torch.int32, device=DEV)
    act = torch.ones(B, dtype=torch.uint8, device=DEV)
    fr = T.TrackFrame(B, N, T._view(pc1), T._view(flow), T._view(f1), T._view(prop), T._view(cls), nv.data_ptr(), act.data_ptr())
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=DEV)
    labels, obj, num, flags = i32(B, N), i32(B, N), i32(B), i32(B)
    need = B * N * T.DBSCAN_POINT_BYTES
    work = torch.empty(need, dtype=torch.uint8, device=DEV)
    _lib.call("rtk_dbscan_batched", ctypes.addressof(fr), 0.5, 1.5, min_samples, K, labels.data_ptr(), obj.data_ptr(), num.data_ptr(),
              flags.data_ptr(), work.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    return fr, (nv, act, work), labels, obj, num, flags


@pytest.mark.parametrize("min_samples", [2, 3])
def test_dbscan_batched_labels_and_order_equal_rtk_dbscan(min_samples):
    # stream 0 has no movers; stream 2 exceeds the LDS tables (workspace path, N * 48 B > 128 KiB); padding everywhere else
    n_valid = [180, 256, 3000, 77]
    B, N = 4, 3000
    frame = blob_frame(B, N, n_valid, movers=[0.0, 0.7, 0.6, 1.0], seed=5 + min_samples)
    _, keep, labels, obj, num, flags = run_dbscan_batched(frame, n_valid, K=197, min_samples=min_samples)
    pc1, flow, f1, prop, cls = frame
    labels, obj, num, flags = labels.cpu().numpy(), obj.cpu().numpy(), num.cpu().numpy(), flags.cpu().numpy()
    chan = torch.tensor([3, 4, 5, 6, 7, 8, 10, 11], dtype=torch.int32, device=DEV)
    for b in range(B):
        n = n_valid[b]
        pf = torch.cat((pc1[b] + flow[b], pc1[b], flow[b], f1[b], prop[b]), 0)[:, :n].contiguous()
        ref = torch.empty(n, dtype=torch.int32, device=DEV)
        score = cls[b, :n].contiguous()
        _lib.call("rtk_dbscan", n, pf.data_ptr(), n, chan.data_ptr(), score.data_ptr(), 0.5, 1.5, min_samples, ref.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
        ref = ref.cpu().numpy()
        assert np.array_equal(labels[b, :n], ref), b
        assert (labels[b, n:] == -1).all() and (obj[b, n:] == -1).all(), b
        if n <= 400:             # the host restatement of sklearn's algorithm (O(n^2) in numpy)
            mv = cls[b, :n].cpu().numpy() > 0.5
            f = torch.cat((pf[3:9], pf[10:12]), 0).t().cpu().numpy()[mv]
            host = np.full(n, -1, dtype=np.int64)
            host[np.nonzero(mv)[0]] = A.dbscan(f, 1.5, min_samples)
            assert np.array_equal(labels[b, :n], host), b
        assert np.array_equal(obj[b, :n], reference_order(ref)), b
        assert num[b] == (ref.max() + 1 if (ref >= 0).any() else 0)
        assert flags[b] == 0
    assert num[0] == 0
    if min_samples == 3:
        assert (labels[1:] >= 0).any()


def test_descriptors_match_batched_descriptors():
    n_valid = [256, 140, 200]
    B, N, K = 3, 256, 128
    frame = blob_frame(B, N, n_valid, movers=[0.8, 0.9, 0.5], seed=11)
    fr, keep, labels, obj, num, flags = run_dbscan_batched(frame, n_valid, K, 2)
    pc1, flow, f1, prop, cls = frame
    desc = torch.zeros(B, K, 141, device=DEV)
    prev = torch.zeros(B, K, 141, device=DEV)
    pc = torch.zeros(B, dtype=torch.int32, device=DEV)
    _lib.call("rtk_object_descriptors", ctypes.addressof(fr), K, obj.data_ptr(), num.data_ptr(), pc.data_ptr(), prev.data_ptr(),
              desc.data_ptr(), torch.cuda.current_stream().cuda_stream)
    objn, numh = obj.cpu(), num.cpu().tolist()
    for b in range(B):
        assert numh[b] > 0
        pf = torch.cat((pc1[b] + flow[b], pc1[b], flow[b], f1[b], prop[b]), 0)
        objs = [pf[:, torch.nonzero(objn[b] == k).reshape(-1).to(DEV)].unsqueeze(0) for k in range(numh[b])]
        ref = A.batched_descriptors(objs)
        got = desc[b, :numh[b]]
        assert torch.allclose(got, ref, rtol=1e-5, atol=1e-6), (b, (got - ref).abs().max().item())
        one = A.object_descriptor(objs[0], 128).reshape(-1)
        assert torch.allclose(got[0], one, rtol=1e-5, atol=1e-6)


def test_affinity_pairs_match_the_affinity_mlp():
    net = ref_net()
    W = T.pack_affinity(net.affinity).to(DEV)
    B, K = 3, 24
    g = torch.Generator(device=DEV).manual_seed(3)
    prev = torch.randn(B, K, 141, device=DEV, generator=g)
    curr = torch.randn(B, K, 141, device=DEV, generator=g)
    # stream 2: near-identical descriptors 80 m away (centre ~ 80, differences ~1e-4): cancellation stays exact in curr - prev
    prev[2, :, 0:3] += 80.0
    curr[2] = prev[2] + torch.randn(K, 141, device=DEV, generator=g) * 1e-4
    counts, nobj = [5, 24, 7], [8, 17, 7]
    pc = torch.tensor(counts, dtype=torch.int32, device=DEV)
    num = torch.tensor(nobj, dtype=torch.int32, device=DEV)
    reset = torch.tensor([0, 0, 0], dtype=torch.uint8, device=DEV)
    aff = torch.full((B, K, K), -7.0, device=DEV)
    _lib.call("rtk_affinity_pairs", B, K, W.data_ptr(), prev.data_ptr(), pc.data_ptr(), reset.data_ptr(), curr.data_ptr(), num.data_ptr(),
              aff.data_ptr(), torch.cuda.current_stream().cuda_stream)
    with torch.no_grad():
        for b in range(B):
            m, n = counts[b], nobj[b]
            diff = (curr[b, :n].unsqueeze(0) - prev[b, :m].unsqueeze(1)).reshape(m * n, 141)
            ref = net.affinity.affinity(diff).reshape(m, n)
            assert (aff[b, :m, :n] - ref).abs().max().item() <= 1e-5, b
            assert (aff[b, m:] == -7.0).all() and (aff[b, :, n:] == -7.0).all()      # nothing past the live block


def run_associate(aff_list, prev_ids_list, counter0, K=16, reset=None):
    """rtk_associate_batched on crafted (m_b, n_b) affinity matrices -> per-stream (ids, confs, indices1, counter, scores)."""
    B = len(aff_list)
    aff = torch.zeros(B, K, K, device=DEV)
    num = torch.zeros(B, dtype=torch.int32)
    pc = torch.zeros(B, dtype=torch.int32)
    prev_ids = torch.full((B, K), -1, dtype=torch.int32)
    for b, a in enumerate(aff_list):
        m, n = a.shape
        aff[b, :m, :n] = a.to(DEV)
        num[b], pc[b] = n, m
        prev_ids[b, :m] = torch.tensor(prev_ids_list[b], dtype=torch.int32)
    N = 8
    obj = torch.full((B, N), -1, dtype=torch.int32, device=DEV)
    act = torch.ones(B, dtype=torch.uint8, device=DEV)
    rst = torch.zeros(B, dtype=torch.uint8, device=DEV) if reset is None else torch.tensor(reset, dtype=torch.uint8, device=DEV)
    counter = torch.tensor(counter0, dtype=torch.int32, device=DEV)
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=DEV)
    ids, count, oid, idx, nprev, pid = i32(B, K), i32(B), i32(B, K), i32(B, K), i32(B), i32(B, N)
    conf = torch.empty(B, K, device=DEV)
    scores = torch.full((B, K + 1, K + 1), float("nan"), device=DEV)
    num_d, pc_d, prev_d = num.to(DEV), pc.to(DEV), prev_ids.to(DEV)
    _lib.call("rtk_associate_batched", B, N, K, act.data_ptr(), rst.data_ptr(), aff.data_ptr(), num_d.data_ptr(), obj.data_ptr(),
              prev_d.data_ptr(), pc_d.data_ptr(), 0.9, 500, counter.data_ptr(), ids.data_ptr(), count.data_ptr(), oid.data_ptr(),
              conf.data_ptr(), idx.data_ptr(), nprev.data_ptr(), pid.data_ptr(), scores.data_ptr(), torch.cuda.current_stream().cuda_stream)
    res = []
    for b, a in enumerate(aff_list):
        m, n = a.shape
        res.append(dict(ids=oid[b, :n].cpu().tolist(), conf=conf[b, :n].cpu().tolist(), idx=idx[b, :n].cpu().tolist(),
                         counter=int(counter[b]), count=int(count[b]), state_ids=ids[b, :n].cpu().tolist(), scores=scores[b, :m + 1, :n + 1]))
    return res


def test_batched_sinkhorn_is_bit_equal_to_rtk_log_sinkhorn():
    g = torch.Generator().manual_seed(9)
    shapes = [(3, 5), (19, 23), (1, 1), (40, 33), (64, 64)]
    affs = [torch.rand(m, n, generator=g) for m, n in shapes]
    res = run_associate(affs, [list(range(m)) for m, _ in shapes], [0] * len(shapes), K=64)
    for a, r in zip(affs, res):
        m, n = a.shape
        s = a.to(DEV).contiguous()
        ref = torch.empty(m + 1, n + 1, device=DEV)
        _lib.call("rtk_log_sinkhorn", m, n, s.data_ptr(), 0.9, 500, ref.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert torch.equal(r["scores"], ref), (m, n)


def associator_reference(aff, prev_ids, counter, monkeypatch):
    """Associator.__call__ on a crafted affinity matrix (the MLP is bypassed) -> (ids, confs, indices1, max_id)."""
    m, n = aff.shape
    aff_d = aff.to(DEV)
    monkeypatch.setattr(A, "affinity_matrix", lambda net, oc, op, d=None: (aff_d.reshape(-1), aff_d.unsqueeze(0), m, n))
    assoc = A.Associator(None)
    assoc.max_id = counter
    dummy = lambda: torch.zeros(1, 139, 1, device=DEV)
    objects_curr = [dummy() for _ in range(n)]
    objects_prev = {k: dummy() for k in prev_ids}
    _, _, indices1, confs, objects = assoc(objects_curr, objects_prev)
    order = {id(o): j for j, o in enumerate(objects_curr)}
    assert [order[id(o)] for o in objects.values()] == list(range(n))
    idx = None if indices1 is None else indices1[0].tolist()
    return list(objects.keys()), [float(c) for c in confs], idx, assoc.max_id


def test_association_decisions_equal_the_associator(monkeypatch):
    g = torch.Generator().manual_seed(4)
    cases = {
        "all_below_threshold": torch.rand(4, 4, generator=g) * 0.009,
        "m0": torch.zeros(0, 3),
        "n0": torch.zeros(3, 0),
        "m_ne_n": torch.rand(5, 8, generator=g),
        "dustbin": torch.tensor([[0.95, 0.02, 0.01], [0.03, 0.001, 0.9], [0.01, 0.002, 0.02]]),
        "strong_diagonal": torch.eye(6) * 0.9 + torch.rand(6, 6, generator=g) * 0.05,
    }
    names = list(cases)
    prev_ids = [[100 + 3 * i for i in range(cases[k].shape[0])] for k in names]
    res = run_associate([cases[k] for k in names], prev_ids, [7] * len(names))
    for k, pid, r in zip(names, prev_ids, res):
        ids, confs, idx, max_id = associator_reference(cases[k], pid, 7, monkeypatch)
        assert r["ids"] == ids, k
        assert r["state_ids"] == ids, k
        assert np.allclose(r["conf"], confs, rtol=0, atol=0), k
        assert r["counter"] == max_id, k
        m, n = cases[k].shape
        if idx is None:
            assert r["idx"] == [-1] * n, k
        else:
            assert r["idx"] == idx, k
    assert res[names.index("all_below_threshold")]["ids"] == [7, 8, 9, 10]
    assert res[names.index("m0")]["ids"] == [7, 8, 9]


def test_exact_ties_go_to_the_lowest_index():
    # two identical current objects: the Sinkhorn plan ties exactly; the previous object 0 keeps the FIRST (documented rule)
    aff = torch.tensor([[0.8, 0.8], [0.1, 0.1]])
    r = run_associate([aff], [[41, 42]], [5])[0]
    s = r["scores"][:2, :2]
    assert s[0, 0].item() == s[0, 1].item()
    assert r["idx"][0] == 0 and r["idx"][1] == -1
    assert r["ids"] == [41, 5] and r["counter"] == 6


# ---- 5. no host round trip ------------------------------------------------------------------------------
def test_association_stage_runs_without_host_synchronisation():
    net = ref_net()
    B = 4
    trk = T.BatchedTracker(net, streams=B)
    pairs = synth_pairs(B, 256, 50)
    for step in range(2):
        pc1, pc2, f1, f2, nv = vod_gt.pad_frame_pairs(pairs, device=DEV)
        reset = torch.zeros(B, dtype=torch.uint8, device=DEV)
        active = torch.ones(B, dtype=torch.uint8, device=DEV)
        with torch.no_grad():
            flow, h, cls, _, _, _, prop = net._fused_engine().backbone(pc1, pc2, f1, f2, trk.h, n_valid=nv)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = trk.associate(pc1, f1, flow, cls, prop, nv, reset, active)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        trk.h = h
        out.check()
    assert int(out.num_objects.sum()) >= 0


# ---- 6. overflow ----------------------------------------------------------------------------------------
def test_overflow_raises_naming_the_stream_and_spares_the_others():
    case = load_case("forward_b1_n256")
    net = ref_net()
    g = lambda k: torch.from_numpy(case["f0_in_%s" % k])
    gold = (g("pc1"), g("pc2"), g("feature1"), g("feature2"))        # 23 objects
    small = synth_pairs(2, 24, 60)
    pairs = [small[0], gold, small[1]]
    pc1, pc2, f1, f2, nv = vod_gt.pad_frame_pairs(pairs, device=DEV)
    with torch.no_grad():
        big = T.BatchedTracker(net, streams=3).step(pc1, pc2, f1, f2, n_valid=nv)
        trk = T.BatchedTracker(net, streams=3, max_objects=4)
        out = trk.step(pc1, pc2, f1, f2, n_valid=nv)
    assert int(big.num_objects[1]) > 4
    with pytest.raises(RuntimeError, match="stream 1"):
        trk.check()
    with pytest.raises(RuntimeError, match="stream 1"):
        out.objects(1)
    with pytest.raises(RuntimeError, match="stream 1"):
        trk.write_results("/nonexistent-root", ["a", "b", "c"], [0, 0, 0], out)
    assert int(out.num_objects[1]) == 4
    for b in (0, 2):
        n = int(big.num_objects[b])
        if n > 4:
            continue
        o_small, c_small = out.objects(b)
        o_big, c_big = big.objects(b)
        assert list(o_small) == list(o_big)
        assert all(torch.equal(o_small[k], o_big[k]) for k in o_big)
        assert torch.equal(out.point_track_id[b], big.point_track_id[b])
