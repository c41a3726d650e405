"""Shared by tests/test_track_train_cpu.py and tests/test_track_train_gpu.py: the torch restatement of the reference's tracking term
(the arbiter in float64, the yardstick in float32), the tolerance rule, and the synthetic inputs of the kernel pins."""
import copy

import torch
import torch.nn.functional as F

from ratrack_amd import association as A

DESC = 141


# ---- the tolerance rule ------------------------------------------------------------------------------------------------------------
def rel(a, ref):
    """max|a - ref| / max|ref| (0 for two all-zero tensors)."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    scale = float(ref.abs().max())
    err = float((a - ref).abs().max())
    return 0.0 if err == 0.0 else err / max(scale, 1e-300)


def bound(g32, g64):
    """The HIP result must stay within 4x the distance of float32 torch -- the reference's own arithmetic -- from float64, or within
    1e-6 if that is larger: the factor allows another summation order of the same fp32 arithmetic, not lower precision."""
    return max(4.0 * rel(g32, g64), 1e-6)


def check_grad(name, ours, g32, g64, rows=None):
    e, e32, lim = rel(ours, g64), rel(g32, g64), bound(g32, g64)
    print("   %-28s ours %.2e   torch fp32 %.2e   bound %.2e" % (name, e, e32, lim))
    if rows is not None:
        rows.append((name, e, e32, lim))
    assert e <= lim, "%s: %.3e from float64, float32 torch is %.3e away: bound %.3e" % (name, e, e32, lim)


# ---- the reference formulation -----------------------------------------------------------------------------------------------------
def mlp_copy(affinity, dtype):
    """A CPU copy of Affinity.affinity (the nn.Sequential) in `dtype`, parameters as fresh leaves."""
    return copy.deepcopy(affinity.affinity).cpu().to(dtype)


def pair_loss(mlp, curr, prev, target):
    """F.binary_cross_entropy of the MLP on curr_j - prev_i, pairs in the reference's order (i previous, j current)."""
    m, n = prev.shape[0], curr.shape[0]
    diff = (curr.unsqueeze(0) - prev.unsqueeze(1)).reshape(m * n, DESC)
    return F.binary_cross_entropy(mlp(diff).reshape(-1), target.reshape(-1).to(diff.dtype))


def desc_term(mlp, desc, desc_prev, prev_count, num_objects, target, defined, scale):
    """sum_b scale[b] * loss[b] over the streams that take part, on descriptor tensors (B,K,141) of the MLP's dtype; -> (total, [loss_b])."""
    dtype = desc.dtype
    total, losses = torch.zeros((), dtype=dtype), []
    for b in range(desc.shape[0]):
        m, n = int(prev_count[b]), int(num_objects[b])
        if not defined[b] or m * n == 0:
            losses.append(torch.zeros((), dtype=dtype))
            continue
        l = pair_loss(mlp, desc[b, :n], desc_prev[b, :m].detach(), target[b, :m, :n])
        losses.append(l)
        total = total + float(scale[b]) * l
    return total, losses


def descriptors_of(pc1, flow, feature1, prop, obj, num_objects, active=None):
    """association.object_descriptor(o, 128) of every object of every stream, objects built as the reference builds them:
    index_select of cat(pc1 + flow, pc1, flow, feature1, prop) by obj == k.  -> list over b of (n_b, 141) tensors (None: no objects)."""
    out = []
    for b in range(pc1.shape[0]):
        n = int(num_objects[b])
        if n == 0 or (active is not None and not active[b]):
            out.append(None)
            continue
        pf = torch.cat((pc1[b] + flow[b], pc1[b], flow[b], feature1[b], prop[b]), dim=0)
        rows = []
        for k in range(n):
            idx = torch.nonzero(obj[b] == k).reshape(-1)
            rows.append(A.object_descriptor(pf.index_select(1, idx).unsqueeze(0), 128).reshape(1, DESC))
        out.append(torch.cat(rows, dim=0))
    return out


def frame_term(mlp, pc1, flow, feature1, prop, obj, num_objects, desc_prev, num_prev, target, defined):
    """The batch's tracking term as SequenceTrainer forms it: the mean over the B streams of the per-stream loss (undefined: 0).
    Tensors of one device and of the MLP's dtype; obj, num_objects, num_prev, defined: host lists / CPU tensors."""
    B = pc1.shape[0]
    descs = descriptors_of(pc1, flow, feature1, prop, obj, num_objects)
    total, losses = torch.zeros((), dtype=flow.dtype, device=flow.device), []
    for b in range(B):
        m, n = int(num_prev[b]), int(num_objects[b])
        if not defined[b] or m * n == 0:
            losses.append(None)
            continue
        l = pair_loss(mlp, descs[b], desc_prev[b, :m].detach(), target[b, :m, :n])
        losses.append(l)
        total = total + l
    return total / B, losses


# ---- inputs of the kernel pins -----------------------------------------------------------------------------------------------------
def blob_frame(B, N, n_valid, movers, seed, device):
    """Clustered synthetic frame: (pc1, flow, feature1, prop, cls) (B,C,N) with blobs in the 8 clustering channels; the padding
    columns are copies of column 0 and movers (they would cluster with it if they took part)."""
    g = torch.Generator().manual_seed(seed)
    pc1 = torch.zeros(B, 3, N); flow = torch.zeros(B, 3, N); f1 = torch.zeros(B, 2, N); prop = torch.zeros(B, 128, N)
    cls = torch.zeros(B, N)
    for b in range(B):
        n = n_valid[b]
        centres = torch.rand(min(max(n // 6, 1), 60), 8, generator=g) * 30.0
        which = torch.randint(0, centres.shape[0], (n,), generator=g)
        x = centres[which] + torch.randn(n, 8, generator=g) * 0.45
        pc1[b, :, :n], flow[b, :, :n] = x[:, 0:3].t(), x[:, 3:6].t()
        f1[b, 0, :n], f1[b, 1, :n] = torch.randn(n, generator=g), x[:, 6]
        prop[b, 0, :n] = x[:, 7]
        prop[b, 1:, :n] = torch.rand(127, n, generator=g)
        cls[b, :n] = (torch.rand(n, generator=g) < movers[b]).float() * 0.98 + 0.01
        for t_ in (pc1, flow, f1, prop):
            t_[b, :, n:] = t_[b, :, :1]
        cls[b, n:] = 0.99
    return [t.to(device) for t in (pc1, flow, f1, prop, cls)]


def pair_case(device, diff_scale=None):
    """The descriptors of tests/test_tracker_gpu.py::test_affinity_pairs_match_the_affinity_mlp, one stream more: B = 4, K = 24;
    stream 2 holds near-identical descriptors 80 m away (cancellation in curr - prev); stream 3 is reset.  40, 408 and 49 live
    pairs: no multiple of a 16-pair tile.  Random 0/1 targets, all zero in stream 0; a distinct scale per stream.
    diff_scale: stream 1's current descriptors are moved so far from the previous ones that affinities saturate."""
    B, K = 4, 24
    g = torch.Generator().manual_seed(3)
    prev = torch.randn(B, K, DESC, generator=g)
    curr = torch.randn(B, K, DESC, generator=g)
    prev[2, :, 0:3] += 80.0
    curr[2] = prev[2] + torch.randn(K, DESC, generator=g) * 1e-4
    if diff_scale is not None:
        curr[1] = prev[1] + (curr[1] - prev[1]) * diff_scale
    target = (torch.rand(B, K, K, generator=g) < 0.3).float()
    target[0] = 0.0
    d = dict(B=B, K=K, prev=prev, curr=curr, target=target, prev_count=[5, 24, 7, 6], num_objects=[8, 17, 7, 9], reset=[0, 0, 0, 1],
             scale=[0.5, 1.25, -0.75, 2.0])
    d["m"] = [0 if r else c for c, r in zip(d["prev_count"], d["reset"])]
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=device)
    u8 = lambda v: torch.tensor(v, dtype=torch.uint8, device=device)
    d["dev"] = dict(prev=prev.to(device), curr=curr.to(device), target=target.to(device), prev_count=i32(d["prev_count"]),
                    num_objects=i32(d["num_objects"]), reset=u8(d["reset"]), scale=torch.tensor(d["scale"], device=device))
    return d
