"""Float64 restatements of the grouped stage kernels, written from the contracts in include/rtk_fused.h (not from the kernels).

Every function takes torch tensors of one floating dtype on one device and computes in that dtype: float64 is the truth the GPU
tests measure the kernels against, the same code in float32 is the yardstick of an fp32 GEMM.  Point-major (B, rows, C) layouts,
index tables as the kernels take them.  The ops are torch's (relu / leaky_relu / amax / sum), so NaN and inf propagate as in the
reference's module graph.
"""
import torch


def _gather(t, idx):
    """t (B, n, C), idx (B, S, k) integer -> (B, S, k, C)."""
    B = t.shape[0]
    return t[torch.arange(B, device=t.device).view(B, 1, 1), idx.long()]


def weight_net(d, wn):
    """WeightNet (model_utils.py:359-390, bn=False): 3 -> 8 -> 8 -> C, ReLU after every layer.  d (..., 3), wn [(W, b)] * 3."""
    w = d
    for W, b in wn:
        w = torch.relu(w @ W.T + b)
    return w


def sa_scale_f64(xyz, new_xyz, idx, q, wx, b1, layers, src_nuniq=None, out=None, out_offset=0, dst_nuniq=None):
    """rtk_sa_scale / rtk_sa_scale_split (rtk_fused.h:79-90, 141-146).
    xyz (B, n, 3), new_xyz (B, S, 3), idx (B, S, ns) from rtk_ball_query, q (B, n, c1) the per-point layer-1 projection.
    Layer 1 = relu(q[idx'] + Wx.(xyz[idx] - centroid) + b1) with idx' = 0 where idx >= src_nuniq[b] (xyz keeps the real idx);
    then every (W, b) of `layers` with ReLU; then the max over the ns neighbours -> (B, S, cout).
    With `out` ((B * S, pitch)): a copy of it with rows < dst_nuniq[b] written at columns out_offset .. + cout, the rest as given."""
    B, n = xyz.shape[:2]
    idx = idx.long()
    qidx = idx if src_nuniq is None else torch.where(idx < src_nuniq.to(idx.device).long().view(B, 1, 1), idx, torch.zeros_like(idx))
    h = torch.relu(_gather(q, qidx) + (_gather(xyz, idx) - new_xyz[:, :, None, :]) @ wx.T + b1)
    for W, b in layers:
        h = torch.relu(h @ W.T + b)
    y = h.amax(2)
    if out is None:
        return y
    S, cout = y.shape[1], y.shape[2]
    res = out.clone().to(y.dtype)
    live = torch.ones(B, S, dtype=torch.bool, device=y.device)
    if dst_nuniq is not None:
        live = torch.arange(S, device=y.device)[None, :] < dst_nuniq.to(y.device).long()[:, None]
    block = res[:, out_offset:out_offset + cout].reshape(B, S, cout)
    block[live] = y[live]
    res[:, out_offset:out_offset + cout] = block.reshape(B * S, cout)
    return res


def cost_volume_f64(xyz1, xyz2, knn, p1, p2, wd, layers, wn, decisions=None, with_acts=False):
    """rtk_cost_volume / _split / _split_shared (rtk_fused.h:92-99).  xyz1 (B, n1, 3), xyz2 (B, n2, 3), knn (B, n1, 16) into xyz2,
    p1 (B, n1, 256) (bias folded in), p2 (B, n2, 256), wd (256, 3).
    Layer 1 = leaky(p1[i] + p2[idx] + Wd.(xyz2[idx] - xyz1[i])), then layers (two 256 -> 256, LeakyReLU 0.1); the WeightNet wn
    on the same direction vectors; out[i] = sum over the 16 neighbours of wn * feat -> (B, n1, 256).
    decisions: three boolean (B, n1, 16, 256) tensors -- layer l is z * where(decisions[l], 1, 0.1) instead of leaky_relu(z, 0.1): the
    slopes a training forward saved for its backward (rtk_cost_volume_train: mask1, mask2, a3 > 0), so that autograd through this
    function differentiates the branch the operator took.  with_acts: -> (out, [a1, a2, a3]), the three (B, n1, 16, 256) activations."""
    if decisions is None:
        lk = lambda t, l: torch.nn.functional.leaky_relu(t, 0.1)
    else:
        one, slope = torch.ones((), dtype=p1.dtype, device=p1.device), torch.full((), 0.1, dtype=p1.dtype, device=p1.device)
        lk = lambda t, l: t * torch.where(decisions[l], one, slope)
    d = _gather(xyz2, knn) - xyz1[:, :, None, :]
    x = lk(p1[:, :, None, :] + _gather(p2, knn) + d @ wd.T, 0)
    acts = [x]
    for l, (W, b) in enumerate(layers):
        x = lk(x @ W.T + b, l + 1)
        acts.append(x)
    out = (weight_net(d, wn) * x).sum(2)
    return (out, acts) if with_acts else out


def decode_sign_masks(words):
    """The sign-mask words rtk_cost_volume_train / _split_train save for the backward kernels (rtk_fused.h), (M, 4) int64 -> (M, 256)
    bool: bit 4v + r of word (position, g) <-> channel 16v + 4g + r  (v < 16, g < 4, r < 4)."""
    M = words.shape[0]
    bits = (words.view(M, 4, 1) >> torch.arange(64, device=words.device).view(1, 1, 64)) & 1          # bit 4v + r
    return bits.view(M, 4, 16, 4).permute(0, 2, 1, 3).reshape(M, 256).bool()                          # channel 16v + 4g + r


# ---- WeightNet ReLU decisions: which of them a comparison across precisions can rely on -----------------------------------------
MARGIN = 1e-4


def margin(xyz1, xyz2, knn, wn):
    """min over the three WeightNet layers of (smallest |pre-activation|) / (largest |pre-activation| of the layer), on the
    directions xyz2[knn] - xyz1 (one cloud: xyz2 = xyz1)."""
    h = _gather(xyz2, knn) - xyz1[:, :, None, :]
    worst = float("inf")
    for W, b in wn:
        z = h @ W.T + b
        worst = min(worst, float(z.abs().min() / z.abs().max()))
        h = torch.relu(z)
    return worst


def clear_of_zero(xyz1, xyz2, knn, wn):
    """-> (keep (B, n1, 256) bool, number of channels of the three layers whose sign changes between positions).  keep[b, i, c]: no
    pre-activation that the gradient of out[b, i, c] passes through lies within MARGIN of its layer's largest magnitude of zero --
    none of the 16 hidden ones at any of query i's 16 positions, nor output channel c at any of them.  Directions xyz2[knn] - xyz1."""
    h = _gather(xyz2, knn) - xyz1[:, :, None, :]
    keep, mixed = None, 0
    for li, (W, b) in enumerate(wn):
        z = h @ W.T + b                                            # (B, n1, 16, C)
        near = z.abs() < MARGIN * z.abs().max()
        on = (z > 0).reshape(-1, z.shape[-1]).double().mean(0)
        mixed += int(((on > 0.02) & (on < 0.98)).sum())
        k = ~near.any(2) if li == 2 else ~near.any(3).any(2)[:, :, None]
        keep = k if keep is None else keep & k
        h = torch.relu(z)
    return keep, mixed


def patch_cost_f64(xyz, knn, feat, wn):
    """rtk_patch_cost (rtk_fused.h:101-104): out[i] = sum_k WeightNet(xyz[idx[i, k]] - xyz[i]) * feat[idx[i, k]].
    xyz (B, n, 3), knn (B, n, 16), feat (B, n, 256) -> (B, n, 256) point-major (the kernel's channel-major output is its transpose)."""
    d = _gather(xyz, knn) - xyz[:, :, None, :]
    return (weight_net(d, wn) * _gather(feat, knn)).sum(2)
