"""Float64 restatement of the per-point chain family -- rtk_pointwise_mlp, rtk_pointwise_mlp_tap, rtk_pointwise_mlp_pair -- written
from the contract in include/rtk_fused.h (not from the kernels), in the style of tests/_stage_f64.py.

Every function takes torch tensors of one floating dtype on one device and computes in that dtype: float64 is the truth the GPU
tests measure the kernels against, the same code in float32 is the yardstick of an fp32 GEMM.  The ops are torch's, so NaN and inf
propagate as in the reference's module graph.

Layouts: a per-point source is (B, n, C), a per-sample one (B, C); the interpolation segment's known rows are (B, m, C); a layer is
(W (cout, cin), b (cout), act) with act one of RTK_ACT_* (0 none, 1 ReLU, 2 LeakyReLU 0.1, 3 sigmoid)."""
import torch

ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_SIGMOID = 0, 1, 2, 3


def ceil16(c):
    return (c + 15) // 16 * 16


def activation(x, act):
    if act == ACT_RELU:
        return torch.relu(x)
    if act == ACT_LEAKY:
        return torch.nn.functional.leaky_relu(x, 0.1)
    if act == ACT_SIGMOID:
        return torch.sigmoid(x)
    assert act == ACT_NONE
    return x


def interp_segment(known, idx, dist2, nuniq=None):
    """rtk_interp_t: r = 1 / (sqrt(d2) + 1e-8), w = r / sum r, the weighted sum of the three known rows idx names; known rows at or
    past nuniq[b] are read as row 0.  known (B, m, C), idx (B, n, 3) integer, dist2 (B, n, 3) -> (B, n, C)."""
    B = known.shape[0]
    idx = idx.long()
    if nuniq is not None:
        idx = torch.where(idx < nuniq.to(idx.device).long().view(B, 1, 1), idx, torch.zeros_like(idx))
    r = 1.0 / (torch.sqrt(dist2.to(known.dtype)) + 1e-8)
    w = r / r.sum(2, keepdim=True)
    rows = known[torch.arange(B, device=known.device).view(B, 1, 1), idx]          # (B, n, 3, C)
    return (rows * w[..., None]).sum(2)


def input_vector(n, srcs, interp=None):
    """[interp segment] || srcs[0] || srcs[1] ..., each segment zero-padded to a multiple of 16 channels -> (B, n, 16 U).
    srcs: list of (tensor, per_sample); interp: (known, idx, dist2, nuniq or None)."""
    segs = []
    if interp is not None:
        segs.append(interp_segment(*interp))
    for t, per_sample in srcs:
        segs.append(t[:, None, :].expand(t.shape[0], n, t.shape[1]) if per_sample else t)
    return torch.cat([torch.nn.functional.pad(s, (0, ceil16(s.shape[-1]) - s.shape[-1])) for s in segs], 2)


def _pad_layer(w, b, cin):
    """(W, b) zero-extended to (ceil16(cout), cin): the 16-channel blocks a kernel computes (the padding channels see W = 0, b = 0)."""
    cout = ceil16(w.shape[0])
    wp = torch.zeros(cout, cin, dtype=w.dtype, device=w.device)
    wp[:w.shape[0], :w.shape[1]] = w
    bp = torch.zeros(cout, dtype=w.dtype, device=w.device)
    bp[:b.shape[0]] = b
    return wp, bp


def chain(x, layers, sample_bias=None):
    """y = act(W x + b) layer after layer on x (B, n, 16 U) -> (B, n, 16 * last cout16); sample_bias (B, >= cout of layer 0) is added
    to layer 0's pre-activation."""
    for i, (w, b, act) in enumerate(layers):
        wp, bp = _pad_layer(w, b, x.shape[-1])
        x = x @ wp.T + bp
        if i == 0 and sample_bias is not None:
            sb = torch.zeros(x.shape[0], x.shape[-1], dtype=x.dtype, device=x.device)
            c = min(sample_bias.shape[1], x.shape[-1])
            sb[:, :c] = sample_bias[:, :c]
            x = x + sb[:, None, :]
        x = activation(x, act)
    return x


def pointwise_f64(n, srcs, layers, interp=None, sample_bias=None, out_channels=None, out=None, channel_major=False, row_nuniq=None,
                  colmax=False):
    """rtk_pointwise_mlp (rtk_fused.h): B samples of n rows.
    Without `out`: the (B, n, out_channels) result of every row.  With `out` -- what the output buffer held before the launch,
    point-major (>= B n rows, pitch >= out_channels) or, channel_major, (B, out_channels, n) -- a copy of it with channels
    < out_channels of the rows r < row_nuniq[b] written and everything else as given.
    colmax: also return the (B, 16 * last cout16) maximum over the live rows of every output channel, started from the caller's
    zeros (a sample's padding channels see W = 0 and b = 0: act(0))."""
    x = input_vector(n, srcs, interp)
    B = x.shape[0]
    y = chain(x, layers, sample_bias)
    oc = layers[-1][0].shape[0] if out_channels is None else out_channels
    live = torch.ones(B, n, dtype=torch.bool, device=y.device)
    if row_nuniq is not None:
        live = torch.arange(n, device=y.device)[None, :] < row_nuniq.to(y.device).long()[:, None]
    res = y[:, :, :oc]
    if out is not None:
        res = out.clone().to(y.dtype)
        if channel_major:
            block = res.permute(0, 2, 1)                                             # a view: (B, n, oc)
            block[live] = y[:, :, :oc][live]
        else:
            block = res[:B * n, :oc].reshape(B, n, oc)
            block[live] = y[:, :, :oc][live]
            res[:B * n, :oc] = block.reshape(B * n, oc)
    if not colmax:
        return res
    neg = torch.full_like(y, float("-inf"))
    cm = torch.where(live[:, :, None], y, neg).amax(1).clamp_min(0.0)
    return res, cm


def tap_f64(n, interp, layer, proj, frame_split):
    """rtk_pointwise_mlp_tap: the layer on the 128-channel interpolation segment alone, with its column maximum, and proj[k] (k = 0
    for samples < frame_split, 1 for the others) applied to the layer's output -> (out (B, n, 128), colmax (B, 128),
    proj_out (B, n, 256))."""
    out, cm = pointwise_f64(n, [], [layer], interp=interp, colmax=True)
    B = out.shape[0]
    p = [pointwise_f64(n, [(out, False)], [proj[k]]) for k in (0, 1)]
    first = (torch.arange(B, device=out.device) < frame_split).view(B, 1, 1)
    return out, cm, torch.where(first, p[0], p[1])


def pair_f64(n, srcs, sample_bias, layer_a, layers_b, out_b_channels):
    """rtk_pointwise_mlp_pair: chain A (one layer) on every source with its sample bias -> (B, n, cout A); chain B on the last source
    alone -> channel-major (B, out_b_channels, n)."""
    a = pointwise_f64(n, srcs, [layer_a], sample_bias=sample_bias)
    b = pointwise_f64(n, srcs[-1:], layers_b, out_channels=out_b_channels)
    return a, b.permute(0, 2, 1)
