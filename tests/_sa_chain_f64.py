"""The contract of the set-abstraction training chain (ratrack_amd/train_ops.py sa_chain / _SAChain) restated in plain torch, in the
dtype of its inputs: no project kernel, no nn.BatchNorm.  tests/test_sa_chain_f64_cpu.py ties it to the framework's modules in
float64; tests/test_sa_chain_f64_gpu.py holds the kernels against it.  Also the cases of the GPU file (inputs drawn on the CPU from a
seed, so that a seed can be chosen on any machine), a host ball-query table and the launchers' sizing rules.

    proj           = W0[:, 3:] . cat(feats)                                          per source point
    z1[s,c,r,k]    = proj[s,c,idx[s,r,k]] + W0[c,:3] . dxyz[s,:,r,k]
    per layer and statistics group (S / groups consecutive samples), with w = row_w[s,r] (1 without weights):
        mean = sum w z / count,   var = sum w z^2 / count - mean^2
        y    = gamma (z - mean) rsqrt(var + eps) + beta,   a = [y > 0] y,   next z = W a
    last layer:  out[s,c,r] = max_k a, the gradient to the lowest k among equals, none where the max is not positive
    running statistics: group after group, running = (1 - m) running + m (mean, var count / (count - 1)); num_batches_tracked += groups
"""
import collections

import torch

BAND = 2e-6          # the forward's bound (_cost_volume_cases.BAND, tests/test_stage_f64_gpu.py::_check): a decision between values this
                     # close, relative to their layer's largest magnitude, may go either way
NO_ARG = 255         # karg of a row without gradient (its maximum is not positive)

Layer = collections.namedtuple("Layer", "weight gamma beta running_mean running_var eps momentum")      # weight: None for the first layer
Acts = collections.namedtuple("Acts", "zs ys means variances running decisions")


def sa_chain_f64(feats, w0, idx, dxyz, layers, row_w, count, groups, decisions=None, with_acts=False):
    """feats: list of (S,C_i,n_src); w0 (C1, 3 + sum C_i); idx (S,rows,ns) integer; dxyz (S,3,rows,ns); layers: list of Layer; row_w (S,rows)
    or None; decisions: None or ([mask_1 .. mask_L] bool (S,C_l,rows,ns), karg (S,C_L,rows) integer, NO_ARG = no gradient) replacing the
    y > 0 tests and the arg-max.  -> out (S,C_L,rows) [, Acts: the z and y of every layer, mean and biased variance (groups,C_l) per layer, the
    running statistics after the pass [(mean, var, batches added)], the decisions taken ([masks], karg)]."""
    S, rows, ns = idx.shape
    W0 = w0.reshape(w0.shape[0], -1)
    C1 = W0.shape[0]
    proj = torch.einsum("cf,sfn->scn", W0[:, 3:], torch.cat(list(feats), 1))
    gathered = torch.gather(proj, 2, idx.reshape(S, 1, rows * ns).expand(S, C1, rows * ns).long()).view(S, C1, rows, ns)
    z = gathered + torch.einsum("ca,sark->scrk", W0[:, :3], dxyz)
    w = row_w if row_w is not None else torch.ones(S, rows, dtype=z.dtype, device=z.device)
    per = S // groups
    zs, ys, means, variances, running, masks = [], [], [], [], [], []
    a = None
    for l, layer in enumerate(layers):
        if l > 0:
            z = torch.einsum("oc,scrk->sork", layer.weight.reshape(layer.weight.shape[0], -1), a)
        rm, rv = layer.running_mean.detach().clone(), layer.running_var.detach().clone()
        parts, mean_l, var_l = [], [], []
        for g in range(groups):
            zg, wg = z[g * per:(g + 1) * per], w[g * per:(g + 1) * per]
            mean = torch.einsum("sr,scrk->c", wg, zg) / count
            var = torch.einsum("sr,scrk->c", wg, zg * zg) / count - mean * mean
            parts.append(layer.gamma.view(1, -1, 1, 1) * (zg - mean.view(1, -1, 1, 1)) * torch.rsqrt(var + layer.eps).view(1, -1, 1, 1)
                         + layer.beta.view(1, -1, 1, 1))
            mean_l.append(mean)
            var_l.append(var)
            rm = (1 - layer.momentum) * rm + layer.momentum * mean.detach()
            rv = (1 - layer.momentum) * rv + layer.momentum * var.detach() * (count / (count - 1.0))
        y = torch.cat(parts, 0)
        mask = (y > 0) if decisions is None else decisions[0][l]
        a = torch.where(mask, y, torch.zeros_like(y))
        zs.append(z)
        ys.append(y)
        masks.append(mask)
        means.append(torch.stack(mean_l))
        variances.append(torch.stack(var_l))
        running.append((rm, rv, groups))
    if decisions is None:
        karg = first_argmax(a.detach())
    else:
        karg = decisions[1].long()
    pick = torch.arange(ns, device=a.device).view(1, 1, 1, ns) == karg.unsqueeze(-1)         # all false in a NO_ARG row
    out = torch.where(pick, a, torch.zeros_like(a)).sum(-1)
    if not with_acts:
        return out
    return out, Acts([t.detach() for t in zs], [t.detach() for t in ys], [t.detach() for t in means], [t.detach() for t in variances], running,
                     (masks, karg))


def first_argmax(a):
    """(.., ns) -> the lowest index of the maximum over the last axis, NO_ARG where the maximum is not positive."""
    ns = a.shape[-1]
    amax = a.max(-1, keepdim=True).values
    k = torch.where(a == amax, torch.arange(ns, device=a.device).expand_as(a), torch.full_like(a, ns, dtype=torch.long)).min(-1).values
    return torch.where(amax.squeeze(-1) > 0, k, torch.full_like(k, NO_ARG))


def ball_table(src, centres, radius, ns):
    """The ball-query table and the neighbour offsets in float64 on the host: src (S,n_src,3), centres (S,rows,3) -> idx (S,rows,ns) int32
    = the first ns source points, in index order, within `radius` of the centre, a short neighbourhood padded with its FIRST index (the
    reference's ball_query), dxyz (S,3,rows,ns) = src[idx] - centre, and the number of distinct neighbours (S,rows)."""
    src, centres = src.double(), centres.double()
    S, n_src, _ = src.shape
    inside = ((centres[:, :, None, :] - src[:, None, :, :]) ** 2).sum(-1) < radius * radius                  # (S,rows,n_src)
    order = torch.where(inside, torch.arange(n_src).expand_as(inside), torch.full(inside.shape, n_src)).sort(-1).values[:, :, :ns]
    found = inside.sum(-1).clamp(max=ns)
    assert (found > 0).all(), "an empty ball"
    idx = torch.where(order < n_src, order, order[:, :, :1].expand_as(order))
    nb = torch.gather(src, 1, idx.reshape(S, -1, 1).expand(S, idx.shape[1] * ns, 3)).view(S, idx.shape[1], ns, 3)
    dxyz = (nb - centres[:, :, None, :]).permute(0, 3, 1, 2).contiguous()
    return idx.to(torch.int32).contiguous(), dxyz, found


def first_copy(idx, dxyz):
    """(S,rows,ns) long: for every slot the lowest slot of its row that holds the same position (same index, same offset: the padding of
    a short neighbourhood).  Such slots tie EXACTLY in every layer; they are one value, not a near-tie."""
    same = (idx[:, :, :, None] == idx[:, :, None, :]) & (dxyz[:, :, :, :, None] == dxyz[:, :, :, None, :]).all(1)      # (S,rows,ns,ns)
    ns = idx.shape[2]
    return torch.where(same, torch.arange(ns, device=idx.device).view(1, 1, 1, ns).expand_as(same), torch.full_like(same, ns, dtype=torch.long)).min(-1).values


def band_shares(acts, idx, dxyz, live, skip=None):
    """From the float64 reference alone -> (share of the activations y of all layers within BAND of their layer's largest magnitude of
    zero, share of the live rows of the pooled layer whose best two DISTINCT positions lie within BAND of that magnitude of each other).
    live (S,rows) bool; skip: per layer the channels left out (channels a test sets to exactly zero)."""
    inside = total = 0
    for l, y in enumerate(acts.ys):
        near = y.abs() <= BAND * y.abs().max()
        if skip is not None and skip[l]:
            keep = torch.ones(y.shape[1], dtype=torch.bool, device=y.device)
            keep[skip[l]] = False
            near = near[:, keep]
        inside, total = inside + int(near.sum()), total + near.numel()
    y = acts.ys[-1]
    gap = top_two_gap(y, idx, dxyz)
    close = (gap <= BAND * y.abs().max()) & live.view(live.shape[0], 1, -1)
    if skip is not None and skip[-1]:
        close[:, skip[-1]] = False
    return inside / total, int(close.sum()) / max(int(live.sum()) * y.shape[1], 1)


def top_two_gap(y, idx, dxyz):
    """(S,C,rows): the pooled layer's largest y of a row minus the largest among the row's OTHER positions (first_copy); inf where the row
    holds one position only."""
    ns = y.shape[-1]
    fc = first_copy(idx.long(), dxyz).unsqueeze(1)                                                            # (S,1,rows,ns)
    top = y.max(-1, keepdim=True).values
    kbest = torch.where(y == top, torch.arange(ns, device=y.device).expand_as(y), torch.full_like(y, ns, dtype=torch.long)).min(-1, keepdim=True).values
    other = fc.expand_as(y) != torch.gather(fc.expand_as(y), 3, kbest)
    second = torch.where(other, y, torch.full_like(y, float("-inf"))).max(-1).values
    return top.squeeze(-1) - second


# ---- the cases -------------------------------------------------------------------------------------------------------------------

Spec = collections.namedtuple("Spec", "name chans ns S rows n_src groups seed feats weights table radius signs")
# feats: channels of the features tensors (virtual concatenation); weights: row weights (dead rows, heavy row 0) or None; table: the inverse
# table of the gather-form first-layer backward is passed; radius: a real ball table (ball_table) instead of random indices; signs: gammas
# of both signs.  What each case enters is in the table of tests/test_sa_chain_f64_gpu.py.
CASES = [
    Spec("model_16_16_32_ns4", [16, 16, 32], 4, 4, 57, 100, 2, 11, (13, 11), True, True, None, False),
    Spec("model_32_64_ns16", [32, 64], 16, 4, 61, 61, 2, 12, (24,), True, True, None, False),
    Spec("model_64_64_ns32", [64, 64], 32, 2, 37, 64, 1, 13, (24,), False, True, None, False),
    Spec("model_32_32_ns8_no_table", [32, 32], 8, 3, 50, 77, 1, 14, (24,), True, False, None, False),
    Spec("other_16_64_32_16", [16, 64, 32, 16], 8, 4, 45, 60, 2, 15, (24,), True, True, None, False),
    Spec("other_64_16", [64, 16], 4, 2, 45, 60, 1, 16, (24,), True, True, None, False),
    Spec("ball_padded", [16, 16, 32], 8, 4, 64, 64, 2, 17, (24,), True, True, 0.3, True),
    # the cheapest shape at which all three chain kernels loop (sizing): 5 chunks of 64 positions, so the apply kernel starts from a grid of
    # 2 and needs 2 S > 4096 to shrink it; S a multiple of 8 (the flattened grid of the first-layer backward, as in production)
    Spec("looping", [16, 16, 32], 16, 2056, 19, 24, 2, 18, (8,), True, True, None, False),
]
LOOPING = {"looping"}
HEAVY = {"looping"}          # too heavy for the CPU file: their band condition is asserted by the GPU file


def spec_by_name(name):
    return next(c for c in CASES if c.name == name)


class Case:
    """The inputs of one case in fp32 on the CPU, drawn from the spec's seed: feats, w0, idx (int32), dxyz, the layers' W / gamma / beta /
    running statistics, row_w (row 0 carries the copies of the rows de-duplicated away, rows from nuniq[s] on weigh 0), count, the
    cotangent ct (zero on dead rows)."""

    def __init__(self, spec):
        g = torch.Generator().manual_seed(spec.seed)
        self.spec = spec
        S, rows, ns, n_src = spec.S, spec.rows, spec.ns, spec.n_src
        self.feats = [torch.randn(S, c, n_src, generator=g) for c in spec.feats]
        cf = sum(spec.feats)
        self.w0 = torch.randn(spec.chans[0], 3 + cf, generator=g) / (3 + cf) ** 0.5 * 1.5
        self.found = None
        if spec.radius is None:
            self.idx = torch.randint(0, n_src, (S, rows, ns), generator=g, dtype=torch.int32)
            self.dxyz = torch.randn(S, 3, rows, ns, generator=g)
        else:
            src = torch.rand(S, n_src, 3, generator=g)
            self.idx, d64, self.found = ball_table(src, src[:, :rows], spec.radius, ns)
            self.dxyz = d64.float()          # (the fp32 offsets ARE the case's input: every precision starts from them)
        self.W, self.gamma, self.beta, self.rmean, self.rvar = [None], [], [], [], []
        for l, c in enumerate(spec.chans):
            if l > 0:
                self.W.append(torch.randn(c, spec.chans[l - 1], generator=g) / spec.chans[l - 1] ** 0.5 * 1.5)
            ga = torch.rand(c, generator=g) + 0.5
            if spec.signs:
                ga = ga * (1.0 - 2.0 * (torch.rand(c, generator=g) < 0.5).float())
            self.gamma.append(ga)
            self.beta.append(torch.rand(c, generator=g) - 0.5)
            self.rmean.append(torch.randn(c, generator=g))
            self.rvar.append(torch.rand(c, generator=g) * 1.5 + 0.5)
        self.npoint = rows + 7
        if spec.weights:
            self.nuniq = torch.tensor([max(rows - (0, 13, 0, rows // 2, 3)[s % 5], 1) for s in range(S)])
        else:
            self.nuniq = torch.full((S,), rows)
        self.live = torch.arange(rows).view(1, rows) < self.nuniq.view(S, 1)
        self.row_w = None
        if spec.weights:
            self.row_w = self.live.float()
            self.row_w[:, 0] += (self.npoint - self.nuniq).float()
        self.count = float((S // spec.groups) * (self.npoint if spec.weights else rows) * ns)
        self.ct = torch.randn(S, spec.chans[-1], rows, generator=g) * self.live.view(S, 1, rows).float()

    def leaves(self, dtype, device):
        """[w0, feats.., gamma_0, beta_0, W_1, gamma_1, beta_1, ..] as new leaves."""
        t = [self.w0] + self.feats
        for l in range(len(self.spec.chans)):
            t += ([self.W[l]] if l > 0 else []) + [self.gamma[l], self.beta[l]]
        return [x.detach().to(device=device, dtype=dtype).clone().requires_grad_(True) for x in t]

    def grad_names(self):
        n = ["dW0"] + ["dfeats%d" % i for i in range(len(self.feats))]
        for l in range(len(self.spec.chans)):
            n += (["dW%d" % l] if l > 0 else []) + ["dgamma%d" % l, "dbeta%d" % l]
        return n

    def reference(self, dtype, device, decisions=None, ct=None, grads=True):
        """sa_chain_f64 in `dtype` on `device` -> (out, Acts, the gradients of leaves() under the cotangent `ct`; None without `grads`)."""
        c = lambda t: None if t is None else t.detach().to(device=device, dtype=dtype)
        leaves = self.leaves(dtype, device)
        nf, L = len(self.feats), len(self.spec.chans)
        rest = leaves[1 + nf:]
        layers, p = [], 0
        for l in range(L):
            W = None
            if l > 0:
                W, p = rest[p], p + 1
            layers.append(Layer(W, rest[p], rest[p + 1], c(self.rmean[l]), c(self.rvar[l]), 1e-5, 0.1))
            p += 2
        with torch.set_grad_enabled(grads):
            out, acts = sa_chain_f64(leaves[1:1 + nf], leaves[0], self.idx.to(device), c(self.dxyz), layers, c(self.row_w), self.count,
                                     self.spec.groups, decisions=decisions, with_acts=True)
        g = list(torch.autograd.grad(out, leaves, c(self.ct if ct is None else ct))) if grads else None
        return out.detach(), acts, g


# ---- the launchers' sizing rules -------------------------------------------------------------------------------------------------

def sizing(S, rows, ns, chans, n_src):
    """{kernel: (units, workgroups, units a workgroup takes per pass)} from the launchers, for a chain without a workspace limit beyond
    train_ops' own (2 max(S, 1024) cin cout floats).  A kernel loops where units > workgroups x per pass.
      conv_fwd / conv_apply (csrc/train_conv.hip launch<MODE>): chunks of 64 positions, 4 per workgroup and pass; gx = ceil(chunks / 4)
          halved (rounding up) while gx S > 1024 (forward) / 4096 (apply) and gx > 1; per sample;
      wgrad_stats (rtk_conv_wgrad_stats): tiles of 32 positions, 4 per workgroup and pass; gx = ceil(tiles / 4) halved while
          gx S > 512 or gx S > max(S, 1024) (the workspace) and gx > 1; per sample;
      first_layer (csrc/train_bn.hip rtk_sa_first_layer): float4s of a plane, 256 per pass, one workgroup per sample and 8 channels
          (where C1 % 8 == 0, n_src <= 2048 and (C1 / 8) S >= 1024), 4 channels, or 1;
      pool_fwd (rtk_bn_relu_pool_fwd_fin_arg): float4s of a plane, 256 per pass, one workgroup per (channel, sample);
      pool_bwd_stats (rtk_pool_bwd_stats_arg): one wave per (channel, sample) plane of `rows` elements, 64 per pass;
      first_layer_bwd (csrc/train_group.hip rtk_sa_first_layer_bwd, P <= 8192): planes, one workgroup per sample and cg channels, cg =
          8 / 4 / 1 for C1 S >= 4096 / >= 1024 / less: `units` = cg planes walked by one workgroup, one per pass."""
    P = rows * ns
    chunks, tiles = -(-P // 64), -(-P // 32)

    def shrink(gx, limit):
        while gx * S > limit and gx > 1:
            gx = (gx + 1) // 2
        return gx
    res = {"conv_fwd": (chunks, shrink(-(-chunks // 4), 1024), 4), "conv_apply": (chunks, shrink(-(-chunks // 4), 4096), 4),
           "wgrad_stats": (tiles, shrink(-(-tiles // 4), min(512, max(S, 1024))), 4)}
    c1 = chans[0]
    cpb = 8 if (c1 % 8 == 0 and n_src * 32 <= 65536 and (c1 // 8) * S >= 1024) else 4 if (c1 % 4 == 0 and n_src * 16 <= 65536) else 1
    res["first_layer"] = (P // 4, 1, 256)
    res["first_layer_cpb"] = cpb
    res["pool_fwd"] = (P // 4, 1, 256)
    res["pool_bwd_stats"] = (rows, 1, 64)
    planes = c1 * S
    cg = 8 if planes >= 4096 else 4 if planes >= 1024 else 1
    res["first_layer_bwd"] = (cg, 1, 1)
    res["first_layer_bwd_flat_grid"] = S % 8 == 0
    return res


def loops(entry):
    units, wgs, per = entry
    return units > wgs * per


def last_unit_through_loop(entry):
    """The last (partial) unit's index is at or past the units of the first pass: a workgroup reaches it through its loop (and, in the
    conv kernels, through the prefetch across the back-edge)."""
    units, wgs, per = entry
    return units - 1 >= wgs * per


def memory_estimate(spec):
    """(bytes of the operator's saved fp32 z tensors, rough bytes of the float64 graph: z, z^2, y, a and a mask per layer + the gather)."""
    pos = spec.S * spec.rows * spec.ns
    ch = sum(spec.chans)
    return 4 * pos * ch, 8 * pos * (4 * ch + spec.chans[0]) + pos * ch
