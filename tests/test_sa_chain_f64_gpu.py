"""GPU: the set-abstraction training operator (train_ops.sa_chain: rtk_sa_first_layer, rtk_conv_bn_fwd_fin, rtk_bn_relu_pool_fwd_fin_arg
forward; rtk_pool_bwd_stats_arg, rtk_conv_wgrad_stats, rtk_conv_bn_bwd_apply, rtk_sa_first_layer_bwd or rtk_group_points_grad_set + bmm,
and the projection's rtk_pw_conv / rtk_pw_wgrad backward) against float64 autograd through the restatement of its contract
(tests/_sa_chain_f64.py, tied to the framework's modules by tests/test_sa_chain_f64_cpu.py): the output, every saved z, the published
BatchNorm constants, the running statistics and the gradients of every leaf under a random cotangent that is zero on dead rows, with
the batch statistics as float64 atomics and as fixed-point limbs (train_ops.DETERMINISTIC off and on).

The bound is the project's rule (tests/test_stage_f64_gpu.py::_check): the error relative to the tensor's largest element is at most
3 x the error of the same restatement run by torch in fp32 + 2e-7, and at most 2e-6 (CAPS: a tensor's own cap where torch fp32 itself
is past 2e-6 / 3 on it, set from torch fp32's measured error with the same factor 3).

The backward kernels recompute the ReLU decisions fma(z, scale, shift) > 0 from the fp32 z and constants the forward saved and read the
arg-max as saved; both references therefore run on the operator's own decisions, decoded from out.grad_fn.saved_tensors
(sa_chain_f64(decisions=...)), and separate assertions say that those are float64's own outside a band: a mask differs only where
float64's |y| is within BAND = 2e-6 of its layer's largest magnitude, karg is float64's lowest arg-max unless float64 puts the
operator's choice within the band of its own, karg is 255 exactly where float64's maximum is not positive (up to the band), and at
most 1e-3 of a case's activations / of its rows' top-two gaps between distinct positions lie inside the band (asserted without a GPU
in the CPU file for every case but `looping`, whose share is asserted here).

| id | chain, ns | S, rows, n_src, groups | what it enters |
|---|---|---|---|
| model_16_16_32_ns4 | [16,16,32], 4 | 4, 57, 100, 2 | instances (1,1), (1,2); P = 228: a partial 64-chunk and a partial 32-tile; two features tensors; dead rows, heavy row 0 |
| model_32_64_ns16 | [32,64], 16 | 4, 61, 61, 2 | instance (2,4), pooled source on a 64-channel layer (quarter passes) |
| model_64_64_ns32 | [64,64], 32 | 2, 37, 64, 1 | instance (4,4); no row weights |
| model_32_32_ns8_no_table | [32,32], 8 | 3, 50, 77, 1 | instance (2,2); inv=None: the scatter form of the first-layer backward |
| other_16_64_32_16 | [16,64,32,16], 8 | 4, 45, 60, 2 | instances (1,4), (4,2), (2,1) |
| other_64_16 | [64,16], 4 | 2, 45, 60, 1 | instance (4,1) |
| ball_padded | [16,16,32], 8 | 4, 64, 64, 2 | a real ball table, most neighbourhoods padded with their first index: exact ties; gammas of both signs |
| looping | [16,16,32], 16 | 2056, 19, 24, 2 | P = 304 = 4 x 64 + 48: 5 chunks / 10 tiles on ONE workgroup per sample in the forward, apply and weight-gradient kernels (the partial chunk and tile through the loop and the prefetch); 8-channel first layer; flattened grid of its backward |

The property tests (negative and zero gammas, rewritten dead rows) run the first case under the same rule: measured worst of any tensor
3.9e-7, torch fp32 4.2e-7.
"""
import pytest
import torch

from ratrack_amd import _lib
from ratrack_amd import train_ops as T
from ratrack_amd.pytorch_utils import SharedMLP

from _sa_chain_f64 import BAND, CASES, LOOPING, NO_ARG, Case, band_shares, first_argmax, first_copy, last_unit_through_loop, loops, \
    sizing, spec_by_name

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = [pytest.param(False, id="atomics"), pytest.param(True, id="fixed_point")]
# (case, tensor) -> the tensor's own cap = 3 x torch fp32's measured error on that case (module docstring).  The three are sums over the
# looping case's 0.6 M positions that the weight-gradient kernel carries in fp32 (G and H of rtk_conv_wgrad_stats: MFMA accumulators, then
# 1028 workgroup partials per group added in fp32); they pass the relative part of the rule, and torch fp32 is at or past 2e-6 / 3 itself:
# kernel / torch fp32 measured on an MI355X, either statistics mode: dgamma1 3.73e-6 / 1.50e-6, dbeta1 3.18e-6 / 1.93e-6, dW2 2.34e-6 / 7.41e-6.
CAPS = {("looping", "dgamma1"): 3 * 1.50e-6, ("looping", "dbeta1"): 3 * 1.93e-6, ("looping", "dW2"): 3 * 7.41e-6}


def operator(case, ct=None):
    """train_ops.sa_chain under torch.autograd.grad -> dict: out, zs, pars [(4, groups, C)], karg, zarg, running [(mean, var, batches)],
    grads in Case.grad_names() order."""
    spec = case.spec
    S, rows, ns, L = spec.S, spec.rows, spec.ns, len(spec.chans)
    mlp = SharedMLP([3 + sum(spec.feats)] + spec.chans, bn=True).to(DEV)
    layers = list(mlp.children())
    with torch.no_grad():
        layers[0].conv.weight.copy_(case.w0.view_as(layers[0].conv.weight))
        for l, layer in enumerate(layers):
            if l > 0:
                layer.conv.weight.copy_(case.W[l].view_as(layer.conv.weight))
            bn = layer.bn.bn
            bn.weight.copy_(case.gamma[l]); bn.bias.copy_(case.beta[l])
            bn.running_mean.copy_(case.rmean[l]); bn.running_var.copy_(case.rvar[l])
    feats = [f.to(DEV).clone().requires_grad_(True) for f in case.feats]
    idx, dxyz = case.idx.to(DEV).contiguous(), case.dxyz.to(DEV).contiguous()
    row_w = case.row_w.to(DEV).contiguous() if case.row_w is not None else None
    inv = None
    if spec.table:
        off = torch.empty(S, spec.n_src + 1, dtype=torch.int32, device=DEV)
        table = torch.empty(S, rows * ns, dtype=torch.int16, device=DEV)
        _lib.call("rtk_group_inverse_index", S, spec.n_src, rows * ns, idx.data_ptr(), off.data_ptr(), table.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
        inv = (off, table)
    out = T.sa_chain(feats, layers[0].conv.weight, idx, dxyz, layers, row_w, case.count, spec.groups, inv=inv)
    saved = out.grad_fn.saved_tensors
    zarg, karg = saved[3].clone(), saved[4].clone()
    zs, pars = [t.clone() for t in saved[5:5 + L]], [t.clone() for t in saved[5 + L:5 + 2 * L]]
    leaves = [layers[0].conv.weight] + feats
    for l, layer in enumerate(layers):
        leaves += ([layer.conv.weight] if l > 0 else []) + [layer.bn.bn.weight, layer.bn.bn.bias]
    grads = torch.autograd.grad(out, leaves, (case.ct if ct is None else ct).to(DEV))
    torch.cuda.synchronize()
    grads = [g.detach().reshape(g.shape[0], -1) if k.startswith("dW") else g.detach() for k, g in zip(case.grad_names(), grads)]
    running = [(l.bn.bn.running_mean.clone(), l.bn.bn.running_var.clone(), int(l.bn.bn.num_batches_tracked)) for l in layers]
    return dict(out=out.detach(), zs=zs, pars=pars, karg=karg, zarg=zarg, running=running, grads=grads)


def decode(case, op):
    """The operator's decisions from what its forward saved: ([fma(z, scale, shift) > 0 per layer], karg).  The product of two fp32
    numbers is exact in float64 and the sum's rounding keeps its sign: the sign of the float64 expression is the sign of the fp32 fma."""
    per = case.spec.S // case.spec.groups
    masks = []
    for z, par in zip(op["zs"], op["pars"]):
        sc, sh = (par[k].double().repeat_interleave(per, 0)[:, :, None, None] for k in (2, 3))
        masks.append(z.double() * sc + sh > 0)
    return masks, op["karg"].long()


def scale_err(got, r64):
    return float((got.double() - r64).abs().max() / r64.abs().max().clamp_min(1e-300))


def rule(rows, case_name):
    """rows: [(name, kernel, float64, torch fp32)].  The project's rule for every tensor; prints both errors of each."""
    bad = []
    for k, g, a, b in rows:
        assert g.shape == a.shape and torch.isfinite(g).all(), k
        e, e32 = scale_err(g, a), scale_err(b, a)
        print("   %-14s kernel %.2e  torch fp32 %.2e" % (k, e, e32))
        if not (e <= CAPS.get((case_name, k), 2e-6) and e <= 3 * e32 + 2e-7):
            bad.append((k, e, e32))
    assert not bad, bad


def constants(acts, gamma, beta, eps=1e-5):
    """[(mean, rstd, scale, shift) (groups, C)] of every layer as rtk_bn_fin publishes them, from a restatement's statistics."""
    res = []
    for m, v, ga, be in zip(acts.means, acts.variances, gamma, beta):
        rstd = torch.rsqrt(v + eps)
        res.append((m, rstd, ga.to(m) * rstd, be.to(m) - m * ga.to(m) * rstd))
    return res


def check_decisions(case, op, skip=None):
    """The operator's decisions are float64's own outside the band; the band is thin (module docstring)."""
    spec = case.spec
    _, free, _ = case.reference(torch.float64, DEV, grads=False)                      # float64 on its own decisions
    masks, karg = decode(case, op)
    flips = 0
    for l, (m, y) in enumerate(zip(masks, free.ys)):
        differ = m != (y > 0)
        flips += int(differ.sum())
        assert (y.abs()[differ] <= BAND * y.abs().max()).all(), "layer %d: a ReLU decision differs outside the band" % l
    y = free.ys[-1]
    M = y.abs().max()
    k64 = first_argmax(y.clamp_min(0))
    top = y.max(-1).values
    assert torch.equal(free.decisions[1], k64)
    both = (karg != NO_ARG) & (k64 != NO_ARG)
    chosen = torch.gather(y, 3, karg.clamp(max=spec.ns - 1).unsqueeze(-1)).squeeze(-1)
    differ = both & (karg != k64)
    assert (top[differ] - chosen[differ] <= BAND * M).all(), "an arg-max differs outside the band"
    assert (top[(karg == NO_ARG) != (k64 == NO_ARG)].abs() <= BAND * M).all(), "karg = 255 differs from 'the maximum is not positive' outside the band"
    # exact ties (padded slots): the lowest slot of the chosen position
    fc = first_copy(case.idx.to(DEV).long(), case.dxyz.to(DEV))
    lowest = torch.gather(fc.unsqueeze(1).expand(-1, karg.shape[1], -1, -1), 3, karg.clamp(max=spec.ns - 1).unsqueeze(-1)).squeeze(-1)
    assert (lowest == karg)[karg != NO_ARG].all(), "an exact tie went to a higher slot"
    near_zero, near_tie = band_shares(free, case.idx.to(DEV), case.dxyz.to(DEV).double(), case.live.to(DEV), skip)
    print("   %.1e of the activations near zero, %.1e of the rows near a tie; %d ReLU decisions and %d arg-maxes differ from float64's, %d rows "
          "without gradient" % (near_zero, near_tie, flips, int(differ.sum()), int((karg == NO_ARG).sum())))
    assert near_zero <= 1e-3 and near_tie <= 1e-3
    return free


def compare(case, ct=None, forward=True, decisions=True, skip=None):
    """The assertions of a case under the cotangent `ct` -> (operator's results, float64's gradients, torch fp32's)."""
    print("\n%s (DETERMINISTIC %s)" % (case.spec.name, T.DETERMINISTIC))
    op = operator(case, ct)
    dec = decode(case, op)
    if decisions:
        check_decisions(case, op, skip)
    o64, a64, g64 = case.reference(torch.float64, DEV, decisions=dec, ct=ct)
    o32, a32, g32 = case.reference(torch.float32, DEV, decisions=dec, ct=ct)
    rows = []
    if forward:
        rows.append(("out", op["out"], o64, o32))
        c64, c32 = constants(a64, case.gamma, case.beta), constants(a32, case.gamma, case.beta)
        for l in range(len(case.spec.chans)):
            rows.append(("z%d" % l, op["zs"][l], a64.zs[l], a32.zs[l]))
            for k, name in enumerate(("mean", "rstd", "scale", "shift")):
                rows.append(("%s%d" % (name, l), op["pars"][l][k], c64[l][k], c32[l][k]))
            rows.append(("running_mean%d" % l, op["running"][l][0], a64.running[l][0], a32.running[l][0]))
            rows.append(("running_var%d" % l, op["running"][l][1], a64.running[l][1], a32.running[l][1]))
            assert op["running"][l][2] == case.spec.groups == a64.running[l][2]
    rule(rows + list(zip(case.grad_names(), op["grads"], g64, g32)), case.spec.name)
    return op, g64, g32


def assert_loops(case):
    spec = case.spec
    sz = sizing(spec.S, spec.rows, spec.ns, spec.chans, spec.n_src)
    for k in ("conv_fwd", "conv_apply", "wgrad_stats"):
        assert loops(sz[k]) and last_unit_through_loop(sz[k]), (k, sz[k])
    assert case.live[:, -1].any() and (case.ct[:, :, -1] != 0).any()              # the last row (the partial chunk) carries cotangent


@pytest.mark.parametrize("det", MODES)
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_sa_chain_matches_float64_autograd(name, det, monkeypatch):
    """Every case of the table, both statistics modes: output, saved z, BatchNorm constants, running statistics, all gradients.
    Measured on an MI355X, error relative to the tensor's largest element against float64, kernel / torch fp32 (the two statistics
    modes agree to the figures shown).  Worst of the seven small cases, worst layer:
    out 3.4e-7 / 5.0e-7;  z 3.8e-7 / 4.0e-7;  mean 2.1e-7 / 3.6e-7;  rstd 7.8e-8 / 5.5e-7;  scale 1.1e-7 / 4.2e-7;  shift 1.5e-7 / 9.5e-7;
    running_mean 1.4e-7 / 1.5e-7;  running_var 1.4e-7 / 2.1e-7;  dW0 2.8e-7 / 6.1e-7;  dfeats 3.4e-7 / 4.4e-7;  dW 3.7e-7 / 9.4e-7;
    dgamma 4.8e-7 / 6.8e-7;  dbeta 5.2e-7 / 6.2e-7.  No ReLU decision and no arg-max of a small case differs from float64's; at most 1.6e-5
    of the activations and 1.5e-4 of the rows' top-two gaps lie inside the band.
    looping: out 2.4e-7 / 1.5e-6;  z 2.0e-7 / 7.9e-7;  mean 6.8e-8 / 1.7e-6;  rstd 8.8e-8 / 1.5e-6;  scale 8.2e-8 / 1.4e-6;  shift 1.2e-7 /
    2.2e-6;  running_mean 1.6e-7 / 1.6e-7;  running_var 9.0e-8 / 3.1e-7;  dW0 5.9e-7 / 5.4e-6;  dfeats 2.0e-7 / 1.0e-6;  dgamma0 1.3e-6 /
    1.1e-6;  dbeta0 1.1e-6 / 9.6e-7;  dW1 8.1e-7 / 3.4e-6;  dgamma1 3.7e-6 / 1.5e-6;  dbeta1 3.2e-6 / 1.9e-6;  dW2 2.3e-6 / 7.4e-6;  dgamma2
    1.2e-7 / 8.7e-7;  dbeta2 2.2e-8 / 1.4e-7: dgamma1, dbeta1 and dW2 pass the relative part of the rule but not the 2e-6 cap and take the
    caps of CAPS; 3 of its 40 M ReLU decisions differ from float64's, inside the band; 1.5e-5 of the activations and 4.5e-5 of the
    top-two gaps lie inside it.  No kernel was found wrong."""
    monkeypatch.setattr(T, "DETERMINISTIC", det)
    case = Case(spec_by_name(name))
    if name in LOOPING:
        assert_loops(case)
    compare(case)


@pytest.mark.parametrize("det", MODES)
def test_sa_chain_exact_ties_go_to_the_lowest_slot(det, monkeypatch):
    """ball_padded: in every row whose maximum sits at a position that padding repeats, karg is the lowest of that position's slots (the
    maximum is then shared exactly: same index, same offset, same z in every layer) -- more than 1000 such rows --, and the forward,
    dfeats, dW0 and everything else still meet the rule (compare; figures in test_sa_chain_matches_float64_autograd)."""
    monkeypatch.setattr(T, "DETERMINISTIC", det)
    case = Case(spec_by_name("ball_padded"))
    op, _, _ = compare(case)
    fc = first_copy(case.idx.long(), case.dxyz).to(DEV).unsqueeze(1)                  # (S,1,rows,ns)
    karg, z = op["karg"].long(), op["zs"][-1]
    has = karg != NO_ARG
    kc = karg.clamp(max=case.spec.ns - 1).unsqueeze(-1)
    position = torch.gather(fc.expand(-1, karg.shape[1], -1, -1), 3, kc)                # the chosen slot's position (its lowest slot)
    copies = fc == position                                                              # (S,C,rows,ns): all slots of that position
    shared = (copies.sum(-1) > 1) & has
    assert int(shared.sum()) > 1000
    assert (torch.where(copies, z, torch.gather(z, 3, kc)) == torch.gather(z, 3, kc)).all()      # ... which do tie exactly
    assert torch.equal(position.squeeze(-1)[shared], karg[shared])


@pytest.mark.parametrize("det", MODES)
@pytest.mark.parametrize("name", ["model_16_16_32_ns4", "looping"])
@pytest.mark.parametrize("exponent", [-30, 13])
def test_sa_chain_cotangent_of_any_magnitude(name, exponent, det, monkeypatch):
    """The whole cotangent times 2^-30 and 2^13 (the range test_batch_statistics_hold_at_any_scale claims for the fixed-point backward
    sums): every gradient under the same rule.  Measured on an MI355X, kernel / torch fp32, worst of the two exponents and modes:
    model_16_16_32_ns4: dW0 1.3e-7 / 2.7e-7;  dfeats 2.9e-7 / 3.2e-7;  dgamma0 2.4e-7 / 3.9e-7;  dbeta0 1.4e-7 / 1.7e-7;  dW1 1.8e-7 / 3.3e-7;
    dgamma1 3.0e-7 / 2.9e-7;  dbeta1 1.5e-7 / 1.6e-7;  dW2 2.8e-7 / 2.0e-7;  dgamma2 1.7e-7 / 2.1e-7;  dbeta2 1.8e-8 / 9.7e-8.
    looping: dW0 1.0e-6 / 5.4e-6, everything else the figures of the unit cotangent (test_sa_chain_matches_float64_autograd)."""
    monkeypatch.setattr(T, "DETERMINISTIC", det)
    case = Case(spec_by_name(name))
    compare(case, ct=case.ct * 2.0 ** exponent, forward=False, decisions=False)


@pytest.mark.parametrize("det", MODES)
def test_sa_chain_negative_gamma_takes_the_smallest_z(det, monkeypatch):
    """Every second gamma of every layer negative: the pooled maximum of such a channel sits at the row's SMALLEST z (row_argmax takes
    the max of fma(z, scale, shift), not of z), from the saved z and karg; and the rule for everything."""
    monkeypatch.setattr(T, "DETERMINISTIC", det)
    case = Case(spec_by_name("model_16_16_32_ns4"))
    for ga in case.gamma:
        ga[1::2] *= -1.0
    op, _, _ = compare(case)
    z, karg = op["zs"][-1], op["karg"].long()
    has = karg != NO_ARG
    zsel = torch.gather(z, 3, karg.clamp(max=case.spec.ns - 1).unsqueeze(-1)).squeeze(-1)
    neg = (case.gamma[-1] < 0).to(DEV).view(1, -1, 1).expand_as(has)
    assert (has & neg).sum() > 100 and (has & ~neg).sum() > 100
    assert torch.equal(zsel[has & neg], z.min(-1).values[has & neg]) and torch.equal(zsel[has & ~neg], z.max(-1).values[has & ~neg])
    assert torch.equal(zsel[has], op["zarg"][has])


@pytest.mark.parametrize("det", MODES)
def test_sa_chain_zero_gamma_and_beta_give_exact_zeros(det, monkeypatch):
    """gamma = beta = 0 on channel 3 of the first layer and channel 5 of the last: y is exactly 0 there, the masks all false, karg 255,
    the output 0, and every gradient through them exactly zero, as in the reference."""
    monkeypatch.setattr(T, "DETERMINISTIC", det)
    case = Case(spec_by_name("model_16_16_32_ns4"))
    L = len(case.spec.chans)
    case.gamma[0][3] = case.beta[0][3] = 0.0
    case.gamma[-1][5] = case.beta[-1][5] = 0.0
    skip = [[3]] + [[] for _ in range(L - 2)] + [[5]]
    op, g64, _ = compare(case, skip=skip)
    masks, karg = decode(case, op)
    assert not masks[0][:, 3].any() and not masks[-1][:, 5].any()
    assert (karg[:, 5] == NO_ARG).all() and (op["out"][:, 5] == 0).all()
    g = dict(zip(case.grad_names(), op["grads"]))
    r = dict(zip(case.grad_names(), g64))
    last = L - 1
    for k, t in (("dW0", lambda d: d["dW0"][3]), ("dgamma0", lambda d: d["dgamma0"][3]), ("dbeta0", lambda d: d["dbeta0"][3]),
                 ("dW1", lambda d: d["dW1"][:, 3]), ("dW%d" % last, lambda d: d["dW%d" % last][5]),
                 ("dgamma%d" % last, lambda d: d["dgamma%d" % last][5]), ("dbeta%d" % last, lambda d: d["dbeta%d" % last][5])):
        assert (t(g) == 0).all() and (t(r) == 0).all(), k


@pytest.mark.parametrize("det", MODES)
def test_sa_chain_dead_rows_are_inert(det, monkeypatch):
    """Other finite idx / dxyz content in the weight-0 rows: with the fixed-point statistics the output on live rows, every gradient and
    the running statistics are unchanged bit for bit (every contribution of such a row carries the factor w = 0 or the zero
    cotangent); with the atomics the rewritten case meets the rule."""
    monkeypatch.setattr(T, "DETERMINISTIC", det)
    a, b = Case(spec_by_name("model_16_16_32_ns4")), Case(spec_by_name("model_16_16_32_ns4"))
    g = torch.Generator().manual_seed(77)
    dead = ~b.live
    assert dead.any()
    b.idx[dead] = torch.randint(0, b.spec.n_src, b.idx.shape, generator=g, dtype=torch.int32)[dead]
    b.dxyz.copy_(torch.where(dead[:, None, :, None], torch.randn(b.dxyz.shape, generator=g) * 3.0, b.dxyz))
    if not det:
        compare(b)
        return
    ra, rb = operator(a), operator(b)
    live = a.live.to(DEV)[:, None, :].expand_as(ra["out"])
    assert not torch.equal(ra["zs"][0], rb["zs"][0])
    assert torch.equal(ra["out"][live], rb["out"][live])
    for k, x, y in zip(a.grad_names(), ra["grads"], rb["grads"]):
        assert torch.equal(x, y), k
    for (m1, v1, n1), (m2, v2, n2) in zip(ra["running"], rb["running"]):
        assert torch.equal(m1, m2) and torch.equal(v1, v2) and n1 == n2


def test_sa_chain_groups_are_independent(monkeypatch):
    """groups = 2, fixed-point statistics: other samples in group 1 (features, table, offsets, cotangent) leave group 0's output rows
    and dfeats bit for bit, and change group 1's."""
    monkeypatch.setattr(T, "DETERMINISTIC", True)
    a, b = Case(spec_by_name("model_16_16_32_ns4")), Case(spec_by_name("model_16_16_32_ns4"))
    g = torch.Generator().manual_seed(78)
    h = a.spec.S // 2
    for f in b.feats:
        f[h:] = torch.randn(f[h:].shape, generator=g) * 2.0
    b.idx[h:] = torch.randint(0, b.spec.n_src, b.idx[h:].shape, generator=g, dtype=torch.int32)
    b.dxyz[h:] = torch.randn(b.dxyz[h:].shape, generator=g)
    b.ct[h:] = torch.randn(b.ct[h:].shape, generator=g) * b.live[h:, None, :].float()
    ra, rb = operator(a), operator(b)
    assert torch.equal(ra["out"][:h], rb["out"][:h]) and not torch.equal(ra["out"][h:], rb["out"][h:])
    for i in range(len(a.feats)):
        assert torch.equal(ra["grads"][1 + i][:h], rb["grads"][1 + i][:h]) and not torch.equal(ra["grads"][1 + i][h:], rb["grads"][1 + i][h:])


def test_sa_chain_looping_is_reproducible_run_to_run(monkeypatch):
    """Fixed-point statistics: two runs of the looping case give bit-identical outputs, saved tensors and gradients."""
    monkeypatch.setattr(T, "DETERMINISTIC", True)
    case = Case(spec_by_name("looping"))
    ra, rb = operator(case), operator(case)
    assert torch.equal(ra["out"], rb["out"]) and torch.equal(ra["karg"], rb["karg"])
    for x, y in zip(ra["zs"] + ra["pars"] + ra["grads"], rb["zs"] + rb["pars"] + rb["grads"]):
        assert torch.equal(x, y)
