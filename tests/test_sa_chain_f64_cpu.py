"""No GPU: the restatement of the set-abstraction training chain (tests/_sa_chain_f64.py) against the framework's own modules in
float64, and the conditions on the cases of tests/test_sa_chain_f64_gpu.py that the float64 reference and the launchers' sizing rules
alone decide (so a seed or a shape can be chosen on any machine).

The looping case is too heavy for this file (0.6 M positions): its band condition is asserted by the GPU file, on the device.
"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from _sa_chain_f64 import CASES, HEAVY, LOOPING, Case, ball_table, band_shares, first_copy, last_unit_through_loop, loops, \
    memory_estimate, sizing, spec_by_name

LIGHT = [c.name for c in CASES if c.name not in HEAVY]


def framework_chain(case):
    """Conv2d / BatchNorm2d(train) / ReLU / max_pool2d in float64 on the EXPANDED tensor: row r of sample s repeated row_w[s, r] times
    (dead rows not at all), the statistics groups as sequential calls.  -> (out on the expanded rows, position of every live row's first
    copy, the leaves in Case.leaves() order, the BatchNorm modules)."""
    spec = case.spec
    S, rows, ns, L = spec.S, spec.rows, spec.ns, len(spec.chans)
    leaves = case.leaves(torch.float64, "cpu")
    w0, feats, rest = leaves[0], leaves[1:1 + len(case.feats)], leaves[1 + len(case.feats):]
    reps = case.row_w.long() if case.row_w is not None else torch.ones(S, rows, dtype=torch.long)
    rid = torch.stack([torch.repeat_interleave(torch.arange(rows), reps[s]) for s in range(S)])              # (S, npoint)
    first = torch.cumsum(reps, 1) - reps                                                                        # first copy of row r
    idx = torch.gather(case.idx.long(), 1, rid[:, :, None].expand(S, rid.shape[1], ns))
    dxyz = torch.gather(case.dxyz.double(), 2, rid[:, None, :, None].expand(S, 3, rid.shape[1], ns))
    x = torch.cat(feats, 1)
    grouped = torch.gather(x, 2, idx.reshape(S, 1, -1).expand(S, x.shape[1], -1)).view(S, x.shape[1], rid.shape[1], ns)
    h = torch.cat([dxyz, grouped], 1)
    bns, p = [], 0
    per = S // spec.groups
    for l in range(L):
        W = w0 if l == 0 else rest[p]
        p += 1 if l > 0 else 0
        bn = nn.BatchNorm2d(spec.chans[l]).double()          # holds the running statistics; the affine parameters are the leaves
        with torch.no_grad():
            bn.running_mean.copy_(case.rmean[l])
            bn.running_var.copy_(case.rvar[l])
        z = F.conv2d(h, W.view(W.shape[0], -1, 1, 1))
        # sequential calls, as the reference's per-frame passes
        parts = [F.batch_norm(z[g * per:(g + 1) * per], bn.running_mean, bn.running_var, rest[p], rest[p + 1], True, bn.momentum, bn.eps)
                 for g in range(spec.groups)]
        bn.num_batches_tracked += spec.groups
        h = F.relu(torch.cat(parts, 0))
        bns.append(bn)
        p += 2
    out = F.max_pool2d(h, kernel_size=[1, ns]).squeeze(-1)
    return out, first, leaves, bns


@pytest.mark.parametrize("name", LIGHT)
def test_restatement_matches_the_framework_in_float64(name):
    """Output on the live rows, every gradient and the running statistics of the restatement (decisions=None) against nn.functional
    conv2d / batch_norm(training) / relu / max_pool2d on the expanded tensor, to 1e-12 of each tensor's largest element."""
    case = Case(spec_by_name(name))
    spec = case.spec
    out, acts, grads = case.reference(torch.float64, "cpu")
    fo, first, leaves, bns = framework_chain(case)
    S, C, rows = out.shape
    pos = first.clamp(max=fo.shape[2] - 1)[:, None, :].expand(S, C, rows)
    live = case.live[:, None, :].expand(S, C, rows)
    def close(a, b, what):
        a, b = a.detach(), b.detach()
        assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max()), "%s: %.2e" % (what, float((a - b).abs().max() / b.abs().max()))
    close(out[live], torch.gather(fo, 2, pos)[live], "out")
    ct = torch.zeros_like(fo)
    ct.scatter_add_(2, pos, case.ct.double() * live)             # the cotangent on the first copy only: the copies have no consumers
    fg = torch.autograd.grad(fo, leaves, ct)
    for k, a, b in zip(case.grad_names(), grads, fg):
        close(a, b, k)
    for l, bn in enumerate(bns):
        # F.batch_norm updates the buffers it is given
        close(acts.running[l][0], bn.running_mean, "running_mean %d" % l)
        close(acts.running[l][1], bn.running_var, "running_var %d" % l)
        assert acts.running[l][2] == spec.groups == int(bn.num_batches_tracked)


@pytest.mark.parametrize("name", ["model_16_16_32_ns4", "ball_padded"])
def test_restatement_on_its_own_decisions_reproduces_itself(name):
    case = Case(spec_by_name(name))
    out, acts, grads = case.reference(torch.float64, "cpu")
    out2, acts2, grads2 = case.reference(torch.float64, "cpu", decisions=acts.decisions)
    assert torch.equal(out, out2) and torch.equal(acts.decisions[1], acts2.decisions[1])
    for k, a, b in zip(case.grad_names(), grads, grads2):
        assert torch.equal(a, b), k


@pytest.mark.parametrize("name", LIGHT)
def test_cases_stay_clear_of_the_band(name):
    """At most 1e-3 of a case's activations lie within BAND of zero, and at most 1e-3 of its live rows have their two best distinct
    positions within BAND of each other, by the float64 reference alone."""
    case = Case(spec_by_name(name))
    _, acts, _ = case.reference(torch.float64, "cpu", grads=False)
    near_zero, near_tie = band_shares(acts, case.idx, case.dxyz.double(), case.live)
    print("%s: %.1e of the activations near zero, %.1e of the rows near a tie" % (name, near_zero, near_tie))
    assert near_zero <= 1e-3 and near_tie <= 1e-3


def test_ball_table_pads_short_neighbourhoods_with_their_first_index():
    """The host table against a loop, and what the ball_padded case is for: most of its neighbourhoods are short, so that most rows hold
    exact ties; the dead rows and gammas of both signs are there too."""
    g = torch.Generator().manual_seed(3)
    src = torch.rand(2, 30, 3, generator=g)
    idx, dxyz, found = ball_table(src, src[:, :9], 0.35, 4)
    for s in range(2):
        for r in range(9):
            near = [q for q in range(30) if float(((src[s, q].double() - src[s, r].double()) ** 2).sum()) < 0.35 ** 2]
            want = (near + [near[0]] * 4)[:4] if len(near) < 4 else near[:4]
            assert idx[s, r].tolist() == want and int(found[s, r]) == min(len(near), 4)
            assert torch.equal(dxyz[s, :, r, :].T, src[s, want].double() - src[s, r].double())
    case = Case(spec_by_name("ball_padded"))
    short = case.found < case.spec.ns
    assert float(short.float().mean()) > 0.5
    fc = first_copy(case.idx.long(), case.dxyz)
    assert ((fc != torch.arange(case.spec.ns)).any(-1) == short).all()              # a padded row, and only a padded row, repeats a position
    assert all((ga > 0).any() and (ga < 0).any() for ga in case.gamma)
    assert (case.row_w == 0).any() and (case.row_w[:, 0] > 1).all()


def test_every_instance_of_the_chain_kernels_is_entered():
    """The table launches all nine (cin / 16, cout / 16) instances that sa_chain_supported admits, the pooled source on each last pair."""
    pairs = {(a // 16, b // 16) for c in CASES for a, b in zip(c.chans, c.chans[1:])}
    assert pairs == {(u, v) for u in (1, 2, 4) for v in (1, 2, 4)}
    assert {c.ns for c in CASES} == {4, 8, 16, 32}


@pytest.mark.parametrize("name", sorted(LOOPING))
def test_looping_case_loops(name):
    """By the launchers' sizing rules the forward conv kernel, the apply kernel and the weight-gradient + statistics kernel all give a
    workgroup more units than one pass takes, the partial last 64-position chunk and the partial last 32-position tile among those
    reached through the loop; the first layer takes its 8-channel form and its backward the flattened grid, as in production."""
    spec = spec_by_name(name)
    P = spec.rows * spec.ns
    sz = sizing(spec.S, spec.rows, spec.ns, spec.chans, spec.n_src)
    for k in ("conv_fwd", "conv_apply", "wgrad_stats"):
        assert loops(sz[k]) and last_unit_through_loop(sz[k]), "%s: %r does not loop: the sizing rules or the shape changed" % (k, sz[k])
    assert P % 64 != 0 and P % 32 != 0 and P % 4 == 0
    assert sz["first_layer_cpb"] == 8 and sz["first_layer_bwd"][0] == 8 and sz["first_layer_bwd_flat_grid"]
    saved, graph = memory_estimate(spec)
    assert saved <= 512 << 20 and graph <= 3 << 30, (saved, graph)
    # ... and no other case does: what they enter is one pass per workgroup
    for c in CASES:
        if c.name not in LOOPING:
            s2 = sizing(c.S, c.rows, c.ns, c.chans, c.n_src)
            assert not any(loops(s2[k]) for k in ("conv_fwd", "conv_apply", "wgrad_stats")), c.name
