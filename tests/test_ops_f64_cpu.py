"""CPU: the ground tests/test_ops_f64_gpu.py stands on (tests/_ops_f64.py) -- the oracle's fp32 results satisfy every derived bound
on every case, the checker rejects a dropped / doubled / misplaced contribution and a wrong prefill, the case table reaches every
kernel instance the dispatch mirror can return, and the constants the mirror restates still stand in ops_pointnet2.hip."""
import pytest
import torch

from oracle import pointnet2_ref as P

import _ops_f64 as O


# ------------------------------------------------------------------------------------------------
# the oracle through both conventions: zero-filled buffer ("set") and prefilled buffer ("accumulate")
# ------------------------------------------------------------------------------------------------
def _oracle_group_grad(d, prefill):
    k = d.case
    out = torch.zeros(k.b, k.c, k.n) if prefill is None else prefill.clone()
    P.group_points_grad_wrapper(k.b, k.c, k.n, k.npoint, k.nsample, d.go, d.idx, out)
    return out


def _oracle_gather_grad(d, prefill):
    k = d.case
    out = torch.zeros(k.b, k.c, k.n) if prefill is None else prefill.clone()
    P.gather_points_grad_wrapper(k.b, k.c, k.n, k.npoint, d.go, d.idx, out)
    return out


def _oracle_interpolate_grad(d, prefill):
    k = d.case
    out = torch.zeros(k.b, k.c, k.m) if prefill is None else prefill.clone()
    P.three_interpolate_grad_wrapper(k.b, k.c, k.n, k.m, d.go, d.idx, d.w, out)
    return out


def _contributions(op, d):
    """((B,C,T) float64 contributions, (B,T) addresses) of a gradient case."""
    if op == "interpolate":
        return O.interpolate_contributions(d.go, d.idx, d.w)
    B, C = d.go.shape[:2]
    return d.go.double().reshape(B, C, -1), d.idx.reshape(B, -1).long()


GRAD_OPS = {
    "group": (O.GROUP_GRAD_CASES, O.group_grad_data, _oracle_group_grad),
    "gather": (O.GATHER_CASES, O.gather_data, _oracle_gather_grad),
    "interpolate": (O.INTERPOLATE_GRAD_CASES, O.interpolate_grad_data, _oracle_interpolate_grad),
}
GRAD_PARAMS = [(op, name) for op, (cases, _, _) in GRAD_OPS.items() for name in O.names(cases)]


@pytest.mark.parametrize("op,name", GRAD_PARAMS)
def test_oracle_gradients_satisfy_the_bound(op, name):
    _, data, oracle = GRAD_OPS[op]
    d = data(name)
    assert O.check_scatter(oracle(d, None), d.st) <= 1.0
    assert O.check_scatter(oracle(d, d.prefill), d.st, d.prefill) <= 1.0


def _addresses(op, name):
    case = next(k for k in GRAD_OPS[op][0] if k.name == name)
    return case.m if op == "interpolate" else case.n


@pytest.mark.parametrize("op,name,corruption", [(op, name, corruption) for op, name in GRAD_PARAMS for corruption in ("drop", "double", "move")
                                                if corruption != "move" or _addresses(op, name) > 1])      # `move` needs a second address
def test_checker_rejects_a_wrong_contribution(op, name, corruption):
    """One contribution (the largest of the case) dropped, added twice, or added to the neighbouring address: rejected in both
    conventions."""
    _, data, oracle = GRAD_OPS[op]
    d = data(name)
    n = d.st.sum.shape[2]
    x, addr = _contributions(op, d)
    b, c, t = (x.abs() == x.abs().max()).nonzero()[0].tolist()
    a, xt = int(addr[b, t]), float(x[b, c, t])
    assert xt != 0.0
    for prefill in (None, d.prefill):
        got = oracle(d, prefill)
        O.check_scatter(got, d.st, prefill)
        bad = got.double()
        if corruption == "drop":
            bad[b, c, a] -= xt
        elif corruption == "double":
            bad[b, c, a] += xt
        else:
            bad[b, c, a] -= xt
            bad[b, c, a + 1 if a + 1 < n else a - 1] += xt
        with pytest.raises(O.Mismatch):
            O.check_scatter(bad.float(), d.st, prefill)


@pytest.mark.parametrize("op,name", GRAD_PARAMS)
def test_checker_rejects_a_wrong_prefill(op, name):
    """An accumulate that leaves the prefill out, a set that keeps it in."""
    _, data, oracle = GRAD_OPS[op]
    d = data(name)
    with pytest.raises(O.Mismatch):
        O.check_scatter(oracle(d, None), d.st, d.prefill)
    with pytest.raises(O.Mismatch):
        O.check_scatter(oracle(d, d.prefill), d.st)


def test_checker_rejects_stale_and_nan():
    """K = 0 addresses are exact (-0.0 is not +0.0; a NaN left from the prefill is not a zero) and a NaN where a sum belongs fails."""
    d = O.group_grad_data("global_c4_n16385")
    got = _oracle_group_grad(d, None)
    free = (d.st.k[0, 0] == 0).nonzero()[0].item()
    used = (d.st.k[0, 0] > 0).nonzero()[0].item()
    for where, value in ((free, -0.0), (free, float("nan")), (used, float("nan"))):
        bad = got.clone()
        bad[0, 0, where] = value
        with pytest.raises(O.Mismatch):
            O.check_scatter(bad, d.st)


# ------------------------------------------------------------------------------------------------
# forwards
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", O.names(O.INTERPOLATE_CASES))
def test_oracle_interpolate_satisfies_the_bound(name):
    d = O.interpolate_data(name)
    out = P.three_interpolate(d.points, d.idx, d.w)
    assert O.check_interpolate(out, d.points, d.idx, d.w, out) <= 1.0
    bad = out.clone()
    bad.view(-1)[-1] = d.points.view(-1)[0] + 7.0           # a value from elsewhere
    with pytest.raises(O.Mismatch):
        O.check_interpolate(bad, d.points, d.idx, d.w)
    flipped = (O.bits(out) ^ 1).view(torch.float32)          # one ulp everywhere: inside the float64 bound or not, never the oracle's bits
    with pytest.raises(O.Mismatch):
        O.check_interpolate(flipped, d.points, d.idx, d.w, out)


@pytest.mark.parametrize("name", O.names(O.GATHER_CASES))
def test_oracle_gather_is_a_copy(name):
    d = O.gather_data(name)
    out = P.gather(d.points, d.idx)
    O.check_copy(out, d.points, d.idx)
    with pytest.raises(O.Mismatch):
        O.check_copy((O.bits(out) ^ 1).view(torch.float32), d.points, d.idx)


@pytest.mark.parametrize("name", O.names(O.GROUP_CASES))
def test_oracle_group_is_a_copy(name):
    d = O.group_data(name)
    out = P.group(d.points, d.idx)
    O.check_copy(out, d.points, d.idx)
    with pytest.raises(O.Mismatch):
        O.check_copy((O.bits(out) ^ 1).view(torch.float32), d.points, d.idx)


# ------------------------------------------------------------------------------------------------
# dispatch mirror and case table
# ------------------------------------------------------------------------------------------------
GROUP_GRAD_EXPECTED = {
    "cpb4_vec4_ball": ("lds", 4, "vec4"), "cpb4_vec4_round2": ("lds", 4, "vec4"), "cpb4_scalar": ("lds", 4, "scalar"),
    "cpb1_c37_vec4": ("lds", 1, "vec4"), "cpb1_c37_scalar": ("lds", 1, "scalar"),
    "cpb1_c1_vec4": ("lds", 1, "vec4"), "cpb1_c1_scalar": ("lds", 1, "scalar"),
    "cpb4_n4096": ("lds", 4, "vec4"), "cpb1_n4097": ("lds", 1, "vec4"), "cpb1_n16384": ("lds", 1, "vec4"),
    "global_c1_n16385": ("global",), "global_c4_n16385": ("global",),
    "collide_vec4": ("lds", 4, "vec4"), "collide_scalar": ("lds", 1, "scalar"),
    "n1_vec4": ("lds", 4, "vec4"), "n1_scalar": ("lds", 1, "scalar"),
}
INTERPOLATE_GRAD_EXPECTED = {
    "c37_tail5": ("lds", 5), "c3_n257": ("lds", 3), "c8_n256": ("lds", 8), "c1_n1": ("lds", 1), "c2_m1": ("lds", 2),
    "c4_coincide": ("lds", 4), "c6_zero_weights": ("lds", 6), "c7_same_three": ("lds", 7), "c9_m2048": ("lds", 1),
    "c9_m2049": ("global",), "c3_m2049": ("global",),
}
INTERPOLATE_EXPECTED = {"cpb8_at_4096": 8, "cpb8_c37": 8, "cpb1_at_4095": 1, "cpb1_m1": 1, "cpb1_n1": 1}


def test_case_table_reaches_every_instance():
    got = {k.name: O.group_grad_instance(k.c, k.n, k.npoint, k.nsample) for k in O.GROUP_GRAD_CASES}
    assert got == GROUP_GRAD_EXPECTED
    assert set(got.values()) == O.GROUP_GRAD_INSTANCES
    got = {k.name: O.interpolate_grad_instance(k.c, k.n, k.m) for k in O.INTERPOLATE_GRAD_CASES}
    assert got == INTERPOLATE_GRAD_EXPECTED
    assert set(got.values()) == O.INTERPOLATE_GRAD_INSTANCES
    got = {k.name: O.interpolate_instance(k.b, k.c, k.n) for k in O.INTERPOLATE_CASES}
    assert got == INTERPOLATE_EXPECTED
    assert set(got.values()) == O.INTERPOLATE_INSTANCES
    assert O.MODES == ("set", "accumulate")          # crossed with every gradient case by the GPU tests' parametrisation


def test_mirror_boundaries():
    assert O.group_grad_instance(4, 4096, 16, 4)[1] == 4 and O.group_grad_instance(4, 4097, 16, 4)[1] == 1
    assert O.group_grad_instance(1, 16384, 16, 4)[0] == "lds" and O.group_grad_instance(1, 16385, 16, 4) == ("global",)
    assert O.interpolate_grad_instance(9, 300, 2048)[0] == "lds" and O.interpolate_grad_instance(9, 300, 2049) == ("global",)
    assert O.interpolate_instance(2, 4, 512 * 256) == 8 and O.interpolate_instance(2, 4, 511 * 256) == 1
    k = next(k for k in O.INTERPOLATE_CASES if k.name == "cpb8_at_4096")
    assert k.b * k.c * ((k.n + 255) // 256) == 4096 and k.n % 256 != 0 and k.c % 8 != 0
    k = next(k for k in O.INTERPOLATE_CASES if k.name == "cpb1_at_4095")
    assert k.b * k.c * ((k.n + 255) // 256) == 4095 and k.n % 256 != 0


def test_source_constants_still_stand():
    """The conditions the mirror quotes, as plain text of the source: a change of the dispatch fails here until the table is revisited."""
    with open(O.OPS_SOURCE) as f:
        src = f.read()
    for text in O.SOURCE_CONSTANTS:
        assert text in src, text
    for text in ("TIG_CPB = 8", "64 * 1024", ">= 4096", "c % 4 == 0", "(sn & 3) == 0"):
        assert text in src, text


def _float4_runs(flat):
    """(run lengths of equal neighbours that occur inside a float4, whether an equal pair straddles two float4s)."""
    q = flat.reshape(-1, 4)
    lengths = set()
    for row in q.tolist():
        run = 1
        for e in range(1, 4):
            if row[e] == row[e - 1]:
                run += 1
            else:
                lengths.add(run)
                run = 1
        lengths.add(run)
    return lengths, bool((q[:-1, 3] == q[1:, 0]).any())


def test_index_patterns_are_what_the_cases_claim():
    for name in ("cpb4_vec4_ball", "cpb1_c37_vec4", "cpb1_c1_vec4"):
        d = O.group_grad_data(name)
        for s in range(d.case.b):
            lengths, straddles = _float4_runs(d.idx[s].reshape(-1))
            assert {1, 2, 3, 4} <= lengths and straddles
        assert (d.idx[:, :, -1] == d.idx[:, :, 0]).any() and (d.idx[:, :, -1] != d.idx[:, :, 0]).any()      # padded and full rows
    d = O.group_grad_data("cpb4_vec4_round2")
    n4 = d.case.npoint * d.case.nsample // 4
    assert 1024 < n4 < 2048 and (n4 - 1024) % 256 != 0 and (n4 - 1024) > 256        # second round: a full and a partial chunk
    flat = d.idx.reshape(d.case.b, -1)
    same = (flat[:, 1:] == flat[:, :-1]).float().mean().item()
    assert 0.45 < same < 0.56
    assert {1, 2, 3, 4} <= _float4_runs(flat[0])[0]
    for name in ("cpb4_n4096", "cpb1_n4097", "cpb1_n16384", "global_c1_n16385", "global_c4_n16385"):
        d = O.group_grad_data(name)
        assert int(d.idx.min()) == 0 and int(d.idx.max()) == d.case.n - 1
        assert (d.st.k == 0).any()                                                # unreferenced addresses: the memset is observable
    d = O.group_grad_data("collide_vec4")
    assert d.st.k[0, 0, -1] == d.case.npoint * d.case.nsample and (d.st.k[..., :-1] == 0).all()
    d = O.interpolate_grad_data("c4_coincide")
    same = (d.idx[..., 0] == d.idx[..., 1]) & (d.idx[..., 1] == d.idx[..., 2])
    assert same.float().mean() >= 1 / 3
    d = O.interpolate_grad_data("c6_zero_weights")
    assert (d.w == 0).any() and (d.w[:, 0] == 0).all()
    d = O.interpolate_grad_data("c7_same_three")
    assert (d.st.k > 0).sum() == 3 * d.case.b
    for name in ("c9_m2049", "c3_m2049"):
        assert (O.interpolate_grad_data(name).st.k == 0).any()


def test_gamma():
    assert O.gamma(1) == pytest.approx(2.0 ** -24, rel=1e-6)
    assert O.gamma(514) > 514 * O.U and float(O.gamma(torch.tensor(3.0, dtype=torch.float64))) == O.gamma(3.0)
