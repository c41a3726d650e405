"""Float64 statements, derived bounds, dispatch mirror and case table of the gather / group / interpolate family
(ratrack_amd/csrc/ops_pointnet2.hip), shared by tests/test_ops_f64_cpu.py and tests/test_ops_f64_gpu.py.

Forwards: gather_points and group_points are copies (bit-equal to torch indexing); three_interpolate is
fma(w2,p2, fma(w1,p1, w0*p0)) in fp32 -- bit-equal to the oracle, and within gamma_3 * sum|w_i p_i| of the float64 sum.

Gradients: a scatter_add_ of the float64 contributions (g for gather / group, g*w for interpolate).  The kernels add in a free order
(LDS or global float atomics, equal neighbours merged in registers), so no bits are compared; the bound is the standard one for fp32
summation in ANY order: an address that receives K contributions x_i onto a prefill p satisfies
    |got - ref64| <= gamma_{K+2} * (|p| + sum|x_i|),     gamma_k = k u / (1 - k u),  u = 2^-24
(K - 1 additions among the contributions, one rounding of g*w, one addition onto the prefill; K + 2 leaves one to spare).  Addresses
with K = 0 are exact: +0.0 after a `_set` entry point (over a NaN prefill), the prefill's own bits after an accumulating one.
Nothing here is measured on the code under test.
"""
import functools
import os
import zlib
from collections import namedtuple

import torch

U = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS_SOURCE = os.path.join(ROOT, "ratrack_amd", "csrc", "ops_pointnet2.hip")


def gamma(k):
    """k u / (1 - k u) for a number or a float64 tensor of counts."""
    return k * U / (1.0 - k * U)


class Mismatch(AssertionError):
    """A result outside its derived bound (or a wrong bit at an exact address)."""


# ------------------------------------------------------------------------------------------------
# float64 statements
# ------------------------------------------------------------------------------------------------
Statement = namedtuple("Statement", "sum sabs k")      # (B,C,n) float64 sum, (B,C,n) float64 sum of magnitudes, (B,1,n) float64 counts


def scatter_f64(x, addr, n):
    """x (B,C,T) float64 contributions, addr (B,T) integer addresses in [0, n) -> Statement."""
    B, C, T = x.shape
    addr = addr.long()
    assert addr.shape == (B, T) and int(addr.min()) >= 0 and int(addr.max()) < n
    a = addr[:, None, :].expand(B, C, T)
    s = torch.zeros(B, C, n, dtype=torch.float64).scatter_add_(2, a, x)
    sa = torch.zeros(B, C, n, dtype=torch.float64).scatter_add_(2, a, x.abs())
    k = torch.zeros(B, n, dtype=torch.float64).scatter_add_(1, addr, torch.ones(B, T, dtype=torch.float64))
    return Statement(s, sa, k[:, None, :])


def scatter_grad_f64(go, idx, n):
    """gather_points_grad / group_points_grad: go (B,C,...) fp32, idx (B,...) -> Statement over (B,C,n)."""
    B, C = go.shape[:2]
    return scatter_f64(go.double().reshape(B, C, -1), idx.reshape(B, -1), n)


def interpolate_contributions(go, idx, w):
    """go (B,C,n), idx (B,n,3), w (B,n,3) -> ((B,C,3n) float64 g*w, (B,3n) addresses)."""
    B, C, n = go.shape
    x = go.double()[:, :, :, None] * w.double()[:, None, :, :]
    return x.reshape(B, C, 3 * n), idx.reshape(B, 3 * n)


def interpolate_grad_f64(go, idx, w, m):
    return scatter_f64(*interpolate_contributions(go, idx, w), m)


def interpolate_f64(points, idx, w):
    """points (B,C,m), idx (B,n,3), w (B,n,3) -> ((B,C,n) float64 sum, (B,C,n) float64 sum|w_i p_i|)."""
    B, C, m = points.shape
    n = idx.shape[1]
    a = idx.long().reshape(B, 1, 3 * n).expand(B, C, 3 * n)
    t = torch.gather(points.double(), 2, a).reshape(B, C, n, 3) * w.double()[:, None]
    return t.sum(-1), t.abs().sum(-1)


def index_copy_ref(points, idx):
    """gather_points / group_points as torch indexing: points (B,C,n), idx (B,...) -> (B,C,...)."""
    B, C, _ = points.shape
    a = idx.long().reshape(B, 1, -1).expand(B, C, -1)
    return torch.gather(points, 2, a).reshape(B, C, *idx.shape[1:])


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------
# checkers
# ------------------------------------------------------------------------------------------------
def check_scatter(got, st, prefill=None):
    """got (B,C,n) fp32 against Statement st.  prefill None: the result of a `_set` entry point (K = 0 addresses hold +0.0);
    else the fp32 buffer an accumulating entry point started from (K = 0 addresses keep its bits).
    Raises Mismatch; returns the largest error / bound over the addresses with K > 0 (information only)."""
    if got.dtype != torch.float32 or got.shape != st.sum.shape:
        raise Mismatch("result is %s %s, expected float32 %s" % (got.dtype, tuple(got.shape), tuple(st.sum.shape)))
    hit = (st.k > 0).expand_as(st.sum)
    if prefill is None:
        p = torch.zeros_like(st.sum)
        want_bits = torch.zeros_like(bits(got))
    else:
        p = prefill.double()
        want_bits = bits(prefill)
    stale = ~hit & (bits(got) != want_bits)
    if stale.any():
        where = tuple(stale.nonzero()[0].tolist())
        raise Mismatch("address %s receives nothing and holds %r: expected %s (%d such addresses)"
                       % (where, got[where].item(), "+0.0" if prefill is None else "the prefill's bits", int(stale.sum())))
    ref = p + st.sum
    bound = gamma(st.k + 2.0) * (p.abs() + st.sabs)
    err = (got.double() - ref).abs()
    bad = hit & ~(err <= bound)            # ~(<=): a NaN is a failure
    if bad.any():
        where = tuple(bad.nonzero()[0].tolist())
        raise Mismatch("address %s: got %r, float64 %r, error %.3e > bound %.3e (K = %d; %d such addresses)"
                       % (where, got[where].item(), ref[where].item(), err[where].item(), bound[where].item(),
                          int(st.k.expand_as(st.sum)[where]), int(bad.sum())))
    live = hit & (bound > 0)
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


def check_interpolate(got, points, idx, w, oracle_out=None):
    """three_interpolate forward: within gamma_3 * sum|w_i p_i| of float64, and bit-equal to the oracle where one is given."""
    ref, mag = interpolate_f64(points, idx, w)
    if got.dtype != torch.float32 or got.shape != ref.shape:
        raise Mismatch("result is %s %s, expected float32 %s" % (got.dtype, tuple(got.shape), tuple(ref.shape)))
    err = (got.double() - ref).abs()
    bound = gamma(3.0) * mag
    bad = ~(err <= bound)
    if bad.any():
        where = tuple(bad.nonzero()[0].tolist())
        raise Mismatch("output %s: got %r, float64 %r, error %.3e > bound %.3e" % (where, got[where].item(), ref[where].item(),
                                                                                   err[where].item(), bound[where].item()))
    if oracle_out is not None and not torch.equal(bits(got), bits(oracle_out)):
        where = tuple((bits(got) != bits(oracle_out)).nonzero()[0].tolist())
        raise Mismatch("output %s: got %r, oracle %r: not the same bits" % (where, got[where].item(), oracle_out[where].item()))
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


def check_copy(got, points, idx):
    ref = index_copy_ref(points, idx)
    if got.dtype != ref.dtype or got.shape != ref.shape or not torch.equal(bits(got), bits(ref)):
        raise Mismatch("not the bits of points[b, c, idx[b, ...]]")


# ------------------------------------------------------------------------------------------------
# dispatch mirror: the instance a shape selects, with the host conditions it restates (ops_pointnet2.hip)
# ------------------------------------------------------------------------------------------------
SOURCE_CONSTANTS = (
    "constexpr int TIG_CPB = 8;",
    "if ((size_t)n * sizeof(float) <= 64 * 1024) {",
    "const bool four = (c % 4 == 0) && (size_t)n * 4 * sizeof(float) <= 64 * 1024;",
    "if ((sn & 3) == 0) {",
    "if ((size_t)TIG_CPB * m * sizeof(float) <= 64 * 1024) {",
    "if ((long)b * c * rtk_divup(n, 256) >= 4096)",
    "const int nc = min(TIG_CPB, c - c0);",
)
TIG_CPB = 8


def group_grad_instance(c, n, npoint, nsample):
    """group_points_grad_impl -> ("lds", CPB, "vec4" | "scalar") or ("global",)."""
    sn = npoint * nsample
    if n * 4 <= 64 * 1024:                                   # if ((size_t)n * sizeof(float) <= 64 * 1024)
        four = c % 4 == 0 and n * 4 * 4 <= 64 * 1024         # four = (c % 4 == 0) && (size_t)n * 4 * sizeof(float) <= 64 * 1024
        return ("lds", 4 if four else 1, "vec4" if (sn & 3) == 0 else "scalar")      # kernel: if ((sn & 3) == 0)
    return ("global",)                                       # else: memset (set) + group_points_grad_kernel


GROUP_GRAD_INSTANCES = {("lds", cpb, path) for cpb in (1, 4) for path in ("vec4", "scalar")} | {("global",)}


def interpolate_grad_instance(c, n, m):
    """three_interpolate_grad_impl -> ("lds", nc_tail) or ("global",); nc_tail = the channels of the last workgroup, 1..TIG_CPB."""
    if TIG_CPB * m * 4 <= 64 * 1024:                         # if ((size_t)TIG_CPB * m * sizeof(float) <= 64 * 1024)
        return ("lds", c - TIG_CPB * ((c - 1) // TIG_CPB))   # grid rtk_divup(c, TIG_CPB); nc = min(TIG_CPB, c - c0)
    return ("global",)                                       # else: memset (set) + three_interpolate_grad_kernel


INTERPOLATE_GRAD_INSTANCES = {("lds", t) for t in range(1, TIG_CPB + 1)} | {("global",)}


def interpolate_instance(b, c, n):
    """rtk_three_interpolate -> TI_CPB."""
    return 8 if b * c * ((n + 255) // 256) >= 4096 else 1    # if ((long)b * c * rtk_divup(n, 256) >= 4096) <8> else <1>


INTERPOLATE_INSTANCES = {1, 8}
MODES = ("set", "accumulate")      # every gradient case runs through both entry points


# ------------------------------------------------------------------------------------------------
# case table
# ------------------------------------------------------------------------------------------------
GroupCase = namedtuple("GroupCase", "name b c n npoint nsample kind")
GROUP_GRAD_CASES = [
    # CPB=4, float4 path, n4 = 128 < 256 float4s; ball-query-like neighbourhoods (runs of 2, 3, 4 inside and across float4s)
    GroupCase("cpb4_vec4_ball", 2, 8, 300, 64, 8, "ball"),
    # CPB=4, float4 path, n4 = 1300: a second round of the four-chunk loop whose second chunk is partial
    GroupCase("cpb4_vec4_round2", 2, 4, 64, 650, 8, "sticky"),
    GroupCase("cpb4_scalar", 2, 4, 50, 77, 3, "random"),
    GroupCase("cpb1_c37_vec4", 2, 37, 300, 64, 8, "ball"),
    GroupCase("cpb1_c37_scalar", 2, 37, 50, 77, 3, "random"),
    GroupCase("cpb1_c1_vec4", 2, 1, 300, 64, 8, "ball"),
    GroupCase("cpb1_c1_scalar", 2, 1, 50, 77, 3, "random"),
    GroupCase("cpb4_n4096", 1, 4, 4096, 16, 4, "ends"),          # CPB=4 at exactly 64 KiB of LDS
    GroupCase("cpb1_n4097", 1, 4, 4097, 16, 4, "ends"),          # CPB=1 from the size
    GroupCase("cpb1_n16384", 1, 1, 16384, 16, 4, "ends"),        # the 64 KiB end of CPB=1
    GroupCase("global_c1_n16385", 1, 1, 16385, 16, 4, "ends"),   # the fallback (memset under _set)
    GroupCase("global_c4_n16385", 1, 4, 16385, 16, 4, "ends"),
    GroupCase("collide_vec4", 2, 4, 50, 64, 8, "last"),          # K = 512 on address n-1, exact zeros elsewhere
    GroupCase("collide_scalar", 2, 1, 50, 77, 3, "last"),
    GroupCase("n1_vec4", 2, 4, 1, 4, 4, "random"),
    GroupCase("n1_scalar", 2, 1, 1, 5, 3, "random"),
]

GatherCase = namedtuple("GatherCase", "name b c n npoint kind")
GATHER_CASES = [
    GatherCase("np1", 2, 3, 40, 1, "random"),
    GatherCase("np255", 2, 3, 40, 255, "random"),
    GatherCase("np256", 2, 3, 40, 256, "random"),
    GatherCase("np257", 2, 3, 300, 257, "random"),
    GatherCase("all_equal", 2, 3, 40, 257, "last"),
    GatherCase("n1", 2, 3, 1, 5, "random"),
]
GROUP_CASES = [      # forward: npoint * nsample at 1, 255, 256, 257
    GroupCase("sn1", 2, 3, 40, 1, 1, "random"),
    GroupCase("sn255", 2, 3, 40, 85, 3, "random"),
    GroupCase("sn256", 2, 3, 40, 64, 4, "ball"),
    GroupCase("sn257", 2, 3, 300, 257, 1, "random"),
    GroupCase("all_equal", 2, 3, 40, 85, 3, "last"),
    GroupCase("n1", 2, 3, 1, 5, 3, "random"),
]

InterpCase = namedtuple("InterpCase", "name b c n m kind")      # n unknown points interpolate from m known ones
INTERPOLATE_GRAD_CASES = [
    InterpCase("c37_tail5", 2, 37, 300, 100, "random"),
    InterpCase("c3_n257", 2, 3, 257, 300, "random"),
    InterpCase("c8_n256", 2, 8, 256, 300, "random"),
    InterpCase("c1_n1", 2, 1, 1, 5, "random"),
    InterpCase("c2_m1", 2, 2, 40, 1, "random"),
    InterpCase("c4_coincide", 2, 4, 300, 300, "coincide"),      # a third of the points with i0 == i1 == i2
    InterpCase("c6_zero_weights", 2, 6, 300, 300, "zero_weights"),
    InterpCase("c7_same_three", 2, 7, 300, 300, "same_three"),  # every point refers to the same three known points
    InterpCase("c9_m2048", 1, 9, 300, 2048, "ends"),            # exactly 64 KiB of LDS
    InterpCase("c9_m2049", 1, 9, 300, 2049, "ends"),            # the fallback (memset under _set)
    InterpCase("c3_m2049", 2, 3, 257, 2049, "coincide"),
]
INTERPOLATE_CASES = [      # forward; b * c * ceil(n / 256) on both sides of 4096
    InterpCase("cpb8_at_4096", 2, 4, 512 * 256 - 100, 50, "random"),      # 2 * 4 * 512 = 4096: <8> with 4 of 8 channels live
    InterpCase("cpb8_c37", 4, 37, 7000, 50, "coincide"),                  # 4 * 37 * 28 = 4144: <8>, tail of 5
    InterpCase("cpb1_at_4095", 1, 15, 273 * 256 - 3, 50, "zero_weights"),  # 15 * 273 = 4095: <1>
    InterpCase("cpb1_m1", 2, 5, 300, 1, "random"),
    InterpCase("cpb1_n1", 2, 3, 1, 7, "random"),
]


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _indices(gen, kind, b, n, npoint, nsample):
    """int32 (b, npoint, nsample) neighbour indices in [0, n)."""
    sn = npoint * nsample
    if kind == "random":
        idx = torch.randint(0, n, (b, sn), generator=gen)
    elif kind == "ends":           # random, with indices 0 and n-1 present
        idx = torch.randint(0, n, (b, sn), generator=gen)
        idx[:, 0], idx[:, sn // 2], idx[:, -1] = 0, n - 1, n - 1
        idx[:, 1] = 0
    elif kind == "last":
        idx = torch.full((b, sn), n - 1)
    elif kind == "sticky":         # each index equals its predecessor with probability 1/2
        fresh = torch.randint(0, n, (b, sn), generator=gen)
        keep = torch.rand(b, sn, generator=gen) < 0.5
        keep[:, 0] = False
        src = torch.where(keep, torch.zeros(b, sn, dtype=torch.long), torch.arange(sn).expand(b, sn)).cummax(1).values
        idx = torch.gather(fresh, 1, src)
    elif kind == "ball":           # a prefix of L distinct hits in index order, padded with copies of the first; L cycles 1..nsample
        idx = torch.empty(b, npoint, nsample, dtype=torch.long)
        for s in range(b):
            for p in range(npoint):
                L = min(1 + (p + s) % nsample, n)
                hits = torch.randperm(n, generator=gen)[:L].sort().values
                idx[s, p] = hits[0]
                idx[s, p, :L] = hits
    else:
        raise ValueError(kind)
    return idx.reshape(b, npoint, nsample).to(torch.int32).contiguous()


ScatterData = namedtuple("ScatterData", "case idx go prefill st")


@functools.lru_cache(maxsize=None)
def group_grad_data(name):
    """Inputs and statement of a GROUP_GRAD_CASES entry (shared: do not write to them)."""
    case = next(k for k in GROUP_GRAD_CASES if k.name == name)
    gen = _gen("group_grad", name)
    idx = _indices(gen, case.kind, case.b, case.n, case.npoint, case.nsample)
    go = torch.randn(case.b, case.c, case.npoint, case.nsample, generator=gen)
    prefill = torch.randn(case.b, case.c, case.n, generator=gen)
    return ScatterData(case, idx, go, prefill, scatter_grad_f64(go, idx, case.n))


ForwardData = namedtuple("ForwardData", "case idx points go prefill st")


def _special_values(points):
    """A copy moves bits: -0.0, an infinity and a NaN among the features (where there is room)."""
    flat = points.view(-1)
    for k, v in enumerate((-0.0, float("inf"), float("nan"))):
        if flat.numel() > 3 * k + 1:
            flat[3 * k + 1] = v
    return points


@functools.lru_cache(maxsize=None)
def gather_data(name):
    case = next(k for k in GATHER_CASES if k.name == name)
    gen = _gen("gather", name)
    idx = _indices(gen, case.kind, case.b, case.n, case.npoint, 1).reshape(case.b, case.npoint)
    points = _special_values(torch.randn(case.b, case.c, case.n, generator=gen))
    go = torch.randn(case.b, case.c, case.npoint, generator=gen)
    prefill = torch.randn(case.b, case.c, case.n, generator=gen)
    return ForwardData(case, idx, points, go, prefill, scatter_grad_f64(go, idx, case.n))


@functools.lru_cache(maxsize=None)
def group_data(name):
    case = next(k for k in GROUP_CASES if k.name == name)
    gen = _gen("group", name)
    idx = _indices(gen, case.kind, case.b, case.n, case.npoint, case.nsample)
    points = _special_values(torch.randn(case.b, case.c, case.n, generator=gen))
    return ForwardData(case, idx, points, None, None, None)


def _interp_inputs(gen, case):
    b, n, m = case.b, case.n, case.m
    idx = torch.randint(0, m, (b, n, 3), generator=gen)
    w = torch.rand(b, n, 3, generator=gen)
    if case.kind == "coincide":
        idx[:, ::3, 1] = idx[:, ::3, 0]
        idx[:, ::3, 2] = idx[:, ::3, 0]
    elif case.kind == "zero_weights":
        w[torch.rand(b, n, 3, generator=gen) < 0.25] = 0.0
        w[:, 0] = 0.0                                        # a point with no weight at all
    elif case.kind == "same_three":
        idx[:] = torch.tensor([m - 1, 0, m // 2])
    elif case.kind == "ends":
        idx[:, 0], idx[:, -1] = torch.tensor([0, m - 1, 0]), torch.tensor([m - 1, m - 1, 0])
    elif case.kind != "random":
        raise ValueError(case.kind)
    return idx.to(torch.int32).contiguous(), w.contiguous()


InterpData = namedtuple("InterpData", "case idx w go prefill st points")


@functools.lru_cache(maxsize=None)
def interpolate_grad_data(name):
    case = next(k for k in INTERPOLATE_GRAD_CASES if k.name == name)
    gen = _gen("interpolate_grad", name)
    idx, w = _interp_inputs(gen, case)
    go = torch.randn(case.b, case.c, case.n, generator=gen)
    prefill = torch.randn(case.b, case.c, case.m, generator=gen)
    return InterpData(case, idx, w, go, prefill, interpolate_grad_f64(go, idx, w, case.m), None)


@functools.lru_cache(maxsize=None)
def interpolate_data(name):
    case = next(k for k in INTERPOLATE_CASES if k.name == name)
    gen = _gen("interpolate", name)
    idx, w = _interp_inputs(gen, case)
    points = torch.randn(case.b, case.c, case.m, generator=gen)
    return InterpData(case, idx, w, None, None, None, points)


def names(cases):
    return [k.name for k in cases]
