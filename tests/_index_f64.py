"""Float64 statements, ambiguity bands, dispatch mirror and case table of the index-table family of ratrack_amd/csrc/ops_pointnet2.hip --
ball query, three-NN, kNN, kNN-point, their masked / paired forms and the two product launches -- shared by
tests/test_index_f64_cpu.py and tests/test_index_f64_gpu.py.

Statements.  Distances are formed in float64 from the fp32 coordinates; `radius2` is the fp32 product float32(radius) * float32(radius),
as the host code forms it.
  knn_point   the k smallest of max(-2 q.p + |q|^2 + |p|^2, 0) by (distance, index);
  knn         the same under sum (q - p)^2, (+inf, 0) in slots without a candidate;
  three_nn    knn with k = 3;
  ball_query  the first `nsample` indices with d2 < radius2 in index order, the remaining slots the first hit, the row as the caller
              left it when the ball is empty (rtk_ball_query) or zeros (rtk_ball_query_pair).
On integer lattices (small integer coordinates, radii whose fp32 square is an integer) every distance is exact in fp32 and in float64,
under either formula, so the statements are exact references there: results are compared with torch.equal.

Ambiguity band (clouds that are not lattices).  u = 2^-24, gamma_k = k u / (1 - k u).
  Direct form, rtk_sqdist = fma(dz,dz, fma(dy,dy, dx*dx)): the x term passes five roundings (the subtraction twice, the product, two
  fmas), the others fewer, so fp32(d) = d (1 + t), |t| <= gamma_5.  A chosen candidate x that is not among the k nearest in float64
  displaced some y with d_y <= c (c = the k-th smallest float64 distance): fp32(x) <= fp32(y), hence d_x <= c (1 + gamma_5) /
  (1 - gamma_5) < c (1 + 12 u); an unchosen x was displaced by some chosen y with d_y >= c, hence d_x > c (1 - 12 u).
      beta_direct = 12 u c;          for the ball predicate fp32(d) < radius2:  beta_ball = 6 u radius2.
  Expansion form, fl(fl(-2 dot + qn) + pn) with dot = fma(qz,pz, fma(qy,py, qx*px)), pn = fl(fl(px^2 + py^2) + pz^2), A = sum |q_i p_i|:
  |dot error| <= 3 u A (doubled by the factor -2), |pn error| <= 3 u |p|^2, the first addition rounds a number of magnitude
  <= 2 A + |q|^2, the second one of magnitude ~ d; the error of qn is the same number for every candidate of a query and cancels in a
  comparison; the clamp at 0 moves a value towards the true one (d >= 0) and keeps the order.  To first order
      E(q, p) = u (8 A + |q|^2 + 3 |p|^2 + d)          (times 1.001 for the second-order terms)
  and two candidates can only be exchanged when their float64 distances differ by at most E_x + E_y:
      beta_expand(q) = 2 max_p E(q, p),
  a dozen units of u (|q|^2 + |p|^2) on a cluster far from the origin, 1e-9 relative on a cloud around it.
Rules: a chosen candidate lies no further out than the cut-off plus beta; a candidate nearer than the cut-off minus beta is chosen; the
order of the result ascends up to beta; inside the band only the oracle, bit for bit, decides.  Nothing here is measured on the code
under test.

Masked contracts (include/rtk_fused.h).
  rtk_knn_point_masked   candidates are rows [0, n_valid[b]) (all n rows when n_valid[b] >= n); with n_valid[b] < k the candidates are
                         rows [0, k): the caller's padding rows n_valid[b] .. k-1 take part with the coordinates they hold.
  rtk_three_nn_masked    rows < unknown_nuniq[b] hold the full scan over all m known rows (known rows >= known_nuniq[b] being copies of
                         known row 0); rows at or past roundup(unknown_nuniq[b], 64) are untouched; the rows between hold valid indices.
  rtk_ball_query_pair    rows < nuniq[b] hold both tables; rows [nuniq[b], roundup(nuniq[b], RTK_BALL_TAIL_ROWS)) read as zeros; rows
                         beyond keep the caller's bits.
"""
import functools
import math
import os
import re
import zlib
from collections import namedtuple

import torch

U = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS_SOURCE = os.path.join(ROOT, "ratrack_amd", "csrc", "ops_pointnet2.hip")
COMMON_SOURCE = os.path.join(ROOT, "ratrack_amd", "csrc", "rtk_common.h")


class Mismatch(AssertionError):
    """A table that is not the statement's, or outside the band."""


def roundup(x, q):
    return (x + q - 1) // q * q


def divup(x, q):
    return (x + q - 1) // q


# ------------------------------------------------------------------------------------------------
# dispatch mirror: constants read from the sources, host conditions restated
# ------------------------------------------------------------------------------------------------
SOURCE_TEXTS = (      # the conditions the mirror restates, as plain text of ops_pointnet2.hip
    "constexpr int KV_QPW = 256 / KV_LPQ;",
    "for (int base = 0; base < n; base += KV_LPQ * K) {",
    "const size_t lds = (size_t)n * 4 * sizeof(float);",
    "const bool use_lds = lds <= 64 * 1024;",
    "if (k > 32) {",
    "} else if (k <= 16) {",
    "const size_t lds = (size_t)n * 3 * sizeof(float);",
    "const size_t lds = (size_t)m * 3 * sizeof(float);",
    "if (lds <= 64 * 1024)",
    "RTK_REQUIRE(b <= 65535 && (size_t)n * 12 <= 64 * 1024, \"ball_query_pair: b or n too large (n=%d)\", n);",
    "const int want = rtk_divup(GEO_TABLES_WGS, 9 * samples);",
    "const int ball_chunks = rtk_divup(npoint, BQ_WAVES * BQ_CENTROIDS_PER_WAVE);",
    "P.ball_wgs = want < ball_chunks ? want : ball_chunks;",
    "T.wgs = want < rtk_divup(T.n, KV_QPW) ? want : rtk_divup(T.n, KV_QPW);",
    "n = nv < n ? (nv < k ? k : nv) : n;",
    "const int z1 = min(m, (climit + RTK_BALL_TAIL_ROWS - 1) & ~(RTK_BALL_TAIL_ROWS - 1));",
    "if (li >= 1 && li <= 2 && ke + li - 1 < m_full) {",
    "RTK_REQUIRE(n <= 2048 && npoint <= 512,",
)
LDS_BYTES = 64 * 1024


def _read(path):
    with open(path) as f:
        return f.read()


def _one(pattern, src, what):
    found = re.findall(pattern, src, re.M)
    if len(found) != 1:
        raise Mismatch("%s: %d matches of %r in the source" % (what, len(found), pattern))
    return found[0]


Constants = namedtuple("Constants", "KV_LPQ KV_QPW BQ_WAVES BQ_CENTROIDS_PER_WAVE GEO_TABLES_WGS RTK_BALL_TAIL_ROWS RTK_INTERP_ROW_GROUP "
                                    "FPS_PPL FRONT_PPL")


@functools.lru_cache(maxsize=None)
def constants():
    ops, common = _read(OPS_SOURCE), _read(COMMON_SOURCE)
    define = lambda name: int(_one(r"^#define %s\s+(\d+)" % name, ops, name))
    constexpr = lambda name: int(_one(r"^constexpr int %s = (\d+);" % name, common, name))
    # fps_launch: `n <= 64 * P` selects fps_wave_kernel<P>; rtk_geometry_front: geometry_front_kernel<P, 8>, the last one by `else`
    fps = [(int(a), int(b)) for a, b in re.findall(r"if \(n <= 64 \* (\d+)\) fps_wave_kernel<(\d+)>", ops)]
    front = [(int(a), int(b)) for a, b in re.findall(r"if \(n <= 64 \* (\d+)\) geometry_front_kernel<(\d+), 8>", ops)]
    front.append((None, int(_one(r"^\s+else geometry_front_kernel<(\d+), 8>", ops, "geometry_front else"))))
    lpq = define("KV_LPQ")
    return Constants(lpq, 256 // lpq, define("BQ_WAVES"), define("BQ_CENTROIDS_PER_WAVE"), define("GEO_TABLES_WGS"),
                     constexpr("RTK_BALL_TAIL_ROWS"), constexpr("RTK_INTERP_ROW_GROUP"), tuple(fps), tuple(front))


C = constants()
BALL_CHUNK = C.BQ_WAVES * C.BQ_CENTROIDS_PER_WAVE      # centroids per ball chunk
KNN_LDS_MAX = LDS_BYTES // 16                          # the largest n whose 4 n floats fit the LDS stage
BALL_LDS_MAX = LDS_BYTES // 12                         # ball query (n) and three-NN (m): 3 floats per point
NPOINT = 512                                           # centroids per level of the product geometry


def knn_point_instance(k, n):
    """knn_point_impl -> (kernel, K, staged in LDS)."""
    lds = n * 4 * 4 <= LDS_BYTES                       # const bool use_lds = lds <= 64 * 1024
    if k > 32:                                         # if (k > 32): the selection kernel
        return ("select", 0, lds)
    return ("sort", 16 if k <= 16 else 32, lds)        # else if (k <= 16) <16> else <32>


def knn_point_steps(k, n):
    """Trips of `for (base = 0; base < n; base += KV_LPQ * K)`."""
    return divup(n, C.KV_LPQ * knn_point_instance(k, n)[1])


def ball_lds(n):
    return n * 3 * 4 <= LDS_BYTES


def fps_ppl(n, table=None):
    for limit, ppl in (table or C.FPS_PPL):
        if limit is None or n <= 64 * limit:
            return ppl
    return None                                        # the block kernel


def tables_workgroups(samples, n, npoint=NPOINT):
    """rtk_geometry_tables -> (want, ball workgroups per (level, sample), ball chunks, three-NN workgroups of [fp3, fp2, fp1], their chunks)."""
    want = divup(C.GEO_TABLES_WGS, 9 * samples)
    ball_chunks = divup(npoint, BALL_CHUNK)
    nn_chunks = [divup(r, C.KV_QPW) for r in (npoint, npoint, n)]
    return want, min(want, ball_chunks), ball_chunks, [min(want, c) for c in nn_chunks], nn_chunks


def geometry_cloud_counts(npoint=NPOINT):
    """Cloud counts (even: pairs) that put `want` at 1, at 2, and at no fewer than the ball chunks."""
    one = roundup(divup(C.GEO_TABLES_WGS, 9), 2)
    two = 128 if divup(C.GEO_TABLES_WGS, 9 * 128) == 2 else roundup(divup(C.GEO_TABLES_WGS, 18), 2)
    return one, two, 2


# ------------------------------------------------------------------------------------------------
# float64 statements
# ------------------------------------------------------------------------------------------------
def d2_direct(q, p):
    """q (B,S,3), p (B,N,3) fp32 -> (B,S,N) float64 sum (q - p)^2."""
    return ((q.double()[:, :, None, :] - p.double()[:, None, :, :]) ** 2).sum(-1)


def d2_expand(q, p):
    """max(-2 q.p + |q|^2 + |p|^2, 0) in float64."""
    q, p = q.double(), p.double()
    dot = (q[:, :, None, :] * p[:, None, :, :]).sum(-1)
    return (-2.0 * dot + (q * q).sum(-1)[:, :, None] + (p * p).sum(-1)[:, None, :]).clamp_min(0.0)


def k_smallest(d, k):
    """The k smallest of d (..., N) by (distance, index) -> (indices int64 (..., k), distances); (0, +inf) in slots past N."""
    N = d.shape[-1]
    s = torch.sort(d, dim=-1, stable=True)
    idx, val = s.indices[..., :k], s.values[..., :k]
    if k > N:
        pad = d.shape[:-1] + (k - N,)
        idx = torch.cat([idx, torch.zeros(pad, dtype=idx.dtype)], -1)
        val = torch.cat([val, torch.full(pad, float("inf"), dtype=val.dtype)], -1)
    idx = torch.where(torch.isinf(val), torch.zeros_like(idx), idx)      # a masked (infinitely far) candidate is no candidate
    return idx, val


def knn_point_f64(k, points, query, n_valid=None):
    """rtk_knn_point / rtk_knn_point_masked -> (idx int64 (B,S,k), float64 distances, the float64 distance matrix with masked rows at +inf)."""
    d = d2_expand(query, points)
    n = points.shape[1]
    if n_valid is not None:
        for b, nv in enumerate(n_valid.tolist()):
            nc = n if nv >= n else max(nv, k)
            d[b, :, nc:] = float("inf")
    idx, val = k_smallest(d, k)
    return idx, val, d


def knn_f64(k, unknown, known):
    """rtk_knn / rtk_three_nn (k = 3) -> (idx int32 (B,n,k), float64 squared distances, the distance matrix)."""
    d = d2_direct(unknown, known)
    idx, val = k_smallest(d, k)
    return idx.to(torch.int32), val, d


def three_nn_f64(unknown, known):
    return knn_f64(3, unknown, known)


def radius2_f32(radius):
    """float32(radius) * float32(radius), rounded to fp32, as a float64 number."""
    r = torch.tensor(radius, dtype=torch.float32)
    return float((r * r).double())


def ball_query_f64(radius, nsample, xyz, new_xyz, prefill=0):
    """-> (idx int32 (B,M,nsample), hit counts (B,M), the distance matrix).  An empty ball's row holds `prefill` (a number or a tensor of
    the result's shape): the row as the caller left it."""
    d = d2_direct(new_xyz, xyz)
    return (ball_from_d2(d, radius2_f32(radius), nsample, prefill),) + ((d < radius2_f32(radius)).sum(-1), d)


def ball_from_d2(d, r2, nsample, prefill=0):
    B, M, N = d.shape
    hit = d < r2
    ar = torch.arange(N).expand(B, M, N)
    key = torch.where(hit, ar, ar + N).sort(-1).values[..., :nsample]
    if nsample > N:
        key = torch.cat([key, torch.full((B, M, nsample - N), 2 * N, dtype=key.dtype)], -1)
    cnt = hit.sum(-1)
    slot = torch.arange(nsample).expand(B, M, nsample)
    out = torch.where(slot < cnt[..., None], key, key[..., :1].expand_as(key))
    fill = prefill if torch.is_tensor(prefill) else torch.full_like(out, prefill)
    return torch.where((cnt > 0)[..., None], out, fill.to(out.dtype)).to(torch.int32)


# ------------------------------------------------------------------------------------------------
# bands
# ------------------------------------------------------------------------------------------------
BETA_DIRECT = 12.0      # units of u * cut-off
BETA_BALL = 6.0         # units of u * radius2


def beta_direct(cutoff):
    return BETA_DIRECT * U * cutoff


def beta_ball(r2):
    return BETA_BALL * U * r2


def expansion_error(query, points, d):
    """E(q, p) (B,S,N) float64 of the module docstring."""
    q, p = query.double(), points.double()
    A = (q[:, :, None, :].abs() * p[:, None, :, :].abs()).sum(-1)
    return 1.001 * U * (8.0 * A + (q * q).sum(-1)[:, :, None] + 3.0 * (p * p).sum(-1)[:, None, :] + torch.where(torch.isinf(d), torch.zeros_like(d), d))


def beta_expand(query, points, d):
    """(B,S): 2 max_p E(q, p) over the candidates (masked candidates, at +inf in d, excluded)."""
    E = expansion_error(query, points, d)
    return 2.0 * torch.where(torch.isinf(d), torch.zeros_like(E), E).max(-1).values


def cutoff_of(d, k):
    """The k-th smallest float64 distance (B,S) and the (k+1)-th (+inf when there is none)."""
    v = torch.sort(d, dim=-1).values
    nxt = v[..., k] if d.shape[-1] > k else torch.full_like(v[..., 0], float("inf"))
    return v[..., k - 1], nxt


def ambiguous_k(d, k, beta):
    """(B,S) bool: the (k+1)-th smallest distance lies inside the band, so the float64 statement does not decide the set.  A candidate
    at exactly the cut-off's float64 distance is not counted: off a lattice these are copies of one point (padding rows, the centroids
    of an over-sampled level), equal in fp32 as well and ordered by index, which the comparison with the oracle pins."""
    c, nxt = cutoff_of(d, k)
    return (nxt <= c + beta) & (nxt > c)


def check_k_band(got, d, k, beta, what=""):
    """got (B,S,k) indices against the float64 distance matrix d (B,S,N) (masked candidates at +inf) and the half-width beta (B,S)."""
    got = got.long()
    N = d.shape[-1]
    if got.shape != d.shape[:-1] + (k,):
        raise Mismatch("%s: result is %s, expected %s" % (what, tuple(got.shape), d.shape[:-1] + (k,)))
    if int(got.min()) < 0 or int(got.max()) >= N:
        raise Mismatch("%s: index outside [0, %d)" % (what, N))
    srt = got.sort(-1).values
    if k > 1 and bool((srt[..., 1:] == srt[..., :-1]).any()):
        raise Mismatch("%s: a candidate chosen twice" % what)
    c, _ = cutoff_of(d, k)
    dg = torch.gather(d, -1, got)
    far = dg > (c + beta)[..., None]
    if far.any():
        w = tuple(far.nonzero()[0].tolist())
        raise Mismatch("%s: query %s chose a candidate at %.9g, cut-off %.9g + beta %.3g" % (what, w[:-1], dg[w].item(), c[w[:-1]].item(), beta[w[:-1]].item()))
    chosen = torch.zeros_like(d, dtype=torch.bool).scatter_(-1, got, True)
    missed = (d < (c - beta)[..., None]) & ~chosen
    if missed.any():
        w = tuple(missed.nonzero()[0].tolist())
        raise Mismatch("%s: query %s left out candidate %d at %.9g, cut-off %.9g - beta %.3g" % (what, w[:-1], w[-1], d[w].item(), c[w[:-1]].item(), beta[w[:-1]].item()))
    if k > 1 and bool((dg[..., :-1] > dg[..., 1:] + beta[..., None]).any()):
        raise Mismatch("%s: result not ascending up to beta" % what)
    return float(((dg - c[..., None]) / beta[..., None].clamp_min(1e-300)).max())      # the largest excursion beyond the cut-off, in betas


def check_ball_band(got, d, r2, nsample, beta, empty=0, what=""):
    """got (B,M,nsample) against d (B,M,N): the hits h_0 < h_1 < ... are the strictly ascending prefix of a row, the rest repeats h_0.
    Every h lies inside r2 + beta; every index skipped before the last hit (before N when the row is not full) lies outside r2 - beta.
    A row of `empty` throughout is an empty ball when no point lies inside r2 - beta (else it is read like any other row)."""
    B, M, N = d.shape
    got = got.long()
    if got.shape != (B, M, nsample):
        raise Mismatch("%s: result is %s, expected %s" % (what, tuple(got.shape), (B, M, nsample)))
    if int(got.min()) < 0 or int(got.max()) >= N:
        raise Mismatch("%s: index outside [0, %d)" % (what, N))
    sure_in, sure_out, rows = (d < r2 - beta).numpy(), (d >= r2 + beta).numpy(), got.numpy()
    for b in range(B):
        for m in range(M):
            row, inside, outside = rows[b, m], sure_in[b, m], sure_out[b, m]
            if (row == empty).all() and not inside.any():
                continue
            L = 1
            while L < nsample and row[L] > row[L - 1]:
                L += 1
            hits = row[:L]
            if (row[L:] != hits[0]).any():
                raise Mismatch("%s: row (%d, %d) = %s: the slots after the hits do not repeat the first hit" % (what, b, m, row.tolist()))
            if outside[hits].any():
                raise Mismatch("%s: row (%d, %d) = %s holds a point outside the ball" % (what, b, m, row.tolist()))
            end = int(hits[-1]) if L == nsample else N
            skipped = inside[:end].copy()
            skipped[hits[hits < end]] = False
            if skipped.any():
                raise Mismatch("%s: row (%d, %d) = %s skips a point inside the ball" % (what, b, m, row.tolist()))


def ambiguous_ball(d, r2, beta):
    """(B,M) bool: a candidate within beta of the rim."""
    return ((d - r2).abs() <= beta).any(-1)


# ------------------------------------------------------------------------------------------------
# clouds
# ------------------------------------------------------------------------------------------------
FAR_CENTRE = (40.0, -20.0, 3.0)
R5 = float(torch.tensor(math.sqrt(5.0), dtype=torch.float32))      # float32(sqrt 5): its fp32 square is 5, its exact square is not


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def lattice_side(n):
    return 3 if n <= 20 else (5 if n <= 130 else (6 if n <= 600 else 16))


def cloud(gen, kind, b, n, side=None):
    """(b, n, 3) fp32.  lattice: integers in [0, side); random: N(0, 6^2); far5 / far50: uniform in a 5 cm / 50 cm cube at FAR_CENTRE."""
    if kind == "lattice":
        return torch.randint(0, side or lattice_side(n), (b, n, 3), generator=gen).float()
    if kind == "random":
        return (torch.randn(b, n, 3, generator=gen) * 6.0).contiguous()
    if kind in ("far5", "far50"):
        edge = 0.05 if kind == "far5" else 0.5
        return (torch.tensor(FAR_CENTRE) + (torch.rand(b, n, 3, generator=gen) - 0.5) * edge).float().contiguous()
    raise ValueError(kind)


def is_lattice(kind):
    return kind == "lattice"


FAR_KINDS = ("far5", "far50")      # exempt, by name, from the 5 % cap on ambiguous queries


# ------------------------------------------------------------------------------------------------
# case table
# ------------------------------------------------------------------------------------------------
STEP16, STEP32 = C.KV_LPQ * 16, C.KV_LPQ * 32      # candidates per trip of the K = 16 / K = 32 instance
KNN_POINT_N = sorted({16, 300} | {STEP16 - 1, STEP16, STEP16 + 1, STEP32 - 1, STEP32, STEP32 + 1})
KNN_POINT_S = [1, C.KV_QPW - 1, C.KV_QPW, C.KV_QPW + 1]
KNN_POINT_K = [1, 3, 16, 17, 32, 33, 64]             # and k = n

KnnPointCase = namedtuple("KnnPointCase", "name kind b n s ks claims")


def _ks(n, ks=KNN_POINT_K):
    return tuple(sorted({k for k in ks if k <= n} | {n})) if n <= 300 else tuple(ks)


KNN_POINT_CASES = [
    KnnPointCase("%s_n%d_s%d" % (kind, n, KNN_POINT_S[(i + j) % 4]), kind, 2, n, KNN_POINT_S[(i + j) % 4], _ks(n),
                 {"tie_at_16": 0.25} if kind == "lattice" and n >= STEP16 - 1 and KNN_POINT_S[(i + j) % 4] > 1 else
                 ({"zero_distances": 0.1} if kind == "far5" and KNN_POINT_S[(i + j) % 4] > 1 and n >= STEP16 - 1 else {}))
    for j, kind in enumerate(("lattice", "random", "far5", "far50")) for i, n in enumerate(KNN_POINT_N)
] + [
    # the LDS switch: 4 n floats at and just past 64 KiB, for the sorting and the selection kernel
    KnnPointCase("lds_at_limit", "lattice", 1, KNN_LDS_MAX, 5, (16, 17, 33), {"tie_at_16": 0.25}),
    KnnPointCase("lds_past_limit", "lattice", 1, KNN_LDS_MAX + 1, 5, (16, 17, 33), {"tie_at_16": 0.25}),
    KnnPointCase("random_past_limit", "random", 1, KNN_LDS_MAX + 1, 5, (16, 33), {}),
]


@functools.lru_cache(maxsize=None)
def knn_point_data(name):
    """-> (case, points (b,n,3), query (b,s,3)).  Far clusters: the first queries are the points themselves (the cost volume's kNN of a
    frame in itself)."""
    case = next(k for k in KNN_POINT_CASES if k.name == name)
    gen = _gen("knn_point", name)
    p = cloud(gen, case.kind, case.b, case.n)
    q = cloud(gen, case.kind, case.b, case.s, lattice_side(case.n))
    if case.kind in FAR_KINDS:
        t = min(case.s, case.n)
        q[:, :t] = p[:, :t]
    return case, p, q


MaskedKnnCase = namedtuple("MaskedKnnCase", "name kind n s k n_valid")


def _masked(kind, k, n=40):
    return MaskedKnnCase("%s_k%d" % (kind, k), kind, n, C.KV_QPW + 1, k, (1, k - 1, k, k + 1, n - 1, n))


MASKED_KNN_CASES = [_masked(kind, k) for kind in ("lattice", "random") for k in (16, 17, 33)]
PADDINGS = ("copies", "garbage")      # padding rows: copies of row 0 / far away


@functools.lru_cache(maxsize=None)
def masked_knn_data(name, padding):
    """-> (case, points (6,n,3) with the padding rows filled, query, n_valid int32)."""
    case = next(k for k in MASKED_KNN_CASES if k.name == name)
    gen = _gen("masked_knn", name)
    b = len(case.n_valid)
    p = cloud(gen, case.kind, b, case.n, 4)
    q = cloud(gen, case.kind, b, case.s, 4)
    for s, nv in enumerate(case.n_valid):
        p[s, nv:] = p[s, 0] if padding == "copies" else torch.tensor([9000.0, -7000.0, 8000.0]) + torch.arange(case.n - nv)[:, None].float()
    return case, p.contiguous(), q, torch.tensor(case.n_valid, dtype=torch.int32)


ThreeNNCase = namedtuple("ThreeNNCase", "name kind b n m unknown_nuniq known_nuniq claims")
Q = C.KV_QPW
THREE_NN_CASES = [ThreeNNCase("m%d" % m, "lattice", 2, Q + 6, m, None, None, {"inf_slots": m < 3}) for m in (1, 2, 3, 4)] + [
    ThreeNNCase("ties", "lattice", 2, 2 * Q + 2, 100, None, None, {"zero_distances": 20, "three_way_ties": 0.25}),
    ThreeNNCase("masked", "lattice", 5, 2 * Q + 2, 40, (1, Q - 1, Q, Q + 1, 2 * Q + 1), (1, 2, 38, 39, 40), {"three_way_ties": 0.25}),
    ThreeNNCase("masked_random", "random", 5, 2 * Q + 2, 40, (1, Q - 1, Q, Q + 1, 2 * Q + 1), (1, 2, 38, 39, 40), {}),
    ThreeNNCase("lds_at_limit", "lattice", 1, 5, BALL_LDS_MAX, None, None, {}),
    ThreeNNCase("lds_past_limit", "lattice", 1, 5, BALL_LDS_MAX + 1, None, None, {}),
    ThreeNNCase("random", "random", 2, Q + 6, 100, None, None, {}),
    ThreeNNCase("far5", "far5", 2, Q + 6, 100, None, None, {"narrow_band": True}),
]


@functools.lru_cache(maxsize=None)
def three_nn_data(name):
    """-> (case, unknown (b,n,3), known (b,m,3)): known rows >= known_nuniq[b] are copies of known row 0."""
    case = next(k for k in THREE_NN_CASES if k.name == name)
    gen = _gen("three_nn", name)
    side = 3 if case.m <= 4 else (4 if case.m <= 100 else 16)
    known = cloud(gen, case.kind, case.b, case.m, side)
    unknown = cloud(gen, case.kind, case.b, case.n, side)
    if case.known_nuniq:
        for s, ke in enumerate(case.known_nuniq):
            known[s, ke:] = known[s, 0]
    return case, unknown.contiguous(), known.contiguous()


KnnCase = namedtuple("KnnCase", "name kind b n m ks")
KNN_CASES = [KnnCase("lattice", "lattice", 2, 70, 300, (1, 5, 200)), KnnCase("random", "random", 2, 70, 300, (1, 5, 200)),
             KnnCase("lattice_m150", "lattice", 2, 70, 150, (5, 200))]      # m < k: (+inf, 0) slots


@functools.lru_cache(maxsize=None)
def knn_data(name):
    case = next(k for k in KNN_CASES if k.name == name)
    gen = _gen("knn", name)
    return case, cloud(gen, case.kind, case.b, case.n, 6), cloud(gen, case.kind, case.b, case.m, 6)


BallCase = namedtuple("BallCase", "name b n m r1 ns1 r2 ns2 nuniq claims")
T = C.RTK_BALL_TAIL_ROWS
BALL_CASES = [
    BallCase("n1", 2, 1, BALL_CHUNK + 1, 1.0, 4, 2.0, 8, None, {"empty_ball": 1}),
    BallCase("n5", 2, 5, BALL_CHUNK + 5, 2.0, 8, R5, 16, None, {"empty_ball": 1, "rim_pairs": 3}),
    BallCase("n63", 2, 63, 37, 1.0, 4, 3.0, 32, None, {"empty_ball": 1, "rim_pairs": 20, "full_balls": 10, "partial_balls": 10}),
    BallCase("n64", 2, 64, 37, 2.0, 16, 3.0, 32, None, {"empty_ball": 1, "rim_pairs": 20, "full_balls": 5, "partial_balls": 10}),
    BallCase("n65", 2, 65, 37, R5, 8, 3.0, 16, None, {"empty_ball": 1, "rim_pairs": 20, "r5_points": 20, "first_hit_above": 64, "full_balls": 10}),
    BallCase("n300", 5, 300, 70, 2.0, 4, R5, 8, (1, 7, T, T + 1, 70),
             {"empty_ball": 1, "rim_pairs": 20, "r5_points": 20, "first_hit_above": 64, "full_balls": 50, "last_hit_mid_step": 20}),
    BallCase("n300_wide", 5, 300, 70, 2.0, 16, 3.0, 32, (70, T + 1, T, 7, 1),
             {"empty_ball": 1, "rim_pairs": 20, "first_hit_above": 64, "full_balls": 50, "partial_balls": 20, "last_hit_mid_step": 20}),
    BallCase("lds_at_limit", 1, BALL_LDS_MAX, BALL_CHUNK + 1, 2.0, 4, 3.0, 32, None, {"empty_ball": 1, "rim_pairs": 20}),
    BallCase("lds_past_limit", 1, BALL_LDS_MAX + 1, BALL_CHUNK + 1, 2.0, 4, 3.0, 32, None, {"empty_ball": 1, "rim_pairs": 20}),      # rtk_ball_query only
]
BALL_SINGLE_NSAMPLE = 7      # the single-table entry point also runs with (r2, 7)


@functools.lru_cache(maxsize=None)
def ball_data(name):
    """-> (case, xyz (b,n,3), new_xyz (b,m,3)).  Centroid 0 is far from everything (an empty ball); from n = 65 on, centroid 1 sits in a
    far group of three points whose first index is past 64."""
    case = next(k for k in BALL_CASES if k.name == name)
    gen = _gen("ball", name)
    side = lattice_side(case.n)
    xyz, new_xyz = cloud(gen, "lattice", case.b, case.n, side), cloud(gen, "lattice", case.b, case.m, side)
    new_xyz[:, 0] = torch.tensor([100.0, 100.0, 100.0])
    if case.n >= 65:
        first = 70 if case.n >= 300 else 64
        last = 200 if case.n >= 300 else first
        xyz[:, first] = torch.tensor([40.0, 40.0, 40.0])
        if first + 1 < case.n and last > first:
            xyz[:, first + 1] = torch.tensor([40.0, 40.0, 41.0])
            xyz[:, last] = torch.tensor([40.0, 41.0, 41.0])
        new_xyz[:, 1] = torch.tensor([40.0, 40.0, 40.0])
    return case, xyz.contiguous(), new_xyz.contiguous()


# ---- the two product launches, through fused.Geometry ----------------------------------------------------------------------------
# clouds: "one" / "two" / "few" = the cloud counts of geometry_cloud_counts(), else a number of clouds.  pairs: the API's channel-major
# frame pairs with the kNN tables; else point-major clouds of one frame without them.  unique: distinct clouds per frame (repeated to the count).
GeoCase = namedtuple("GeoCase", "name kind n clouds pairs unique n_valid claims")
GEO_CASES = [
    GeoCase("lattice_n16", "lattice", 16, 4, True, 2, None, {}),
    GeoCase("lattice_n48", "lattice", 48, 2, True, 1, None, {"oversampled": True}),
    GeoCase("lattice_n243", "lattice", 243, 4, True, 2, None, {"oversampled": True}),
    GeoCase("lattice_n256", "lattice", 256, 2, True, 1, None, {"oversampled": True}),
    GeoCase("lattice_n300", "lattice", 300, 4, True, 2, None, {"oversampled": True}),
    GeoCase("lattice_n512", "grid", 512, "few", True, 1, None, {"all_chunks_live": True}),
    GeoCase("lattice_n513", "lattice", 513, 4, True, 2, None, {}),
    GeoCase("point_major_n300", "lattice", 300, 5, False, 5, None, {"oversampled": True}),
    GeoCase("far_cluster", "far", 256, 4, True, 2, None, {}),
    GeoCase("padded", "random", 352, 8, True, 4, ((322, 352, 16, 5), (300, 17, 352, 1)), {}),
    GeoCase("wgs_one", "grid", 512, "one", True, 3, None, {"all_chunks_live": True}),
    GeoCase("wgs_two", "grid", 512, "two", True, 3, None, {"all_chunks_live": True}),
    # half the clouds over-sampled (48 valid points, the rest copies of point 0): live and dead chunks interleave
    GeoCase("wgs_two_half_oversampled", "grid", 512, "two", True, 2, ((512, 48), (48, 512)), {"all_chunks_live": False}),
]


def geo_clouds(case):
    one, two, few = geometry_cloud_counts()
    return {"one": one, "two": two, "few": few}.get(case.clouds, case.clouds)


@functools.lru_cache(maxsize=None)
def geo_data(name):
    """-> (case, frames: a list of one or two (unique, n, 3) point-major fp32 clouds, n_valid: None or int32 (frames, unique))."""
    case = next(k for k in GEO_CASES if k.name == name)
    gen = _gen("geometry", name)
    frames = []
    for f in range(2 if case.pairs else 1):
        if case.kind == "grid":          # all 512 points of the 8 x 8 x 8 lattice, each cloud in its own order, shifted by integers
            g = torch.stack(torch.meshgrid(*[torch.arange(8.0)] * 3, indexing="ij"), -1).reshape(512, 3)
            x = torch.stack([g[torch.randperm(512, generator=gen)] + float(3 * f + s) for s in range(case.unique)])
        elif case.kind == "far":
            x = cloud(gen, "far5" if f == 0 else "far50", case.unique, case.n)
        else:
            x = cloud(gen, case.kind, case.unique, case.n, 6 - f)
        frames.append(x)
    nv = None
    if case.n_valid is not None:
        nv = torch.tensor(case.n_valid, dtype=torch.int32)
        for f, x in enumerate(frames):
            for s in range(case.unique):
                x[s, int(nv[f, s]):] = x[s, 0]
    return case, [x.contiguous() for x in frames], nv


RADII = ((2.0, 4.0), (4.0, 8.0), (8.0, 16.0))      # ratrack_amd.fused._PNHeadWeights (asserted by the GPU test)
NSAMPLES = ((4, 8), (8, 16), (16, 32))


def names(cases):
    return [k.name for k in cases]


# ------------------------------------------------------------------------------------------------
# verification: a table against its float64 statement (torch.equal on a lattice, the band elsewhere)
# ------------------------------------------------------------------------------------------------
def _equal(got, ref, what):
    if got.shape != ref.shape or got.dtype != ref.dtype:
        raise Mismatch("%s: result is %s %s, expected %s %s" % (what, got.dtype, tuple(got.shape), ref.dtype, tuple(ref.shape)))
    if not torch.equal(got, ref):
        w = tuple((got != ref).nonzero()[0].tolist())
        raise Mismatch("%s: entry %s is %s, the float64 statement says %s (%d entries differ)" % (what, w, got[w].item(), ref[w].item(), int((got != ref).sum())))


def _live(got, ref, live):
    """got with the rows outside `live` (B,R) replaced by the statement's: only live rows are judged."""
    return got if live is None else torch.where(live[..., None], got, ref.to(got.dtype))


def verify_knn_point(got, k, points, query, lattice, n_valid=None, what="knn_point"):
    """-> the fraction of ambiguous queries (0 on a lattice)."""
    idx, _, d = knn_point_f64(k, points, query, n_valid)
    if got.dtype != torch.int64:
        raise Mismatch("%s: indices are %s" % (what, got.dtype))
    if lattice:
        _equal(got, idx, what)
        return 0.0
    beta = beta_expand(query, points, d)
    check_k_band(got, d, k, beta, what)
    return float(ambiguous_k(d, k, beta).float().mean())


def verify_knn(got_idx, got_d2, k, unknown, known, lattice, live=None, what="knn"):
    """Direct form (rtk_knn, rtk_three_nn): indices as above; squared distances exact on a lattice, within gamma_5 d elsewhere."""
    idx, val, d = knn_f64(k, unknown, known)
    if got_idx.dtype != torch.int32 or got_d2.dtype != torch.float32:
        raise Mismatch("%s: result is %s / %s" % (what, got_idx.dtype, got_d2.dtype))
    gi, gd = _live(got_idx, idx, live), _live(got_d2, val.float(), live)
    if lattice:
        _equal(gi, idx, what + " indices")
        _equal(gd.double(), val, what + " distances")
        return 0.0
    kk = min(k, known.shape[1])
    c, _ = cutoff_of(d, kk)
    beta = beta_direct(c)
    check_k_band(gi[..., :kk], d, kk, beta, what)
    dg = torch.gather(d, -1, gi[..., :kk].long())
    if not bool(((gd[..., :kk].double() - dg).abs() <= 6.0 * U * dg).all()):
        raise Mismatch("%s: a squared distance further than 6 u d from float64" % what)
    return float(ambiguous_k(d, kk, beta).float().mean())


def verify_ball(got, radius, nsample, xyz, new_xyz, lattice, prefill=0, live=None, what="ball_query"):
    """prefill: what an empty ball's row holds (a number).  -> the fraction of ambiguous centroids."""
    ref, _, d = ball_query_f64(radius, nsample, xyz, new_xyz, prefill)
    if got.dtype != torch.int32:
        raise Mismatch("%s: indices are %s" % (what, got.dtype))
    g = _live(got, ref, live)
    if lattice:
        _equal(g, ref, what)
        return 0.0
    r2 = radius2_f32(radius)
    check_ball_band(g, d, r2, nsample, beta_ball(r2), prefill, what)
    return float(ambiguous_ball(d, r2, beta_ball(r2)).float().mean())


def rows_below(limit, rows):
    """limit (B,) -> (B, rows) bool: row index < limit[b]."""
    return torch.arange(rows)[None, :] < torch.as_tensor(limit).long()[:, None]


def verify_pair_tail(got, nuniq, fill, what):
    """rtk_ball_query_pair's rows past nuniq: zeros up to the next multiple of RTK_BALL_TAIL_ROWS, then the caller's `fill`."""
    B, M, _ = got.shape
    for b, nu in enumerate(torch.as_tensor(nuniq).tolist()):
        nu = min(nu, M)
        z1 = min(M, roundup(nu, C.RTK_BALL_TAIL_ROWS))
        if bool((got[b, nu:z1] != 0).any()):
            raise Mismatch("%s: sample %d: rows [%d, %d) do not read as zeros" % (what, b, nu, z1))
        if bool((got[b, z1:] != fill).any()):
            raise Mismatch("%s: sample %d: rows from %d on were written" % (what, b, z1))


def verify_three_nn_tail(got_idx, got_d2, nuniq, m, fill, what):
    """rtk_three_nn_masked's rows past unknown_nuniq: valid indices up to the next multiple of KV_QPW, untouched (index `fill`, NaN
    distance -- got_d2 None: not prefilled) beyond."""
    B, R, _ = got_idx.shape
    for b, nu in enumerate(torch.as_tensor(nuniq).tolist()):
        nu = min(nu, R)
        w1 = min(R, roundup(nu, C.KV_QPW))
        mid = got_idx[b, nu:w1]
        if mid.numel() and (int(mid.min()) < 0 or int(mid.max()) >= m):
            raise Mismatch("%s: sample %d: rows [%d, %d) hold an index outside [0, %d)" % (what, b, nu, w1, m))
        if bool((got_idx[b, w1:] != fill).any()) or (got_d2 is not None and not bool(torch.isnan(got_d2[b, w1:]).all())):
            raise Mismatch("%s: sample %d: rows from %d on were written" % (what, b, w1))


# ------------------------------------------------------------------------------------------------
# the C oracle, the second witness (test infrastructure; imported where used)
# ------------------------------------------------------------------------------------------------
def oracle_knn_point(k, points, query, n_valid=None):
    from oracle import pointnet2_ref as P
    if n_valid is None:
        return P.knn_point(k, points, query)
    n = points.shape[1]
    out = []
    for b, nv in enumerate(n_valid.tolist()):
        nc = n if nv >= n else max(nv, k)
        out.append(P.knn_point(k, points[b:b + 1, :nc].contiguous(), query[b:b + 1].contiguous()))
    return torch.cat(out)


def oracle_ball(radius, nsample, xyz, new_xyz, prefill=0):
    from oracle import pointnet2_ref as P
    B, N, _ = xyz.shape
    idx = torch.full((B, new_xyz.shape[1], nsample), prefill, dtype=torch.int32)
    P.ball_query_wrapper(B, N, new_xyz.shape[1], float(radius), nsample, new_xyz.contiguous(), xyz.contiguous(), idx)
    return idx


# ------------------------------------------------------------------------------------------------
# the product geometry: levels, tables, witnesses
# ------------------------------------------------------------------------------------------------
GEO_NN = (("fp3", 2, 3), ("fp2", 1, 2), ("fp1", 0, 1))      # (table, level of the unknown rows, level of the known rows)


def geo_batch(name):
    """-> (case, xyz0 (S,n,3) point-major: frame 1's clouds then frame 2's, n_valid int32 (S,) or None, pairs B or 0)."""
    case, frames, nv = geo_data(name)
    S = geo_clouds(case)
    per = S // len(frames)
    rep = [torch.arange(per) % case.unique for _ in frames]
    xyz0 = torch.cat([x[r] for x, r in zip(frames, rep)]).contiguous()
    n_valid = torch.cat([nv[f][r] for f, r in enumerate(rep)]).contiguous() if nv is not None else None
    return case, xyz0, n_valid, (per if case.pairs else 0)


def distinct_rows(x):
    return int(torch.unique(x, dim=0).shape[0])


def geo_levels_oracle(xyz0, n_valid=None, npoint=NPOINT):
    """The three FPS levels by the CPU oracle -> (idx [3] of (S,npoint) int32, xyz [4] of levels, nuniq [3] of (S,) int32).
    nuniq = min(npoint, distinct points of the cloud): the picks made before the cloud is exhausted."""
    from oracle import pointnet2_ref as P
    S, n, _ = xyz0.shape
    nv = n_valid.tolist() if n_valid is not None else [n] * S
    idx1 = torch.cat([P.fps(xyz0[s:s + 1, :nv[s]].contiguous(), npoint) for s in range(S)])
    idx, xyz = [idx1], [xyz0]
    for l in range(3):
        if l > 0:
            idx.append(P.fps(xyz[l], npoint))
        xyz.append(torch.gather(xyz[l], 1, idx[l].long()[..., None].expand(-1, -1, 3)).contiguous())
    nu = torch.tensor([min(npoint, distinct_rows(xyz0[s, :nv[s]])) for s in range(S)], dtype=torch.int32)
    return idx, xyz, [nu, nu.clone(), nu.clone()]


def geo_oracle_tables(levels, nuniq, B, n_valid, fill):
    """Every table of the two launches by the C oracle, with the rows the contracts leave alone holding `fill`
    -> (tables, compare: name -> (S, rows) bool of the rows that are the oracle's to decide)."""
    from oracle import pointnet2_ref as P
    S, npoint = levels[1].shape[:2]
    t, cmp_ = {}, {}
    for l in range(3):
        nu = nuniq[l].long().clamp_max(npoint)
        for s in range(2):
            full = P.ball_query(RADII[l][s], NSAMPLES[l][s], levels[l], levels[l + 1])
            rows = torch.arange(npoint)[None, :]
            z1 = ((nu + C.RTK_BALL_TAIL_ROWS - 1) // C.RTK_BALL_TAIL_ROWS * C.RTK_BALL_TAIL_ROWS).clamp_max(npoint)
            out = torch.where((rows < nu[:, None])[..., None], full, torch.zeros_like(full))
            out = torch.where((rows >= z1[:, None])[..., None], torch.full_like(full, fill), out)
            t["ball%d%d" % (l, s)], cmp_["ball%d%d" % (l, s)] = out, torch.ones(S, npoint, dtype=torch.bool)
    for name, u, k in GEO_NN:
        d2, idx = P.three_nn(levels[u], levels[k])
        live = rows_below(nuniq[u - 1], levels[u].shape[1]) if u > 0 else torch.ones(S, levels[u].shape[1], dtype=torch.bool)
        if u > 0:      # rows at or past roundup(unknown_nuniq, KV_QPW) are untouched
            w1 = (nuniq[u - 1].long() + C.KV_QPW - 1) // C.KV_QPW * C.KV_QPW
            idx = torch.where((torch.arange(idx.shape[1])[None, :] >= w1[:, None])[..., None], torch.full_like(idx, fill), idx)
        t["nn_idx_" + name], t["nn_d2_" + name] = idx, d2
        cmp_["nn_idx_" + name] = cmp_["nn_d2_" + name] = live
    if B:
        x1, x2 = levels[0][:B], levels[0][B:]
        t["knn12"] = oracle_knn_point(16, x2, x1, n_valid[B:] if n_valid is not None else None)
        t["knn11"] = oracle_knn_point(16, x1, x1, n_valid[:B] if n_valid is not None else None)
        cmp_["knn12"] = cmp_["knn11"] = torch.ones(B, x1.shape[1], dtype=torch.bool)
    return t, cmp_


def verify_geo_tables(t, levels, nuniq, B, n_valid, lattice, fill=None, first=None):
    """Every table of the two launches (CPU tensors, named as in geo_oracle_tables) against the float64 statements, level by level
    from the given centroids.  fill: the in-range index the workspace was pre-filled with (None: the untouched rows are not judged).
    first: judge the first `first` clouds of each frame only (a batch of repeated clouds).  -> {table: fraction of ambiguous rows}."""
    S, npoint = levels[1].shape[:2]
    per = S // 2 if B else S
    keep = torch.arange(S) if first is None else torch.cat([torch.arange(min(first, per)) + o for o in range(0, S, per)])
    lv = [x[keep] for x in levels]
    nu = [c[keep] for c in nuniq]
    amb = {}
    for l in range(3):
        live = rows_below(nu[l], npoint)
        for s in range(2):
            key = "ball%d%d" % (l, s)
            got = t[key][keep]
            amb[key] = verify_ball(got, RADII[l][s], NSAMPLES[l][s], lv[l], lv[l + 1], lattice, 0, live, key)
            if fill is not None:
                verify_pair_tail(got, nu[l], fill, key)
    for name, u, k in GEO_NN:
        rows = lv[u].shape[1]
        live = rows_below(nu[u - 1], rows) if u > 0 else None
        gi, gd = t["nn_idx_" + name][keep], t["nn_d2_" + name][keep]
        amb["nn_" + name] = verify_knn(gi, gd, 3, lv[u], lv[k], lattice, live, "three-NN " + name)
        if fill is not None and u > 0:
            verify_three_nn_tail(gi, None, nu[u - 1], lv[k].shape[1], fill, "three-NN " + name)
    if B:
        kb = keep[keep < B]
        x1, x2 = levels[0][:B][kb], levels[0][B:][kb]
        nv1, nv2 = (n_valid[:B][kb], n_valid[B:][kb]) if n_valid is not None else (None, None)
        amb["knn12"] = verify_knn_point(t["knn12"][kb], 16, x2, x1, lattice, nv2, "knn12")
        amb["knn11"] = verify_knn_point(t["knn11"][kb], 16, x1, x1, lattice, nv1, "knn11")
    return amb
