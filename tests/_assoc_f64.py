"""Float64 statements, tolerance rule, source constants and case tables of the association stage -- rtk_dbscan_batched,
rtk_object_descriptors, rtk_affinity_pairs, rtk_associate_batched (ratrack_amd/csrc/track_batched.hip) and their B = 1 forms rtk_dbscan
and rtk_log_sinkhorn (csrc/fused_misc.hip), which share csrc/assoc_common.h.  Shared by tests/test_assoc_f64_cpu.py (no GPU: the
statements against the shipped Python formulation, the margins, the coverage of the tables, the teeth of the bound) and
tests/test_assoc_f64_gpu.py (the kernels against the statements).

The rule (`_track_train_util.bound`): a HIP value lies within 4x the distance of float32 torch -- the reference's own arithmetic, run on
the CPU on the same case -- from float64, or within 1e-6 of the tensor's largest element if that is larger.  Integer results (indices1,
ids, counters, point_track_id, labels, obj) are exact, the max-prop channels are bit-exact, conf is the bits of the aff element it copies.
A decision is compared only where float64 itself is decided: every crafted decision case has a float64 margin (smallest top-two gap of
the plan's rows and columns) of at least MARGIN, asserted on the CPU, except the deliberate exact ties.  Nothing here is measured on the
code under test.
"""
import functools
import os
import re
import zlib
from collections import namedtuple

import numpy as np
import torch

from ratrack_amd import association as A
from ratrack_amd.track4d import Affinity

from _track_train_util import DESC, bound, check_grad, descriptors_of, mlp_copy, rel  # noqa: F401  (re-exported to the two test files)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = {
    "track_batched.hip": os.path.join(ROOT, "ratrack_amd", "csrc", "track_batched.hip"),
    "fused_misc.hip": os.path.join(ROOT, "ratrack_amd", "csrc", "fused_misc.hip"),
    "assoc_common.h": os.path.join(ROOT, "ratrack_amd", "csrc", "assoc_common.h"),
    "rtk_fused.h": os.path.join(ROOT, "include", "rtk_fused.h"),
}
MARGIN = 1e-3                 # float64 decision margin of every crafted decision case
ALPHA, ITERS = 0.9, 500       # Track4D's dustbin score and iteration count
THRESHOLD32 = float(np.float32(0.01))      # below 0.01 as a double: a matched pair with this affinity starts a fresh track


# ------------------------------------------------------------------------------------------------
# constants read from the sources
# ------------------------------------------------------------------------------------------------
def _product(text):
    out = 1
    for f in text.replace("(", "").replace(")", "").split("*"):
        out *= int(f)
    return out


def _match(source, pattern):
    with open(SOURCES[source]) as f:
        m = re.search(pattern, f.read())
    assert m, "%s no longer contains /%s/: tests/_assoc_f64.py restates it and its case tables are stale" % (source, pattern)
    return _product(m.group(1))


@functools.lru_cache(maxsize=None)
def source_constants():
    num = r"(\(?\d+(?: \* \d+)*\)?)"
    c = {
        "AFF_P": _match("track_batched.hip", r"#define AFF_P " + num),                      # pairs per tile of rtk_affinity_pairs
        "AFF_Q": _match("track_batched.hip", r"#define AFF_Q " + num),
        "AFF_GRID_TARGET": _match("track_batched.hip", r"int g = rtk_divup\((\d+), B\)"),   # g = clamp(ceil(2048 / B), 4, tiles)
        "AFF_GRID_MIN": _match("track_batched.hip", r"g = g < (\d+) \? \d+ : \(g > tiles \? tiles : g\);"),
        "DESC_G": _match("track_batched.hip", r"#define DESC_G " + num),                    # object slots per stream in flight
        "DESC_CHUNK": _match("track_batched.hip", r"for \(int base = 0; base < n; base \+= (\d+)\) \{\n\s+const int p = base \+ t;"),
        "DB_LDS_BYTES": _match("track_batched.hip", r"#define DB_LDS_BYTES " + num),
        "ASSOC_LDS_LIMIT": _match("track_batched.hip", r"#define ASSOC_LDS_LIMIT " + num),
        "RTK_DBSCAN_POINT_BYTES": _match("rtk_fused.h", r"#define RTK_DBSCAN_POINT_BYTES " + num),
        "RTK_DESC": _match("rtk_fused.h", r"#define RTK_DESC " + num),
        "SINKHORN_LDS_BYTES": _match("fused_misc.hip", r"RTK_REQUIRE\(lds <= (\d+ \* \d+), \"log_sinkhorn"),
        "DBSCAN_LDS_BYTES": _match("fused_misc.hip", r"if \(bytes <= (\d+ \* \d+)\) \{"),
        "DB_D": _match("assoc_common.h", r"#define DB_D " + num),
        "OT_ROWS": _match("assoc_common.h", r"for \(int i0 = 0; i0 < R; i0 \+= (\d+)\)"),   # rows (then columns) per pass of log_ot_lds
    }
    _match("fused_misc.hip", r"\(size_t\)n \* \(DB_D \* sizeof\(float\) \+ (3) \* sizeof\(int\)\)")
    c["DBSCAN_B1_POINT_BYTES"] = c["DB_D"] * 4 + 3 * 4                                      # f (n,8) | src | lab | aux
    return c


def assoc_lds_bytes(K):
    """track_batched.hip: assoc_lds_bytes."""
    return ((K + 1) * ((K + 1) | 1) + 2 * (K + 1) + 5 * K) * 4


def max_objects():
    """track_batched.hip: rtk_track_max_objects."""
    K = 1
    while K < 256 and assoc_lds_bytes(K + 1) + 64 <= source_constants()["ASSOC_LDS_LIMIT"]:
        K += 1
    return K


def sinkhorn_b1_fits(m, n):
    """fused_misc.hip: rtk_log_sinkhorn's LDS requirement."""
    return ((m + 1) * ((n + 1) | 1) + (m + 1) + (n + 1)) * 4 <= source_constants()["SINKHORN_LDS_BYTES"]


def affinity_grid(B, K):
    """rtk_affinity_pairs: workgroups per stream."""
    c = source_constants()
    g, tiles = -(-c["AFF_GRID_TARGET"] // B), -(-K * K // c["AFF_P"])
    return c["AFF_GRID_MIN"] if g < c["AFF_GRID_MIN"] else (tiles if g > tiles else g)      # g = g < 4 ? 4 : (g > tiles ? tiles : g)


KMAX = 197                    # rtk_track_max_objects() today; the CPU test holds it against max_objects()


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def names(cases):
    return [k.name for k in cases]


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------
# statements
# ------------------------------------------------------------------------------------------------
def descriptors_f64(pc1, flow, feature1, prop, obj, num_objects, K=None, n_valid=None):
    """rtk_fused.h: [centre(3) | var xyz(3) | max prop(128) | mean flow(3) | mean (RCS, v_r)(2) | var (RCS, v_r)(2)] of the members
    (obj == k among the stream's first n_valid columns) of every object k < num_objects[b]; population variance about the mean.
    Inputs (B,C,N) of any float dtype, widened here.  -> (B,K,141) float64, NaN in the rows past num_objects[b]."""
    B, _, N = pc1.shape
    K = int(max(num_objects)) if K is None else K
    out = torch.full((B, K, DESC), float("nan"), dtype=torch.float64)
    stat = torch.cat((pc1, flow, feature1), dim=1).double()          # xyz(3) | flow(3) | (RCS, v_r)(2)
    prop = prop.double()
    for b in range(B):
        n = N if n_valid is None else int(n_valid[b])
        for k in range(int(num_objects[b])):
            idx = torch.nonzero(obj[b, :n] == k).reshape(-1)
            x = stat[b][:, idx]
            mean = x.sum(1) / idx.numel()
            var = ((x - mean[:, None]) ** 2).sum(1) / idx.numel()
            out[b, k] = torch.cat((mean[0:3], var[0:3], prop[b][:, idx].max(1).values, mean[3:6], mean[6:8], var[6:8]))
    return out


# channel groups of a descriptor: each is held against the bound on its own scale (the centre of a far object would hide its variance)
DESC_GROUPS = (("centre", slice(0, 3)), ("var_xyz", slice(3, 6)), ("mean_flow", slice(134, 137)), ("mean_rrv", slice(137, 139)),
               ("var_rrv", slice(139, 141)))
DESC_PROP = slice(6, 134)


def affinity_f64(mlp, desc_prev, m, desc, n):
    """The Affinity MLP on desc[j] - desc_prev[i]: the difference in float32, as the kernel and the reference take it, then widened to
    the MLP's dtype.  -> ((m, n) affinities, (m, n) pre-sigmoid logits), pair (i, j) from row i * n + j."""
    dtype = next(mlp.parameters()).dtype
    diff = (desc[:n].float().unsqueeze(0) - desc_prev[:m].float().unsqueeze(1)).reshape(m * n, DESC).to(dtype)
    with torch.no_grad():
        logit = mlp[:-1](diff)
        return mlp[-1](logit).reshape(m, n), logit.reshape(m, n)


def plan(aff, alpha, iters, dtype):
    """association.log_optimal_transport of an (m, n) affinity block in `dtype`; alpha is the fp32 value the kernels receive."""
    a = torch.tensor(float(np.float32(alpha)), dtype=dtype)
    return A.log_optimal_transport(aff.to(dtype).unsqueeze(0), a, iters)[0]


def plan_f64(aff, alpha=ALPHA, iters=ITERS):
    return plan(aff, alpha, iters, torch.float64)


def first_argmax(x, axis):
    return np.argmax(x, axis=axis)            # numpy: the first occurrence of the maximum


Decision = namedtuple("Decision", "indices1 ids conf counter margin row_gap col_gap")


def _gaps(S, axis):
    """top-two gap along `axis` of every line across it (inf where the line has one entry)."""
    if S.shape[axis] < 2:
        return np.full(S.shape[1 - axis], np.inf)
    top = np.sort(S, axis=axis)
    return (top[-1] - top[-2]) if axis == 0 else (top[:, -1] - top[:, -2])


def decide_f64(plan64, aff32, prev_ids, counter, argmax=first_argmax, threshold=0.01):
    """rtk_fused.h, rtk_associate_batched: on the (m, n) block of the plan, ind0 = row-wise best column, ind1 = column-wise best row
    (exact ties: the lowest index), indices1[j] = ind1[j] when ind0[ind1[j]] == j and exp(max) > 0, else -1; object j takes a fresh ID
    (counter, counter + 1, ... in current-object order; conf 0) when unmatched or float(aff[k, j]) < 0.01, else prev_ids[k] with
    conf = aff[k, j].  plan64: (m+1, n+1) float64, or None when m or n is 0; aff32 (m, n) float32.
    margin: the smallest top-two gap over the columns of the block and the rows some column points at.
    `argmax` and `threshold` are the header's; the CPU test passes wrong ones to show that the cases notice."""
    m, n = aff32.shape
    aff = aff32.numpy()
    assert aff.dtype == np.float32
    idx = [-1] * n
    row_gap, col_gap = np.full(m, np.inf), np.full(n, np.inf)
    margin = float("inf")
    if m > 0 and n > 0:
        S = plan64[:m, :n].numpy()
        ind0, ind1 = argmax(S, 1), argmax(S, 0)
        max0 = S[np.arange(m), ind0]
        for j in range(n):
            k = int(ind1[j])
            if int(ind0[k]) == j and np.exp(max0[k]) > 0:
                idx[j] = k
        row_gap, col_gap = _gaps(S, 1), _gaps(S, 0)
        margin = float(min(col_gap.min(), row_gap[np.unique(ind1)].min()))
    ids, conf = [], []
    for j in range(n):
        k = idx[j]
        if k < 0 or float(aff[k, j]) < threshold:
            ids.append(counter)
            conf.append(np.float32(0))
            counter += 1
        else:
            ids.append(int(prev_ids[k]))
            conf.append(aff[k, j])
    return Decision(idx, ids, conf, counter, margin, row_gap, col_gap)


def associator_decision(aff32, prev_ids, counter, device="cpu"):
    """association.Associator.__call__ on a crafted (m, n) affinity matrix (the MLP bypassed) -> (ids, confs, indices1 or None, max_id)."""
    m, n = aff32.shape
    aff_d = aff32.to(device)
    shipped = A.affinity_matrix
    A.affinity_matrix = lambda net, oc, op, d=None: (aff_d.reshape(-1), aff_d.unsqueeze(0), m, n)
    try:
        assoc = A.Associator(None)
        assoc.max_id = counter
        objects_curr = [torch.zeros(1, 139, 1, device=device) for _ in range(n)]
        objects_prev = {int(k): torch.zeros(1, 139, 1, device=device) for k in prev_ids}
        _, _, indices1, confs, objects = assoc(objects_curr, objects_prev)
    finally:
        A.affinity_matrix = shipped
    order = {id(o): j for j, o in enumerate(objects_curr)}
    ids = [None] * n
    for key, o in objects.items():
        ids[order[id(o)]] = key
    return ids, [float(c) for c in confs], None if indices1 is None else indices1[0].tolist(), assoc.max_id


# ------------------------------------------------------------------------------------------------
# Sinkhorn plan: cases
# ------------------------------------------------------------------------------------------------
def strong_diagonal(m, n, gen):
    """A permuted strong diagonal plus small noise: min(m, n) entries of 0.9 on distinct rows and columns over 0.05 * rand.  A row or
    column the diagonal leaves out (m != n) gets one entry of 0.3, so that its own best is decided by a margin as well."""
    a = torch.rand(m, n, generator=gen) * 0.05
    k = min(m, n)
    rows, cols = torch.randperm(m, generator=gen), torch.randperm(n, generator=gen)
    a[rows[:k], cols[:k]] += 0.9
    for i in rows[k:].tolist():
        a[i, int(torch.randint(0, n, (1,), generator=gen))] += 0.3
    for j in cols[k:].tolist():
        a[int(torch.randint(0, m, (1,), generator=gen)), j] += 0.3
    return a


def affinity_content(kind, m, n, gen):
    if kind == "rand":
        return torch.rand(m, n, generator=gen)
    if kind == "zeros_ones":          # exactly 0.0 and 1.0 among the random entries
        a, r = torch.rand(m, n, generator=gen), torch.rand(m, n, generator=gen)
        a[r < 0.2], a[r > 0.8] = 0.0, 1.0
        return a
    if kind == "equal":
        return torch.full((m, n), 0.37)
    if kind == "diag":
        return strong_diagonal(m, n, gen)
    raise ValueError(kind)


PlanCase = namedtuple("PlanCase", "name m n content alpha iters edge")
_R, _D = "rand", "diag"
PLAN_CASES = [
    # m+1 and n+1 at 2, 16, 17, 32, 33 on each axis independently (OT_ROWS = 16 rows, then columns, per pass of log_ot_lds)
    PlanCase("m1_n1", 1, 1, _R, ALPHA, ITERS, "2 x 2: one partial pass on each axis"),
    PlanCase("m1_n15", 1, 15, _R, ALPHA, ITERS, "C = 16: one full column pass, every lane of a row holds one entry"),
    PlanCase("m15_n1", 15, 1, _R, ALPHA, ITERS, "R = 16: one full row pass"),
    PlanCase("m15_n16", 15, 16, _R, ALPHA, ITERS, "R = 16, C = 17: a second column pass with one live column"),
    PlanCase("m16_n15", 16, 15, _R, ALPHA, ITERS, "R = 17, C = 16: a second row pass with one live row"),
    PlanCase("m16_n31", 16, 31, _R, ALPHA, ITERS, "R = 17, C = 32: lanes hold exactly two entries"),
    PlanCase("m31_n32", 31, 32, _R, ALPHA, ITERS, "R = 32, C = 33: a third column pass with one live column"),
    PlanCase("m32_n31", 32, 31, _R, ALPHA, ITERS, "R = 33, C = 32: a third row pass with one live row"),
    PlanCase("m1_n120", 1, 120, _R, ALPHA, ITERS, "a two-row table 121 wide"),
    PlanCase("m120_n1", 120, 1, _R, ALPHA, ITERS, "a two-column table 121 high"),
    PlanCase("m40_n9", 40, 9, _R, ALPHA, ITERS, "clearly rectangular: log m and log n differ in the dustbin marginals"),
    PlanCase("m126_n126", 126, 126, _R, ALPHA, ITERS, "the largest table rtk_log_sinkhorn admits (65532 B of its 64 KiB)"),
    # content
    PlanCase("zeros_ones", 16, 31, "zeros_ones", ALPHA, ITERS, "entries of exactly 0.0 and 1.0"),
    PlanCase("all_equal", 15, 16, "equal", ALPHA, ITERS, "every row and column ties exactly"),
    PlanCase("diag_15_16", 15, 16, _D, ALPHA, ITERS, "permuted strong diagonal (decision case)"),
    PlanCase("diag_33_31", 33, 31, _D, ALPHA, ITERS, "permuted strong diagonal, R = 34, C = 32 (decision case)"),
    # iterations and alpha on one small shape
    PlanCase("iters0", 15, 16, _R, ALPHA, 0, "no iteration: the plan is Z - norm"),
    PlanCase("iters1", 15, 16, _R, ALPHA, 1, "one iteration"),
    PlanCase("alpha05", 15, 16, _R, 0.5, ITERS, "another dustbin score"),
    # beyond rtk_log_sinkhorn: the batched kernel only
    PlanCase("kmax_square", KMAX, KMAX, _R, ALPHA, ITERS, "K = rtk_track_max_objects(): the whole 160 KiB of LDS (plan only: random)"),
    PlanCase("kmax_row", 1, KMAX, _R, ALPHA, ITERS, "(1, K) next to it"),
    PlanCase("kmax_col", KMAX, 1, _R, ALPHA, ITERS, "(K, 1) next to it"),
    PlanCase("diag_kmax", KMAX, KMAX, _D, ALPHA, ITERS, "permuted strong diagonal at K x K (decision case)"),
    PlanCase("diag_126_127", 126, 127, _D, ALPHA, ITERS, "one step past rtk_log_sinkhorn's limit: the framework path (decision case)"),
]
PLAN_BY_NAME = {k.name: k for k in PLAN_CASES}
B1_PLAN_CASES = [k for k in PLAN_CASES if sinkhorn_b1_fits(k.m, k.n)]
B1_EXCEED = [(127, 126), (126, 127)]          # one step over (126, 126) on either axis

PlanData = namedtuple("PlanData", "case aff p64 p32")


def _special_affinity(name):
    """The crafted matrices of the decision table that are no PlanCase content."""
    gen = _gen("special", name)
    if name == "tie_17_33":       # columns 3 and 20 identical: row 5's best is both, across two 16-lane passes
        a = torch.rand(17, 33, generator=gen) * 0.05
        cols = [c for c in torch.randperm(33, generator=gen).tolist() if c not in (3, 20)]
        for i in range(17):
            a[i, 3 if i == 5 else cols[i]] += 0.9
        for j in cols[17:]:           # the columns the diagonal leaves out: one entry of 0.3 each, their best is decided as well
            a[int(torch.randint(0, 17, (1,), generator=gen)), j] += 0.3
        a[:, 20] = a[:, 3]
        return a
    if name in ("threshold_at", "threshold_above"):      # the matched pair (1, 1) holds float32(0.01) / the next float32 above it
        a = torch.tensor([[0.9, 0.0, 0.02], [0.0, 0.0, 0.0], [0.03, 0.0, 0.8]])
        v = np.float32(0.01)
        a[1, 1] = float(v if name == "threshold_at" else np.nextafter(v, np.float32(1)))
        return a
    if name == "below_threshold":
        return torch.eye(4) * 0.008 + torch.rand(4, 4, generator=gen) * 0.0005          # a decided diagonal, every entry < 0.01
    if name == "m0":
        return torch.zeros(0, 3)
    if name == "n0":
        return torch.zeros(3, 0)
    raise KeyError(name)


SPECIAL = ("tie_17_33", "threshold_at", "threshold_above", "below_threshold", "m0", "n0")


@functools.lru_cache(maxsize=None)
def plan_data(name):
    """Affinity block, float64 plan and float32 torch plan of a PLAN_CASES entry or a SPECIAL matrix (shared: do not write to them)."""
    if name in PLAN_BY_NAME:
        case = PLAN_BY_NAME[name]
        aff = affinity_content(case.content, case.m, case.n, _gen("plan", name))
    else:
        aff = _special_affinity(name)
        case = PlanCase(name, aff.shape[0], aff.shape[1], "special", ALPHA, ITERS, "")
    if case.m == 0 or case.n == 0:
        return PlanData(case, aff, None, None)
    return PlanData(case, aff, plan(aff, case.alpha, case.iters, torch.float64), plan(aff, case.alpha, case.iters, torch.float32))


# a launch of rtk_associate_batched: streams are plan-case names, or "reset:<name>" (a reset stream: its block is not associated),
# "inactive:<name>" (sits the frame out), "empty_prev" (0, 5), "empty_curr" (5, 0)
PlanGroup = namedtuple("PlanGroup", "name K alpha iters streams edge")
PLAN_GROUPS = [
    PlanGroup("k128", 128, ALPHA, ITERS, tuple(k.name for k in B1_PLAN_CASES if (k.alpha, k.iters) == (ALPHA, ITERS) and max(k.m, k.n) <= 128),
              "every B = 1 shape as one stream of a K = 128 launch (row stride K, not n)"),
    PlanGroup("iters0", 16, ALPHA, 0, ("iters0",), ""),
    PlanGroup("iters1", 16, ALPHA, 1, ("iters1",), ""),
    PlanGroup("alpha05", 16, 0.5, ITERS, ("alpha05",), ""),
    PlanGroup("kmax", KMAX, ALPHA, ITERS, ("kmax_square", "kmax_row", "kmax_col", "empty_prev", "empty_curr", "reset:m15_n16",
                                           "inactive:m15_n16"), "the largest table next to degenerate, reset and inactive streams"),
]

# decision launches: (K, N, streams); every stream's float64 margin >= MARGIN except the exact ties named in TIES
DecisionGroup = namedtuple("DecisionGroup", "name K N streams counters edge")
DECISION_GROUPS = [
    DecisionGroup("margins", 40, 300, ("diag_15_16", "diag_33_31", "tie_17_33", "threshold_at", "threshold_above", "below_threshold",
                                       "m0", "n0", "reset:diag_15_16", "inactive:diag_15_16"),
                  (7, 1000, 0, 41, 41, 5, 90, 91, 2000000000, 17), "N = 300: no multiple of 256, two trips of the point loop"),
    DecisionGroup("kmax", KMAX, 513, ("diag_kmax", "diag_15_16"), (123, 0), "K x K decisions at the LDS limit"),
]
TIES = {"tie_17_33": (5, (3, 20))}      # name -> (tied row, its two columns)


def stream_spec(s):
    """-> (mode, plan-data name or None, m, n)."""
    if s == "empty_prev":
        return "live", None, 0, 5
    if s == "empty_curr":
        return "live", None, 5, 0
    mode, _, name = s.rpartition(":")
    d = plan_data(name)
    return (mode or "live"), name, d.case.m, d.case.n


def prev_ids_of(s, m):
    """Distinct previous IDs of a stream (a function of its position-independent name)."""
    base = 100 + zlib.crc32(s.encode()) % 1000
    return [base + 3 * i for i in range(m)]


def point_objects(s, n, N):
    """obj (N,) int32 of a decision stream: object indices in [0, n) mixed with entries equal to n, greater than n and -1 (all of
    which map to -1 in point_track_id)."""
    gen = _gen("obj", s)
    obj = torch.randint(0, max(n, 1), (N,), generator=gen).to(torch.int32) if n > 0 else torch.full((N,), -1, dtype=torch.int32)
    r = torch.rand(N, generator=gen)
    obj[r < 0.1] = -1
    obj[(r >= 0.1) & (r < 0.2)] = n
    obj[(r >= 0.2) & (r < 0.3)] = n + 3
    obj[0], obj[N - 1], obj[256 % N] = n, max(n - 1, -1), n + 1
    return obj


# ------------------------------------------------------------------------------------------------
# descriptors: cases
# ------------------------------------------------------------------------------------------------
DescCase = namedtuple("DescCase", "name B N K n_valid counts kind layout active prev_count edge")
DESC_CASES = [
    DescCase("n_valid", 5, 513, 40, (1, 255, 256, 257, 513), (1, 16, 17, 33, 33), ("one", "random", "random", "random", "straddle"),
             "contig", None, (0,) * 5,
             "n_valid at 1, 255, 256, 257, 513 of N = 513: one, two and three 256-column chunks; 1, 16, 17, 33 objects on DESC_G = 16 "
             "slots; an object across both chunk boundaries; objects of one point; padding = copies of column 0 with obj = -1"),
    DescCase("k8_all_points", 2, 513, 8, (513, 300), (1, 8), ("all", "random"), "contig", None, (0, 0),
             "grid y = K = 8 < DESC_G; one object holding every point"),
    DescCase("kmax", 1, 513, KMAX, (513,), (KMAX,), ("random",), "contig", None, (0,), "K = the maximum, every slot an object"),
    DescCase("views", 2, 513, 40, (513, 257), (33, 17), ("straddle", "random"), "views", None, (0, 0),
             "all five inputs as non-contiguous views: a (B,N,C) buffer permuted, a slice of a wider buffer"),
    DescCase("far80", 2, 513, 40, (513, 513), (6, 1), ("far80", "far80_all"), "contig", None, (0, 0),
             "80 m away with 1e-2 spread in xyz: the variance channels; objects of 2 to 200 points, and one of all 513"),
    DescCase("inactive", 4, 300, 12, (300, 300, 300, 300), (5, 3, 3, 3), ("random",) * 4, "contig", (1, 0, 0, 0), (0, 5, -3, 17),
             "inactive streams copy desc_prev[:prev_count] bit for bit (prev_count 5; -3 and K + 5 clamped to 0 and K)"),
]
DescData = namedtuple("DescData", "case pc1 flow feature1 prop cls obj num_objects d64 d32")
FAR80_SIZES = (2, 8, 33, 64, 200, 100)


def _assign(gen, kind, n, count, N):
    obj = torch.full((N,), -1, dtype=torch.int32)
    if kind == "one":
        obj[0] = 0
    elif kind == "all" or kind == "far80_all":
        obj[:n] = 0
    elif kind == "far80":
        perm, at = torch.randperm(n, generator=gen), 0
        for k, size in enumerate(FAR80_SIZES[:count]):
            obj[perm[at:at + size]] = k
            at += size
    elif kind in ("random", "straddle"):
        obj[:n] = torch.randint(0, count, (n,), generator=gen).to(torch.int32)
        obj[:n][torch.rand(n, generator=gen) < 0.2] = -1
        if kind == "straddle":        # object 0 across both chunk boundaries; objects 1 and 2 of one point each
            obj[:n][(obj[:n] >= 0) & (obj[:n] <= 2)] = 3
            obj[torch.tensor([254, 255, 256, 257, 511, 512])] = 0
            obj[300], obj[0] = 1, 2
            keep = {0: (254, 255, 256, 257, 511, 512), 1: (300,), 2: (0,)}
        else:
            keep = {}
        free = [p for p in torch.randperm(n, generator=gen).tolist() if not any(p in v for v in keep.values())]
        for k in range(len(keep), count):       # no object is empty
            obj[free[k]] = k
    else:
        raise ValueError(kind)
    return obj


@functools.lru_cache(maxsize=None)
def desc_data(name):
    case = next(k for k in DESC_CASES if k.name == name)
    gen = _gen("desc", name)
    B, N = case.B, case.N
    pc1 = torch.randn(B, 3, N, generator=gen) * 10.0
    flow, f1 = torch.randn(B, 3, N, generator=gen), torch.randn(B, 2, N, generator=gen)
    prop = torch.rand(B, 128, N, generator=gen)
    obj = torch.full((B, N), -1, dtype=torch.int32)
    for b in range(B):
        n = case.n_valid[b]
        if case.kind[b].startswith("far80"):
            pc1[b] = torch.tensor([80.0, -3.0, 1.0])[:, None] + torch.randn(3, N, generator=gen) * 1e-2
        obj[b] = _assign(gen, case.kind[b], n, case.counts[b], N)
        for t in (pc1, flow, f1, prop):          # padding: copies of column 0, obj = -1
            t[b, :, n:] = t[b, :, :1]
    num = list(case.counts)
    live = [bool(a) for a in case.active] if case.active is not None else [True] * B
    num_live = [c if a else 0 for c, a in zip(num, live)]
    d64 = descriptors_f64(pc1, flow, f1, prop, obj, num_live, K=case.K, n_valid=case.n_valid)
    d32 = torch.full((B, case.K, DESC), float("nan"))
    valid_obj = obj.clone()
    for b in range(B):
        valid_obj[b, case.n_valid[b]:] = -1
    for b, d in enumerate(descriptors_of(pc1, flow, f1, prop, valid_obj, num_live)):      # association.object_descriptor in float32
        if d is not None:
            d32[b, :d.shape[0]] = d
    return DescData(case, pc1, flow, f1, prop, torch.full((B, N), 0.9), obj, num, d64, d32)


def one_pass_descriptors32(d):
    """A deliberately wrong float32 variant: var = E[x^2] - E[x]^2 (the CPU test shows the far-object case rejects it)."""
    out = d.d32.clone()
    stat = torch.cat((d.pc1, d.flow, d.feature1), dim=1)
    for b in range(d.case.B):
        for k in range(d.case.counts[b]):
            idx = torch.nonzero(d.obj[b, :d.case.n_valid[b]] == k).reshape(-1)
            x = stat[b][:, idx]
            var = (x * x).mean(1) - x.mean(1) ** 2
            out[b, k, 3:6], out[b, k, 139:141] = var[0:3], var[6:8]
    return out


# ------------------------------------------------------------------------------------------------
# affinity pairs: cases
# ------------------------------------------------------------------------------------------------
AffCase = namedtuple("AffCase", "name B K prev_count num_objects reset weights kind edge")
_LIVE_1024 = {0: (12, 12), 511: (5, 7), 512: (7, 5), 1023: (3, 12)}
AFF_CASES = [
    AffCase("tile_edge", 6, 20, (1, 3, 4, 1, 17, 20), (1, 5, 4, 17, 1, 3), (0,) * 6, "seeded", "unit",
            "m * n at 1, 15, 16, 17 (both ways round) and 60 around AFF_P = 16: one partial tile, a full one, a second with one pair"),
    AffCase("pairs_256", 3, 43, (15, 16, 6), (17, 16, 43), (0,) * 3, "seeded", "unit",
            "m * n at 255, 256 and 258 = 6 x 43 (257 is prime and beyond K: the first product past 256): the last tile full, absent, "
            "two pairs"),
    AffCase("grid_stride", 1024, 12, tuple(_LIVE_1024.get(b, (0, 0))[0] for b in range(1024)),
            tuple(_LIVE_1024.get(b, (0, 0))[1] for b in range(1024)), (0,) * 1024, "seeded", "unit",
            "B = 1024: ceil(2048 / B) = 2 clamps to 4 workgroups per stream; stream 0 has 144 pairs = 9 tiles: three trips of the "
            "grid-stride loop; four live streams, the others without pairs"),
    AffCase("clamped", 5, 12, (5, 4, -3, 17, 6), (6, 0, 5, 17, -3), (1, 0, 0, 0, 0), "seeded", "unit",
            "a reset stream, num_objects = 0, counts of -3 and K + 5: nothing is written for the first three and the last, the "
            "fourth is clamped to K x K"),
    AffCase("far80", 4, 24, (5, 24, 7, 6), (8, 17, 7, 9), (0, 0, 0, 1), "seeded", "far80",
            "near-identical descriptors 80 m away in stream 2 (cancellation in curr - prev); 40, 408, 49 pairs; stream 3 reset"),
    AffCase("reference_weights", 3, 24, (5, 24, 7), (8, 17, 7), (0, 0, 0), "reference", "unit",
            "the reference state dict's Affinity (its outputs all lie near 0.5: kept once, as the shipped weights)"),
]
AffData = namedtuple("AffData", "case prev curr m n a64 a32 logit64")
WEIGHT_GAIN = 3.0             # every layer's weight matrix of the seeded Affinity is scaled by this: float64 logits spread >= 1


@functools.lru_cache(maxsize=None)
def affinity_net(kind):
    """The Affinity module (float32, CPU) of a case: a seeded default initialisation with every weight matrix scaled by WEIGHT_GAIN
    (the default initialisation and the reference weights give logits within a few hundredths of each other, so that a wrong
    channel hardly moves them), or the reference state dict's."""
    if kind == "reference":
        from _util import reference_state_dict
        net = Affinity(141)
        sd = reference_state_dict()
        net.load_state_dict({k[len("affinity."):]: v for k, v in sd.items() if k.startswith("affinity.")}, strict=True)
        return net.eval()
    with torch.random.fork_rng(devices=[]):          # the module's default initialisation draws from the global generator
        torch.manual_seed(1234)
        net = Affinity(141)
    with torch.no_grad():
        for l in net.affinity:
            if isinstance(l, torch.nn.Linear):
                l.weight *= WEIGHT_GAIN
    return net.eval()


def live_counts(case):
    clamp = lambda v: min(max(int(v), 0), case.K)
    m = [0 if r else clamp(c) for c, r in zip(case.prev_count, case.reset)]
    return m, [clamp(c) for c in case.num_objects]


@functools.lru_cache(maxsize=None)
def aff_data(name):
    case = next(k for k in AFF_CASES if k.name == name)
    gen = _gen("aff", name)
    B, K = case.B, case.K
    prev, curr = torch.randn(B, K, DESC, generator=gen), torch.randn(B, K, DESC, generator=gen)
    if case.kind == "far80":
        prev[2, :, 0:3] += 80.0
        curr[2] = prev[2] + torch.randn(K, DESC, generator=gen) * 1e-4
    m, n = live_counts(case)
    net = affinity_net(case.weights)
    mlp64, mlp32 = mlp_copy(net, torch.float64), mlp_copy(net, torch.float32)
    a64, a32, logit = {}, {}, {}
    for b in range(B):
        if m[b] * n[b]:
            a64[b], logit[b] = affinity_f64(mlp64, prev[b], m[b], curr[b], n[b])
            a32[b], _ = affinity_f64(mlp32, prev[b], m[b], curr[b], n[b])
    return AffData(case, prev, curr, m, n, a64, a32, logit)


# ------------------------------------------------------------------------------------------------
# DBSCAN: cases
# ------------------------------------------------------------------------------------------------
DbCase = namedtuple("DbCase", "name N n_valid kind min_samples work edge")
EPS = 1.5
DBSCAN_CASES = [
    DbCase("chain_at_eps", 64, (40, 40), ("chain", "chain_gap"), 2, True,
           "a chain on a lattice of spacing exactly eps = 1.5 (multiples of 0.5: exact arithmetic): one cluster, the ball is closed; the "
           "same chain with one gap of 2.0: two clusters"),
    DbCase("min_samples_1", 200, (200, 150), ("sparse", "blobs"), 1, True, "every mover is core, singletons are clusters"),
    DbCase("movers_255_256_257", 400, (400, 400, 400), ("movers255", "movers256", "movers257"), 3, True,
           "the compaction and the pair loops at 255, 256 and 257 movers (one and two trips of 256 threads); border points"),
    DbCase("b1_lds_edge", 2979, (2978, 2979), ("blobs600", "blobs600"), 2, True,
           "rtk_dbscan on both sides of 128 KiB / 44 B = 2978.9 points: LDS tables, then the workspace"),
    DbCase("batched_lds_edge", 2731, (2731, 2730, 100), ("blobs600", "blobs600", "blobs"), 2, True,
           "rtk_dbscan_batched past DB_LDS_BYTES / 48 = 2730.7: stream 0 needs the workspace, streams 1 and 2 fit the LDS"),
    DbCase("batched_n2730", 2730, (2730,), ("blobs600",), 3, False, "the last N whose tables fit the LDS: no workspace is passed"),
]
DbData = namedtuple("DbData", "case x cls labels obj num_objects")


def _db_stream(gen, kind, n):
    """-> (x (n, 8) float32 clustering channels, mover mask (n,))."""
    x = torch.zeros(n, 8)
    mover = torch.ones(n, dtype=torch.bool)
    if kind in ("chain", "chain_gap"):
        steps = torch.full((n,), EPS)
        if kind == "chain_gap":
            steps[n // 2] = 2.0
        pos = torch.cumsum(steps, 0) - EPS
        order = torch.randperm(n, generator=gen)          # column order is not chain order
        x[order, 0] = pos
        x[:, 1], x[:, 7] = 4.5, -2.0
    elif kind == "sparse":        # isolated points 10 apart and a few pairs
        x[:, 0] = torch.arange(n) * 10.0
        x[1::7, 0] = x[0::7, 0][:len(range(1, n, 7))] + 1.0
        mover = torch.rand(n, generator=gen) < 0.7
    else:
        movers = {"blobs": int(n * 0.6), "blobs600": 600, "movers255": 255, "movers256": 256, "movers257": 257}[kind]
        centres = torch.rand(max(movers // 8, 2), 8, generator=gen) * 30.0
        x = centres[torch.randint(0, centres.shape[0], (n,), generator=gen)] + torch.randn(n, 8, generator=gen) * 0.45
        mover = torch.zeros(n, dtype=torch.bool)
        mover[torch.randperm(n, generator=gen)[:movers]] = True
    return x, mover


def reference_order(labels):
    """Object index of every point: clusters ranked by their first member point (models/track4d.py:119-125)."""
    out = np.full(labels.shape, -1, dtype=np.int64)
    pts = np.nonzero(labels >= 0)[0]
    if pts.size:
        ids, first = np.unique(labels[pts], return_index=True)
        rank = np.empty(int(ids.max()) + 1, dtype=np.int64)
        rank[ids[np.argsort(first, kind="stable")]] = np.arange(ids.size)
        out[pts] = rank[labels[pts]]
    return out


@functools.lru_cache(maxsize=None)
def db_data(name):
    """x (B, N, 8) clustering channels (xyz, flow, v_r, prop[0]) and cls (B, N); labels / obj / num_objects from association.dbscan on
    the movers of each stream's first n_valid columns.  Padding columns are copies of column 0 and movers."""
    case = next(k for k in DBSCAN_CASES if k.name == name)
    B, N = len(case.n_valid), case.N
    x, cls = torch.zeros(B, N, 8), torch.full((B, N), 0.99)
    labels, obj, num = np.full((B, N), -1, dtype=np.int64), np.full((B, N), -1, dtype=np.int64), []
    for b in range(B):
        n = case.n_valid[b]
        xs, mover = _db_stream(_gen("db", name, b), case.kind[b], n)
        x[b, :n], x[b, n:] = xs, xs[0]
        cls[b, :n] = torch.where(mover, 0.97, 0.03)
        mv = mover.numpy()
        labels[b, np.nonzero(mv)[0]] = A.dbscan(xs.numpy()[mv], EPS, case.min_samples)
        obj[b] = reference_order(labels[b])
        num.append(int(labels[b].max()) + 1)
    return DbData(case, x, cls, labels, obj, num)
