"""Shared by tests/test_track_assign_cpu.py and tests/test_track_assign_gpu.py: the host statement of rtk_associate_optimal
(include/rtk_fused.h; csrc/track_assign.hip, csrc/lds_assignment.h `la_solve_dense`; `BatchedTracker(assign="optimal")`), the case
tables both files walk, and the decision rules the statement must tell apart.  No GPU is needed to import this module.

  quantise        the gate in float64, the weight (int)(aff * 2^28) in fp32, truncated
  host_solve      the maximum-weight one-to-one matching of a weight block by tests/_track_identity_util.min_assignment
  scipy_total     the same optimum by scipy.optimize.linear_sum_assignment          } cross-checks
  brute_total     the same optimum over all permutations (blocks up to 6 x 6)       }
  fast_total      the same optimum by a numpy form of the Hungarian method: what `is_unique` re-solves with
  device_method   la_solve_dense line by line (one lane instead of 64): its matching, its total and its search rounds
  is_unique       the optimum is unique iff removing any one matched edge gives a strictly smaller optimum: a different optimal
                  matching either lacks a matched edge (then the optimum survives that edge's removal) or is a strict superset (then it
                  weighs more, all weights being positive)
  bookkeeping     IDs, confidences, counter, the next ids / count and point_track_id from a given matching"""
import itertools

import numpy as np

from _track_identity_util import min_assignment

ONE = 1 << 28
GATE = 0.01
F32_GATE = np.float32(0.01)                          # below the double 0.01: not admissible
F32_ABOVE = np.nextafter(F32_GATE, np.float32(1))    # the first float that is
INF = 0x7fffffff


# ---- the statement ---------------------------------------------------------------------------------------------------------------------
def quantise(aff, gate=GATE):
    """aff (m, n) float32 -> (m, n) int64 weights: 0 where the pair is not admissible."""
    aff = np.asarray(aff, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        ok = aff.astype(np.float64) >= float(gate)                      # a NaN compares false
        q = (np.minimum(np.where(ok, aff, np.float32(0)), np.float32(1)) * np.float32(ONE)).astype(np.int64)      # fp32 product, truncated
    return np.where(ok, q, 0)


def host_solve(w):
    """w (m, n) ints >= 0 -> (total, indices1): indices1[j] = the row matched to column j or -1; matched pairs have w > 0."""
    w = np.asarray(w, dtype=np.int64)
    m, n = w.shape
    idx = [-1] * n
    if m == 0 or n == 0:
        return 0, idx
    rows_first = m <= n
    a = w if rows_first else w.T
    col = min_assignment([[-int(x) for x in r] for r in a])             # a pair that is no edge costs 0: matched or not, it adds nothing
    total = 0
    for r, c in enumerate(col):
        i, j = (r, c) if rows_first else (c, r)
        if w[i, j] > 0:
            idx[j] = i
            total += int(w[i, j])
    return total, idx


def scipy_total(w):
    from scipy.optimize import linear_sum_assignment
    w = np.asarray(w, dtype=np.int64)
    if w.size == 0:
        return 0
    r, c = linear_sum_assignment(-w)
    return int(w[r, c].sum())


def brute_total(w):
    w = np.asarray(w, dtype=np.int64)
    m, n = w.shape
    assert m <= 6 and n <= 6
    if m == 0 or n == 0:
        return 0
    a = w if m <= n else w.T
    return max(sum(int(a[i, p[i]]) for i in range(a.shape[0])) for p in itertools.permutations(range(a.shape[1]), a.shape[0]))


def fast_total(w):
    """The optimum by the Hungarian method with the column loop in numpy."""
    w = np.asarray(w, dtype=np.int64)
    if w.size == 0:
        return 0
    if w.shape[0] > w.shape[1]:
        w = w.T
    n, m = w.shape
    cost = -w
    big = np.int64(1) << 60
    u, v = np.zeros(n + 1, dtype=np.int64), np.zeros(m + 1, dtype=np.int64)
    p, way = np.zeros(m + 1, dtype=np.int64), np.zeros(m + 1, dtype=np.int64)
    for i in range(1, n + 1):
        p[0], j0 = i, 0
        minv, used = np.full(m + 1, big, dtype=np.int64), np.zeros(m + 1, dtype=bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            cur = cost[i0 - 1] - u[i0] - v[1:]
            upd = ~used[1:] & (cur < minv[1:])
            minv[1:][upd] = cur[upd]
            way[1:][upd] = j0
            cand = np.where(used[1:], big, minv[1:])
            j1 = int(np.argmin(cand)) + 1
            delta = cand[j1 - 1]
            u[p[used]] += delta
            v[used] -= delta
            minv[~used] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    return int(sum(w[p[j] - 1, j - 1] for j in range(1, m + 1) if p[j]))


def device_method(w):
    """la_solve_dense (csrc/lds_assignment.h) statement for statement -> (total, cp, search rounds): rows enter in index order, every
    row owns a private column of cost 0, the nearest column wins and ties go to the smaller index."""
    w = np.asarray(w, dtype=np.int64)
    R, C = w.shape
    u, v, cp = [0] * R, [0] * C, [-1] * C
    rounds = 0
    for r in range(R):
        most = max([0] + [int(w[r, j]) + v[j] for j in range(C) if w[r, j] > 0])
        ur = -most
        dist, way, done = [INF] * C, [-1] * C, [False] * C
        i, ui, base, jin, dd, jdd, D, jend = r, ur, 0, -1, INF, -1, 0, -1
        for _ in range(C + 1):
            rounds += 1
            if base - ui < dd:
                dd, jdd = base - ui, jin
            near = (INF, 0xffffffff)
            wi = w[i]
            for j in range(C):
                if done[j]:
                    continue
                if wi[j] > 0:
                    nd = base + (-int(wi[j]) - ui - v[j])
                    if nd < dist[j]:
                        dist[j], way[j] = nd, jin
                if dist[j] != INF:
                    near = min(near, (dist[j], j))
            d, j = near
            if d == INF or dd <= d:
                D, jend = dd, jdd
                break
            owner = cp[j]
            done[j] = True
            if owner < 0:
                D, jend = d, j
                break
            i, ui, base, jin = owner, u[owner], d, j
        for j in range(C):
            if done[j]:
                gap = D - dist[j]
                v[j] -= gap
                if cp[j] >= 0:
                    u[cp[j]] += gap
        u[r] = ur + D
        j = jend
        while j >= 0:
            jp = way[j]
            cp[j] = r if jp < 0 else cp[jp]
            j = jp
    return sum(int(w[cp[j], j]) for j in range(C) if cp[j] >= 0), cp, rounds


def is_unique(w):
    w = np.asarray(w, dtype=np.int64)
    if w.size == 0:
        return True
    if ((w > 0).sum(axis=0) <= 1).all() and ((w > 0).sum(axis=1) <= 1).all():
        return True                                   # every edge stands alone: the matching is the edge set
    total, idx = host_solve(w)
    for j, i in enumerate(idx):
        if i >= 0:
            w2 = w.copy()
            w2[i, j] = 0
            if fast_total(w2) >= total:
                return False
    return True


def check_matching(w, idx):
    """idx (n) is a one-to-one matching of admissible pairs of w -> its weight."""
    m, n = w.shape
    rows = [i for i in idx if i >= 0]
    assert len(idx) == n and all(0 <= i < m for i in rows) and len(set(rows)) == len(rows), idx
    assert all(w[i, j] > 0 for j, i in enumerate(idx) if i >= 0), idx
    return sum(int(w[i, j]) for j, i in enumerate(idx) if i >= 0)


# ---- the decision rules the statement differs from -------------------------------------------------------------------------------------
def mutual_best(aff, gate=GATE):
    """The pairs that are each other's best (lowest index among equals), at or above the gate -> indices1."""
    aff = np.asarray(aff, dtype=np.float32)
    m, n = aff.shape
    idx = [-1] * n
    for j in range(n):
        i = int(np.argmax(aff[:, j]))
        if int(np.argmax(aff[i])) == j and float(aff[i, j]) >= gate:
            idx[j] = i
    return idx


def greedy(aff, gate=GATE):
    """Heaviest admissible pair first, every row and column once -> indices1."""
    aff = np.asarray(aff, dtype=np.float32)
    m, n = aff.shape
    idx, rows = [-1] * n, set()
    for e in np.argsort(-aff.reshape(-1), kind="stable"):
        i, j = divmod(int(e), n)
        if float(aff[i, j]) >= gate and i not in rows and idx[j] < 0:
            idx[j] = i
            rows.add(i)
    return idx


def quantise_fp32_gate(aff, gate=GATE):
    """The gate applied as an fp32 constant: float32(0.01) >= float32(0.01) is admitted."""
    aff = np.asarray(aff, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        ok = aff >= np.float32(gate)
    return np.where(ok, (np.minimum(np.where(ok, aff, np.float32(0)), np.float32(1)) * np.float32(ONE)).astype(np.int64), 0)


def quantise_rounded(aff, gate=GATE):
    aff = np.asarray(aff, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        ok = aff.astype(np.float64) >= float(gate)
    return np.where(ok, np.rint(np.where(ok, aff, np.float32(0)).astype(np.float64) * ONE).astype(np.int64), 0)


# ---- the tail --------------------------------------------------------------------------------------------------------------------------
def bookkeeping(indices1, aff, prev_ids, counter, obj, K):
    """One active stream: indices1 (n) a matching, aff (m, n) float32, prev_ids (>= m), counter its next ID, obj (N) the object of every
    point -> dict(object_ids, object_conf (float32), indices1 (all K long: -1 / 0 / -1 past n), counter, ids (n: the next table's first
    rows), count, point_track_id (N))."""
    n = len(indices1)
    ids, conf, nxt = [], [], int(counter)
    for j, i in enumerate(indices1):
        if i >= 0:
            ids.append(int(prev_ids[i]))
            conf.append(np.float32(aff[i][j]))
        else:
            ids.append(nxt)
            conf.append(np.float32(0))
            nxt += 1
    pid = [ids[o] if 0 <= o < n else -1 for o in obj]
    return dict(object_ids=ids + [-1] * (K - n), object_conf=np.array(conf + [np.float32(0)] * (K - n), dtype=np.float32),
                indices1=list(indices1) + [-1] * (K - n), counter=nxt, ids=ids, count=n, point_track_id=pid)


# ---- the case tables ---------------------------------------------------------------------------------------------------------------------
TWO_BY_TWO = np.array([[0.9, 0.8], [0.8, 0.1]], dtype=np.float32)
SHAPES = ((0, 3), (3, 0), (1, 1), (1, 5), (5, 1), (2, 2), (5, 7), (7, 5), (63, 65), (64, 64), (65, 63), (128, 128), (197, 1), (1, 197),
          (197, 197))
DECISION_LIMIT = 65          # a dense block's uniqueness is established (and its decisions compared) up to this size: is_unique re-solves
                             # the block once per matched pair


def _k_of(m, n):
    return 8 if max(m, n) <= 8 else 128 if max(m, n) <= 128 else 197


def permuted_diagonal(rng, m, n):
    """0.9 on a permuted diagonal over 0.05 * rand: with a gate of 0.5 every admissible pair stands alone."""
    a = (0.05 * rng.random((m, n))).astype(np.float32)
    k = min(m, n)
    rows, cols = rng.permutation(m)[:k], rng.permutation(n)[:k]
    a[rows, cols] = np.float32(0.9)
    return a


def product_matrix(m, n):
    """aff[i][j] proportional to (i + 1)(j + 1), the largest 0.98: every row prefers the last column -- long augmenting paths, and the
    potentials move at every step."""
    return (np.outer(np.arange(1, m + 1), np.arange(1, n + 1)).astype(np.float64) * (0.98 / (m * n))).astype(np.float32)


def cases():
    """[dict(name, K, m, n, aff (m, n) float32, gate, decision)] -- decision: the optimum is unique (held to it by the CPU test) and the
    device's indices1 is compared; else only the plan's validity and its total are."""
    rng = np.random.default_rng(20)
    out = []

    def add(name, aff, gate=GATE, decision=False, K=None):
        aff = np.asarray(aff, dtype=np.float32)
        m, n = aff.shape
        out.append(dict(name=name, K=K or _k_of(m, n), m=m, n=n, aff=aff, gate=gate, decision=decision))
    for m, n in SHAPES:
        if (m, n) == (2, 2):
            add("two_by_two", TWO_BY_TWO, decision=True)
            continue
        if m == 0 or n == 0:
            add("empty_%dx%d" % (m, n), np.zeros((m, n), dtype=np.float32))
            continue
        add("diagonal_%dx%d" % (m, n), permuted_diagonal(rng, m, n), gate=0.5, decision=True)
        add("dense_%dx%d" % (m, n), (0.02 + 0.97 * rng.random((m, n))).astype(np.float32), decision=max(m, n) <= DECISION_LIMIT)
    add("product_64x64", product_matrix(64, 64), decision=True)
    add("ties_5x7", np.full((5, 7), 0.625, dtype=np.float32))
    edge = np.full((2, 2), 0.001, dtype=np.float32)
    edge[0, 0], edge[1, 1] = F32_GATE, F32_ABOVE                    # only the second is admissible
    add("float32_gate", edge, decision=True)
    half = np.array([[0.5, 0.4999999], [0.3, 0.6]], dtype=np.float32)      # 0.5 is exactly the gate: admissible; its neighbour below is not
    add("exactly_at_gate", half, gate=0.5, decision=True)
    nan = (0.2 + 0.7 * rng.random((5, 7))).astype(np.float32)
    nan[2, 3] = np.nan
    add("nan_inside", nan, decision=True)
    return out


def expected(case):
    """-> (w, total, indices1) of the statement."""
    w = quantise(case["aff"], case["gate"])
    total, idx = host_solve(w)
    return w, total, idx
