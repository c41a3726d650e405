"""CPU: the ground tests/test_assoc_f64_gpu.py stands on (tests/_assoc_f64.py) -- the case tables straddle every constant read from the
kernels' sources, the float64 statements agree with the shipped Python formulation, every crafted decision case is decided in float64
by a margin, the seeded Affinity spreads its logits, and the bound rejects five deliberately wrong float32 variants."""
import numpy as np
import pytest
import torch

from ratrack_amd import association as A, tracker as T

import _assoc_f64 as F

C = F.source_constants()


def stale(table, constant):
    return "%s = %d in the sources: the %s table of tests/_assoc_f64.py no longer straddles it" % (constant, C[constant], table)


# ------------------------------------------------------------------------------------------------
# coverage: the tables against the constants of the sources
# ------------------------------------------------------------------------------------------------
def test_plan_table_straddles_the_pass_width_and_the_lds_limits():
    assert F.max_objects() == F.KMAX, stale("PLAN_CASES / DESC_CASES (KMAX)", "ASSOC_LDS_LIMIT")
    r = C["OT_ROWS"]
    want = {2, r, r + 1, 2 * r, 2 * r + 1}
    b1 = [k for k in F.B1_PLAN_CASES if k.content == "rand" and (k.alpha, k.iters) == (F.ALPHA, F.ITERS)]
    assert want <= {k.m + 1 for k in b1}, stale("PLAN_CASES (rows)", "OT_ROWS")
    assert want <= {k.n + 1 for k in b1}, stale("PLAN_CASES (columns)", "OT_ROWS")
    assert any(k.m >= 4 * k.n for k in b1) and {(1, 120), (120, 1)} <= {(k.m, k.n) for k in b1}
    # (126, 126) is the largest square rtk_log_sinkhorn admits; one step over it on either axis is refused -- and association.py's own
    # statement of the limit sends exactly those shapes down the framework path
    big = max(k.m for k in b1 if k.m == k.n)
    assert F.sinkhorn_b1_fits(big, big) and F.B1_EXCEED == [(big + 1, big), (big, big + 1)], stale("PLAN_CASES (largest)", "SINKHORN_LDS_BYTES")
    for m, n in [(big, big)] + F.B1_EXCEED:
        shipped = (m + 1) * ((n + 1) | 1) + m + n + 2 <= 16 * 1024          # association.sinkhorn_assignment
        assert shipped == F.sinkhorn_b1_fits(m, n), stale("PLAN_CASES (largest)", "SINKHORN_LDS_BYTES")
    assert not F.sinkhorn_b1_fits(126, 127) and F.PLAN_BY_NAME["diag_126_127"]
    assert {0, 1, F.ITERS} <= {k.iters for k in F.PLAN_CASES} and len({k.alpha for k in F.PLAN_CASES}) == 2
    assert {"rand", "zeros_ones", "equal", "diag"} <= {k.content for k in F.PLAN_CASES}
    # every B = 1 case also runs as a stream of a batched launch; the K-max launch holds what the issue names
    grouped = {F.stream_spec(s)[1] for g in F.PLAN_GROUPS for s in g.streams}
    assert {k.name for k in F.B1_PLAN_CASES} <= grouped
    kmax = next(g for g in F.PLAN_GROUPS if g.name == "kmax")
    assert kmax.K == F.KMAX and sorted(F.stream_spec(s)[2:] for s in kmax.streams if not s.startswith(("reset", "inactive"))) == \
        sorted([(F.KMAX, F.KMAX), (1, F.KMAX), (F.KMAX, 1), (0, 5), (5, 0)])
    assert any(s.startswith("reset:") for s in kmax.streams) and any(s.startswith("inactive:") for s in kmax.streams)
    for g in list(F.PLAN_GROUPS) + list(F.DECISION_GROUPS):
        assert all(max(F.stream_spec(s)[2:]) <= g.K for s in g.streams), g.name
    for g in F.DECISION_GROUPS:
        assert len(g.counters) == len(g.streams) and g.N % 256 != 0 and g.N > 256
    assert len(set(F.DECISION_GROUPS[0].counters)) > 3


def test_descriptor_table_straddles_the_chunk_and_the_slot_count():
    ch, g = C["DESC_CHUNK"], C["DESC_G"]
    nv = next(k for k in F.DESC_CASES if k.name == "n_valid")
    assert set(nv.n_valid) == {1, ch - 1, ch, ch + 1, 2 * ch + 1} and nv.N == 2 * ch + 1, stale("DESC_CASES (n_valid)", "DESC_CHUNK")
    assert {1, g, g + 1, 2 * g + 1} <= set(nv.counts), stale("DESC_CASES (object counts)", "DESC_G")
    assert any(k.K < g for k in F.DESC_CASES), stale("DESC_CASES (K < DESC_G)", "DESC_G")
    assert any(k.K == F.KMAX and F.KMAX in k.counts for k in F.DESC_CASES)
    d = F.desc_data("n_valid")
    straddler = torch.nonzero(d.obj[4] == 0).reshape(-1).tolist()
    assert min(straddler) < ch <= max(p for p in straddler if p < 2 * ch) and max(straddler) >= 2 * ch, stale("DESC_CASES (straddle)", "DESC_CHUNK")
    assert int((d.obj[4] == 1).sum()) == 1 and int((d.obj[0] == 0).sum()) == 1          # objects of one point
    for name in F.names(F.DESC_CASES):
        d = F.desc_data(name)
        for b in range(d.case.B):
            n = d.case.n_valid[b]
            assert (d.obj[b, n:] == -1).all() and torch.equal(d.pc1[b, :, n:], d.pc1[b, :, :1].expand(-1, d.case.N - n))
            members = [int((d.obj[b, :n] == k).sum()) for k in range(d.case.counts[b])]
            assert min(members) >= 1, (name, b)
    assert int((F.desc_data("k8_all_points").obj[0] == 0).sum()) == 513
    assert F.DESC_PROP.stop - F.DESC_PROP.start == 128 and C["RTK_DESC"] == F.DESC


def test_affinity_table_straddles_the_tile_and_the_grid():
    p = C["AFF_P"]
    pairs = set()
    for k in F.AFF_CASES:
        m, n = F.live_counts(k)
        pairs |= {a * b for a, b in zip(m, n)}
    assert {1, p - 1, p, p + 1} <= pairs, stale("AFF_CASES (pairs)", "AFF_P")
    assert {16 * p - 1, 16 * p, 16 * p + 2} <= pairs, stale("AFF_CASES (pairs)", "AFF_P")
    tile = next(k for k in F.AFF_CASES if k.name == "tile_edge")
    m, n = F.live_counts(tile)
    assert any(a < b for a, b in zip(m, n)) and any(a > b for a, b in zip(m, n))
    gs = next(k for k in F.AFF_CASES if k.name == "grid_stride")
    assert -(-C["AFF_GRID_TARGET"] // gs.B) < C["AFF_GRID_MIN"] == F.affinity_grid(gs.B, gs.K), stale("AFF_CASES (grid_stride)", "AFF_GRID_MIN")
    m, n = F.live_counts(gs)
    assert -(-(-(-m[0] * n[0] // p)) // F.affinity_grid(gs.B, gs.K)) == 3, stale("AFF_CASES (grid_stride: three trips)", "AFF_P")
    assert 3 <= sum(1 for a, b in zip(m, n) if a * b) <= 4
    cl = next(k for k in F.AFF_CASES if k.name == "clamped")
    assert {-3, cl.K + 5} <= set(cl.prev_count) and {-3, cl.K + 5, 0} <= set(cl.num_objects) and 1 in cl.reset
    # the tile order the other cases rely on: every tile_edge stream takes one tile per workgroup (grid = tiles there)
    assert F.affinity_grid(tile.B, tile.K) == -(-tile.K * tile.K // p)


def test_dbscan_table_straddles_both_lds_limits():
    b1 = C["DBSCAN_LDS_BYTES"] // C["DBSCAN_B1_POINT_BYTES"]
    bt = C["DB_LDS_BYTES"] // C["RTK_DBSCAN_POINT_BYTES"]
    by = {k.name: k for k in F.DBSCAN_CASES}
    assert by["b1_lds_edge"].n_valid == (b1, b1 + 1), stale("DBSCAN_CASES (b1_lds_edge)", "DBSCAN_LDS_BYTES")
    assert by["batched_lds_edge"].n_valid[:2] == (bt + 1, bt) and by["batched_lds_edge"].N == bt + 1, stale("DBSCAN_CASES (batched_lds_edge)", "DB_LDS_BYTES")
    assert by["batched_n2730"].N == bt and not by["batched_n2730"].work, stale("DBSCAN_CASES (batched_n2730)", "DB_LDS_BYTES")
    assert T.DBSCAN_POINT_BYTES == C["RTK_DBSCAN_POINT_BYTES"] and T.DBSCAN_LDS_BYTES == C["DB_LDS_BYTES"]
    movers = lambda name, b: int((F.db_data(name).cls[b, :F.db_data(name).case.n_valid[b]] > 0.5).sum())
    assert [movers("movers_255_256_257", b) for b in range(3)] == [255, 256, 257]
    for k in F.DBSCAN_CASES:
        d = F.db_data(k.name)
        for b in range(len(k.n_valid)):
            assert movers(k.name, b) <= 600 and d.num_objects[b] <= F.KMAX, (k.name, b)
    chain = F.db_data("chain_at_eps")
    assert chain.num_objects == [1, 2] and (chain.labels[0, :40] == 0).all()          # closed ball: spacing == eps joins
    assert float(chain.x[0, :40, 0].sort().values.diff().max()) == F.EPS and float(chain.x[1, :40, 0].sort().values.diff().max()) == 2.0
    ms1 = F.db_data("min_samples_1")
    for b in range(2):          # every mover is a cluster member, some clusters are singletons
        mv = ms1.cls[b, :ms1.case.n_valid[b]].numpy() > 0.5
        assert (ms1.labels[b, :ms1.case.n_valid[b]][mv] >= 0).all()
    assert (np.bincount(ms1.labels[0][ms1.labels[0] >= 0]) == 1).any()
    assert any((F.db_data("movers_255_256_257").labels[b] >= 0).any() for b in range(3))


# ------------------------------------------------------------------------------------------------
# statements against the shipped formulation
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.names(F.DESC_CASES))
def test_descriptor_statement_equals_the_shipped_formulation_in_float64(name):
    d = F.desc_data(name)
    k = d.case
    valid = d.obj.clone()
    for b in range(k.B):
        valid[b, k.n_valid[b]:] = -1
    dbl = [t.double() for t in (d.pc1, d.flow, d.feature1, d.prop)]
    live = [bool(a) for a in k.active] if k.active is not None else [True] * k.B
    per_object = F.descriptors_of(*dbl, valid, [c if a else 0 for c, a in zip(k.counts, live)])          # association.object_descriptor
    for b in range(k.B):
        if not live[b]:
            assert per_object[b] is None and torch.isnan(d.d64[b]).all()
            continue
        n = k.counts[b]
        assert F.rel(d.d64[b, :n], per_object[b]) <= 1e-13, (name, b)
        assert torch.equal(d.d64[b, :n, F.DESC_PROP], per_object[b][:, F.DESC_PROP])
        pf = torch.cat((dbl[0][b] + dbl[1][b], dbl[0][b], dbl[1][b], dbl[2][b], dbl[3][b]), 0)
        objs = [pf[:, torch.nonzero(valid[b] == j).reshape(-1)].unsqueeze(0) for j in range(n)]
        assert F.rel(d.d64[b, :n], A.batched_descriptors(objs)) <= 1e-13, (name, b)
        assert torch.isnan(d.d64[b, n:]).all()
        # float32 torch, the yardstick, is a float32 rounding away and no more
        for group, sl in F.DESC_GROUPS:
            assert F.rel(d.d32[b, :n, sl], d.d64[b, :n, sl]) <= 1e-5, (name, b, group)
        assert torch.equal(d.d32[b, :n, F.DESC_PROP].double(), d.d64[b, :n, F.DESC_PROP])
    single = F.desc_data("n_valid")
    assert (single.d64[0, 0, 3:6] == 0).all() and (single.d64[0, 0, 139:141] == 0).all()          # one point: variance exactly 0


def test_affinity_statement_equals_affinity_matrix():
    """association.affinity_matrix on objects whose descriptors are the case's: same pair order (i * n + j), same difference."""
    d = F.desc_data("n_valid")
    b, m, n = 3, 5, 9
    pf = torch.cat((d.pc1[b] + d.flow[b], d.pc1[b], d.flow[b], d.feature1[b], d.prop[b]), 0)
    objs = [pf[:, torch.nonzero(d.obj[b, :257] == k).reshape(-1)].unsqueeze(0) for k in range(m + n)]
    curr, prev = objs[:n], {100 + i: o for i, o in enumerate(objs[n:])}
    net = F.affinity_net("seeded")
    with torch.no_grad():
        aff_list, aff_mat, mm, nn = A.affinity_matrix(net, curr, prev)
    desc = A.batched_descriptors(objs)
    got, _ = F.affinity_f64(F.mlp_copy(net, torch.float32), desc[n:], m, desc[:n], n)
    assert (mm, nn) == (m, n) and aff_mat.shape == (1, m, n)
    assert torch.allclose(got, aff_mat[0], rtol=0, atol=1e-6) and torch.equal(aff_list.reshape(m, n), aff_mat[0])
    a64, _ = F.affinity_f64(F.mlp_copy(net, torch.float64), desc[n:], m, desc[:n], n)
    assert F.rel(aff_mat[0], a64) <= 1e-5 and float(a64.std()) > 0.05


def decision_streams():
    seen = []
    for g in F.DECISION_GROUPS:
        for s, counter in zip(g.streams, g.counters):
            mode, name, m, n = F.stream_spec(s)
            if mode == "live" and name is not None and (name, counter) not in seen:
                seen.append((name, counter))
    return seen + [("diag_126_127", 3)]


@pytest.mark.parametrize("name,counter", decision_streams())
def test_decision_statement_equals_sinkhorn_assignment_and_the_associator(name, counter):
    d = F.plan_data(name)
    m, n = d.case.m, d.case.n
    prev_ids = F.prev_ids_of(name, m)
    dec = F.decide_f64(d.p64, d.aff, prev_ids, counter)
    if m and n:
        shipped = A.sinkhorn_assignment(d.aff.double().unsqueeze(0))[0].tolist()          # on the CPU: the framework formulation
        assert shipped == dec.indices1, name
        assert F.rel(A.log_optimal_transport(d.aff.double().unsqueeze(0), torch.tensor(0.9), 500)[0], d.p64) == 0.0
    if max(m, n) <= 40:
        ids, confs, idx, max_id = F.associator_decision(d.aff, prev_ids, counter)
        assert ids == dec.ids and max_id == dec.counter, name
        assert confs == [float(c) for c in dec.conf], name
        assert idx is None and not (m and n) or idx == dec.indices1, name


# ------------------------------------------------------------------------------------------------
# margins and spread
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,counter", decision_streams())
def test_every_decision_case_is_decided_in_float64_by_a_margin(name, counter):
    d = F.plan_data(name)
    if d.p64 is None:
        return
    dec = F.decide_f64(d.p64, d.aff, F.prev_ids_of(name, d.case.m), counter)
    print("   %-16s float64 decision margin %.3e" % (name, dec.margin))
    if name not in F.TIES:
        assert dec.margin >= F.MARGIN, "%s: margin %.3e" % (name, dec.margin)
        return
    row, (c0, c1) = F.TIES[name]          # the deliberate tie: that row's two best are equal, everything else is decided
    assert dec.margin == 0.0 and dec.row_gap[row] == 0.0 and d.p64[row, c0] == d.p64[row, c1] == d.p64[row, :d.case.n].max()
    assert dec.col_gap.min() >= F.MARGIN and np.delete(dec.row_gap, row).min() >= F.MARGIN
    assert dec.indices1[c0] == row and dec.indices1[c1] == -1


def test_threshold_cases_sit_on_the_two_sides_of_float32_001():
    at, above = F.plan_data("threshold_at"), F.plan_data("threshold_above")
    assert float(at.aff[1, 1]) == F.THRESHOLD32 < 0.01 < float(above.aff[1, 1])
    assert np.nextafter(np.float32(at.aff[1, 1]), np.float32(1)) == np.float32(above.aff[1, 1])
    ids = F.prev_ids_of("threshold_at", 3)
    a, b = F.decide_f64(at.p64, at.aff, ids, 41), F.decide_f64(above.p64, above.aff, ids, 41)
    assert a.indices1 == b.indices1 == [0, 1, 2]
    assert a.ids == [ids[0], 41, ids[2]] and a.conf[1] == 0 and a.counter == 42
    assert b.ids == ids and b.conf[1] == above.aff[1, 1].numpy() and b.counter == 41


@pytest.mark.parametrize("name", [k.name for k in F.AFF_CASES if k.weights == "seeded"])
def test_seeded_affinity_spreads_its_logits(name):
    d = F.aff_data(name)
    logits = torch.cat([v.reshape(-1) for v in d.logit64.values()])
    print("   %-16s %d pairs, float64 logit std %.2f, affinities %.3f .. %.3f" % (
        name, logits.numel(), float(logits.std()), float(torch.sigmoid(logits).min()), float(torch.sigmoid(logits).max())))
    assert float(logits.std()) >= 1.0
    for b, a in d.a64.items():
        assert F.rel(d.a32[b], a) <= 1e-5


def test_reference_weights_hardly_spread():
    """Why the seeded weights exist: the reference state dict's affinities over unit-scale differences all lie near 0.5."""
    d = F.aff_data("reference_weights")
    a = torch.cat([v.reshape(-1) for v in d.a64.values()])
    assert 0.4 < float(a.min()) and float(a.max()) < 0.6


# ------------------------------------------------------------------------------------------------
# the bound has teeth: five wrong float32 variants
# ------------------------------------------------------------------------------------------------
def outside(wrong, g32, g64):
    return F.rel(wrong, g64) > F.bound(g32, g64)


def test_teeth_one_pass_variance():
    d = F.desc_data("far80")
    wrong = F.one_pass_descriptors32(d)
    n = d.case.counts[0]
    assert outside(wrong[0, :n, 3:6], d.d32[0, :n, 3:6], d.d64[0, :n, 3:6])
    assert not outside(d.d32[0, :n, 3:6], d.d32[0, :n, 3:6], d.d64[0, :n, 3:6])


def swapped_marginals_plan32(aff, alpha, iters):
    """log_optimal_transport with log m and log n exchanged in the dustbin marginals, float32."""
    m, n = aff.shape
    a = torch.tensor(float(np.float32(alpha)))
    Z = torch.cat([torch.cat([aff, a.expand(m, 1)], 1), a.expand(1, n + 1)], 0).unsqueeze(0)
    norm = -torch.tensor(float(m + n)).log()
    log_mu = torch.cat([norm.expand(m), torch.tensor(float(m)).log()[None] + norm])[None]
    log_nu = torch.cat([norm.expand(n), torch.tensor(float(n)).log()[None] + norm])[None]
    return (A.log_sinkhorn_iterations(Z, log_mu, log_nu, iters) - norm)[0]


def test_teeth_swapped_dustbin_marginals():
    d = F.plan_data("m40_n9")
    assert outside(swapped_marginals_plan32(d.aff, F.ALPHA, F.ITERS), d.p32, d.p64)
    sq = F.plan_data("m1_n1")          # with m == n the swap is no mistake: the variant is the plan
    assert not outside(swapped_marginals_plan32(sq.aff, F.ALPHA, F.ITERS), sq.p32, sq.p64)


def test_teeth_pair_order():
    d = F.aff_data("tile_edge")
    caught = 0
    for b, a32 in d.a32.items():
        m, n = d.m[b], d.n[b]
        wrong = a32.t().contiguous().reshape(m, n)          # pair (i, j) taken from row j * m + i
        if m > 1 and n > 1:
            assert outside(wrong, a32, d.a64[b]), b
            caught += 1
    assert caught >= 2


def last_argmax(x, axis):
    flipped = np.flip(x, axis=axis)
    return x.shape[axis] - 1 - np.argmax(flipped, axis=axis)


def test_teeth_ties_from_the_highest_index():
    d = F.plan_data("tie_17_33")
    ids = F.prev_ids_of("tie_17_33", 17)
    right, wrong = F.decide_f64(d.p64, d.aff, ids, 0), F.decide_f64(d.p64, d.aff, ids, 0, argmax=last_argmax)
    assert right.indices1 != wrong.indices1 and right.ids != wrong.ids
    assert wrong.indices1[20] == 5 and wrong.indices1[3] == -1


def test_teeth_threshold_as_a_float32_constant():
    d = F.plan_data("threshold_at")
    ids = F.prev_ids_of("threshold_at", 3)
    right, wrong = F.decide_f64(d.p64, d.aff, ids, 41), F.decide_f64(d.p64, d.aff, ids, 41, threshold=F.THRESHOLD32)
    assert right.ids != wrong.ids and wrong.ids == ids and wrong.counter == 41 and right.counter == 42
