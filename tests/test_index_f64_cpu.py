"""CPU: the ground tests/test_index_f64_gpu.py stands on (tests/_index_f64.py).  On every lattice case the float64 statements equal
the C oracle exactly, indices and distances; on every other case the oracle lies inside the derived band, and the band leaves at most
5 % of the queries of a cloud around the origin undecided (the far clusters are exempt by name: there the band is wide by construction
and the bit-for-bit comparison with the oracle is the assertion).  Every case has the properties it claims, the checkers reject a
wrong table, the dispatch mirror matches the sources and every limit has a case on each side."""
import pytest
import torch

from oracle import pointnet2_ref as P

import _index_f64 as I

C = I.C
WORST = {}      # form -> the oracle's largest excursion beyond the cut-off, in betas (printed: information for DESIGN 4.2)


def _cap(kind, fraction, what):
    if kind not in I.FAR_KINDS and kind != "far":
        assert fraction <= 0.05, "%s: %.3f of the queries are ambiguous: the band excuses too much" % (what, fraction)


# ------------------------------------------------------------------------------------------------
# the oracle against the statements
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", I.names(I.KNN_POINT_CASES))
def test_knn_point_oracle(name):
    case, p, q = I.knn_point_data(name)
    for k in case.ks:
        ref, dist = P.knn_point(k, p, q, with_dist=True)
        amb = I.verify_knn_point(ref, k, p, q, I.is_lattice(case.kind), what="%s k=%d" % (name, k))
        if I.is_lattice(case.kind):
            assert torch.equal(dist.double(), I.knn_point_f64(k, p, q)[1])
        else:
            _cap(case.kind, amb, "%s k=%d" % (name, k))
            _, _, d = I.knn_point_f64(k, p, q)
            beta = I.beta_expand(q, p, d)
            worst = I.check_k_band(ref, d, k, beta)
            WORST[case.kind] = max(WORST.get(case.kind, 0.0), worst)
            print("EXCURSION knn_point %s k=%d: %.3f beta (beta up to %.3e)" % (name, k, worst, float(beta.max())))


@pytest.mark.parametrize("padding", I.PADDINGS)
@pytest.mark.parametrize("name", I.names(I.MASKED_KNN_CASES))
def test_masked_knn_point_oracle(name, padding):
    case, p, q, nv = I.masked_knn_data(name, padding)
    ref = I.oracle_knn_point(case.k, p, q, nv)
    I.verify_knn_point(ref, case.k, p, q, I.is_lattice(case.kind), nv, name)
    for s, v in enumerate(case.n_valid):
        assert int(ref[s].max()) < max(v, case.k)                      # only valid candidates, or the first k rows
    other = I.oracle_knn_point(case.k, I.masked_knn_data(name, I.PADDINGS[1 - I.PADDINGS.index(padding)])[1], q, nv)
    enough = torch.tensor(case.n_valid) >= case.k
    assert torch.equal(ref[enough], other[enough])                     # with n_valid >= k the padding rows do not matter
    for s in (~enough).nonzero().flatten().tolist():                   # with fewer: the first k rows, whatever they hold
        assert ref[s].sort(-1).values.eq(torch.arange(case.k)).all() and other[s].sort(-1).values.eq(torch.arange(case.k)).all()
    assert case.n_valid == (1, case.k - 1, case.k, case.k + 1, case.n - 1, case.n)


@pytest.mark.parametrize("name", I.names(I.THREE_NN_CASES))
def test_three_nn_oracle(name):
    case, unknown, known = I.three_nn_data(name)
    d2, idx = P.three_nn(unknown, known)
    amb = I.verify_knn(idx, d2, 3, unknown, known, I.is_lattice(case.kind), what=name)
    _cap("random" if case.claims.get("narrow_band") else case.kind, amb, name)      # the direct form: narrow on a far cluster as well
    if case.known_nuniq:      # the duplicate-aware scan's premise: scanning the unique prefix plus the first two copies changes nothing
        for s, ke in enumerate(case.known_nuniq):
            assert bool((known[s, ke:] == known[s, 0]).all())
            short = torch.cat([known[s, :ke], known[s, ke:ke + 2]])[None]
            d2s, idxs = P.three_nn(unknown[s:s + 1], short.contiguous())
            assert torch.equal(idxs, idx[s:s + 1]) and torch.equal(d2s, d2[s:s + 1])


@pytest.mark.parametrize("name", I.names(I.KNN_CASES))
def test_knn_oracle(name):
    case, unknown, known = I.knn_data(name)
    for k in case.ks:
        d2, idx = P.knn(k, unknown, known)
        _cap(case.kind, I.verify_knn(idx, d2, k, unknown, known, I.is_lattice(case.kind), what="%s k=%d" % (name, k)), name)


@pytest.mark.parametrize("name", I.names(I.BALL_CASES))
def test_ball_query_oracle(name):
    case, xyz, new_xyz = I.ball_data(name)
    for r, ns in ((case.r1, case.ns1), (case.r2, case.ns2), (case.r2, I.BALL_SINGLE_NSAMPLE)):
        for prefill in (0, case.n - 1):
            ref = I.oracle_ball(r, ns, xyz, new_xyz, prefill)
            I.verify_ball(ref, r, ns, xyz, new_xyz, True, prefill, what="%s r=%g ns=%d" % (name, r, ns))


@pytest.mark.parametrize("name", I.names(I.GEO_CASES))
def test_geometry_oracle(name):
    """The tables of the two launches as the oracle builds them, level by level, against the float64 statements."""
    case, frames, nv = I.geo_data(name)
    xyz0 = torch.cat(frames)                                           # the distinct clouds only
    n_valid = nv.reshape(-1) if nv is not None else None
    B = case.unique if case.pairs else 0
    idx, levels, nuniq = I.geo_levels_oracle(xyz0, n_valid)
    for l in range(3):                                                 # nuniq as stated: the index list is exhausted exactly there
        for s in range(xyz0.shape[0]):
            nu = int(nuniq[l][s])
            assert I.distinct_rows(levels[l + 1][s]) == nu and bool((idx[l][s, nu:] == 0).all())
    tables, _ = I.geo_oracle_tables(levels, nuniq, B, n_valid, 1)
    lattice = case.kind in ("lattice", "grid")
    amb = I.verify_geo_tables(tables, levels, nuniq, B, n_valid, lattice, 1)
    if not lattice:
        for key, a in amb.items():
            print("AMBIGUOUS geometry %s %s: %.4f" % (name, key, a))
            if case.kind != "far" or not key.startswith("knn"):        # the direct form stays narrow on the far cluster too
                assert a <= 0.05, (key, a)


# ------------------------------------------------------------------------------------------------
# the cases have the properties they claim
# ------------------------------------------------------------------------------------------------
EXPECTED_CLAIMS = {
    "ball": {"n1": {"empty_ball"}, "n5": {"empty_ball", "rim_pairs"}, "n63": {"empty_ball", "rim_pairs", "full_balls", "partial_balls"},
             "n64": {"empty_ball", "rim_pairs", "full_balls", "partial_balls"},
             "n65": {"empty_ball", "rim_pairs", "r5_points", "first_hit_above", "full_balls"},
             "n300": {"empty_ball", "rim_pairs", "r5_points", "first_hit_above", "full_balls", "last_hit_mid_step"},
             "n300_wide": {"empty_ball", "rim_pairs", "first_hit_above", "full_balls", "partial_balls", "last_hit_mid_step"},
             "lds_at_limit": {"empty_ball", "rim_pairs"}, "lds_past_limit": {"empty_ball", "rim_pairs"}},
    "three_nn": {"m1": {"inf_slots"}, "m2": {"inf_slots"}, "m3": {"inf_slots"}, "m4": {"inf_slots"}, "ties": {"zero_distances", "three_way_ties"},
                 "masked": {"three_way_ties"}, "masked_random": set(), "lds_at_limit": set(), "lds_past_limit": set(), "random": set(),
                 "far5": {"narrow_band"}},
}


def test_claims_are_the_expected_ones():
    """A property taken out of the table fails here; a property the inputs lost fails in the tests below."""
    assert {k.name: set(k.claims) for k in I.BALL_CASES} == EXPECTED_CLAIMS["ball"]
    assert {k.name: set(k.claims) for k in I.THREE_NN_CASES} == EXPECTED_CLAIMS["three_nn"]
    tie = {k.name for k in I.KNN_POINT_CASES if "tie_at_16" in k.claims}
    assert tie == {k.name for k in I.KNN_POINT_CASES if k.kind == "lattice" and k.n >= I.STEP16 - 1 and k.s > 1} and len(tie) >= 6
    zero = {k.name for k in I.KNN_POINT_CASES if "zero_distances" in k.claims}
    assert zero == {k.name for k in I.KNN_POINT_CASES if k.kind == "far5" and k.n >= I.STEP16 - 1 and k.s > 1} and len(zero) >= 4
    assert {k.name: k.claims for k in I.GEO_CASES if k.claims} == {
        "lattice_n48": {"oversampled": True}, "lattice_n243": {"oversampled": True}, "lattice_n256": {"oversampled": True},
        "lattice_n300": {"oversampled": True}, "point_major_n300": {"oversampled": True}, "lattice_n512": {"all_chunks_live": True},
        "wgs_one": {"all_chunks_live": True}, "wgs_two": {"all_chunks_live": True}, "wgs_two_half_oversampled": {"all_chunks_live": False}}


@pytest.mark.parametrize("name", I.names(I.BALL_CASES))
def test_ball_cases_have_what_they_claim(name):
    case, xyz, new_xyz = I.ball_data(name)
    d = I.d2_direct(new_xyz, xyz)
    got = {}
    radii = (case.r1, case.r2)
    r2s = [I.radius2_f32(r) for r in radii]
    got["rim_pairs"] = sum(int((d == r2).sum()) for r2 in r2s)                                   # pairs exactly on a sphere
    got["empty_ball"] = min(int(((d < r2).sum(-1) == 0).sum()) for r2 in r2s)
    cnt = [((d < r2).sum(-1), ns) for r2, ns in zip(r2s, (case.ns1, case.ns2))]
    got["full_balls"] = sum(int((c > ns).sum()) for c, ns in cnt)                                # more hits than slots
    got["partial_balls"] = sum(int(((c > 0) & (c < ns)).sum()) for c, ns in cnt)
    hit = d < r2s[1]
    first = torch.where(hit.any(-1), hit.float().argmax(-1), torch.full(hit.shape[:2], -1))
    got["first_hit_above"] = int(first.max())
    # a radius whose exact square is not its fp32 square: the points between the two are decided by the rounded product
    got["r5_points"] = sum(int(((d < float(r) * float(r)) != (d < r2)).sum()) for r, r2 in zip(radii, r2s))
    rank = hit.long().cumsum(-1)
    last = ((rank == case.ns2) & hit).float().argmax(-1)[(hit.sum(-1) >= case.ns2)]             # index of the nsample-th hit
    got["last_hit_mid_step"] = int(((last >= 64) & (last % 64 >= 8) & (last % 64 < 56)).sum())
    for key, want in case.claims.items():
        assert got[key] >= want, (key, got[key], want)
    if "r5_points" in case.claims:
        assert I.R5 in radii and I.radius2_f32(I.R5) == 5.0 and I.R5 * I.R5 > 5.0 and int((d == 5.0).sum()) >= 20
    assert case.m % I.BALL_CHUNK != 0                                                              # the last chunk is partial
    if case.nuniq:
        assert sorted(case.nuniq) == sorted({1, 7, C.RTK_BALL_TAIL_ROWS, C.RTK_BALL_TAIL_ROWS + 1, case.m}) and len(case.nuniq) == case.b


@pytest.mark.parametrize("name", I.names(I.THREE_NN_CASES))
def test_three_nn_cases_have_what_they_claim(name):
    case, unknown, known = I.three_nn_data(name)
    d = I.d2_direct(unknown, known)
    v = d.sort(-1).values
    got = {"inf_slots": case.m < 3, "zero_distances": int((d == 0).sum())}
    got["three_way_ties"] = float((v[..., 2] == v[..., 3]).float().mean()) if case.m > 3 else 0.0      # third and fourth nearest tie
    c, _ = I.cutoff_of(d, min(3, case.m))
    got["narrow_band"] = float(I.beta_direct(c).max()) <= 12 * I.U * 3 * 0.05 ** 2
    for key, want in case.claims.items():
        assert got[key] >= want, (key, got[key], want)
    assert case.n % C.KV_QPW != 0 or case.n < C.KV_QPW
    if case.known_nuniq:
        assert case.known_nuniq == (1, 2, case.m - 2, case.m - 1, case.m)
        assert case.unknown_nuniq[:4] == (1, C.KV_QPW - 1, C.KV_QPW, C.KV_QPW + 1) and I.roundup(case.unknown_nuniq[4], C.KV_QPW) > case.n


@pytest.mark.parametrize("name", [k.name for k in I.KNN_POINT_CASES if k.claims])
def test_knn_point_cases_have_what_they_claim(name):
    case, p, q = I.knn_point_data(name)
    if "tie_at_16" in case.claims:
        v = I.d2_expand(q, p).sort(-1).values
        assert float((v[..., 15] == v[..., 16]).float().mean()) >= case.claims["tie_at_16"]
    if "zero_distances" in case.claims:      # the expansion formula far from the origin: the oracle's nearest distances collapse to 0
        _, dist = P.knn_point(16, p, q, with_dist=True)
        assert float((dist == 0).float().mean()) >= case.claims["zero_distances"]
        assert float((P.knn_point(16, p, q)[:, :min(case.s, case.n), 0] == torch.arange(min(case.s, case.n))).float().mean()) < 0.9


@pytest.mark.parametrize("name", I.names(I.GEO_CASES))
def test_geometry_cases_have_what_they_claim(name):
    case, xyz0, n_valid, B = I.geo_batch(name)
    S, n, _ = xyz0.shape
    assert S == I.geo_clouds(case) and (not case.pairs or S == 2 * B)
    nv = n_valid.tolist() if n_valid is not None else [n] * S
    distinct = [I.distinct_rows(xyz0[s, :nv[s]]) for s in range(min(S, 2 * case.unique))]
    if "oversampled" in case.claims:
        assert max(distinct) < I.NPOINT
    if case.claims.get("all_chunks_live") is True:
        assert min(distinct) == I.NPOINT == n
    if case.claims.get("all_chunks_live") is False:
        assert I.NPOINT in distinct and min(distinct) <= I.NPOINT // 8


# ------------------------------------------------------------------------------------------------
# the checkers reject a wrong table
# ------------------------------------------------------------------------------------------------
def test_checkers_reject_wrong_tables():
    case, p, q = I.knn_point_data("random_n%d_s%d" % (I.KNN_POINT_N[7], I.KNN_POINT_S[(7 + 1) % 4]))
    ref = P.knn_point(16, p, q)
    I.verify_knn_point(ref, 16, p, q, False)
    far = I.d2_expand(q, p).argmax(-1)
    bad = ref.clone(); bad[0, 0, 15] = far[0, 0]                      # a far candidate instead of the 16th
    with pytest.raises(I.Mismatch):
        I.verify_knn_point(bad, 16, p, q, False)
    bad = ref.clone(); bad[0, 0, 15] = bad[0, 0, 14]                   # one candidate twice
    with pytest.raises(I.Mismatch):
        I.verify_knn_point(bad, 16, p, q, False)
    bad = ref.clone(); bad[0, 0] = bad[0, 0].flip(-1)                  # descending
    with pytest.raises(I.Mismatch):
        I.verify_knn_point(bad, 16, p, q, False)
    # lattice: the tie order is part of the statement
    case, p, q = I.knn_point_data("lattice_n%d_s%d" % (I.KNN_POINT_N[7], I.KNN_POINT_S[(7 + 0) % 4]))
    ref, dist = P.knn_point(16, p, q, with_dist=True)
    b, s, a = (dist[..., 1:] == dist[..., :-1]).nonzero()[0].tolist()
    bad = ref.clone(); bad[b, s, a], bad[b, s, a + 1] = ref[b, s, a + 1], ref[b, s, a]
    with pytest.raises(I.Mismatch):
        I.verify_knn_point(bad, 16, p, q, True)
    # ball query on a cloud that is no lattice: a point outside, a skipped point inside, a wrong filler
    gen = I._gen("checker")
    xyz, new_xyz = I.cloud(gen, "random", 2, 200), I.cloud(gen, "random", 2, 30)
    ref = P.ball_query(6.0, 8, xyz, new_xyz)
    I.verify_ball(ref, 6.0, 8, xyz, new_xyz, False)
    d = I.d2_direct(new_xyz, xyz)
    b, m = ((d < 36.0).sum(-1) >= 3).nonzero()[0].tolist()
    for slot, value in ((1, int(d[b, m].argmax())), (0, int(ref[b, m, 1]))):
        bad = ref.clone(); bad[b, m, slot] = value
        with pytest.raises(I.Mismatch):
            I.verify_ball(bad, 6.0, 8, xyz, new_xyz, False)
    # the rim is strict: a statement with <= differs on a lattice case
    case, xyz, new_xyz = I.ball_data("n300")
    d = I.d2_direct(new_xyz, xyz)
    loose = I.ball_from_d2(d - 0.5, I.radius2_f32(case.r1), case.ns1)      # integers: d - 0.5 < r2  <=>  d <= r2
    with pytest.raises(I.Mismatch):
        I.verify_ball(loose, case.r1, case.ns1, xyz, new_xyz, True)
    # tails
    t = torch.full((1, 70, 4), 9, dtype=torch.int32); t[0, :7] = 3; t[0, 7:32] = 0
    I.verify_pair_tail(t, [7], 9, "tail")
    for row in (31, 32):
        bad = t.clone(); bad[0, row, 0] = 5
        with pytest.raises(I.Mismatch):
            I.verify_pair_tail(bad, [7], 9, "tail")


# ------------------------------------------------------------------------------------------------
# the dispatch mirror
# ------------------------------------------------------------------------------------------------
def test_source_texts_still_stand():
    src = I._read(I.OPS_SOURCE)
    for text in I.SOURCE_TEXTS:
        assert text in src, text
    assert C.KV_QPW * C.KV_LPQ == 256 and C.KV_QPW % C.RTK_INTERP_ROW_GROUP == 0
    assert [p for _, p in C.FPS_PPL] == [lim for lim, _ in C.FPS_PPL] and len(C.FPS_PPL) == 4
    assert [p for _, p in C.FRONT_PPL] == [p for _, p in C.FPS_PPL] and C.FRONT_PPL[-1][0] is None
    assert 64 * C.FPS_PPL[-1][0] == 2048                               # RTK_REQUIRE(n <= 2048 ...) of rtk_geometry_front
    from ratrack_amd import fused
    assert tuple(map(tuple, fused._PNHeadWeights.RADII)) == I.RADII and tuple(map(tuple, fused._PNHeadWeights.NSAMPLES)) == I.NSAMPLES


def test_every_limit_has_a_case_on_each_side():
    kp = [(k, case.n, case.s) for case in I.KNN_POINT_CASES for k in case.ks]
    inst = {I.knn_point_instance(k, n) for k, n, _ in kp}
    assert inst == {(kern, K, lds) for kern, K in (("select", 0), ("sort", 16), ("sort", 32)) for lds in (True, False)}
    for k_lo, k_hi in ((16, 17), (32, 33)):                            # k = 16 | 17 and 32 | 33 switch instance
        assert I.knn_point_instance(k_lo, 64)[:2] != I.knn_point_instance(k_hi, 64)[:2]
        assert {k_lo, k_hi} <= {k for k, _, _ in kp}
    assert I.knn_point_instance(16, I.KNN_LDS_MAX)[2] and not I.knn_point_instance(16, I.KNN_LDS_MAX + 1)[2]
    for k in (16, 33):
        assert {(k, I.KNN_LDS_MAX), (k, I.KNN_LDS_MAX + 1)} <= {(kk, n) for kk, n, _ in kp}
    for k, step in ((16, I.STEP16), (32, I.STEP32)):                   # the trip count of the candidate loop: 1 | 2 and 2 | 3 at the step
        trips = {n: I.knn_point_steps(k, n) for kk, n, _ in kp if kk == k and n <= 300}
        for n in (step - 1, step, step + 1):
            assert n in trips
        assert trips[step] + 1 == trips[step + 1] and trips[step - 1] == trips[step]
    ss = {s for _, _, s in kp}
    assert {1, C.KV_QPW - 1, C.KV_QPW, C.KV_QPW + 1} <= ss              # a partial chunk, a full one, one query in a second chunk
    # ball query / three-NN: the LDS switch, the chunk of centroids, the chunk of queries
    assert I.ball_lds(I.BALL_LDS_MAX) and not I.ball_lds(I.BALL_LDS_MAX + 1)
    assert {I.BALL_LDS_MAX, I.BALL_LDS_MAX + 1} <= {k.n for k in I.BALL_CASES} and {I.BALL_LDS_MAX, I.BALL_LDS_MAX + 1} <= {k.m for k in I.THREE_NN_CASES}
    assert {1, 5, 63, 64, 65, 300} <= {k.n for k in I.BALL_CASES}
    assert all(k.m % I.BALL_CHUNK for k in I.BALL_CASES) and {k.m < I.BALL_CHUNK * 2 for k in I.BALL_CASES} == {True, False}
    assert {1, 2, 3, 4} <= {k.m for k in I.THREE_NN_CASES}
    # FPS instances of the front launch and the workgroup counts of the tables launch
    ns = {k.n for k in I.GEO_CASES}
    assert {16, 48, 243, 256, 300, 512, 513} <= ns
    assert {I.fps_ppl(n, C.FRONT_PPL) for n in ns} >= {4, 8, 16} and I.fps_ppl(256) != I.fps_ppl(300) and I.fps_ppl(512) != I.fps_ppl(513)
    one, two, few = I.geometry_cloud_counts()
    assert I.tables_workgroups(one, 512)[0] == 1 and I.tables_workgroups(one - 2, 512)[0] == 2
    assert I.tables_workgroups(two, 512)[0] == 2
    want, ball_wgs, ball_chunks, nn_wgs, nn_chunks = I.tables_workgroups(few, 512)
    assert want >= ball_chunks == ball_wgs and nn_wgs == nn_chunks
    counts = {I.geo_clouds(k) for k in I.GEO_CASES}
    assert {one, two, few} <= counts
    mid = [I.tables_workgroups(c, 512) for c in counts if c not in (one, two, few)]
    assert any(1 < w[1] < w[2] for w in mid)                            # and the small batches: a few chunks per workgroup


def test_statements_on_hand_made_inputs():
    """The statements themselves, on inputs small enough to read."""
    xyz = torch.tensor([[[0., 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 1], [1, 0, 0]]])
    q = torch.tensor([[[0., 0, 0], [9, 9, 9]]])
    idx, cnt, _ = I.ball_query_f64(2.0, 3, xyz, q, prefill=7)           # (0,2,0) is on the rim of r = 2: not a hit
    assert idx.tolist() == [[[0, 1, 3], [7, 7, 7]]] and cnt.tolist() == [[4, 0]]
    idx, _, _ = I.ball_query_f64(1.0, 4, xyz, q)
    assert idx.tolist() == [[[0, 0, 0, 0], [0, 0, 0, 0]]]
    i3, d3, _ = I.three_nn_f64(q, xyz)
    assert i3[0, 0].tolist() == [0, 1, 3] and d3[0, 0].tolist() == [0.0, 1.0, 1.0]      # ties -> earlier index: 1, 3 before 4
    i3, d3, _ = I.three_nn_f64(q, xyz[:, :2])
    assert i3[0, 0].tolist() == [0, 1, 0] and d3[0, 0, 2] == float("inf")
    ik, _, _ = I.knn_point_f64(2, xyz, q, torch.tensor([1], dtype=torch.int32))          # n_valid < k: the first k rows
    assert ik[0, 0].tolist() == [0, 1]
    ik, _, _ = I.knn_point_f64(2, xyz, q, torch.tensor([3], dtype=torch.int32))
    assert ik[0, 1].tolist() == [2, 1]
    assert I.radius2_f32(I.R5) == 5.0
