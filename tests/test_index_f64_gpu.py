"""GPU: every index-table kernel of ops_pointnet2.hip -- ball query, three-NN, kNN, kNN-point, their masked / paired forms, and the two
product launches rtk_geometry_front / rtk_geometry_tables -- against the float64 statements of tests/_index_f64.py (torch.equal on
integer lattices, the derived band elsewhere; validated without a GPU by tests/test_index_f64_cpu.py) and against the C oracle bit for
bit.  Output buffers are pre-filled with an in-range sentinel index and NaN distances: an unwritten row shows, and the rows a contract
leaves alone must keep the sentinel."""
import pytest
import torch

from oracle import pointnet2_ref as P
from ratrack_amd import _lib
from ratrack_amd import fused as F
from ratrack_amd.abi import stream

import _index_f64 as I

pytestmark = pytest.mark.gpu
DEV = "cuda"
C = I.C


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _i32(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV) if values is not None else None


def _bits_equal(got, ref, what, rows=None):
    """Same bits (NaN-safe), on the rows `rows` (leading dims bool mask) or everywhere."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    if got.dtype.is_floating_point:
        got, ref = got.contiguous().view(torch.int32), ref.contiguous().view(torch.int32)
    if rows is not None:
        got, ref = got[rows], ref[rows]
    assert torch.equal(got, ref), "%s: not the oracle's bits (%d entries differ)" % (what, int((got != ref).sum()))


# ------------------------------------------------------------------------------------------------
# ball query: the single-table entry point and the pair
# ------------------------------------------------------------------------------------------------
def _ball_query(xyz, new_xyz, r, ns, sentinel):
    (b, n, _), m = xyz.shape, new_xyz.shape[1]
    idx = torch.full((b, m, ns), sentinel, dtype=torch.int32, device=DEV)
    _lib.call("rtk_ball_query", b, n, m, float(r), ns, new_xyz.data_ptr(), xyz.data_ptr(), idx.data_ptr(), stream())
    return idx.cpu()


@pytest.mark.parametrize("name", I.names(I.BALL_CASES))
def test_ball_query(name):
    """rtk_ball_query at both radii and with nsample = 7: an empty ball keeps the caller's row."""
    case, xyz, new_xyz = I.ball_data(name)
    x, q, sentinel = xyz.to(DEV), new_xyz.to(DEV), case.n - 1
    for r, ns in ((case.r1, case.ns1), (case.r2, case.ns2), (case.r2, I.BALL_SINGLE_NSAMPLE)):
        got = _ball_query(x, q, r, ns, sentinel)
        I.verify_ball(got, r, ns, xyz, new_xyz, True, sentinel, what="%s r=%g ns=%d" % (name, r, ns))
        _bits_equal(got, I.oracle_ball(r, ns, xyz, new_xyz, sentinel), name)
        if case.n > 1:
            assert bool((got[:, 0] == sentinel).all())                 # centroid 0: the empty ball


@pytest.mark.parametrize("name", I.names(I.BALL_CASES))
def test_ball_query_pair(name):
    """rtk_ball_query_pair without and with the duplicate-centroid counter: rows below it hold both tables (an empty ball zeros), the
    rows up to the next multiple of RTK_BALL_TAIL_ROWS read as zeros, the rows beyond keep the sentinel."""
    case, xyz, new_xyz = I.ball_data(name)
    x, q, fill = xyz.to(DEV), new_xyz.to(DEV), case.n - 1
    for nuniq in ((None, case.nuniq) if case.nuniq else (None,)):
        a = torch.full((case.b, case.m, case.ns1), fill, dtype=torch.int32, device=DEV)
        b = torch.full((case.b, case.m, case.ns2), fill, dtype=torch.int32, device=DEV)
        args = (case.b, case.n, case.m, float(case.r1), case.ns1, float(case.r2), case.ns2, q.data_ptr(), x.data_ptr(), a.data_ptr(), b.data_ptr(),
                _ptr(_i32(nuniq)), stream())
        if not I.ball_lds(case.n):                                     # the pair has no unstaged instance: refused, nothing written
            with pytest.raises(_lib.RtkError, match="too large"):
                _lib.call("rtk_ball_query_pair", *args)
            torch.cuda.synchronize()
            assert bool((a == fill).all()) and bool((b == fill).all())
            continue
        _lib.call("rtk_ball_query_pair", *args)
        live = I.rows_below(nuniq, case.m) if nuniq else None
        for got, r, ns in ((a.cpu(), case.r1, case.ns1), (b.cpu(), case.r2, case.ns2)):
            what = "%s r=%g ns=%d nuniq=%s" % (name, r, ns, nuniq)
            I.verify_ball(got, r, ns, xyz, new_xyz, True, 0, live, what)
            I.verify_pair_tail(got, nuniq if nuniq else [case.m] * case.b, fill, what)
            _bits_equal(got, P.ball_query(r, ns, xyz, new_xyz), what, live if live is not None else None)


# ------------------------------------------------------------------------------------------------
# three-NN and the exported kNN (direct form)
# ------------------------------------------------------------------------------------------------
def _three_nn(unknown, known, sentinel, masked=None):
    (b, n, _), m = unknown.shape, known.shape[1]
    d2 = torch.full((b, n, 3), float("nan"), device=DEV)
    idx = torch.full((b, n, 3), sentinel, dtype=torch.int32, device=DEV)
    if masked is None:
        _lib.call("rtk_three_nn", b, n, m, unknown.data_ptr(), known.data_ptr(), d2.data_ptr(), idx.data_ptr(), stream())
    else:
        uu, kk = _i32(masked[0]), _i32(masked[1])
        _lib.call("rtk_three_nn_masked", b, n, m, unknown.data_ptr(), known.data_ptr(), d2.data_ptr(), idx.data_ptr(), _ptr(uu), _ptr(kk), stream())
    return d2.cpu(), idx.cpu()


@pytest.mark.parametrize("name", I.names(I.THREE_NN_CASES))
def test_three_nn(name):
    """rtk_three_nn, and rtk_three_nn_masked with neither, one and both counters: the full scan's table on the rows below
    unknown_nuniq, nothing written from the next multiple of KV_QPW on."""
    case, unknown, known = I.three_nn_data(name)
    u, k, sentinel = unknown.to(DEV), known.to(DEV), case.m - 1
    lattice = I.is_lattice(case.kind)
    rd2, ridx = P.three_nn(unknown, known)
    variants = [None, (None, None)]
    if case.known_nuniq:
        variants += [(None, case.known_nuniq), (case.unknown_nuniq, None), (case.unknown_nuniq, case.known_nuniq)]
    for masked in variants:
        d2, idx = _three_nn(u, k, sentinel, masked)
        what = "%s masked=%s" % (name, masked)
        limit = masked[0] if masked and masked[0] else None
        live = I.rows_below(limit, case.n) if limit else None
        I.verify_knn(idx, d2, 3, unknown, known, lattice, live, what)
        _bits_equal(idx, ridx, what, live)
        _bits_equal(d2, rd2, what, live)
        if limit:
            I.verify_three_nn_tail(idx, d2, limit, case.m, sentinel, what)
    if case.m < 3:
        assert bool(torch.isinf(d2[..., case.m:]).all()) and bool((idx[..., case.m:] == 0).all())


@pytest.mark.parametrize("name", I.names(I.KNN_CASES))
def test_knn(name):
    case, unknown, known = I.knn_data(name)
    u, kn = unknown.to(DEV), known.to(DEV)
    for k in case.ks:
        d2 = torch.full((case.b, case.n, k), float("nan"), device=DEV)
        idx = torch.full((case.b, case.n, k), case.m - 1, dtype=torch.int32, device=DEV)
        _lib.call("rtk_knn", case.b, case.n, case.m, k, u.data_ptr(), kn.data_ptr(), d2.data_ptr(), idx.data_ptr(), stream())
        d2, idx = d2.cpu(), idx.cpu()
        what = "%s k=%d" % (name, k)
        I.verify_knn(idx, d2, k, unknown, known, I.is_lattice(case.kind), what=what)
        rd2, ridx = P.knn(k, unknown, known)
        _bits_equal(idx, ridx, what)
        _bits_equal(d2, rd2, what)


# ------------------------------------------------------------------------------------------------
# kNN-point (expansion form)
# ------------------------------------------------------------------------------------------------
def _knn_point(k, points, query, n_valid=None, masked=False):
    (b, n, _), s = points.shape, query.shape[1]
    idx = torch.full((b, s, k), n - 1, dtype=torch.int64, device=DEV)
    if masked:
        _lib.call("rtk_knn_point_masked", b, s, n, k, query.data_ptr(), points.data_ptr(), idx.data_ptr(), _ptr(n_valid), stream())
    else:
        _lib.call("rtk_knn_point", b, s, n, k, query.data_ptr(), points.data_ptr(), idx.data_ptr(), stream())
    return idx.cpu()


@pytest.mark.parametrize("name", I.names(I.KNN_POINT_CASES))
def test_knn_point(name):
    """Every k of the case (both sorting instances, the selection kernel, k = n) on one cloud."""
    case, p, q = I.knn_point_data(name)
    pd, qd = p.to(DEV), q.to(DEV)
    for k in case.ks:
        got = _knn_point(k, pd, qd)
        what = "%s k=%d" % (name, k)
        I.verify_knn_point(got, k, p, q, I.is_lattice(case.kind), what=what)
        _bits_equal(got, P.knn_point(k, p, q), what)
    k = case.ks[0]                                                     # the masked entry point without a mask, and with one that masks nothing
    full = torch.full((case.b,), case.n, dtype=torch.int32, device=DEV)
    plain = _knn_point(k, pd, qd)
    assert torch.equal(_knn_point(k, pd, qd, None, True), plain) and torch.equal(_knn_point(k, pd, qd, full, True), plain)


@pytest.mark.parametrize("name", I.names(I.MASKED_KNN_CASES))
def test_knn_point_masked(name):
    """n_valid = 1, k - 1, k, k + 1, n - 1, n within one batch; padding rows as copies of row 0 and as points far away.  With
    n_valid >= k the result does not depend on which; with fewer the candidates are the first k rows, as the header says."""
    got = {}
    for padding in I.PADDINGS:
        case, p, q, nv = I.masked_knn_data(name, padding)
        got[padding] = _knn_point(case.k, p.to(DEV), q.to(DEV), nv.to(DEV), True)
        what = "%s %s" % (name, padding)
        I.verify_knn_point(got[padding], case.k, p, q, I.is_lattice(case.kind), nv, what)
        _bits_equal(got[padding], I.oracle_knn_point(case.k, p, q, nv), what)
    enough = nv >= case.k
    assert torch.equal(got["copies"][enough], got["garbage"][enough])
    for s in (~enough).nonzero().flatten().tolist():
        for g in got.values():
            assert bool(g[s].sort(-1).values.eq(torch.arange(case.k)).all())


# ------------------------------------------------------------------------------------------------
# the two product launches, through fused.Geometry
# ------------------------------------------------------------------------------------------------
POISON = 1      # an in-range index for every table (n >= 16): what the launches do not write keeps it


def _tables(geo):
    t = {}
    for l in range(3):
        for s in range(2):
            t["ball%d%d" % (l, s)] = geo.ball[l][s].cpu()
    for name, (d2, idx, _) in geo.nn.items():
        t["nn_idx_" + name], t["nn_d2_" + name] = idx.cpu(), d2.cpu()
    if geo.knn is not None:
        t["knn12"], t["knn11"] = geo.knn[0].cpu(), geo.knn[1].cpu()
    return t


@pytest.mark.parametrize("name", I.names(I.GEO_CASES))
def test_geometry_launches(name, monkeypatch):
    """rtk_geometry_front + rtk_geometry_tables on an index workspace filled with POISON: the FPS levels against the oracle, then every
    table against the float64 statements and the oracle, built level by level from the centroids the launch itself returned; the rows
    past the duplicate-centroid counters as the contracts say.  Batches of repeated clouds (the workgroup counts of the tables launch
    need up to 228 of them) are judged on the distinct clouds, and every repeat must equal its original."""
    case, xyz0, n_valid, B = I.geo_batch(name)
    S, n, _ = xyz0.shape
    per, frames = (B, 2) if B else (S, 1)
    want, ball_wgs, ball_chunks, nn_wgs, nn_chunks = I.tables_workgroups(S, n)
    if case.clouds in ("one", "two"):
        assert ball_wgs == want == {"one": 1, "two": 2}[case.clouds] and ball_chunks // ball_wgs >= 32      # a workgroup walks its chunks
    monkeypatch.setattr(F, "GEOMETRY_POISON", POISON)
    nv = n_valid.to(DEV) if n_valid is not None else None
    if case.pairs:       # the API's channel-major frames, converted by the front launch
        pc1, pc2 = (x.permute(0, 2, 1).contiguous().to(DEV) for x in (xyz0[:B], xyz0[B:]))
        f1, f2 = torch.zeros(B, 2, n, device=DEV), torch.zeros(B, 2, n, device=DEV)
        xyz = torch.full((S, n, 3), float("nan"), device=DEV)
        raw = torch.empty(S * n, 4, device=DEV)
        geo = F.Geometry(xyz, I.NPOINT, knn_frames=B, n_valid=nv, prepare=(pc1, pc2, f1, f2, raw))
    else:
        xyz = xyz0.to(DEV)
        geo = F.Geometry(xyz, I.NPOINT, n_valid=nv)
    torch.cuda.synchronize()
    assert geo.fused_geometry
    _bits_equal(xyz.cpu(), xyz0, "xyz")
    levels = [xyz0] + [x.cpu() for x in geo.xyz[1:]]
    nuniq = [c.cpu() for c in geo.nuniq]
    fps_idx = [i.cpu() for i in geo.fps_idx]
    t = _tables(geo)
    # repeats equal their originals
    rep = torch.cat([torch.arange(per) % case.unique + f * per for f in range(frames)])
    for key, tab in list(t.items()) + [("xyz%d" % l, levels[l]) for l in (1, 2, 3)] + [("fps%d" % l, fps_idx[l]) for l in range(3)]:
        r = rep[:tab.shape[0]]
        assert torch.equal(tab.view(torch.int32) if tab.dtype == torch.float32 else tab, (tab.view(torch.int32) if tab.dtype == torch.float32 else tab)[r]), key
    # the distinct clouds: frame by frame the first `unique`
    keep = torch.cat([torch.arange(case.unique) + f * per for f in range(frames)])
    sub = lambda x: x[keep[:case.unique] if x.shape[0] == B and B != S else keep] if x is not None else None
    lv, nu, nvs, Bs = [sub(x) for x in levels], [sub(c) for c in nuniq], sub(n_valid), (case.unique if B else 0)
    ridx, rlevels, rnuniq = I.geo_levels_oracle(lv[0], nvs)
    for l in range(3):
        assert torch.equal(sub(fps_idx[l]), ridx[l]), "FPS level %d" % (l + 1)
        _bits_equal(lv[l + 1], rlevels[l + 1], "centroids of level %d" % (l + 1))
        assert torch.equal(nu[l], rnuniq[l]), "nuniq of level %d" % (l + 1)
    ts = {key: sub(tab) for key, tab in t.items()}
    lattice = case.kind in ("lattice", "grid")
    I.verify_geo_tables(ts, lv, nu, Bs, nvs, lattice, POISON)
    oracle, rows = I.geo_oracle_tables(lv, nu, Bs, nvs, POISON)
    assert oracle.keys() == ts.keys()
    for key in ts:
        _bits_equal(ts[key], oracle[key], "%s %s" % (name, key), rows[key])
