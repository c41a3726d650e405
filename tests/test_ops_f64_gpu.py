"""GPU: every gather / group / interpolate kernel instance of ops_pointnet2.hip against the float64 statements and derived bounds of
tests/_ops_f64.py (validated without a GPU by tests/test_ops_f64_cpu.py).  Every gradient case runs through the `_set` entry point
onto a NaN-filled buffer and through the accumulating pointnet2_hip wrapper onto a random prefill.  Each test prints its largest
error / bound (information only: the bound is derived, not measured)."""
import pytest
import torch

from oracle import pointnet2_ref as P
from ratrack_amd import _lib, pointnet2_hip
from ratrack_amd import pointnet2_utils as PU
from ratrack_amd.abi import stream

import _ops_f64 as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _report(op, name, mode, ratio):
    print("RATIO %s %s %s %.4f" % (op, name, mode, ratio))


# ------------------------------------------------------------------------------------------------
# gradients: both entry points
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", O.MODES)
@pytest.mark.parametrize("name", O.names(O.GROUP_GRAD_CASES))
def test_group_points_grad(name, mode):
    d = O.group_grad_data(name)
    k = d.case
    go, idx = d.go.to(DEV), d.idx.to(DEV)
    if mode == "set":
        out = torch.full((k.b, k.c, k.n), float("nan"), device=DEV)
        _lib.call("rtk_group_points_grad_set", k.b, k.c, k.n, k.npoint, k.nsample, go.data_ptr(), idx.data_ptr(), out.data_ptr(), stream())
        ratio = O.check_scatter(out.cpu(), d.st)
    else:
        out = d.prefill.to(DEV)
        pointnet2_hip.group_points_grad_wrapper(k.b, k.c, k.n, k.npoint, k.nsample, go, idx, out)
        ratio = O.check_scatter(out.cpu(), d.st, d.prefill)
    _report("group_points_grad", name, mode, ratio)


@pytest.mark.parametrize("mode", O.MODES)
@pytest.mark.parametrize("name", O.names(O.INTERPOLATE_GRAD_CASES))
def test_three_interpolate_grad(name, mode):
    d = O.interpolate_grad_data(name)
    k = d.case
    go, idx, w = d.go.to(DEV), d.idx.to(DEV), d.w.to(DEV)
    if mode == "set":
        out = torch.full((k.b, k.c, k.m), float("nan"), device=DEV)
        _lib.call("rtk_three_interpolate_grad_set", k.b, k.c, k.n, k.m, go.data_ptr(), idx.data_ptr(), w.data_ptr(), out.data_ptr(), stream())
        ratio = O.check_scatter(out.cpu(), d.st)
    else:
        out = d.prefill.to(DEV)
        pointnet2_hip.three_interpolate_grad_wrapper(k.b, k.c, k.n, k.m, go, idx, w, out)
        ratio = O.check_scatter(out.cpu(), d.st, d.prefill)
    _report("three_interpolate_grad", name, mode, ratio)


@pytest.mark.parametrize("name", O.names(O.GATHER_CASES))
def test_gather_points_and_grad(name):
    """Forward: a copy.  Gradient (accumulate is its only form): onto a random prefill, unreferenced addresses keep their bits."""
    d = O.gather_data(name)
    k = d.case
    idx = d.idx.to(DEV)
    out = torch.full((k.b, k.c, k.npoint), float("nan"), device=DEV)
    pointnet2_hip.gather_points_wrapper(k.b, k.c, k.n, k.npoint, d.points.to(DEV), idx, out)
    O.check_copy(out.cpu(), d.points, d.idx)
    grad = d.prefill.to(DEV)
    pointnet2_hip.gather_points_grad_wrapper(k.b, k.c, k.n, k.npoint, d.go.to(DEV), idx, grad)
    _report("gather_points_grad", name, "accumulate", O.check_scatter(grad.cpu(), d.st, d.prefill))


# ------------------------------------------------------------------------------------------------
# forwards
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", O.names(O.GROUP_CASES))
def test_group_points(name):
    d = O.group_data(name)
    k = d.case
    out = torch.full((k.b, k.c, k.npoint, k.nsample), float("nan"), device=DEV)
    pointnet2_hip.group_points_wrapper(k.b, k.c, k.n, k.npoint, k.nsample, d.points.to(DEV), d.idx.to(DEV), out)
    O.check_copy(out.cpu(), d.points, d.idx)


@pytest.mark.parametrize("name", O.names(O.INTERPOLATE_CASES))
def test_three_interpolate(name):
    """Both instances: the oracle's bits, and within gamma_3 * sum|w_i p_i| of the float64 sum."""
    d = O.interpolate_data(name)
    k = d.case
    out = torch.full((k.b, k.c, k.n), float("nan"), device=DEV)
    pointnet2_hip.three_interpolate_wrapper(k.b, k.c, k.m, k.n, d.points.to(DEV), d.idx.to(DEV), d.w.to(DEV), out)
    ratio = O.check_interpolate(out.cpu(), d.points, d.idx, d.w, P.three_interpolate(d.points, d.idx, d.w))
    _report("three_interpolate", name, "forward", ratio)


# ------------------------------------------------------------------------------------------------
# limits: refused on the host, nothing written
# ------------------------------------------------------------------------------------------------
def _limit_calls():
    """(entry point, call taking the output buffer, output elements per channel) at b = n = m = npoint = nsample = 1."""
    C = 65536
    f = torch.zeros(C, device=DEV)                        # any (1, C, 1) float input
    i1 = torch.zeros(1, dtype=torch.int32, device=DEV)
    i3 = torch.zeros(3, dtype=torch.int32, device=DEV)
    w3 = torch.ones(3, device=DEV)
    s = stream()
    raw = lambda name, *a: (lambda out: _lib.call(name, *[x.data_ptr() if torch.is_tensor(x) else x for x in a], out.data_ptr(), s))
    return C, [
        ("gather_points_wrapper", lambda out: pointnet2_hip.gather_points_wrapper(1, C, 1, 1, f, i1, out)),
        ("gather_points_grad_wrapper", lambda out: pointnet2_hip.gather_points_grad_wrapper(1, C, 1, 1, f, i1, out)),
        ("group_points_wrapper", lambda out: pointnet2_hip.group_points_wrapper(1, C, 1, 1, 1, f, i1, out)),
        ("group_points_grad_wrapper", lambda out: pointnet2_hip.group_points_grad_wrapper(1, C, 1, 1, 1, f, i1, out)),
        ("rtk_group_points_grad_set", raw("rtk_group_points_grad_set", 1, C, 1, 1, 1, f, i1)),
        ("three_interpolate_wrapper", lambda out: pointnet2_hip.three_interpolate_wrapper(1, C, 1, 1, f, i3, w3, out)),
        ("three_interpolate_grad_wrapper", lambda out: pointnet2_hip.three_interpolate_grad_wrapper(1, C, 1, 1, f, i3, w3, out)),
        ("rtk_three_interpolate_grad_set", raw("rtk_three_interpolate_grad_set", 1, C, 1, 1, f, i3, w3)),
    ]


def test_channel_limit_is_refused_before_any_launch():
    """c = 65536 exceeds the grid's y extent: every entry point of the family raises and leaves its output buffer as it was."""
    C, calls = _limit_calls()
    for name, call in calls:
        out = torch.full((C,), 12345.0, device=DEV)
        with pytest.raises(_lib.RtkError, match="exceed grid limits"):
            call(out)
        torch.cuda.synchronize()
        assert bool((out == 12345.0).all()), name


# ------------------------------------------------------------------------------------------------
# autograd front-ends: non-contiguous cotangents, int64 neighbour indices
# ------------------------------------------------------------------------------------------------
def _backward(out, cotangent):
    """cotangent None: out.sum().backward() (an expanded gradient); else a weighted sum in a permuted layout, whose gradient w.r.t.
    out is `cotangent` seen through a permutation -- non-contiguous."""
    if cotangent is None:
        out.sum().backward()
    else:
        dims = list(range(out.dim()))[::-1]
        (out.permute(dims) * cotangent.to(out.device).permute(dims).contiguous()).sum().backward()


@pytest.mark.parametrize("cotangent", ["expanded", "permuted"])
def test_grouping_operation_frontend(cotangent):
    d = O.group_grad_data("cpb4_vec4_ball")
    k = d.case
    feats = torch.randn(k.b, k.c, k.n, generator=torch.Generator().manual_seed(1))
    f = feats.to(DEV).requires_grad_(True)
    idx64 = d.idx.long().to(DEV)                                       # what knn_point returns
    out = PU.grouping_operation(f, idx64)
    O.check_copy(out.detach().cpu(), feats, d.idx)
    go = torch.ones_like(d.go) if cotangent == "expanded" else d.go
    _backward(out, None if cotangent == "expanded" else go)
    _report("grouping_operation", k.name, cotangent, O.check_scatter(f.grad.cpu(), O.scatter_grad_f64(go, d.idx, k.n)))


@pytest.mark.parametrize("cotangent", ["expanded", "permuted"])
def test_three_interpolate_frontend(cotangent):
    d = O.interpolate_grad_data("c37_tail5")
    k = d.case
    feats = torch.randn(k.b, k.c, k.m, generator=torch.Generator().manual_seed(2))
    f = feats.to(DEV).requires_grad_(True)
    out = PU.three_interpolate(f, d.idx.to(DEV), d.w.to(DEV))
    O.check_interpolate(out.detach().cpu(), feats, d.idx, d.w, P.three_interpolate(feats, d.idx, d.w))
    go = torch.ones_like(d.go) if cotangent == "expanded" else d.go
    _backward(out, None if cotangent == "expanded" else go)
    _report("three_interpolate", k.name, cotangent, O.check_scatter(f.grad.cpu(), O.interpolate_grad_f64(go, d.idx, d.w, k.m)))


@pytest.mark.parametrize("cotangent", ["expanded", "permuted"])
def test_gather_operation_frontend(cotangent):
    d = O.gather_data("np257")
    k = d.case
    feats = torch.randn(k.b, k.c, k.n, generator=torch.Generator().manual_seed(3))
    f = feats.to(DEV).requires_grad_(True)
    out = PU.gather_operation(f, d.idx.to(DEV))
    O.check_copy(out.detach().cpu(), feats, d.idx)
    go = torch.ones_like(d.go) if cotangent == "expanded" else d.go
    _backward(out, None if cotangent == "expanded" else go)
    _report("gather_operation", k.name, cotangent, O.check_scatter(f.grad.cpu(), O.scatter_grad_f64(go, d.idx, k.n)))
