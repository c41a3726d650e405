"""GPU: the patch-cost training operator (train_ops.patch_cost: rtk_patch_cost forward; rtk_patch_cost_bwd, then either
rtk_group_inverse_index + rtk_patch_dfeat_gather or the materialised dxg + rtk_scatter_add_rows; rtk_weightnet_bwd) against float64
autograd through the restatement of its contract (tests/_stage_f64.py::patch_cost_f64): the output, the feature gradient and the six
WeightNet gradients under a random cotangent, with the WeightNet of the reference state dict (fc_layer.weightnet2).

The bound is tests/test_stage_f64_gpu.py::_check: the error relative to the tensor's largest element is at most 3 x the error of the same
restatement run by torch in fp32 (another summation order of the same arithmetic) + 2e-7, and at most the file's absolute cap of 2e-6.

Inputs are drawn on the CPU (a seed can be chosen without a GPU) so that, in float64, no WeightNet pre-activation lies within 1e-4
of its layer's largest magnitude of zero (asserted from the reference alone, margin()): no ReLU decision can differ between float64,
torch fp32 and the kernels, and what is left is the arithmetic's error.  A case has 272 pre-activations at each of its 3 696 to 32 784
positions; on clouds of unit size about one in 10^4 of them falls inside that margin whatever the seed (measured: the closest lies
1e-7 ... 1e-11 of the maximum from zero).  The clouds are therefore XYZ_SCALE = 1e-3 across: the direction vectors are small against
the first layer's biases, 4 + 3 of the 16 hidden channels and about 134 of the 256 output channels are live at every position, the
others dead, and the one or two output channels that still change sign between positions are what the seeds were chosen for
(margins 5e-4 ... 2e-3).
"""
import pytest
import torch

from ratrack_amd import _lib
from ratrack_amd import pointnet2_utils as PU
from ratrack_amd import train_ops as T

from _stage_f64 import MARGIN, clear_of_zero, margin, patch_cost_f64
from _util import reference_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ["out", "dfeat", "dwa", "dba", "dwb", "dbb", "dwc", "dbc"]
XYZ_SCALE = 1e-3


def weightnet2(device, dtype):
    """[(W, b)] * 3 of fc_layer.weightnet2 (3 -> 8 -> 8 -> 256) as 2-D / 1-D tensors."""
    sd = reference_state_dict("cpu")
    return [(sd["fc_layer.weightnet2.mlp_convs.%d.weight" % i].reshape(-1, 3 if i == 0 else 8).to(device=device, dtype=dtype),
             sd["fc_layer.weightnet2.mlp_convs.%d.bias" % i].to(device=device, dtype=dtype)) for i in range(3)]


class Case:
    """xyz (B, n, 3), feat and cotangent (B n, 256), drawn on the CPU.  twice: the second half of every cloud repeats the first (every
    point present twice: direction 0 and repeated neighbours).  live (B,): the points from live[b] on are copies of point 0,
    coordinates and features (a padded batch)."""

    def __init__(self, B, n, seed, twice=False, live=None, scale=XYZ_SCALE):
        g = torch.Generator().manual_seed(seed)
        self.B, self.n, self.live = B, n, live
        xyz = torch.randn(B, n, 3, generator=g) * scale
        if twice:
            xyz[:, n - n // 2:] = xyz[:, :n // 2].clone()
        feat = torch.randn(B, n, 256, generator=g)
        if live is not None:
            assert len(live) == B and all(16 <= v <= n for v in live)
            for b, v in enumerate(live):
                xyz[b, v:] = xyz[b, 0]
                feat[b, v:] = feat[b, 0]
        self.xyz, self.feat = xyz.contiguous(), feat.reshape(B * n, 256).contiguous()
        self.ct = torch.randn(B * n, 256, generator=g)

    def knn_host(self):
        """The neighbour table by torch on the host (choosing a seed without a GPU; the tests take the kernels' tables)."""
        x = self.xyz.double()
        d = ((x[:, :, None, :] - x[:, None, :, :]) ** 2).sum(-1)
        if self.live is not None:
            cand = torch.arange(self.n)[None, :] >= torch.tensor(self.live)[:, None]
            d = d.masked_fill(cand[:, None, :], float("inf"))
        return d.topk(16, dim=2, largest=False).indices

    def knn_device(self):
        xyz = self.xyz.to(DEV)
        if self.live is None:
            return PU.knn_point(16, xyz, xyz)
        nv = torch.tensor(self.live, dtype=torch.int32, device=DEV)
        idx = torch.empty(self.B, self.n, 16, dtype=torch.int64, device=DEV)
        _lib.call("rtk_knn_point_masked", self.B, self.n, self.n, 16, xyz.data_ptr(), xyz.data_ptr(), idx.data_ptr(), nv.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
        return idx


def reference(case, knn, dtype, device):
    """[out, dfeat, dwa, dba, dwb, dbb, dwc, dbc] of patch_cost_f64 under autograd in `dtype`: the same (padded) tensors, the same table."""
    B, n = case.B, case.n
    xyz = case.xyz.to(device=device, dtype=dtype)
    feat = case.feat.to(device=device, dtype=dtype).view(B, n, 256).requires_grad_(True)
    wn = [(W.requires_grad_(True), b.requires_grad_(True)) for W, b in weightnet2(device, dtype)]
    out = patch_cost_f64(xyz, knn, feat, wn).reshape(B * n, 256)
    flat = [t for Wb in wn for t in Wb]
    grads = torch.autograd.grad(out, [feat] + flat, case.ct.to(device=device, dtype=dtype))
    return [out.detach(), grads[0].reshape(B * n, 256)] + [g.detach() for g in grads[1:]]


def operator(case, knn):
    feat = case.feat.to(DEV).requires_grad_(True)
    flat = [t.requires_grad_(True) for Wb in weightnet2(DEV, torch.float32) for t in Wb]
    live = None if case.live is None else torch.tensor(case.live, dtype=torch.int32, device=DEV)
    out = T.patch_cost(feat, *flat, case.xyz.to(DEV), knn, live=live)
    grads = torch.autograd.grad(out, [feat] + flat, case.ct.to(DEV))
    torch.cuda.synchronize()
    return [out.detach()] + [g.detach() for g in grads]


def scale_err(got, r64):
    return float((got.double() - r64).abs().max() / r64.abs().max().clamp_min(1e-300))


# (id, B, n, seed, twice, live, the value of train_ops.INVERSE_TABLE_MAX_POINTS or None for the product's)
CASES = [
    ("b3_n77", 3, 77, 10, False, None, None),                      # partial tiles, more than one workgroup per cloud
    ("b2_n300_twice", 2, 300, 20, True, None, None),               # every point present twice
    ("b1_n2049_scatter", 1, 2049, 30, False, None, None),          # the first size past the inverse table: dxg + rtk_scatter_add_rows
    ("b2_n300_twice_forced_scatter", 2, 300, 20, True, None, 0),   # the same inputs through the scatter form
    ("b3_n300_padded", 3, 300, 41, False, (200, 300, 17), None),   # live / row0: padding queries folded into point 0
]


@pytest.mark.parametrize("name,B,n,seed,twice,live,limit", CASES, ids=[c[0] for c in CASES])
def test_patch_cost_backward_matches_float64_autograd(name, B, n, seed, twice, live, limit, monkeypatch):
    """Forward, dfeat and the six WeightNet gradients.  Measured on an MI355X, error relative to the tensor's largest element against
    float64, kernel / torch fp32, worst of the five cases: out 1.3e-7 / 1.1e-7, dfeat 2.9e-7 / 4.5e-7, dwa 4.2e-7 / 2.1e-6,
    dba 3.0e-7 / 3.0e-7, dwb 4.2e-7 / 5.3e-6, dbb 3.5e-7 / 2.7e-7, dwc 2.3e-7 / 1.5e-6, dbc 2.4e-7 / 3.7e-7.  Every tensor stays
    under the file's 2e-6 cap (torch fp32 itself does not, for dwa and dwb at n = 2049): no tensor takes a cap of its own.  The two
    forms of the feature gradient agree to the last digit shown on the same inputs (b2_n300_twice: 1.28e-7 either way)."""
    case = Case(B, n, seed, twice=twice, live=live)
    knn = case.knn_device()
    wn64 = weightnet2(DEV, torch.float64)
    x64 = case.xyz.to(DEV).double()
    m = margin(x64, x64, knn, wn64)
    print("\n%s: smallest |pre-activation| / layer maximum in float64: %.2e" % (name, m))
    assert m >= MARGIN, "a WeightNet pre-activation within %.0e of zero (%.2e): choose another seed" % (MARGIN, m)
    if limit is not None:
        monkeypatch.setattr(T, "INVERSE_TABLE_MAX_POINTS", limit)
    assert (n > T.INVERSE_TABLE_MAX_POINTS) == name.endswith("scatter")
    compare(case, knn)


def compare(case, knn):
    B, n, live = case.B, case.n, case.live
    got = operator(case, knn)
    r64 = reference(case, knn, torch.float64, DEV)
    r32 = reference(case, knn, torch.float32, DEV)
    if live is not None:                                           # nothing gathers a padding row: its gradient is exactly zero
        pad = torch.arange(n, device=DEV)[None, :] >= torch.tensor(live, device=DEV)[:, None]
        assert (r64[1].view(B, n, 256)[pad] == 0).all() and (got[1].view(B, n, 256)[pad] == 0).all()
    bad = []
    for k, g, a, b in zip(NAMES, got, r64, r32):
        assert g.shape == a.shape and torch.isfinite(g).all(), k
        e, e32 = scale_err(g, a), scale_err(b, a)
        print("   %-6s kernel %.2e  torch fp32 %.2e" % (k, e, e32))
        if not (e <= 2e-6 and e <= 3 * e32 + 2e-7):
            bad.append((k, e, e32))
    assert not bad, bad


UNIT_CASES = [
    ("unit_b3_n77", 3, 77, 50, False, None, None),
    ("unit_b2_n300_twice_forced_scatter", 2, 300, 51, True, None, 0),
    ("unit_b3_n300_padded", 3, 300, 52, False, (200, 300, 17), None),
]


@pytest.mark.parametrize("name,B,n,seed,twice,live,limit", UNIT_CASES, ids=[c[0] for c in UNIT_CASES])
def test_patch_cost_backward_with_masks_that_vary_by_position(name, B, n, seed, twice, live, limit, monkeypatch):
    """Clouds of unit size: the ReLU masks of most channels differ from position to position, so a sign mask or a hidden activation
    taken from the wrong position shows -- which the clouds above, 1e-3 across, cannot see.  At this size some pre-activation always
    lies within 1e-4 of zero, and a mask that flips between precisions moves a gradient sum by one whole term.  The condition is
    therefore met per entry: the cotangent is zero at every out[b, i, c] whose gradient passes through a pre-activation inside the
    margin (clear_of_zero, from the float64 reference alone; a padding query shares point 0's positions and decision).  The forward
    and dfeat are continuous in the pre-activations and keep every entry.  Same bound."""
    case = Case(B, n, seed, twice=twice, live=live, scale=1.0)
    knn = case.knn_device()
    x64 = case.xyz.to(DEV).double()
    keep, mixed = clear_of_zero(x64, x64, knn, weightnet2(DEV, torch.float64))
    kept = float(keep.double().mean())
    print("\n%s: %.1f %% of the cotangent kept, %d of 272 channels change sign between positions" % (name, 100 * kept, mixed))
    assert kept >= 0.5 and mixed >= 136, (kept, mixed)
    case.ct = case.ct * keep.reshape(B * n, 256).float().cpu()
    if limit is not None:
        monkeypatch.setattr(T, "INVERSE_TABLE_MAX_POINTS", limit)
    compare(case, knn)
