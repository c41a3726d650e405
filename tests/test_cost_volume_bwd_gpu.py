"""GPU: the cost-volume training operator (train_ops.cost_volume: rtk_cost_volume_train / rtk_cost_volume_split_train forward;
rtk_cost_volume_bwd / rtk_cost_volume_bwd_split, rtk_scatter_add_rows, rtk_tn_gemm256_split, rtk_weightnet_bwd and the host's column
sums backward) against float64 autograd through the restatement of its contract (tests/_stage_f64.py::cost_volume_f64): the output,
the three saved activations and the gradients of all 13 leaves under a random cotangent, with the cost-volume parameters of the
reference state dict (fc_layer.mlp_convs, fc_layer.weightnet1), for both kernel pairs (train_ops.CV_SPLIT True and False).

The bound is tests/test_stage_f64_gpu.py::_check: the error relative to the tensor's largest element is at most 3 x the error of the
same restatement run by torch in fp32 + 2e-7, and at most 2e-6.

Two kinds of decisions separate the precisions, and each has its own cure:
  * The 3 x 256 leaky-ReLU decisions per position.  The backward kernels do not take them: they read what the forward saved (mask1,
    mask2, the sign of a3).  Both references therefore run on the operator's own saved decisions (cost_volume_f64(decisions=...)), and
    a separate assertion says that those equal float64's except where float64's activation lies within the forward's own error bound
    (BAND = 2e-6 of the layer's largest magnitude) of zero, which at most 1e-3 of the entries do.
  * The WeightNet's 272 ReLU decisions per position, which the backward kernels recompute.  The cotangent is zero at every out[b, i, c]
    whose gradient passes through a WeightNet pre-activation within 1e-4 of its layer's largest magnitude of zero (clear_of_zero, from the
    float64 reference alone), as in tests/test_patch_cost_bwd_gpu.py; at least half of the cotangent stays and at least 136 of the 272
    channels change sign between positions.

| id | B, n1, n2 | what it enters |
|---|---|---|
| b3_n77 | 3, 77, 77 | 2-D grid, partial last tile, one tile per workgroup |
| b2_n50_from_131 | 2, 50, 131 | n2 > n1: most p2 rows unreferenced -> exact zeros in dp2 |
| b2_n131_from_50 | 2, 131, 50 | n2 < n1: heavily shared destination rows in the scatter |
| b5_n1_from_16 | 5, 1, 16 | one query: 7 of 8 (3 of 4) tile slots invalid and clamped to n1 - 1 |
| b64_n37_looping | 64, 37, 37 | flattened XCD grid; split backward 5 tiles on 4 workgroups (the partial tile through the prefetch path), fp32 10 on 8, split forward 40 on 32 |
| b100_n22_from_16_looping | 100, 22, 16 | 2-D grid with looping (split 3 tiles on 2 workgroups, fp32 6 on 5); every p2 row referenced by every query |
| b3_n77_padded | 3, 77, 77 | queries and points from live = (40, 77, 17) on are copies of point 0: hot row 0 |
"""
import pytest
import torch

from ratrack_amd import _lib
from ratrack_amd import pointnet2_utils as PU
from ratrack_amd import train_ops as T

from _cost_volume_cases import BAND, CASES, LOOPING, PARAMS, Case, band_share, case_by_name, parameters, tiles_per_workgroup
from _stage_f64 import decode_sign_masks

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRADS = ["dp1", "dp2"] + ["d" + k for k in PARAMS]
SPLITS = [pytest.param(True, id="split"), pytest.param(False, id="fp32")]


def knn_device(case):
    x1, x2 = case.xyz1.to(DEV), case.xyz2.to(DEV)
    if case.live is None:
        return PU.knn_point(16, x2, x1).contiguous()
    nv = torch.tensor(case.live, dtype=torch.int32, device=DEV)
    idx = torch.empty(case.B, case.n1, 16, dtype=torch.int64, device=DEV)
    _lib.call("rtk_knn_point_masked", case.B, case.n1, case.n2, 16, x1.data_ptr(), x2.data_ptr(), idx.data_ptr(), nv.data_ptr(),
              torch.cuda.current_stream().cuda_stream)
    return idx


def operator(case, knn, par, ct):
    """train_ops.cost_volume under torch.autograd.grad -> (out, [a1, a2, a3], the three saved decisions (B n1 16, 256) bool, 13 gradients)."""
    leaves = [t.to(DEV).clone().requires_grad_(True) for t in [case.p1, case.p2] + par]
    out = T.cost_volume(*leaves, case.xyz1.to(DEV), case.xyz2.to(DEV), knn)
    acts, masks = out.grad_fn.saved_tensors[:2]
    acts, masks = acts.clone(), masks.clone()
    grads = torch.autograd.grad(out, leaves, ct.to(DEV))
    torch.cuda.synchronize()
    dec = [decode_sign_masks(masks[0]), decode_sign_masks(masks[1]), acts[2] > 0]
    assert torch.equal(dec[0], acts[0] > 0) and torch.equal(dec[1], acts[1] > 0)          # the masks are the signs of what was saved
    return out.detach(), list(acts.unbind(0)), dec, [g.detach() for g in grads]


def scale_err(got, r64):
    return float((got.double() - r64).abs().max() / r64.abs().max().clamp_min(1e-300))


def rule(rows, bound=2e-6):
    """rows: [(name, kernel, float64, torch fp32)].  The project's rule for every tensor; prints both errors of each."""
    bad = []
    for k, g, a, b in rows:
        assert g.shape == a.shape and torch.isfinite(g).all(), k
        e, e32 = scale_err(g, a), scale_err(b, a)
        print("   %-5s kernel %.2e  torch fp32 %.2e" % (k, e, e32))
        if not (e <= bound and e <= 3 * e32 + 2e-7):
            bad.append((k, e, e32))
    assert not bad, bad


def compare(case, knn, par, ct, forward=True, zeroed=None):
    """The assertions of a case under the cotangent `ct`.  zeroed: per layer the channels a test made exactly zero (left out of the band's
    share).  -> (operator's gradients, float64's, torch fp32's)."""
    B, n1, n2 = case.B, case.n1, case.n2
    out, acts, dec, grads = operator(case, knn, par, ct)
    dec4 = [d.view(B, n1, 16, 256) for d in dec]
    o64, a64, g64 = case.reference(knn, par, torch.float64, DEV, decisions=dec4, ct=ct)
    o32, a32, g32 = case.reference(knn, par, torch.float32, DEV, decisions=dec4, ct=ct)
    rows = [("out", out, o64, o32)] + [("a%d" % (l + 1), acts[l], a64[l], a32[l]) for l in range(3)] if forward else []
    rule(rows + list(zip(GRADS, grads, g64, g32)))
    # the saved decisions are float64's wherever float64 is not within the forward's bound of zero (the sign of a64 is that of its z)
    for l in range(3):
        differ = dec[l] != (a64[l] > 0)
        assert (a64[l].abs()[differ] <= BAND * a64[l].abs().max()).all(), "layer %d: a saved decision differs outside the band" % (l + 1)
    share = band_share(a64, zeroed)
    print("   %.1e of the activations within %.0e of zero; %d saved decisions differ from float64's" % (
        share, BAND, sum(int((dec[l] != (a64[l] > 0)).sum()) for l in range(3))))
    assert share <= 1e-3, share
    # p2 rows that no query references: exactly zero, from a scatter that is fully written without a zero fill
    hit = torch.zeros(B * n2, dtype=torch.bool, device=DEV)
    hit[(knn + (torch.arange(B, device=DEV) * n2).view(B, 1, 1)).view(-1)] = True
    assert (grads[1][~hit] == 0).all() and (g64[1][~hit] == 0).all()
    # dp1[i] depends on dout[i] alone
    dead = (ct == 0).all(1).to(DEV)
    assert (grads[0][dead] == 0).all()
    return grads, g64, g32


def masked_cotangent(case, knn, par):
    keep, mixed = case.keep_mask(knn, [t.to(DEV).double() for t in par])
    kept = float(keep.double().mean())
    print("\n%s: %.1f %% of the cotangent kept, %d of 272 WeightNet channels change sign between positions" % (case.name, 100 * kept, mixed))
    assert kept >= 0.5 and mixed >= 136, (kept, mixed)
    return case.ct * keep.float().cpu(), keep


def assert_loops(case, keep):
    """The shape gives a workgroup of either backward kernel, and of the split forward, more than one tile, the partial last tile among
    those reached through the loop; and the last query of some sample keeps part of its cotangent."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sizing = tiles_per_workgroup(case.B, case.n1, cus if cus >= 8 else 256)
    for kernel, (tiles, wgs) in sizing.items():
        assert tiles > wgs, "%s: %d tiles on %d workgroups do not loop: the sizing rules changed" % (kernel, tiles, wgs)
    assert case.n1 % 8 != 0 and case.n1 % 4 != 0                      # a partial last tile, whose index is >= the number of workgroups
    assert keep.view(case.B, case.n1, 256)[:, -1].any(1).any()


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_cost_volume_backward_matches_float64_autograd(name, split, monkeypatch):
    """Output, saved activations and the 13 gradients of every case of the table, both kernel pairs.  Measured on an MI355X, error
    relative to the tensor's largest element against float64, split kernels, fp32-input kernels / torch fp32, worst of the seven cases:
    out 1.8e-7, 1.8e-7 / 2.5e-7;  a1 1.3e-7, 1.3e-7 / 8.6e-8;  a2 4.6e-7, 7.6e-7 / 8.4e-7;  a3 5.4e-7, 7.6e-7 / 8.8e-7;
    dp1 1.5e-7, 2.7e-7 / 2.0e-7;  dp2 4.4e-7, 6.6e-7 / 5.2e-7;  dwd 3.1e-7, 2.8e-7 / 8.1e-7;  dw2 3.9e-7, 2.5e-7 / 3.9e-6;
    db2 3.6e-7, 2.0e-7 / 2.6e-7;  dw3 4.0e-7, 5.1e-7 / 2.9e-6;  db3 2.0e-7, 1.6e-7 / 3.3e-7;  dwa 4.3e-7, 4.5e-7 / 6.6e-7;
    dba 5.1e-7, 7.1e-7 / 4.8e-7;  dwb 4.2e-7, 4.8e-7 / 1.7e-6;  dbb 3.6e-7, 4.0e-7 / 3.5e-7;  dwc 2.6e-7, 2.7e-7 / 1.3e-6;
    dbc 1.7e-7, 2.3e-7 / 2.7e-7.  Every tensor stays under the 2e-6 cap (torch fp32 itself does not, for dw2 and dw3): no
    tensor takes a cap of its own.  At most 5.7e-5 of the activations lie inside the band, and 0 to 2 saved decisions of a case differ
    from float64's, all inside it."""
    monkeypatch.setattr(T, "CV_SPLIT", split)
    case = case_by_name(name)
    knn = knn_device(case)
    par = parameters("cpu", torch.float32)
    ct, keep = masked_cotangent(case, knn, par)
    if name in LOOPING:
        assert_loops(case, keep)
    if case.n2 == 16:                                                  # every query references every row
        assert torch.equal(knn.sort(2).values, torch.arange(16, device=DEV).expand(case.B, case.n1, 16))
    compare(case, knn, par, ct)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("name", ["b3_n77", "b64_n37_looping"])
@pytest.mark.parametrize("exponent", [-60, 60])
def test_cost_volume_backward_cotangent_of_any_magnitude(name, exponent, split, monkeypatch):
    """The whole cotangent times 2^-60 and 2^+60: every gradient against float64 under the same rule (the backward kernels take a
    power-of-two scale per position, rtk_tn_gemm256_split one per tensor from the dz_amax the backward kernel folds in).  Measured on
    an MI355X, worst of the two cases and the two exponents, split, fp32-input / torch fp32: dp1 1.5e-7, 2.7e-7 / 1.9e-7;  dp2 3.6e-7, 4.2e-7 / 4.3e-7;  dwd 2.2e-7,
    2.2e-7 / 6.9e-7;  dw2 3.9e-7, 2.5e-7 / 3.9e-6;  db2 3.6e-7, 1.8e-7 / 2.4e-7;  dw3 2.3e-7, 2.2e-7 / 1.9e-6;  db3 9.8e-8, 1.2e-7 /
    3.3e-7;  dwa 2.3e-7, 4.5e-7 / 4.4e-7;  dba 3.8e-7, 7.1e-7 / 4.8e-7;  dwb 2.8e-7, 3.3e-7 / 1.7e-6;  dbb 3.6e-7, 3.0e-7 / 3.5e-7;
    dwc 2.6e-7, 2.7e-7 / 1.3e-6;  dbc 1.5e-7, 2.3e-7 / 1.7e-7: the figures of the unit cotangent."""
    monkeypatch.setattr(T, "CV_SPLIT", split)
    case = case_by_name(name)
    knn = knn_device(case)
    par = parameters("cpu", torch.float32)
    ct, _ = masked_cotangent(case, knn, par)
    compare(case, knn, par, ct * 2.0 ** exponent, forward=False)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("name", ["b3_n77", "b64_n37_looping"])
def test_cost_volume_backward_cotangent_rows_spanning_24_binades(name, split, monkeypatch):
    """Cotangent row i times 2^-(i mod 25).  The whole-tensor rule for the 13 gradients, and for dp1 the rule row by row: dp1[i]
    depends on dout[i] alone, so its error is measured against the row's own largest element -- the worst row's error is at most 2e-6
    and at most 3 x the worst row's error of torch fp32 + 2e-7 (worst against worst, as the whole-tensor rule takes the worst element of
    either).  Measured on an MI355X, split, fp32-input / torch fp32, worst of the two cases: dp1 row by row 2.9e-7, 3.8e-7 / 4.2e-7;
    whole tensors dp1 1.5e-7, 2.5e-7 / 2.5e-7;  dp2 4.2e-7, 5.3e-7 / 5.6e-7;  dwd 3.0e-7, 2.9e-7 / 7.3e-7;  dw2 3.0e-7, 2.4e-7 / 3.5e-6;
    db2 3.4e-7, 1.7e-7 / 2.9e-7;  dw3 2.6e-7, 2.6e-7 / 2.2e-6;  db3 1.4e-7, 1.4e-7 / 2.3e-7;  dwa 3.3e-7, 3.5e-7 / 3.9e-7;  dba 3.0e-7,
    1.5e-7 / 3.0e-7;  dwb 2.7e-7, 2.9e-7 / 1.3e-6;  dbb 2.8e-7, 1.5e-7 / 3.1e-7;  dwc 1.6e-7, 2.3e-7 / 1.4e-6;  dbc 1.7e-7, 2.2e-7 / 1.9e-7."""
    monkeypatch.setattr(T, "CV_SPLIT", split)
    case = case_by_name(name)
    knn = knn_device(case)
    par = parameters("cpu", torch.float32)
    ct, _ = masked_cotangent(case, knn, par)
    ct = ct * (2.0 ** -(torch.arange(ct.shape[0]) % 25).double()).float()[:, None]
    grads, g64, g32 = compare(case, knn, par, ct, forward=False)
    live = g64[0].abs().amax(1) > 0
    row_err = lambda g: ((g.double() - g64[0]).abs().amax(1)[live] / g64[0].abs().amax(1)[live]).max().item()
    e, e32 = row_err(grads[0]), row_err(g32[0])
    print("   dp1 row by row: kernel %.2e  torch fp32 %.2e" % (e, e32))
    assert e <= 2e-6 and e <= 3 * e32 + 2e-7, (e, e32)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("negative_zero", [False, True], ids=["plus0", "minus0"])
def test_cost_volume_exact_zeros_take_the_negative_slope(negative_zero, split, monkeypatch):
    """Pre-activations that are exactly zero: channel 5 of layer 1 (p1, p2 columns -- p2's as -0.0 in the second variant -- and the
    row of wd), channel 7 of layer 2 (row of w2, b2[7]) and channel 9 of layer 3 (row of w3, b3[9]).  The saved decisions there are
    "not positive" and the gradients are float64's with slope 0.1: what leaky_relu's backward takes at 0, and with it the module path."""
    monkeypatch.setattr(T, "CV_SPLIT", split)
    case = case_by_name("b3_n77")
    par = parameters("cpu", torch.float32)
    case.p1[:, 5] = 0.0
    case.p2[:, 5] = -0.0 if negative_zero else 0.0
    par[0][5], par[1][7], par[2][7], par[3][9], par[4][9] = 0.0, 0.0, 0.0, 0.0, 0.0
    knn = knn_device(case)
    ct, _ = masked_cotangent(case, knn, par)
    out, acts, dec, _ = operator(case, knn, par, ct)
    for l, ch in enumerate((5, 7, 9)):
        assert (acts[l][:, ch] == 0).all() and not dec[l][:, ch].any(), (l, ch)
    grads, g64, _ = compare(case, knn, par, ct, zeroed=[[5], [7], [9]])
    # the slope is visible: none of the gradients that pass through the zero channels alone is zero
    for k, row in (("dp1", grads[0][:, 5]), ("dp2", grads[1][:, 5]), ("dwd", grads[2][5]), ("dw2", grads[3][7]), ("dw3", grads[5][9])):
        assert float(row.abs().max()) > 0, k


@pytest.mark.parametrize("split", SPLITS)
def test_cost_volume_samples_are_independent(split, monkeypatch):
    """Another sample 1 (coordinates, p1 and p2 rows, cotangent) leaves out, dp1 and dp2 of sample 0 bit for bit."""
    monkeypatch.setattr(T, "CV_SPLIT", split)
    par = parameters("cpu", torch.float32)
    a, b = case_by_name("b3_n77"), case_by_name("b3_n77")
    g = torch.Generator().manual_seed(99)
    n = a.n1
    for t, shape in ((b.xyz1[1], (n, 3)), (b.xyz2[1], (n, 3)), (b.p1[n:2 * n], (n, 256)), (b.p2[n:2 * n], (n, 256)), (b.ct[n:2 * n], (n, 256))):
        t.copy_(torch.randn(*shape, generator=g) * 3.0)
    res = []
    for case in (a, b):
        knn = knn_device(case)
        out, _, _, grads = operator(case, knn, par, case.ct)
        res.append((knn, out, grads[0], grads[1]))
    (ka, oa, da1, da2), (kb, ob, db1, db2) = res
    assert torch.equal(ka[0], kb[0]) and not torch.equal(oa[n:2 * n], ob[n:2 * n])
    assert torch.equal(oa[:n], ob[:n]) and torch.equal(da1[:n], db1[:n]) and torch.equal(da2[:n], db2[:n])
