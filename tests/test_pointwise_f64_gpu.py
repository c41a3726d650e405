"""GPU: the per-point chain family -- rtk_pointwise_mlp (all twelve kernel instances, split and fp32-input images, with and without
the interpolation prologue), rtk_pointwise_mlp_tap and rtk_pointwise_mlp_pair -- against the float64 restatement of their header
contract (tests/_pointwise_f64.py), with the source, output and activation layouts the engine launches them with
(fused.run_pnhead, FusedBackbone) at the smallest shapes the tile logic can go wrong at.

The acceptance rule is test_stage_f64_gpu.py::_check: error relative to scale <= 2e-6 (5e-6 with the interpolation prologue, as
test_fused_gpu.py::test_pointwise_interp_prologue) and <= 3 x the error of the same restatement in torch fp32 + 2e-7.

Buffers: every output is wider and longer than the result and prefilled with SENT; every source is a column slice of a wider
buffer holding POISON where the contract does not make it readable (from ceil4(channels) on, and the whole of the rows at or past
row_nuniq / interp.nuniq).

Measured on an MI355X (worst case of each section, kernel / torch fp32 restatement): every instance 5.1e-7 /
7.2e-7 split and 8.8e-7 / 7.2e-7 fp32-input (dec_q1); magnitudes, worst row 7.8e-7 / 1.2e-6; weight rows within 2^-16 of the
matrix maximum 3.0e-7 split, 2.9e-7 fp32-input, smaller rows of the split images 3.4e-5 of their magnitude (enc_q1) -- inside the
documented 2^-39 floor --, of the fp32-input images 2.6e-7.  Both -0.0 constructions of
test_colmax_of_minus_zero_pre_activations come out of the compiled ReLU as +0.0 (bits 0): store_tile stays as it is."""
import pytest
import torch

from ratrack_amd import fused as F
from ratrack_amd import pointnet2_hip

from _pointwise_f64 import ACT_NONE, ACT_RELU, ACT_SIGMOID, chain as chain_f64, input_vector, pair_f64, pointwise_f64, tap_f64

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -5.0
POISON = 1e30

# samples x rows_per_sample
SHAPES = {
    "small2d": (3, 77),      # 2-D grid; the second 64-row group holds 13 live rows: one partial tile and two wholly invalid waves
    "small1d": (8, 77),      # XCD-aware 1-D grid (samples % 8 == 0)
    "loop": (264, 130),      # PW_WGS_TARGET / samples < 1: every workgroup loops over three groups, the weight stream wraps, the
                             # last group has 2 live rows
    "one": (2, 1),           # rows_per_sample = 1
}
R, N_, S_ = ACT_RELU, ACT_NONE, ACT_SIGMOID

# name: (PW_CASE key, interpolated channels or 0, [(channels, per_sample)], widths, activations, sample_bias, out_channels,
#        channel_major, row_nuniq, colmax) -- as fused.py launches the instance (run_pnhead, FusedBackbone.backbone, the heads)
INSTANCES = {
    "enc_q1":   ((1, 2), 0, [(2, False)], [32], [N_], False, 32, False, False, False),                   # raw (RCS, v_r), pitch-4 rows
    "trans1":   ((4, 6), 0, [(64, False)], [96], [N_], False, 96, False, True, False),                   # sa1 -> linear1 || sa2 projections
    "trans2":   ((6, 12), 0, [(96, False)], [192], [N_], False, 192, False, True, False),
    "lin3":     ((8, 4), 0, [(128, False)], [64], [N_], False, 64, False, True, False),
    "fp1":      ((8, 8), 128, [], [128], [R], False, 128, False, False, True),                           # interpolation alone, colmax
    "fp3_cmp":  ((8, 8), 64, [(64, False)], [128], [R], False, 128, False, True, False),                 # fp3 on linear3's output
    "fp2":      ((10, 8), 128, [(32, False)], [128], [R], False, 128, False, True, False),
    "fp3":      ((12, 8), 128, [(64, False)], [128], [R], False, 128, False, True, False),               # linear3 composed in
    "p1_loc":   ((8, 16), 0, [(128, False)], [256], [N_], True, 256, False, False, False),
    "cls":      ((16, 8, 4, 2, 1), 0, [(256, False)], [128, 64, 32, 1], [R, R, R, S_], False, 1, True, False, True),
    "flow":     ((8, 8, 4, 2, 1), 0, [(128, False)], [128, 64, 32, 3], [R, R, R, N_], True, 3, True, False, False),
    "dec_q1":   ((25, 2), 0, [(2, False), (128, False), (256, False)], [32], [N_], True, 32, False, False, False),
    "u8v2":     ((8, 2), 0, [(128, False)], [32], [N_], False, 32, False, True, False),                  # (no launch of the engine names it)
    # the class head's instance on [local 128 || per-sample 128]: a broadcast source (test_fused_gpu.py's chain)
    "bcast":    ((16, 8, 4, 2, 1), 0, [(128, False), (128, True)], [128, 64, 32, 3], [R, R, R, N_], False, 3, False, False, False),
}
SINGLE, FOUR, INTERP = "dec_q1", "flow", "fp2"      # the representatives of the loop / one / independence cases
MULTI_SOURCE = ["dec_q1", "fp2", "fp3"]             # (25,2), (10,8), (12,8)
NU_OFF = [3, 14, 25, 36, 47, 58, 69, 6]             # rows_per_sample - row_nuniq[b]: 77 -> 74 63 52 41 30 19 8 71, no multiple of 16


def _f32(t):
    """float64 values that fp32 holds exactly."""
    return t.float().double()


def _scale_err(got, r64):
    return float((got.double() - r64).abs().max() / r64.abs().max().clamp_min(1e-300))


def _check(what, got, r64, r32, bound=2e-6):
    e, e32 = _scale_err(got, r64), _scale_err(r32, r64)
    print("\n%s: kernel %.2e  torch fp32 %.2e" % (what, e, e32))
    assert e <= bound and e <= 3 * e32 + 2e-7, (what, e, e32)


def _row_errs(got, r64, r32):
    """Per row, relative to the row's own largest float64 element -> (kernel's worst, torch fp32's worst, live-row mask)."""
    scale = r64.abs().amax(-1)
    live = scale > 0
    e = ((got.double() - r64).abs().amax(-1) / scale)[live]
    e32 = ((r32.double() - r64).abs().amax(-1) / scale)[live]
    return float(e.max()), float(e32.max()), live


class _Case:
    """Operands of one rtk_pointwise_mlp launch as float64 tensors that fp32 holds exactly, the device buffers the launch reads and
    writes, and the restatement's result in either dtype.  Everything the tests vary is an attribute changed between construction
    and launch() / reference()."""

    def __init__(self, name, shape, seed, m=40):
        self.name = name
        (self.key, self.cint, self.segs, widths, self.acts, has_sb, self.oc, self.cm, has_nu, self.has_colmax) = INSTANCES[name]
        self.B, self.n = SHAPES[shape] if isinstance(shape, str) else shape
        B, n = self.B, self.n
        g = torch.Generator(device=DEV).manual_seed(seed)
        rn = self.rn = lambda *s: _f32(torch.randn(*s, generator=g, device=DEV))
        self.gen = g
        self.src = [rn(B, ch) if per else rn(B, n, ch) for ch, per in self.segs]
        cin = F.ceil16(self.cint) + sum(F.ceil16(ch) for ch, _ in self.segs)
        assert cin // 16 == self.key[0] and tuple(F.ceil16(w) // 16 for w in widths) == self.key[1:]
        # layer 0's columns in the kernel's layout: zero where a segment is padded to 16 channels (as FusedBackbone pads dec_q1)
        colmask = torch.zeros(cin, device=DEV, dtype=torch.float64)
        o = 0
        for ch in ([self.cint] if self.cint else []) + [c for c, _ in self.segs]:
            colmask[o:o + ch] = 1
            o += F.ceil16(ch)
        self.layers, cur = [], cin
        for i, w in enumerate(widths):
            W = rn(w, cur) / max(cur, 16) ** 0.5 * (colmask if i == 0 else 1.0)
            self.layers.append([_f32(W), _f32(rn(w) * 0.125)])
            cur = w
        self.widths = widths
        self.sb = _f32(rn(B, F.ceil16(widths[0])) * 0.3) if has_sb else None
        self.row_nu = None
        if has_nu:
            self.row_nu = torch.tensor([max(1, n - NU_OFF[b % 8]) for b in range(B)], dtype=torch.int32, device=DEV)
        self.m = m
        if self.cint:
            self.known = rn(B, m, self.cint)
            self.idx = torch.randint(0, m, (B, n, 3), generator=g, device=DEV, dtype=torch.int32)
            self.d2 = (torch.rand(B, n, 3, generator=g, device=DEV) * 4 + 0.01).sort(-1)[0]
            self.d2[:, 2::16] = 0.0                                          # three coincident known points: equal thirds
            self.d2[:, 5::16, 0] = 0.0                                       # one zero distance: weight exactly 1
            self.known_nu = torch.tensor([max(1, m - 3 - b % 4) for b in range(B)], dtype=torch.int32, device=DEV)
            self.idx[:, 1::7, 1] = m - 1                                     # rows >= interp.nuniq[b]: must be read as row 0
            if self.row_nu is not None:                                      # index rows at or past row_nuniq: in range, other features
                for b in range(B):
                    self.idx[b, int(self.row_nu[b]):] = torch.tensor([1, 2, 3], dtype=torch.int32, device=DEV)

    # ---- device buffers -----------------------------------------------------------------------------------------------------
    @staticmethod
    def _slice_buffer(x, col, dead_from=None):
        """x (rows, ch) as columns col .. col + ch of a POISON buffer; columns ch .. ceil4(ch) hold the zeros the contract asks for;
        dead_from (per block of rows): the rows at or past it hold POISON throughout."""
        rows, ch = x.shape
        c4 = (ch + 3) // 4 * 4
        buf = torch.full((rows, col + c4 + 8), POISON, device=DEV)
        buf[:, col:col + c4] = 0.0
        buf[:, col:col + ch] = x.float()
        return buf, buf[:, col:col + c4]

    def _dead_rows(self, buf, per_block, counts):
        v = buf.view(self.B, per_block, -1)
        for b in range(self.B):
            v[b, int(counts[b]):] = POISON

    def launch(self, split):
        """-> (whole output buffer, colmax buffer (B + 2, 16 V) with the launch's zeros in rows 1 .. B, or None)."""
        B, n = self.B, self.n
        keep, srcs = [], []
        for i, ((ch, per), x) in enumerate(zip(self.segs, self.src)):
            buf, view = self._slice_buffer(x.reshape(-1, ch), 4 * (i + 1))
            if not per and self.row_nu is not None:
                self._dead_rows(buf, n, self.row_nu)
            keep.append(buf)
            srcs.append((view, ch, per))
        interp = None
        if self.cint:
            kbuf, kview = self._slice_buffer(self.known.reshape(-1, self.cint), 8)
            self._dead_rows(kbuf, self.m, self.known_nu)
            keep.append(kbuf)
            interp = (kview, self.cint, self.m, self.idx.reshape(-1, 3).contiguous(), self.d2.float().reshape(-1, 3).contiguous(), self.known_nu)
        ch = F.Chain([(w, b, a) for (w, b), a in zip(self.layers, self.acts)], DEV)
        sb = self.sb.float().contiguous() if self.sb is not None else None
        if self.cm:
            buf = torch.full((B + 2, self.oc, n), SENT, device=DEV)
            view = buf[1:1 + B]
        else:
            buf = torch.full((B * n + 5, 4 + (self.oc + 3) // 4 * 4 + 8), SENT, device=DEV)
            view = buf[:, 4:]
        cmax = None
        if self.has_colmax:
            cmax = torch.full((B + 2, F.ceil16(self.widths[-1])), SENT, device=DEV)
            cmax[1:1 + B] = 0.0
        old = F.PW_SPLIT
        F.PW_SPLIT = split
        try:
            F.pointwise(B * n, n, srcs, ch, view, out_channels=self.oc, sample_bias=sb, interp=interp, channel_major=self.cm,
                        row_nuniq=self.row_nu, colmax=cmax[1:1 + B] if cmax is not None else None)
            torch.cuda.synchronize()
        finally:
            F.PW_SPLIT = old
        return buf, cmax

    def reference(self, dtype):
        """The restatement on the same operands -> (whole output buffer, colmax buffer or None), in dtype."""
        B, n = self.B, self.n
        c = lambda t: t.to(dtype)
        srcs = [(c(x), per) for (_, per), x in zip(self.segs, self.src)]
        interp = (c(self.known), self.idx, c(self.d2), self.known_nu) if self.cint else None
        layers = [(c(w), c(b), a) for (w, b), a in zip(self.layers, self.acts)]
        if self.cm:
            buf = torch.full((B + 2, self.oc, n), SENT, device=DEV, dtype=dtype)
            view = buf[1:1 + B]
        else:
            buf = torch.full((B * n + 5, 4 + (self.oc + 3) // 4 * 4 + 8), SENT, device=DEV, dtype=dtype)
            view = buf[:, 4:]
        res = pointwise_f64(n, srcs, layers, interp=interp, sample_bias=c(self.sb) if self.sb is not None else None, out_channels=self.oc,
                            out=view, channel_major=self.cm, row_nuniq=self.row_nu, colmax=self.has_colmax)
        cmax = None
        if self.has_colmax:
            res, cm = res
            cmax = torch.full((B + 2, cm.shape[1]), SENT, device=DEV, dtype=dtype)
            cmax[1:1 + B] = cm
        view.copy_(res)
        return buf, cmax

    def rows(self, buf):
        """The result region of an output buffer as (B, n, oc)."""
        if self.cm:
            return buf[1:1 + self.B].permute(0, 2, 1)
        return buf[:self.B * self.n, 4:4 + self.oc].reshape(self.B, self.n, self.oc)

    def live(self):
        """(B, n) mask of the rows below row_nuniq."""
        if self.row_nu is None:
            return torch.ones(self.B, self.n, dtype=torch.bool, device=DEV)
        return torch.arange(self.n, device=DEV)[None, :] < self.row_nu.long()[:, None]

    @property
    def bound(self):
        return 5e-6 if self.cint else 2e-6

    def last_layer_input(self):
        """float64 input of the last layer (B, n, cin) and that layer's pre-activation offset (bias + sample bias) (B, 1, cout)."""
        srcs = [(x, per) for (_, per), x in zip(self.segs, self.src)]
        interp = (self.known, self.idx, self.d2.double(), self.known_nu) if self.cint else None
        x = input_vector(self.n, srcs, interp)
        first = [(w, b, a) for (w, b), a in zip(self.layers[:-1], self.acts[:-1])]
        if first:
            x = chain_f64(x, first, self.sb)
        w, b = self.layers[-1]
        off = b.abs()[None, None, :].expand(self.B, 1, -1).clone()
        if len(self.layers) == 1 and self.sb is not None:
            off = off + self.sb[:, None, :w.shape[0]].abs()
        return x[:, :, :w.shape[1]], off


def _run_and_check(case, split, what):
    """One launch against the restatement: the sentinel pattern of the whole buffer, the live region under _check, colmax bit-equal
    to the launch's own output, under _check against the restatement's, and without a sign bit."""
    got, gcm = case.launch(split)
    r64, c64 = case.reference(torch.float64)
    r32, c32 = case.reference(torch.float32)
    assert torch.equal(got == SENT, r64 == SENT), "rows / columns / samples written outside the contract, or live ones left out"
    mask = r64 != SENT
    assert torch.isfinite(got[mask]).all()
    _check(what, got[mask], r64[mask], r32[mask], case.bound)
    if gcm is not None:
        B = case.B
        assert torch.equal(gcm == SENT, c64 == SENT)
        cm = gcm[1:1 + B]
        assert not bool((cm.view(torch.int32) < 0).any()), "a sign bit in colmax"
        own = torch.where(case.live()[:, :, None], case.rows(got), torch.full_like(case.rows(got), float("-inf"))).amax(1)
        assert torch.equal(cm[:, :case.oc], own), "colmax is not the maximum of the launch's own output"
        _check(what + " colmax", cm, c64[1:1 + B], c32[1:1 + B], case.bound)
    return got, gcm


# ---- 3a: every instance, both image kinds ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["small2d", "small1d"])
@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("name", list(INSTANCES))
def test_instance_matches_float64(name, split, shape):
    case = _Case(name, shape, seed=sum(map(ord, name)) + SHAPES[shape][0])
    if case.row_nu is not None:
        nu = case.row_nu.tolist()
        assert len(set(nu)) == len(nu) and all(v % 16 for v in nu) and any(v % 64 for v in nu) and max(nu) < case.n
    if case.cint:
        assert bool((case.idx.long() >= case.known_nu.long().view(-1, 1, 1)).any())
    _run_and_check(case, split, "%s %s %s %s" % (name, case.key, "split" if split else "fp32", shape))


@pytest.mark.parametrize("shape", ["loop", "one"])
@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("name", [SINGLE, FOUR, INTERP, "fp1"])
def test_instance_matches_float64_looping_grid_and_single_row(name, split, shape):
    """264 samples of 130 rows (each workgroup takes three 64-row groups, the last with 2 live rows) and samples of one row."""
    case = _Case(name, shape, seed=sum(map(ord, name)) + 1000)
    _run_and_check(case, split, "%s %s %s %s" % (name, case.key, "split" if split else "fp32", shape))


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("m", [1, 2])
@pytest.mark.parametrize("name", ["fp1", INTERP])
def test_interpolation_from_one_and_two_known_points(name, m, split):
    """Tables of rtk_three_nn itself with m < 3 known points: the unfilled slots are (+inf, 0) and must weigh exactly 0."""
    B, n = SHAPES["small2d"]
    case = _Case(name, "small2d", seed=50 + m, m=m)
    unknown = torch.randn(B, n, 3, generator=case.gen, device=DEV) * 3
    known = torch.randn(B, m, 3, generator=case.gen, device=DEV) * 3
    unknown[:, 4] = known[:, 0]                                             # one zero distance
    d2 = torch.empty(B, n, 3, device=DEV)
    idx = torch.empty(B, n, 3, dtype=torch.int32, device=DEV)
    pointnet2_hip.three_nn_wrapper(B, n, m, unknown.contiguous(), known.contiguous(), d2, idx)
    torch.cuda.synchronize()
    assert bool(torch.isinf(d2[:, :, m:]).all()) and bool((idx[:, :, m:] == 0).all()) and bool(torch.isfinite(d2[:, :, :m]).all())
    case.idx, case.d2 = idx, d2.double()
    case.known_nu = torch.full((B,), m, dtype=torch.int32, device=DEV)
    _run_and_check(case, split, "%s m = %d %s" % (name, m, "split" if split else "fp32"))


# ---- 3b: positions of any magnitude -----------------------------------------------------------------------------------------------
EXPS = torch.tensor([-6.0, 6.0, -3.0, 3.0, 0.0], dtype=torch.float64)


def _row_scales(count):
    """10^e with e cycling through -6, 6, -3, 3, 0 inside every 16-row tile, row 7 of every tile all-zero."""
    t = torch.arange(count) % 16
    s = 10.0 ** EXPS[t % 5]
    s[t == 7] = 0.0
    return s.to(DEV)


def _magnitude_case(name, shape="small1d"):
    """The instance made positively homogeneous (no bias, no sample bias, the sigmoid dropped) with row r's inputs scaled by
    _row_scales: an interpolated row reads the known rows r, r + 80, r + 160, which carry row r's scale.  The last layer of the
    four-layer heads is non-negative: their one / three outputs are then sums without cancellation, and a row's largest element is
    a fair measure of its magnitude."""
    case = _Case(name, shape, seed=sum(map(ord, name)) + 7, m=240)
    B, n = case.B, case.n
    s = _row_scales(n)
    case.src = [x if per else _f32(x * s[None, :, None]) for (_, per), x in zip(case.segs, case.src)]
    if case.cint:
        assert n <= 80
        case.known = _f32(case.known * _row_scales(240)[None, :, None])
        r = torch.arange(n, device=DEV, dtype=torch.int32)
        case.idx = torch.stack([r, r + 80, r + 160], 1)[None].repeat(B, 1, 1).contiguous()
        case.d2 = torch.rand(B, n, 3, generator=case.gen, device=DEV).double() * 4 + 0.01
        case.known_nu = torch.full((B,), 240, dtype=torch.int32, device=DEV)
    for layer in case.layers:
        layer[1].zero_()
    if len(case.layers) == 4:
        case.layers[-1][0] = case.layers[-1][0].abs()
    case.sb = None
    case.acts = [N_ if a == S_ else a for a in case.acts]
    return case, s


@pytest.mark.parametrize("name", [k for k in INSTANCES if k != "bcast"])
def test_positions_of_any_magnitude(name):
    """Split images: every output row is 10^e times an O(1) result and carries the bound relative to ITS OWN largest element
    (test_sa_scale_positions_of_any_magnitude); the all-zero row of every tile gives the bias chain's output: zeros."""
    case, s = _magnitude_case(name)
    got, _ = case.launch(True)
    r64, _ = case.reference(torch.float64)
    r32, _ = case.reference(torch.float32)
    assert torch.equal(got == SENT, r64 == SENT)
    g, want, w32 = case.rows(got), case.rows(r64), case.rows(r32)
    live = case.live()
    zero = (s == 0)[None, :] & live
    assert bool((g[zero] == 0).all()) and bool((want[zero] == 0).all()) and int(zero.sum()) >= case.B
    sel = live & ~zero
    e, e32, nz = _row_errs(g[sel], want[sel], w32[sel])
    assert int(nz.sum()) > 0.9 * int(sel.sum())
    print("\nmagnitudes %s %s: worst row kernel %.2e  torch fp32 %.2e" % (name, case.key, e, e32))
    assert e <= case.bound and e <= 3 * e32 + 2e-7, (name, e, e32)


@pytest.mark.parametrize("name", MULTI_SOURCE)
def test_segments_of_one_row_2_to_the_40_apart(name):
    """One segment of every row at 2^40, the others at O(1).  The position scale is shared by the row, so the small segments lose
    their pieces to it and keep the documented ABSOLUTE floor -- 2^-39 of the row's largest input times sum |w|
    (test_fused_gpu.py::test_split_layers_adversarial_operands, mixed_range) -- asserted here on a layer that reads the small
    segments only (the large one's columns of W are zero), and, with every column live, next to the relative bound of the large."""
    case = _Case(name, "small1d", seed=sum(map(ord, name)) + 40)
    for layer in case.layers:
        layer[1].zero_()
    case.sb = None
    big = 2.0 ** 40
    if case.cint:
        case.known = case.known * big
        lo, hi = 0, F.ceil16(case.cint)
    else:                                                                   # dec_q1: f1 (the second source) is the large one
        case.src[1] = case.src[1] * big
        lo, hi = 16, 16 + 128
    w_full = case.layers[0][0].clone()
    x, _ = case.last_layer_input()
    floor = 2.0 ** -39 * x.abs().amax(-1)                                   # (B, n): per row, times sum |w| below
    small_w = w_full.clone()
    small_w[:, lo:hi] = 0
    sumw = small_w.abs().sum(1)                                             # (cout)
    live = case.live()
    for what, w in (("small segments alone", small_w), ("every segment", w_full)):
        case.layers[0][0] = w
        got, _ = case.launch(True)
        r64, _ = case.reference(torch.float64)
        assert torch.equal(got == SENT, r64 == SENT)
        g, want = case.rows(got), case.rows(r64)
        assert torch.isfinite(g[live]).all()
        err = (g.double() - want).abs()
        allow = floor[:, :, None] * sumw[None, None, :case.oc]
        if what == "every segment":
            allow = allow + case.bound * want.abs().amax(-1, keepdim=True)
        worst = float((err / allow.clamp_min(1e-300))[live].max())
        print("\n2^40 apart %s %s, %s: worst error / allowance %.2e" % (name, case.key, what, worst))
        assert worst <= 1.0, (name, what, worst)


# ---- 3c: weight rows spanning 24 binades ------------------------------------------------------------------------------------------
BINADE_CASES = [(k, len(INSTANCES[k][3]) - 1) for k in INSTANCES] + [(k, l) for k in ("cls", "flow") for l in (0, 1, 2)]


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("name,layer", BINADE_CASES)
def test_weight_rows_spanning_24_binades(name, layer, split):
    """Rows of one layer's W at 2^0 .. 2^-24 of the matrix maximum, its bias scaled alike -- what folding the BatchNorm of a trained
    net produces.  Per output channel, as test_sa_scale_weight_rows_spanning_24_binades: the image holds one power of two per
    matrix, so a row of the LAST layer within 2^-16 of the maximum keeps the full relative bound against the magnitude of its dot
    products, a smaller one 2e-6 mag + 4 floor with floor = 2^-39 max|W| max sum|h|; the fp32-input images have no image scale:
    the full relative bound on every row.  (A scaled earlier layer leaves every row of the last one at full size.)"""
    case = _Case(name, "small1d", seed=sum(map(ord, name)) + 24 + layer)
    w, b = case.layers[layer]
    f = 2.0 ** -torch.linspace(0, 24, w.shape[0], device=DEV, dtype=torch.float64).round()
    case.layers[layer] = [w * f[:, None], b * f]
    if layer == 0 and case.sb is not None:
        case.sb[:, :w.shape[0]] *= f
    if case.acts[-1] == S_ and layer == len(case.layers) - 1:
        assert w.shape[0] == 1                                              # the class head's one output row: nothing to scale
    got, _ = case.launch(split)
    r64, _ = case.reference(torch.float64)
    assert torch.equal(got == SENT, r64 == SENT)
    live = case.live()
    h, off = case.last_layer_input()
    wl = case.layers[-1][0]
    mag = ((h.abs() @ wl.abs().T + off)[live]).amax(0)[:case.oc]
    floor = 2.0 ** -39 * float(wl.abs().max()) * float(h.abs().sum(-1)[live].max())
    err = (case.rows(got).double() - case.rows(r64)).abs()[live].amax(0)
    rel = err / mag
    fl = f[:case.oc] if layer == len(case.layers) - 1 else torch.ones(case.oc, device=DEV, dtype=torch.float64)
    big = fl >= 2.0 ** -16
    small = float(rel[~big].max()) if bool((~big).any()) else 0.0
    print("\nrows 2^0..2^-24 %s %s layer %d %s: rel err rows >= 2^-16 %.2e, rows < 2^-16 %.2e (floor %.2e)" % (
        name, case.key, layer, "split" if split else "fp32", float(rel[big].max()), small, floor))
    assert float(rel[big].max()) <= case.bound
    if not split:
        assert float(rel.max()) <= case.bound
    else:
        assert bool((err[~big] <= case.bound * mag[~big] + 4 * floor).all())


# ---- 3d: rows are independent -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [SINGLE, FOUR, "bcast", "cls", "fp1", INTERP])
def test_rows_and_samples_are_independent(name):
    """Permuting the rows of every sample permutes the output rows bit for bit and leaves colmax bit-identical; permuting the
    samples (with their sample bias, per-sample sources, known rows and counters) likewise.  A position scale or a transposing
    reduction that leaks between the lanes of a tile fails here.  Every row (and every known row) carries a power of two of its
    own, 2^-20 .. 2^20: with operands of one magnitude a scale taken from a neighbour would move the pieces' exponents and no bit
    of the result."""
    case = _Case(name, "small1d", seed=sum(map(ord, name)) + 3)
    B, n = case.B, case.n
    g = torch.Generator().manual_seed(9)
    pw = lambda *s: (2.0 ** torch.randint(-20, 21, s, generator=g).double()).to(DEV)
    k = pw(B, n)
    case.src = [x if per else x * k[:, :, None] for (_, per), x in zip(case.segs, case.src)]
    if case.cint:
        case.known = case.known * pw(B, case.m)[:, :, None]
    if case.row_nu is not None:                                             # the same live count everywhere: a permutation of the live rows
        case.row_nu.fill_(n - 14)
        case.idx[:, n - 14:] = torch.tensor([1, 2, 3], dtype=torch.int32, device=DEV)
    nl = n if case.row_nu is None else n - 14
    got0, cm0 = case.launch(True)
    base = case.rows(got0).clone()
    rp = torch.stack([torch.cat([torch.randperm(nl, generator=g), torch.arange(nl, n)]) for _ in range(B)]).to(DEV)
    ar = torch.arange(B, device=DEV)[:, None]
    src0, idx0, d20 = [x.clone() for x in case.src], (case.idx.clone() if case.cint else None), (case.d2.clone() if case.cint else None)
    case.src = [x if per else x[ar, rp] for (_, per), x in zip(case.segs, src0)]
    if case.cint:
        case.idx, case.d2 = idx0[ar, rp].contiguous(), d20[ar, rp].contiguous()
    got1, cm1 = case.launch(True)
    assert torch.equal(case.rows(got1)[:, :nl], base[ar, rp][:, :nl]), "rows"
    assert cm0 is None or torch.equal(cm1, cm0)
    sp = torch.randperm(B, generator=g).to(DEV)
    case.src = [x[sp] for x in src0]
    if case.cint:
        case.idx, case.d2, case.known, case.known_nu = idx0[sp].contiguous(), d20[sp].contiguous(), case.known[sp], case.known_nu[sp].contiguous()
    if case.sb is not None:
        case.sb = case.sb[sp]
    got2, cm2 = case.launch(True)
    assert torch.equal(case.rows(got2)[:, :nl], base[sp][:, :nl]), "samples"
    assert cm0 is None or torch.equal(cm2[1:1 + B], cm0[1:1 + B][sp])


# ---- 3e: non-finite inputs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("name", ["p1_loc", "fp1", "cls"])
def test_non_finite_inputs(name, split):
    """One NaN, one +inf and one -inf, each in a different row and sample (for fp1: in three known rows, which several rows gather).
    rtk_fused.h: an output is never non-finite where the restatement's is finite -- the ReLU follows maxNum and drops a NaN --,
    and without activation it is non-finite exactly where the restatement is.  Every row that holds (gathers) no bad value, and
    the colmax of every sample that holds none, is bit-identical to the run on the clean operands."""
    case = _Case(name, "small1d", seed=sum(map(ord, name)) + 5)
    B, n = case.B, case.n
    clean, clean_cm = case.launch(split)
    bad = [(1, 10, 3, float("nan")), (4, 33, 70, float("inf")), (6, 70, 101, float("-inf"))]      # (sample, row, channel, value)
    touched = torch.zeros(B, n, dtype=torch.bool, device=DEV)
    if case.cint:
        hit = torch.zeros(B, case.m, dtype=torch.bool, device=DEV)
        for b, r, c, v in bad:
            r = r % int(case.known_nu[b])
            case.known[b, r, c] = v
            hit[b, r] = True
        idx = torch.where(case.idx.long() < case.known_nu.long().view(B, 1, 1), case.idx.long(), torch.zeros_like(case.idx.long()))
        touched = hit[torch.arange(B, device=DEV).view(B, 1, 1), idx].any(-1)
        assert int(touched.sum()) > 3
    else:
        for b, r, c, v in bad:
            case.src[0][b, r, c] = v
            touched[b, r] = True
    got, cm = case.launch(split)
    r64, _ = case.reference(torch.float64)
    g, want = case.rows(got), case.rows(r64)
    bad_g, bad_r = ~torch.isfinite(g), ~torch.isfinite(want)
    print("\nnon-finite %s %s: restatement non-finite %d, kernel non-finite %d, kernel finite where the restatement is not %d" % (
        name, "split" if split else "fp32", int(bad_r.sum()), int(bad_g.sum()), int((bad_r & ~bad_g).sum())))
    assert bool(bad_r.any()) and not bool((bad_r & ~touched[:, :, None]).any())
    assert not bool((bad_g & ~bad_r).any())
    if case.acts == [N_]:
        assert torch.equal(bad_g, bad_r)
    assert torch.equal(g[~touched], case.rows(clean)[~touched])
    if cm is not None:
        ok = ~touched.any(1)
        assert int(ok.sum()) >= B - 3
        assert torch.equal(cm[1:1 + B][ok], clean_cm[1:1 + B][ok])


# ---- 3f: signed zero under colmax -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fp32_minus_zero_bias", "split_underflow"])
def test_colmax_of_minus_zero_pre_activations(kind):
    """store_tile folds the tile maxima into colmax with an unsigned atomic maximum on the float bits: a -0.0 out of the ReLU
    (0x80000000) would beat every positive float.  One sample, two tiles.  In tile 0 every pre-activation of channels 3 and 20 is
    exactly -0.0 -- fp32-input images: zero rows, a -0.0 bias and non-positive weights; split images: inputs of 2^-126 against
    weights 2^-38 of the matrix maximum, a product of -2^-157 that the scale-and-bias fma rounds to -0.0 -- and in tile 1 the same
    channels are positive.  colmax must be the float64 maximum, without a sign bit."""
    split = kind == "split_underflow"
    B, n, C = 1, 32, 128
    g = torch.Generator(device=DEV).manual_seed(11)
    W = _f32(torch.randn(C, C, generator=g, device=DEV) / 11)
    b = _f32(torch.randn(C, generator=g, device=DEV) * 0.125)
    x = torch.zeros(B, n, C, device=DEV, dtype=torch.float64)
    ch = [3, 20]
    if split:
        W[0, 0] = 1.0                                                       # the matrix maximum: the image scale is 2^14
        W[ch] = -(2.0 ** -38)
        b[ch] = 0.0
        x[:, :16] = 2.0 ** -126
    else:
        W[ch] = -W[ch].abs()
        b[ch] = -0.0
    x[:, 16:] = -_f32(torch.randn(B, 16, C, generator=g, device=DEV)).abs() - 2.0 ** -10
    chain = F.Chain([(W, b, R)], DEV)
    if not split:
        assert bool((chain.bias.view(torch.int32)[ch] == -2 ** 31).all())   # the -0.0 survives the packing
    out = torch.full((B * n, C), SENT, device=DEV)
    cm = torch.zeros(B, C, device=DEV)
    old = F.PW_SPLIT
    F.PW_SPLIT = split
    try:
        F.pointwise(B * n, n, [(x.reshape(B * n, C).float().contiguous(), C, False)], chain, out, colmax=cm)
        torch.cuda.synchronize()
    finally:
        F.PW_SPLIT = old
    ref, rcm = pointwise_f64(n, [(x, False)], [(W, b, R)], colmax=True)
    ref32, rcm32 = pointwise_f64(n, [(x.float(), False)], [(W.float(), b.float(), R)], colmax=True)
    print("\ncolmax -0.0 %s: tile 0 bits of channels 3 / 20: %s, colmax %s (float64 %s)" % (
        kind, [hex(v & 0xffffffff) for v in out[:16, ch].contiguous().view(torch.int32).flatten().unique().tolist()],
        cm[0, ch].tolist(), rcm[0, ch].tolist()))
    assert bool((out[:16, ch] == 0).all()) and bool((ref[0, :16, ch] <= 2.0 ** -150).all())
    assert bool((rcm[0, ch] > 0).all())
    assert not bool((cm.view(torch.int32) < 0).any()), "a sign bit in colmax"
    assert torch.equal(cm, out.view(B, n, C).amax(1))
    _check("colmax -0.0 " + kind, cm, rcm, rcm32)


# ---- 3g: tap and pair -------------------------------------------------------------------------------------------------------------
def _tap_operands(B, n, seed, m=40, scales=None, binades=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s: _f32(torch.randn(*s, generator=g, device=DEV))
    bias = 0.0 if scales is not None else 0.125
    layer = [rn(128, 128) / 11, rn(128) * bias, R]
    proj = [[rn(256, 128) / 11, rn(256) * bias, N_] for _ in range(2)]
    if binades:
        f = 2.0 ** -torch.linspace(0, 24, 128, device=DEV, dtype=torch.float64).round()
        layer[0], layer[1] = layer[0] * f[:, None], layer[1] * f
        f2 = 2.0 ** -torch.linspace(0, 24, 256, device=DEV, dtype=torch.float64).round()
        for p in proj:
            p[0], p[1] = p[0] * f2[:, None], p[1] * f2
    if scales is None:
        known = rn(B, m, 128)
        idx = torch.randint(0, m, (B, n, 3), generator=g, device=DEV, dtype=torch.int32)
        nu = torch.tensor([max(1, m - 3 - b % 4) for b in range(B)], dtype=torch.int32, device=DEV)
    else:
        m = 240
        known = _f32(rn(B, m, 128) * _row_scales(m)[None, :, None])
        r = torch.arange(n, device=DEV, dtype=torch.int32)
        idx = torch.stack([r, r + 80, r + 160], 1)[None].repeat(B, 1, 1).contiguous()
        nu = torch.full((B,), m, dtype=torch.int32, device=DEV)
    d2 = (torch.rand(B, n, 3, generator=g, device=DEV) * 4 + 0.01).double()
    return known, idx, d2, nu, m, layer, proj


def _tap_launch(B, n, known, idx, d2, nu, m, layer, proj, frame_split, standalone):
    kbuf, kview = _Case._slice_buffer(known.reshape(-1, 128), 8)
    for b in range(B):
        kbuf.view(B, m, -1)[b, int(nu[b]):] = POISON
    interp = (kview, 128, m, idx.reshape(-1, 3).contiguous(), d2.float().reshape(-1, 3).contiguous(), nu)
    ch = F.Chain([tuple(layer)], DEV)
    pc = [F.Chain([tuple(p)], DEV) for p in proj]
    out = torch.full((B * n + 3, 136), SENT, device=DEV)
    cm = torch.zeros(B, 128, device=DEV)
    po = torch.full((B * n + 3, 264), SENT, device=DEV)
    if standalone:
        F.pointwise(B * n, n, [], ch, out, interp=interp, colmax=cm)
        fs = frame_split * n
        if fs:
            F.pointwise(fs, n, [(out[:fs, :128], 128, False)], pc[0], po)
        if fs < B * n:
            F.pointwise(B * n - fs, n, [(out[fs:B * n, :128], 128, False)], pc[1], po[fs:])
    else:
        F.pointwise_tap(B * n, n, ch, out, cm, interp, pc, frame_split, po)
    torch.cuda.synchronize()
    return out, cm, po, (ch, pc, kbuf)


@pytest.mark.parametrize("shape", ["small2d", "loop"])
def test_tap_is_the_standalone_launches_at_the_edge_shapes(shape):
    """rtk_pointwise_mlp_tap against rtk_pointwise_mlp for the layer and for each frame's projection on its output, bit for bit,
    at the shapes test_projection_tap_gpu.py (the engine's clouds) does not reach; nothing written beyond either output."""
    B, n = SHAPES[shape]
    ops = _tap_operands(B, n, seed=B + n)
    fsplit = B // 2 if B > 3 else 1
    out0, cm0, po0, _ = _tap_launch(B, n, *ops, fsplit, standalone=True)
    out1, cm1, po1, _ = _tap_launch(B, n, *ops, fsplit, standalone=False)
    assert torch.isfinite(out0[:B * n, :128]).all() and float(po0[:B * n, :256].std()) > 0
    assert torch.equal(out1, out0) and torch.equal(cm1, cm0) and torch.equal(po1, po0)
    assert bool((out1[B * n:] == SENT).all()) and bool((out1[:, 128:] == SENT).all())
    assert bool((po1[B * n:] == SENT).all()) and bool((po1[:, 256:] == SENT).all())
    assert not bool((cm1.view(torch.int32) < 0).any())


@pytest.mark.parametrize("what", ["magnitudes", "binades"])
def test_tap_matches_float64(what):
    B, n = SHAPES["small1d"]
    ops = _tap_operands(B, n, seed=21, scales=True if what == "magnitudes" else None, binades=what == "binades")
    known, idx, d2, nu, m, layer, proj = ops
    out, cm, po, _ = _tap_launch(B, n, *ops, 3, standalone=False)
    ref = lambda dt: tap_f64(n, (known.to(dt), idx, d2.to(dt), nu), (layer[0].to(dt), layer[1].to(dt), R),
                             [(p[0].to(dt), p[1].to(dt), N_) for p in proj], 3)
    o64, c64, p64 = ref(torch.float64)
    o32, c32, p32 = ref(torch.float32)
    g_out, g_po = out[:B * n, :128].view(B, n, 128), po[:B * n, :256].view(B, n, 256)
    if what == "magnitudes":
        zero = (_row_scales(n) == 0)[None, :].expand(B, n)
        assert bool((g_out[zero] == 0).all()) and bool((g_po[zero] == 0).all())
        for nm, g, r64, r32 in (("layer", g_out, o64, o32), ("projection", g_po, p64, p32)):
            e, e32, _ = _row_errs(g[~zero], r64[~zero], r32[~zero])
            print("\ntap magnitudes %s: worst row kernel %.2e  torch fp32 %.2e" % (nm, e, e32))
            assert e <= 5e-6 and e <= 3 * e32 + 2e-7, (nm, e, e32)
    else:
        _check("tap binades layer", g_out, o64, o32, 5e-6)
        _check("tap binades projection", g_po, p64, p32, 5e-6)
    _check("tap %s colmax" % what, cm, c64, c32, 5e-6)
    assert torch.equal(cm, g_out.amax(1))


@pytest.mark.parametrize("what", ["magnitudes", "binades"])
def test_pair_matches_float64(what):
    B, n = SHAPES["small1d"]
    g = torch.Generator(device=DEV).manual_seed(31)
    rn = lambda *s: _f32(torch.randn(*s, generator=g, device=DEV))
    mag = what == "magnitudes"
    bias = 0.0 if mag else 0.1
    colmask = torch.ones(400, device=DEV, dtype=torch.float64)
    colmask[2:16] = 0
    la = [rn(32, 400) * 0.05 * colmask, rn(32) * bias, N_]
    dims = [(128, 256), (64, 128), (32, 64), (1, 32)]
    lb = [[rn(co, ci) / ci ** 0.5, rn(co) * bias, a] for (co, ci), a in zip(dims, [R, R, R, N_ if mag else S_])]
    if mag:
        lb[-1][0] = lb[-1][0].abs()                                          # one output: a sum without cancellation (_magnitude_case)
    else:
        f = 2.0 ** -torch.linspace(0, 24, 32, device=DEV, dtype=torch.float64).round()
        la[0], la[1] = la[0] * f[:, None], la[1] * f
        f1 = 2.0 ** -torch.linspace(0, 24, 128, device=DEV, dtype=torch.float64).round()
        lb[0][0], lb[0][1] = lb[0][0] * f1[:, None], lb[0][1] * f1
    s = _row_scales(n) if mag else torch.ones(n, device=DEV, dtype=torch.float64)
    xs = [_f32(rn(B, n, c) * s[None, :, None]) for c in (2, 128, 256)]
    sb = None if mag else _f32(rn(B, 32) * 0.3 * f)
    keep, srcs = [], []
    for i, x in enumerate(xs):
        buf, view = _Case._slice_buffer(x.reshape(B * n, -1), 4 * (i + 1))
        keep.append(buf)
        srcs.append((view, x.shape[-1], False))
    ca = F.Chain([tuple(la)], DEV)
    cb = F.Chain([tuple(l) for l in lb], DEV)
    qa = torch.full((B * n + 3, 40), SENT, device=DEV)
    cls = torch.full((B + 1, 1, n), SENT, device=DEV)
    F.pointwise_pair(B * n, n, srcs, ca, qa, sb.float().contiguous() if sb is not None else None, cb, cls, 1)
    torch.cuda.synchronize()
    assert bool((qa[B * n:] == SENT).all()) and bool((qa[:, 32:] == SENT).all()) and bool((cls[B:] == SENT).all())
    ref = lambda dt: pair_f64(n, [(x.to(dt), False) for x in xs], sb.to(dt) if sb is not None else None, (la[0].to(dt), la[1].to(dt), N_),
                              [(l[0].to(dt), l[1].to(dt), l[2]) for l in lb], 1)
    a64, b64 = ref(torch.float64)
    a32, b32 = ref(torch.float32)
    ga, gb = qa[:B * n, :32].view(B, n, 32), cls[:B]
    if mag:
        zero = (s == 0)[None, :].expand(B, n)
        assert bool((ga[zero] == 0).all()) and bool((gb.permute(0, 2, 1)[zero] == 0).all())
        for nm, gg, r64, r32 in (("chain A", ga, a64, a32), ("chain B", gb.permute(0, 2, 1), b64.permute(0, 2, 1), b32.permute(0, 2, 1))):
            e, e32, _ = _row_errs(gg[~zero], r64[~zero], r32[~zero])
            print("\npair magnitudes %s: worst row kernel %.2e  torch fp32 %.2e" % (nm, e, e32))
            assert e <= 2e-6 and e <= 3 * e32 + 2e-7, (nm, e, e32)
    else:
        # chain A's rows span 24 binades: per channel, the assertion of test_weight_rows_spanning_24_binades
        x = torch.cat([torch.nn.functional.pad(xs[0], (0, 14)), xs[1], xs[2]], 2)
        magc = (x.abs() @ la[0].abs().T + la[1].abs() + sb.abs()[:, None, :]).amax((0, 1))
        floor = 2.0 ** -39 * float(la[0].abs().max()) * float(x.abs().sum(-1).max())
        err = (ga.double() - a64).abs().amax((0, 1))
        big = f >= 2.0 ** -16
        print("\npair binades chain A: rel err rows >= 2^-16 %.2e, rows < 2^-16 %.2e (floor %.2e)" % (
            float((err / magc)[big].max()), float((err / magc)[~big].max()), floor))
        assert float((err / magc)[big].max()) <= 2e-6 and bool((err[~big] <= 2e-6 * magc[~big] + 4 * floor).all())
        _check("pair binades chain B", gb, b64, b32)
