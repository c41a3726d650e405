"""GPU: the grouped stage kernels -- rtk_sa_scale / rtk_sa_scale_split, rtk_cost_volume / _split / _split_shared, rtk_patch_cost --
against the float64 restatements of their header contracts (tests/_stage_f64.py), at the shapes and edges the PNHead and the
cost volume launch them with.  The bound is that of test_fused_gpu.py::test_split_layers_carry_fp32_accuracy: rel-to-scale error
<= 2e-6 and <= 3 x the error of the same restatement in torch fp32 + 2e-7."""
import pytest
import torch

from ratrack_amd import _lib
from ratrack_amd import fused as F
from ratrack_amd import pointnet2_utils as PU

from _stage_f64 import _gather, cost_volume_f64, patch_cost_f64, sa_scale_f64, weight_net

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -5.0          # what the output buffers hold before a launch: rows / columns a kernel must not write keep it
POISON = 1e30        # q columns / rows and feature columns a kernel must not read (large and finite: a NaN could vanish in a ReLU)


@pytest.fixture(scope="module")
def eng():
    from ratrack_amd.track4d import Args, Track4D
    from _util import reference_state_dict
    net = Track4D(Args()).to(DEV).eval()
    net.load_state_dict(reference_state_dict(DEV), strict=True)
    e = F.FusedBackbone(net)
    e.sd = {k: v.detach() for k, v in net.state_dict().items()}
    return e


def _scale_err(got, r64):
    return float((got.double() - r64).abs().max() / r64.abs().max().clamp_min(1e-300))


def _check(what, got, r64, r32, bound=2e-6):
    e, e32 = _scale_err(got, r64), _scale_err(r32, r64)
    print("\n%s: kernel %.2e  torch fp32 %.2e" % (what, e, e32))
    assert e <= bound and e <= 3 * e32 + 2e-7, (what, e, e32)


# ---- set-abstraction scales ---------------------------------------------------------------------------------------------------
# (nsample, c1, widths after the offset layer): the six scales of a PNHead (fused._PNHeadWeights, model_utils.py:176-178); the three
# two-layer 64-channel ones also run split (rtk_sa_scale_split <nsample, c1>)
SA_CONFIGS = [(4, 16, (16, 32)), (8, 16, (16, 32)), (8, 32, (32,)), (16, 32, (64,)), (16, 64, (64,)), (32, 64, (64,))]
SA_KERNELS = [(ns, c1, w, k) for ns, c1, w in SA_CONFIGS for k in (("plain", "split") if w == (64,) else ("plain",))]
RADIUS = {4: 2.0, 8: 4.0, 16: 8.0, 32: 16.0}


class _SaCase:
    """Operands of one scale launch, fp32-representable.  q lives at column qcol of a (samples * n, q_pitch) buffer whose other
    columns -- and its rows >= src_nuniq[b] -- hold POISON; out is a (samples * npoint, out_pitch) buffer of SENT with the scale's
    channels at out_offset (the layouts run_pnhead gives the kernels)."""

    def __init__(self, ns, c1, widths, samples, seed, n=300, npoint=77, xyz=None, new_xyz=None, idx=None, q=None):
        g = torch.Generator(device=DEV).manual_seed(seed)
        rn = lambda *s: torch.randn(*s, generator=g, device=DEV).double()
        self.ns, self.c1, self.samples = ns, c1, samples
        if xyz is None:      # a cloud a few radii across: full balls and balls of a few hits (padded with the first)
            xyz = torch.rand(samples, n, 3, generator=g, device=DEV) * (2.5 * RADIUS[ns])
            new_xyz = xyz[:, :npoint].clone()
            new_xyz[0, 5] = 1e4                                              # an empty ball: its row of idx stays zero
            idx = PU.ball_query(RADIUS[ns], ns, xyz.contiguous(), new_xyz.contiguous())
            assert (idx[0, 5] == 0).all()
        self.n, self.npoint = xyz.shape[1], new_xyz.shape[1]
        n, npoint = self.n, self.npoint
        self.xyz, self.new_xyz, self.idx = xyz.float().contiguous(), new_xyz.float().contiguous(), idx.int().contiguous()
        self.wx, self.b1 = rn(c1, 3) * 0.25, rn(c1) * 0.125
        self.layers, cin = [], c1
        for w in widths:
            self.layers.append([rn(w, cin) / 8.0, rn(w) * 0.125])
            cin = w
        self.cout = cin
        self.layers[-1][1][[3, cin - 2]] = -1e4                              # two channels whose pre-activations are all negative
        self.src_nu = torch.tensor([n - 37 + (b % 3) * 18 for b in range(samples)], dtype=torch.int32, device=DEV).clamp(max=n)
        self.dst_nu = torch.tensor([npoint - 4 if b == 0 else npoint - (b * 7) % (npoint // 2) for b in range(samples)],
                                   dtype=torch.int32, device=DEV)
        self.qcol, self.q_pitch = 16, 16 + c1 + 8
        self.q64 = rn(samples, n, c1) if q is None else q.float().double()
        self.out_pitch, self.out_offset = 2 * self.cout + 32, self.cout

    def q_buffer(self, q64=None):
        q64 = self.q64 if q64 is None else q64
        buf = torch.full((self.samples, self.n, self.q_pitch), POISON, device=DEV)
        buf[:, :, self.qcol:self.qcol + self.c1] = q64.float()
        for b in range(self.samples):
            buf[b, int(self.src_nu[b]):] = POISON                            # duplicate source rows: read as row 0, never themselves
        return buf.reshape(self.samples * self.n, self.q_pitch).contiguous()

    def launch(self, kernel, w1img, chain=None, split=None, q64=None):
        """split: (image, inverse scale, fp32 bias) of rtk_sa_scale_split; chain: the packed layers of rtk_sa_scale."""
        q = self.q_buffer(q64)
        out = torch.full((self.samples * self.npoint, self.out_pitch), SENT, device=DEV)
        common = (self.samples, self.n, self.npoint, self.ns, self.xyz.data_ptr(), self.new_xyz.data_ptr(), self.idx.data_ptr(),
                  q.data_ptr() + 4 * self.qcol, self.q_pitch)
        tail = (out.data_ptr(), self.out_pitch, self.out_offset, self.src_nu.data_ptr(), self.dst_nu.data_ptr(), F._stream())
        if kernel == "split":
            img, inv, b2 = split
            _lib.call("rtk_sa_scale_split", *common, self.c1, w1img.data_ptr(), img.data_ptr(), inv.data_ptr(), b2.data_ptr(), *tail)
        else:
            _lib.call("rtk_sa_scale", *common, F.ceil16(self.c1) // 16, w1img.data_ptr(), chain.n, chain.arr, *tail)
        torch.cuda.synchronize()
        return out

    def run(self, kernel, q64=None):
        w1img = F.offset_image(torch.cat([self.wx, self.b1[:, None]], 1), DEV)
        if kernel == "split":
            (w2, b2), = self.layers
            img, inv = F.pack_split_device(w2.float().contiguous())
            return self.launch(kernel, w1img, split=(img, inv, b2.float().contiguous()), q64=q64)
        return self.launch(kernel, w1img, chain=F.Chain([(w, b, F.ACT_RELU) for w, b in self.layers], DEV), q64=q64)

    def reference(self, dtype, q64=None):
        c = lambda t: t.to(dtype)
        q64 = self.q64 if q64 is None else q64
        sentinel = torch.full((self.samples * self.npoint, self.out_pitch), SENT, device=DEV, dtype=dtype)
        return sa_scale_f64(c(self.xyz), c(self.new_xyz), self.idx, c(q64), c(self.wx), c(self.b1), [(c(w), c(b)) for w, b in self.layers],
                            src_nuniq=self.src_nu, out=sentinel, out_offset=self.out_offset, dst_nuniq=self.dst_nu)

    def region(self, t):
        """(rows < dst_nuniq, the scale's columns) of an output buffer -> (live rows, cout)."""
        t = t.reshape(self.samples, self.npoint, -1)[:, :, self.out_offset:self.out_offset + self.cout]
        live = torch.arange(self.npoint, device=DEV)[None, :] < self.dst_nu.long()[:, None]
        return t[live]


@pytest.mark.parametrize("samples", [3, 8])          # plain 2-D grid / XCD-aware 1-D grid
@pytest.mark.parametrize("ns,c1,widths,kernel", SA_KERNELS)
def test_sa_scale_matches_float64(ns, c1, widths, kernel, samples):
    """Ball-query tables of a real-looking cloud (padded rows, one empty ball), npoint 77 (the last tile partly empty), dst_nuniq
    below npoint and not a multiple of the centroids per tile (rows at or past it keep SENT), src_nuniq below n (the q rows past
    it hold POISON), q read at a column offset of a wider buffer, the scale's channels at an offset of a wider output row, and two
    channels whose pre-activations are all negative (exactly 0)."""
    case = _SaCase(ns, c1, widths, samples, seed=ns * 1000 + c1 * 10 + samples)
    got = case.run(kernel)
    r64, r32 = case.reference(torch.float64), case.reference(torch.float32)
    assert torch.equal(got == SENT, r64 == SENT), "rows / columns written outside the contract"
    g, want = case.region(got), case.region(r64)
    assert torch.isfinite(g).all()
    assert (g[:, [3, case.cout - 2]] == 0).all() and (want[:, [3, case.cout - 2]] == 0).all()
    _check("sa ns%d c1 %d %s %s samples %d" % (ns, c1, widths, kernel, samples), g, want, case.region(r32))


@pytest.mark.parametrize("ns,c1,widths,kernel", SA_KERNELS)
def test_sa_scale_positions_of_any_magnitude(ns, c1, widths, kernel):
    """Centroid c's neighbourhood, offsets and q rows scaled by 10^e_c, e_c cycling through -6, 6, -3, 3, 0 (one tile holds
    positions from 1e-6 to 1e6), every bias zero: the scale is positively homogeneous, each output row is 10^e_c times an O(1)
    result and must carry fp32 accuracy relative to ITSELF, not to the largest row."""
    g = torch.Generator(device=DEV).manual_seed(ns + c1)
    samples, npoint = 2, 40
    exps = torch.tensor([-6.0, 6.0, -3.0, 3.0, 0.0], device=DEV, dtype=torch.float64)
    s = (10.0 ** exps)[torch.arange(npoint, device=DEV) % 5]
    n = npoint * ns
    rn = lambda *sh: torch.randn(*sh, generator=g, device=DEV, dtype=torch.float64)
    new_xyz = rn(samples, npoint, 3) * s[None, :, None]
    xyz = (rn(samples, npoint, ns, 3) * s[None, :, None, None] + new_xyz[:, :, None, :]).reshape(samples, n, 3)
    q = (rn(samples, npoint, ns, c1) * s[None, :, None, None]).reshape(samples, n, c1)
    idx = torch.arange(n, device=DEV, dtype=torch.int32).reshape(1, npoint, ns).repeat(samples, 1, 1)
    case = _SaCase(ns, c1, widths, samples, seed=1, xyz=xyz, new_xyz=new_xyz, idx=idx, q=q)
    case.b1.zero_()
    for layer in case.layers:
        layer[1].zero_()
    case.src_nu.fill_(n)
    case.dst_nu.fill_(npoint)
    got = case.run(kernel)
    r64, r32 = case.reference(torch.float64), case.reference(torch.float32)
    scale = case.region(r64).abs().amax(1)
    live = scale > 0
    err = ((case.region(got).double() - case.region(r64)).abs().amax(1) / scale)[live]
    err32 = ((case.region(r32).double() - case.region(r64)).abs().amax(1) / scale)[live]
    assert int(live.sum()) > npoint
    print("\nsa magnitudes ns%d c1 %d %s: worst row kernel %.2e  torch fp32 %.2e" % (ns, c1, kernel, float(err.max()), float(err32.max())))
    assert float(err.max()) <= 2e-6 and float(err.max()) <= 3 * float(err32.max()) + 2e-7


@pytest.mark.parametrize("ns,c1,widths,kernel", [x for x in SA_KERNELS if x[2] == (64,)])
def test_sa_scale_weight_rows_spanning_24_binades(ns, c1, widths, kernel):
    """Rows of W2 at 2^0 .. 2^-24 of the matrix maximum (bias scaled alike).  The split image holds one power of two per matrix
    (rtk_fused.h:106-112, csrc/split_mfma.h): a row within 2^-16 of the maximum keeps full relative precision; a smaller one keeps
    the documented ABSOLUTE floor of its weights, 2^-39 of the matrix maximum
    (test_fused_gpu.py::test_split_images_are_two_fp16_pieces_and_packed_as_documented).  The fp32-input MFMA kernel has no
    image scale: every row at full relative precision.  Checked per output channel."""
    case = _SaCase(ns, c1, widths, 8, seed=ns + 7 * c1)
    (w2, _), = case.layers
    f = 2.0 ** -torch.linspace(0, 24, w2.shape[0], device=DEV, dtype=torch.float64).round()
    case.layers = [[w2 * f[:, None], torch.randn(w2.shape[0], device=DEV).double() * 0.125 * f]]
    got = case.run(kernel)
    r64 = case.reference(torch.float64)
    assert torch.equal(got == SENT, r64 == SENT)
    # per channel: the magnitude of its dot products (max over positions of |b| + sum |w| |h|), and the floor of the small rows
    B, idx = case.samples, case.idx.long()
    qidx = torch.where(idx < case.src_nu.long().view(B, 1, 1), idx, torch.zeros_like(idx))
    ar = torch.arange(B, device=DEV).view(B, 1, 1)
    h = torch.relu(case.q64[ar, qidx] + (case.xyz.double()[ar, idx] - case.new_xyz.double()[:, :, None]) @ case.wx.T + case.b1)
    h = h[torch.arange(case.npoint, device=DEV)[None, :] < case.dst_nu.long()[:, None]]      # (live rows, ns, c1)
    w, b = case.layers[0]
    mag = (h @ w.abs().T + b.abs()).amax((0, 1))
    floor = 2.0 ** -39 * float(w.abs().max()) * float(h.abs().sum(-1).max())
    err = (case.region(got).double() - case.region(r64)).abs().amax(0)
    rel, big = err / mag, f >= 2.0 ** -16
    print("\nsa rows 2^0..2^-24 ns%d c1 %d %s: rel err rows >= 2^-16 %.2e, rows < 2^-16 %.2e (abs %.2e, floor %.2e)" % (
        ns, c1, kernel, float(rel[big].max()), float(rel[~big].max()), float(err[~big].max()), floor))
    assert float(rel[big].max()) <= 2e-6
    if kernel == "plain":
        assert float(rel.max()) <= 2e-6
    else:
        assert bool((err[~big] <= 2e-6 * mag[~big] + 4 * floor).all())


@pytest.mark.parametrize("lvl,s", [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)])
def test_sa_scale_engine_images_against_folded_state_dict(eng, lvl, s):
    """The images FusedBackbone builds (offset image, packed chain or split image + scale + bias) against fold_bn of the state dict
    itself: BN folding, packing and the kernel under one bound."""
    sc = eng.enc.scales[lvl][s]
    prefix = "pn_head.sa%d.mlps.%d" % (lvl + 1, s)
    ws = []
    while "%s.layer%d.conv.weight" % (prefix, len(ws)) in eng.sd:
        i = len(ws)
        ws.append(F.fold_bn(eng.sd["%s.layer%d.conv.weight" % (prefix, i)], "%s.layer%d.bn.bn" % (prefix, i), eng.sd))
    (w1, b1), rest = ws[0], ws[1:]
    case = _SaCase(sc.nsample, w1.shape[0], tuple(w.shape[0] for w, _ in rest), 8, seed=40 + 2 * lvl + s)
    case.wx, case.b1 = w1[:, :3].to(DEV), b1.to(DEV)
    case.layers = [[w.to(DEV), b.to(DEV)] for w, b in rest]
    if sc.split_image is not None:
        out = case.launch("split", sc.w1img, split=(sc.split_image, sc.split_scale, sc.split_bias))
    else:
        out = case.launch("plain", sc.w1img, chain=sc.chain)
    r64, r32 = case.reference(torch.float64), case.reference(torch.float32)
    assert torch.equal(out == SENT, r64 == SENT)
    _check("engine sa%d scale %d (%s)" % (lvl + 1, s, "split" if sc.split_image is not None else "plain"),
           case.region(out), case.region(r64), case.region(r32))


# ---- cost volume and patch cost -------------------------------------------------------------------------------------------------
CV_SHAPES = [(3, 243), (8, 250), (16, 64), (1, 1024), (2, 17)]
PITCH = 264          # out_pitch / feat_pitch > 256


def _cv_weights(eng):
    """float64 (Wd, [(W2, b2), (W3, b3)], WeightNet 1, WeightNet 2) of the state dict's fc_layer."""
    sd = lambda k: eng.sd[k].double()
    w0 = sd("fc_layer.mlp_convs.0.weight").reshape(256, 515)
    layers = [(sd("fc_layer.mlp_convs.%d.weight" % i).reshape(256, 256), sd("fc_layer.mlp_convs.%d.bias" % i)) for i in (1, 2)]
    wn = lambda name: [(sd("fc_layer.%s.mlp_convs.%d.weight" % (name, i)).reshape(-1, 3 if i == 0 else 8),
                        sd("fc_layer.%s.mlp_convs.%d.bias" % (name, i))) for i in range(3)]
    return w0[:, 512:515], layers, wn("weightnet1"), wn("weightnet2")


def _cv_operands(B, N, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x1 = torch.randn(B, N, 3, generator=g, device=DEV)
    x2 = torch.randn(B, N, 3, generator=g, device=DEV)
    x2[:, N // 2:] = x2[:, :N - N // 2].clone()                          # every point twice: repeated neighbours
    x2[:, 1] = x1[:, 0]                                                   # a neighbour at the query point itself: direction 0
    p1 = torch.randn(B * N, 256, generator=g, device=DEV)
    p2 = torch.randn(B * N, 256, generator=g, device=DEV)
    knn = PU.knn_point(16, x2, x1)
    assert (knn[:, 0, 0] == 1).all()
    return x1, x2, p1, p2, knn


def _cv_launch(eng, variant, B, N, x1, x2, knn, p1, p2, crafted=None):
    """crafted: (split images, inverse scales, fp32 biases (2, 256), packed chain) of _cv_crafted in place of the engine's."""
    images, scales, bias23, chain = crafted if crafted is not None else (eng.cv_images, eng.cv_scales, eng.cv_bias23, eng.cv_layers)
    out = torch.full((B * N + 4, PITCH), SENT, device=DEV)
    a = (B, N, N, x1.data_ptr(), x2.data_ptr(), knn.data_ptr(), p1.data_ptr(), p2.data_ptr(), eng.cv_wd.data_ptr())
    split = (images.data_ptr(), scales.data_ptr(), bias23[0].data_ptr(), bias23[1].data_ptr(), eng.wn1.arr,
             out.data_ptr(), PITCH)
    if variant == "plain":
        _lib.call("rtk_cost_volume", *a, chain.arr, eng.wn1.arr, out.data_ptr(), PITCH, F._stream())
    elif variant == "split":
        _lib.call("rtk_cost_volume_split", *a, *split, F._stream())
    else:
        _lib.call("rtk_cost_volume_split_shared", *a, *split, int(variant[len("shared"):]), F._stream())
    torch.cuda.synchronize()
    return out


def _cv_reference(eng, dtype, B, N, x1, x2, knn, p1, p2, layers=None):
    wd, own, wn1, _ = _cv_weights(eng)
    layers = own if layers is None else layers
    c = lambda t: t.to(dtype)
    return cost_volume_f64(c(x1), c(x2), knn, c(p1).view(B, N, 256), c(p2).view(B, N, 256), c(wd), [(c(w), c(b)) for w, b in layers],
                           [(c(w), c(b)) for w, b in wn1]).reshape(B * N, 256)


@pytest.mark.parametrize("B,N", CV_SHAPES)
def test_cost_volume_matches_float64(eng, B, N):
    """rtk_cost_volume (fp32-input MFMA), rtk_cost_volume_split and rtk_cost_volume_split_shared with 0, 8, cv_shared_workgroups'
    and 12 (not a multiple of 8) workgroups -- the count is ignored unless samples % 8 == 0, and every share is bit for bit the
    full launch -- on the engine's images of the fc_layer weights; rows and columns beyond the (B N, 256) result untouched."""
    x1, x2, p1, p2, knn = _cv_operands(B, N, seed=B * 1000 + N)
    r64 = _cv_reference(eng, torch.float64, B, N, x1, x2, knn, p1, p2)
    r32 = _cv_reference(eng, torch.float32, B, N, x1, x2, knn, p1, p2)
    full = None
    for variant in ["plain", "split", "shared0", "shared8", "shared%d" % F.cv_shared_workgroups(B, N, DEV), "shared12"]:
        out = _cv_launch(eng, variant, B, N, x1, x2, knn, p1, p2)
        assert (out[B * N:] == SENT).all() and (out[:, 256:] == SENT).all(), variant
        got = out[:B * N, :256]
        _check("cost volume %s B %d N %d" % (variant, B, N), got, r64, r32)
        if variant == "split":
            full = got.clone()
        elif variant.startswith("shared"):
            assert torch.equal(got, full), variant


@pytest.mark.parametrize("B,N", CV_SHAPES)
def test_patch_cost_matches_float64(eng, B, N):
    """rtk_patch_cost on kNN tables of frame 1 in itself (every point its own first neighbour: direction 0; every point twice:
    repeated neighbours), features read from a (B N, 264) buffer whose last 8 columns hold POISON; point-major output at pitch
    264 and channel-major output, nothing written beyond either."""
    g = torch.Generator(device=DEV).manual_seed(B * 7 + N)
    x1 = torch.randn(B, N, 3, generator=g, device=DEV)
    x1[:, N // 2:] = x1[:, :N - N // 2].clone()
    knn = PU.knn_point(16, x1, x1)
    feat = torch.full((B * N, PITCH), POISON, device=DEV)
    feat[:, :256] = torch.randn(B * N, 256, generator=g, device=DEV)
    _, _, _, wn2 = _cv_weights(eng)
    ref = lambda dt: patch_cost_f64(x1.to(dt), knn, feat[:, :256].to(dt).reshape(B, N, 256),
                                    [(w.to(dt), b.to(dt)) for w, b in wn2]).reshape(B * N, 256)
    r64, r32 = ref(torch.float64), ref(torch.float32)
    out = torch.full((B * N + 4, PITCH), SENT, device=DEV)
    _lib.call("rtk_patch_cost", B, N, x1.data_ptr(), knn.data_ptr(), feat.data_ptr(), PITCH, eng.wn2.arr, out.data_ptr(), PITCH, 0,
              F._stream())
    cm = torch.full((B * 256 * N + 64,), SENT, device=DEV)
    _lib.call("rtk_patch_cost", B, N, x1.data_ptr(), knn.data_ptr(), feat.data_ptr(), PITCH, eng.wn2.arr, cm.data_ptr(), 0, 1, F._stream())
    torch.cuda.synchronize()
    assert (out[B * N:] == SENT).all() and (out[:, 256:] == SENT).all() and (cm[B * 256 * N:] == SENT).all()
    _check("patch cost point-major B %d N %d" % (B, N), out[:B * N, :256], r64, r32)
    got_cm = cm[:B * 256 * N].view(B, 256, N).permute(0, 2, 1).reshape(B * N, 256)
    _check("patch cost channel-major B %d N %d" % (B, N), got_cm, r64, r32)


# ---- cost volume: crafted inner layers ---------------------------------------------------------------------------------------------
CV_CRAFTED_SHAPES = [(3, 243), (16, 64)]


def _cv_crafted(layers):
    """[(W2, b2), (W3, b3)] float64 -> what the launches take: the two split images and inverse scales back to back
    (rtk_pack_split_layer, as FusedBackbone.__init__ builds them), the fp32 biases, and the packed chain of rtk_cost_volume."""
    images = torch.empty(2 * F.SPLIT_IMAGE_256, dtype=torch.int16, device=DEV)
    scales = torch.empty(2, dtype=torch.float32, device=DEV)
    ws = [w.float().contiguous() for w, _ in layers]
    for l, w in enumerate(ws):
        _lib.call("rtk_pack_split_layer", 256, 256, w.data_ptr(), 0, images[l * F.SPLIT_IMAGE_256:].data_ptr(), scales[l:].data_ptr(),
                  F._stream())
    torch.cuda.synchronize()
    bias = torch.stack([b.float() for _, b in layers]).contiguous()
    return images, scales, bias, F.Chain([(w, b, F.ACT_LEAKY) for w, b in layers], DEV)


def _cv_random_layers(seed, bias=0.1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV).double()
    return [[rn(256, 256) / 16, rn(256) * bias] for _ in range(2)]


def _cv_inner(eng, x1, x2, knn, p1, p2, layers, B, N):
    """float64: (the input of the last crafted layer (B, N, 16, 256), its output feat, the WeightNet's weights (B, N, 16, 256))."""
    lk = lambda t: torch.nn.functional.leaky_relu(t, 0.1)
    wd, _, wn1, _ = _cv_weights(eng)
    d = _gather(x2.double(), knn) - x1.double()[:, :, None, :]
    h = lk(p1.double().view(B, N, 256)[:, :, None, :] + _gather(p2.double().view(B, N, 256), knn) + d @ wd.T)
    (w2, b2), (w3, b3) = layers
    h2 = lk(h @ w2.T + b2)
    return h2, lk(h2 @ w3.T + b3), weight_net(d, wn1)


@pytest.mark.parametrize("B,N", CV_CRAFTED_SHAPES)
@pytest.mark.parametrize("which", [0, 1])
def test_cost_volume_weight_rows_spanning_24_binades(eng, which, B, N):
    """Rows of W2 (which = 0), then of W3 (1), at 2^0 .. 2^-24 of the matrix maximum, the bias scaled alike, on rtk_cost_volume,
    _split and _split_shared.  Per output channel c (= row c of W3), as test_sa_scale_weight_rows_spanning_24_binades, with the
    magnitude of the channel's sums mag_c = max_i sum_k wn_kc (|b3_c| + |W3_c| . |h2_k|): rows of W3 within 2^-16 of the maximum
    carry the full relative bound, smaller ones 2e-6 mag + 4 floor with floor = 2^-39 max|W3| max sum|h2| (times the point's sum
    of WeightNet weights); the fp32-input kernel the full bound on every row.  Scaled rows of W2 leave every row of W3 at full size.
    Measured (MI355X): rows within 2^-16 at most 1.9e-6 split / 1.1e-6 fp32-input -- W2 scaled at (3, 243), a channel whose WeightNet
    weight is nearly dead at every point, so that mag_c is small against the WeightNet's own rounding; 3.7e-7 elsewhere --, smaller
    rows 7.8e-6 of their magnitude split (inside the floor), 9.5e-7 fp32-input."""
    layers = _cv_random_layers(77 + which)
    f = 2.0 ** -torch.linspace(0, 24, 256, device=DEV, dtype=torch.float64).round()
    layers[which] = [layers[which][0] * f[:, None], layers[which][1] * f]
    layers = [[w.float().double(), b.float().double()] for w, b in layers]
    x1, x2, p1, p2, knn = _cv_operands(B, N, seed=B + N + which)
    crafted = _cv_crafted(layers)
    r64 = _cv_reference(eng, torch.float64, B, N, x1, x2, knn, p1, p2, layers=layers)
    h2, _, wn = _cv_inner(eng, x1, x2, knn, p1, p2, layers, B, N)
    (_, _), (w3, b3) = layers
    wsum = wn.sum(2)                                                        # (B, N, 256): the WeightNet's outputs are >= 0
    mag = ((wn * (h2.abs() @ w3.abs().T + b3.abs())).sum(2)).amax((0, 1))
    floor = 2.0 ** -39 * float(w3.abs().max()) * float(h2.abs().sum(-1).max()) * wsum.amax((0, 1))
    big = f >= 2.0 ** -16 if which == 1 else torch.ones(256, dtype=torch.bool, device=DEV)
    for variant in ["plain", "split", "shared%d" % F.cv_shared_workgroups(B, N, DEV)]:
        out = _cv_launch(eng, variant, B, N, x1, x2, knn, p1, p2, crafted=crafted)
        assert (out[B * N:] == SENT).all() and (out[:, 256:] == SENT).all(), variant
        err = (out[:B * N, :256].double() - r64).abs().amax(0)
        rel = err / mag.clamp_min(1e-300)               # (a channel the WeightNet's ReLU leaves at 0 everywhere: mag = err = 0)
        small = float(rel[~big].max()) if bool((~big).any()) else 0.0
        print("\ncost volume rows of W%d 2^0..2^-24 %s B %d N %d: rel err rows >= 2^-16 %.2e, rows < 2^-16 %.2e" % (
            which + 2, variant, B, N, float(rel[big].max()), small))
        assert float(rel[big].max()) <= 2e-6, variant
        if variant == "plain":
            assert float(rel.max()) <= 2e-6
        else:
            assert bool((err[~big] <= 2e-6 * mag[~big] + 4 * floor[~big]).all()), variant


@pytest.mark.parametrize("B,N", CV_CRAFTED_SHAPES)
def test_cost_volume_positions_of_any_magnitude(eng, B, N):
    """The p1 row of point i and the p2 row of point j scaled by 10^e, e cycling through -6, 6, -3, 3, 0 over the points, b2 = b3 = 0:
    the 16 (point, neighbour) positions of one output row differ by up to twelve decades.  Each output row's error is measured
    against its own float64 magnitude max_c sum_k |wn_kc feat_kc|, and accepted on _check's rule with that denominator.
    Measured (MI355X): worst row 1.2e-6 split, 1.1e-6 fp32-input, torch fp32 1.1e-6."""
    layers = [[w.float().double(), b.float().double()] for w, b in _cv_random_layers(91, bias=0.0)]
    x1, x2, p1, p2, knn = _cv_operands(B, N, seed=B * 3 + N)
    s = (10.0 ** torch.tensor([-6.0, 6.0, -3.0, 3.0, 0.0], device=DEV))[torch.arange(N, device=DEV) % 5].repeat(B)
    p1, p2 = (p1 * s[:, None]).contiguous(), (p2 * s.roll(2)[:, None]).contiguous()
    crafted = _cv_crafted(layers)
    r64 = _cv_reference(eng, torch.float64, B, N, x1, x2, knn, p1, p2, layers=layers)
    r32 = _cv_reference(eng, torch.float32, B, N, x1, x2, knn, p1, p2, layers=layers)
    _, feat, wn = _cv_inner(eng, x1, x2, knn, p1, p2, layers, B, N)
    den = (wn * feat).abs().sum(2).amax(-1).reshape(B * N)
    assert bool((den > 0).all())
    e32 = float(((r32.double() - r64).abs().amax(1) / den).max())
    for variant in ["plain", "split", "shared%d" % F.cv_shared_workgroups(B, N, DEV)]:
        out = _cv_launch(eng, variant, B, N, x1, x2, knn, p1, p2, crafted=crafted)
        assert (out[B * N:] == SENT).all() and (out[:, 256:] == SENT).all(), variant
        assert torch.isfinite(out[:B * N, :256]).all()
        e = float(((out[:B * N, :256].double() - r64).abs().amax(1) / den).max())
        print("\ncost volume magnitudes %s B %d N %d: worst row kernel %.2e  torch fp32 %.2e" % (variant, B, N, e, e32))
        assert e <= 2e-6 and e <= 3 * e32 + 2e-7, (variant, e, e32)


# ---- non-finite inputs ------------------------------------------------------------------------------------------------------------
def _nonfinite(what, got, ref):
    """-> (kernel non-finite mask, reference non-finite mask), with a line on where they differ."""
    bad_g, bad_r = ~torch.isfinite(got), ~torch.isfinite(ref)
    print("\n%s: reference non-finite %d, kernel non-finite %d; kernel finite where the reference is not %d, non-finite where it is "
          "finite %d; kernel values there: %s" % (what, int(bad_r.sum()), int(bad_g.sum()), int((bad_r & ~bad_g).sum()),
                                                  int((bad_g & ~bad_r).sum()), got[bad_r & ~bad_g][:6].tolist()))
    return bad_g, bad_r


@pytest.mark.parametrize("ns,c1,widths,kernel", [(4, 16, (16, 32), "plain"), (16, 64, (64,), "plain"), (16, 64, (64,), "split")])
def test_sa_scale_non_finite_inputs(ns, c1, widths, kernel):
    """One +inf and one NaN in one q row that centroids gather.  The SA kernels do NOT propagate non-finite values as the reference
    does (rtk_fused.h, rtk_sa_scale): their ReLU and the max over the neighbours follow IEEE maxNum (v_max / v_med3), which drops a
    NaN operand, and on the split path a non-finite activation turns its whole position into NaN (the two-piece split of inf), which
    the max drops too.  Pinned: an output is non-finite only where the reference's is, and some outputs the reference has as NaN
    come out finite."""
    case = _SaCase(ns, c1, widths, 3, seed=5)
    p = int(case.idx[1, 10, 0])
    assert p < int(case.src_nu[1])
    q = case.q64.clone()
    q[1, p, 0], q[1, p, 1] = float("inf"), float("nan")
    got = case.run(kernel, q64=q)
    ref = case.reference(torch.float64, q64=q)
    bad_g, bad_r = _nonfinite("sa ns%d c1 %d %s" % (ns, c1, kernel), case.region(got), case.region(ref))
    assert bad_r.any()
    assert not (bad_g & ~bad_r).any()
    assert (bad_r & ~bad_g).any()


@pytest.mark.parametrize("variant", ["plain", "split"])
def test_cost_volume_non_finite_inputs(eng, variant):
    """One +inf and one NaN in one gathered p2 row."""
    B, N = 2, 64
    x1, x2, p1, p2, knn = _cv_operands(B, N, seed=3)
    r = int(knn[1, 5, 3]) + N
    p2[r, 7], p2[r, 100] = float("inf"), float("nan")
    got = _cv_launch(eng, variant, B, N, x1, x2, knn, p1, p2)[:B * N, :256]
    ref = _cv_reference(eng, torch.float64, B, N, x1, x2, knn, p1, p2)
    bad_g, bad_r = _nonfinite("cost volume %s" % variant, got, ref)
    assert bad_r.any()
    assert torch.equal(bad_g, bad_r)


def test_patch_cost_non_finite_inputs(eng):
    """One +inf and one NaN in one gathered feature row."""
    B, N = 2, 64
    g = torch.Generator(device=DEV).manual_seed(9)
    x1 = torch.randn(B, N, 3, generator=g, device=DEV)
    knn = PU.knn_point(16, x1, x1)
    feat = torch.randn(B * N, 256, generator=g, device=DEV)
    feat[N + 9, 7], feat[N + 9, 100] = float("inf"), float("nan")
    _, _, _, wn2 = _cv_weights(eng)
    ref = patch_cost_f64(x1.double(), knn, feat.double().view(B, N, 256), wn2).reshape(B * N, 256)
    out = torch.full((B * N, 256), SENT, device=DEV)
    _lib.call("rtk_patch_cost", B, N, x1.data_ptr(), knn.data_ptr(), feat.data_ptr(), 256, eng.wn2.arr, out.data_ptr(), 256, 0, F._stream())
    torch.cuda.synchronize()
    bad_g, bad_r = _nonfinite("patch cost", out, ref)
    assert bad_r.any()
    assert torch.equal(bad_g, bad_r)
