"""CPU: the host launch layer of the per-point chain family (csrc/fused_pointwise.hip) and the layer arrays fused.Chain hands to it.

1. rtk_pointwise_mlp, rtk_pointwise_mlp_tap and rtk_pointwise_mlp_pair refuse the same malformed calls, each under its own name and with
   the return code the three separate validators gave before they were merged (recorded from a build of that commit, written here as
   literals).  The arguments are ctypes structs with made-up non-null addresses, so this runs only where there is NO device: there a
   validator that lets a call through ends in a launch error, on a device it would end in a kernel reading those addresses.
2. Chain's three _Layer arrays (fp32 images, split images, the paired blob) against the closed-form offsets and a second construction
   written out longhand.
"""
import ctypes
import re

import pytest
import torch

from ratrack_amd import _lib, fused
from ratrack_amd.abi import Interp, Layer, Src

INVALID, LAUNCH, UNSUPPORTED = -1, -2, -3      # RTK_ERR_* (include/rtk_pointnet2.h)
MAX_SRC = 4                                    # RTK_MAX_SRC
A = 0x100000                                   # a made-up device address (never dereferenced on the host)
SPLIT, RELU = fused.LAYER_SPLIT, fused.ACT_RELU


def image_bytes(u, v, split):
    """One layer's image from u to v blocks of 16 channels: 1 KiB fragments, u v of them or, split, two pieces per PAIR of input blocks."""
    return 1024 * (((u + 1) // 2) * v * 2 if split else u * v)


def layers(blocks, base, split=True, act=RELU):
    """A contiguous chain from `base` -> (Layer array, address where it ends)."""
    arr = (Layer * (len(blocks) - 1))()
    for l, (u, v) in enumerate(zip(blocks, blocks[1:])):
        arr[l] = Layer(base, A, u, v, act | (SPLIT if split else 0), 1.0)
        base += image_bytes(u, v, split)
    return arr, base


def sources(*channels):
    """MAX_SRC + 1 valid sources (so that a count of MAX_SRC + 1 reads nothing it should not), the first len(channels) as given."""
    arr = (Src * (MAX_SRC + 1))()
    for i in range(MAX_SRC + 1):
        ch = channels[i] if i < len(channels) else 16
        arr[i] = Src(A, (ch + 3) // 4 * 4, ch, 0)
    return arr


ORDER = {
    "pointwise_mlp": ("rows", "rows_per_sample", "interp", "nsrc", "srcs", "sample_bias", "nlayers", "layers", "out", "out_pitch",
                      "out_channels", "out_channel_major", "row_nuniq", "colmax"),
    "pointwise_mlp_tap": ("rows", "rows_per_sample", "interp", "layers", "out", "out_pitch", "colmax", "proj", "frame_split", "proj_out",
                          "proj_pitch"),
    "pointwise_mlp_pair": ("rows", "rows_per_sample", "nsrc", "srcs", "sample_bias", "layers", "out", "out_pitch", "out_channels",
                           "nlayers_b", "layers_b", "out_b", "out_b_channels"),
}


def valid(entry):
    """A call the entry point accepts: 2 samples of 96 rows."""
    a = dict(rows=192, rows_per_sample=96, sample_bias=None, out=A, colmax=None)
    if entry == "pointwise_mlp":       # [interp 64 | 64] -> the flow head's instance <8, 8, 4, 2, 1>
        a.update(interp=Interp(A, 64, 64, 32, A, A, None), nsrc=1, srcs=sources(64), nlayers=4, layers=layers([8, 8, 4, 2, 1], A)[0],
                 out_pitch=16, out_channels=16, out_channel_major=0, row_nuniq=None)
    elif entry == "pointwise_mlp_tap":
        proj = (Layer * 2)(layers([8, 16], A, act=0)[0][0], layers([8, 16], 2 * A, act=0)[0][0])
        a.update(interp=Interp(A, 128, 128, 32, A, A, None), layers=layers([8, 8], A)[0], out_pitch=128, colmax=A, proj=proj, frame_split=1,
                 proj_out=A, proj_pitch=256)
    else:
        la, end = layers([25, 2], A)
        a.update(nsrc=3, srcs=sources(2, 128, 256), layers=la, out_pitch=32, out_channels=32, nlayers_b=4,
                 layers_b=layers([16, 8, 4, 2, 1], end)[0], out_b=A, out_b_channels=1)
    return a


def call(entry, a):
    args = [ctypes.pointer(a[k]) if isinstance(a[k], Interp) else a[k] for k in ORDER[entry]]
    return _lib.call("rtk_" + entry, *args, None)


def put(key, value):
    return lambda a: a.__setitem__(key, value)


def field(key, index, name, value):
    """a[key][index].name = value, or += value for a string "+n"."""
    def f(a):
        s = a[key] if index is None else a[key][index]
        setattr(s, name, getattr(s, name) + int(value) if isinstance(value, str) else value)
    return f


def no_instance(a):      # U = 3, V = 1: a well-formed chain that no PW_CASE covers
    a.update(interp=None, srcs=sources(48), nlayers=1, layers=layers([3, 1], A)[0])


MLP, TAP, PAIR = "pointwise_mlp", "pointwise_mlp_tap", "pointwise_mlp_pair"
# (variant, entry points, the one violation, the code the separate validators returned for it)
VARIANTS = [
    ("rows = 0", (MLP, TAP, PAIR), put("rows", 0), INVALID),
    ("rows not a multiple of rows_per_sample", (MLP, TAP, PAIR), put("rows", 193), INVALID),
    ("more than 65535 samples", (MLP, TAP, PAIR), lambda a: a.update(rows=65536, rows_per_sample=1), INVALID),
    ("source with channels = 0", (MLP, PAIR), field("srcs", 0, "channels", 0), INVALID),
    ("source pitch not a multiple of 4", (MLP, PAIR), field("srcs", 0, "pitch", "+2"), INVALID),
    ("source pitch below its channels rounded up to 4", (MLP,), field("srcs", 0, "pitch", 60), INVALID),
    ("source pitch below its channels rounded up to 4", (PAIR,), field("srcs", 1, "pitch", 124), INVALID),
    ("nsrc = RTK_MAX_SRC + 1", (MLP, PAIR), put("nsrc", MAX_SRC + 1), INVALID),
    ("interpolation segment with a null idx", (MLP, TAP), field("interp", None, "idx", None), INVALID),
    ("interpolation channels not a multiple of 4", (MLP, TAP), field("interp", None, "channels", "-2"), INVALID),
    ("64-channel interpolation segment", (TAP,), field("interp", None, "channels", 64), INVALID),
    ("layer without RTK_LAYER_SPLIT", (TAP, PAIR), field("layers", 0, "act", RELU), INVALID),
    ("projection without RTK_LAYER_SPLIT", (TAP,), field("proj", 1, "act", 0), INVALID),
    ("chain B layer without RTK_LAYER_SPLIT", (PAIR,), field("layers_b", 2, "act", RELU), INVALID),
    ("split and fp32 layers in one chain", (MLP,), field("layers", 2, "act", RELU), INVALID),
    ("second image not contiguous with the first", (MLP,), field("layers", 1, "w_packed", "+1024"), INVALID),
    ("second image not contiguous with the first", (PAIR,), field("layers_b", 0, "w_packed", "+1024"), INVALID),
    ("output pitch not a multiple of 4", (MLP, TAP, PAIR), lambda a: a.update(out_pitch=a["out_pitch"] + 2), INVALID),
    ("output pitch below the channels", (MLP, TAP, PAIR), lambda a: a.update(out_pitch=a["out_pitch"] - 4), INVALID),
    ("projection pitch not a multiple of 4", (TAP,), put("proj_pitch", 258), INVALID),
    ("projection pitch below the channels", (TAP,), put("proj_pitch", 252), INVALID),
    ("no kernel instance (U = 3, V = 1)", (MLP,), no_instance, UNSUPPORTED),
]
CASES = [pytest.param(e, mutate, code, id="%s-%s" % (e, name)) for name, entries, mutate, code in VARIANTS for e in entries]

no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="made-up addresses: only where a call that gets through cannot run")


def refusal(entry, a):
    """-> (return code, the library's message) of a refused call."""
    with pytest.raises(_lib.RtkError) as e:
        call(entry, a)
    m = re.match(r"rtk_%s failed \((-?\d+)\): (.*)" % entry, str(e.value), re.S)
    assert m, str(e.value)
    return int(m.group(1)), m.group(2)


@no_device
@pytest.mark.parametrize("entry", [MLP, TAP, PAIR])
def test_valid_call_gets_to_the_launch(entry):
    """The table's starting points are well formed: nothing refuses them before the launch, which fails for want of a device."""
    code, msg = refusal(entry, valid(entry))
    assert code == LAUNCH and msg.startswith(entry + ": launch failed"), (code, msg)


@no_device
@pytest.mark.parametrize("entry, mutate, expected", CASES)
def test_malformed_call_is_refused(entry, mutate, expected):
    a = valid(entry)
    mutate(a)
    code, msg = refusal(entry, a)
    assert code == expected, (code, msg)
    assert msg.startswith(entry + ": "), msg


# ---- Chain's layer arrays ------------------------------------------------------------------------------------------------------------

PW_CASES = [(1, 2), (4, 6), (6, 12), (8, 4), (8, 8), (10, 8), (12, 8), (8, 16), (16, 8, 4, 2, 1), (8, 8, 4, 2, 1), (25, 2), (8, 2)]


def make_chain(blocks, seed):
    """A chain with the instance's block counts and channel counts that are no multiples of 16 (16 k - 3 in, 16 k - 1 out)."""
    g = torch.Generator().manual_seed(seed)
    spec, cin = [], 16 * blocks[0] - 3
    for l, v in enumerate(blocks[1:]):
        cout = 16 * v - 1
        spec.append((torch.randn(cout, cin, generator=g, dtype=torch.float64) * 2.0 ** l, torch.randn(cout, generator=g, dtype=torch.float64),
                     (fused.ACT_RELU, fused.ACT_LEAKY, fused.ACT_NONE, fused.ACT_SIGMOID)[l]))
        cin = cout
    return spec, fused.Chain(spec, "cpu")


def longhand(spec):
    """(cin16, cout16, act, inverse scale of the split image) per layer, from the weights alone."""
    out = []
    for w, _, act in spec:
        cout, cin = w.shape
        out.append(((cin + 15) // 16, (cout + 15) // 16, act, fused.pack_layer_split16(w)[1]))
    return out


def check_array(arr, want, w_base, bias_base, split):
    assert len(arr) == len(want)
    w_off = b_off = 0
    for l, (u, v, act, inv) in zip(arr, want):
        assert l.w_packed - w_base == (2 * w_off if split else 4 * w_off)
        assert l.bias - bias_base == 4 * b_off
        assert (l.cin16, l.cout16, l.act, l.inv_scale) == ((u, v, act | SPLIT, inv) if split else (u, v, act, 0.0))
        w_off += ((u + 1) // 2) * v * 2 * 512 if split else u * v * 256
        b_off += 16 * v
    return w_off


@pytest.mark.parametrize("blocks", PW_CASES, ids=lambda b: "x".join(map(str, b)))
def test_chain_layer_arrays(blocks):
    spec, c = make_chain(blocks, seed=sum(blocks))
    want = longhand(spec)
    assert (c.n, c.cout, c.cout16) == (len(spec), spec[-1][0].shape[0], blocks[-1]) and c.dims == [tuple(w.shape) for w, _, _ in spec]
    assert c.macs == sum(w.shape[0] * w.shape[1] for w, _, _ in spec)
    assert check_array(c.arr, want, c.blob.data_ptr(), c.bias.data_ptr(), False) == c.blob.numel()
    sp = c.split_arr()
    assert sp is c.split_arr()                                     # built once
    image = c._split[1]
    assert image.dtype == torch.int16 and check_array(sp, want, image.data_ptr(), c.bias.data_ptr(), True) == image.numel()


def test_chain_split_pair():
    (sa, a), (sb, b) = make_chain((25, 2), 1), make_chain((16, 8, 4, 2, 1), 2)
    la, lb = a.split_pair(b)
    assert a.split_pair(b)[0] is la and a._pairs[id(b)][3] is b    # built once per partner, which it keeps alive
    blob = a._pairs[id(b)][2]
    assert torch.equal(blob, torch.cat([a._split[1], b._split[1]]))
    # chain A's images from the blob's start, chain B's first exactly where chain A's end; biases and inverse scales of the unpaired arrays
    end_a = check_array(la, longhand(sa), blob.data_ptr(), a.bias.data_ptr(), True)
    assert end_a == a._split[1].numel() and lb[0].w_packed == blob.data_ptr() + 2 * end_a
    assert end_a + check_array(lb, longhand(sb), blob.data_ptr() + 2 * end_a, b.bias.data_ptr(), True) == blob.numel()
    for pair, alone in ((la, a.split_arr()), (lb, b.split_arr())):
        assert [(l.bias, l.inv_scale) for l in pair] == [(l.bias, l.inv_scale) for l in alone]
