"""GPU: rtk_pointwise_mlp_pair -- the two readers of one wide per-point tensor in one launch (the decoder front: the sa1 projections
of [raw (2) | f1 (128) | cor (256)] with a per-sample bias, row-major, and the class head 256 -> 128 -> 64 -> 32 -> 1 on cor,
channel-major) -- against the two standalone rtk_pointwise_mlp launches it replaces.  Both outputs bit for bit: each chain keeps its
own images, inverse scales, bias and position scale (chain B's from the 16 slots of cor alone).

Shapes, the smallest at which the tile logic can go wrong:
  B = 3,   N = 80    2-D grid; the second row group has one live wave and three wholly invalid ones
  B = 3,   N = 77    ... holds 13 live rows: one partial tile and two wholly invalid waves
  B = 8,   N = 243   XCD-aware 1-D grid; partial last tile
  B = 136, N = 128   one workgroup per sample: every workgroup loops over two groups and the weight stream wraps
  B = 264, N = 130   ... over three groups, the last with 2 live rows
  B = 1,   N = 1024  one sample, 16 groups"""
import pytest
import torch

from ratrack_amd import fused as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(3, 80), (3, 77), (8, 243), (136, 128), (264, 130), (1, 1024)]


def _chains(seed, plain_b=False):
    """Random chains of the decoder front's shapes.  plain_b: chain B without biases and without the final sigmoid, so that its output is
    proportional to its input (the scale case)."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    a = F.Chain([(rnd(32, 400) * 0.05, rnd(32) * 0.1, F.ACT_NONE)], DEV)
    dims = [(128, 256), (64, 128), (32, 64), (1, 32)]
    acts = [F.ACT_RELU, F.ACT_RELU, F.ACT_RELU, F.ACT_NONE if plain_b else F.ACT_SIGMOID]
    b = F.Chain([(rnd(co, ci) / ci ** 0.5, rnd(co) * (0.0 if plain_b else 0.1), act) for (co, ci), act in zip(dims, acts)], DEV)
    return a, b


def _operands(B, N, seed, f1_scale=1.0, cor_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(B * N, 4, generator=g).to(DEV)
    feat = torch.randn(B * N, 256, generator=g).to(DEV) * f1_scale          # f1: the first 128 columns of a 256-wide buffer, as in the backbone
    cor = torch.randn(B * N, 256, generator=g).to(DEV) * cor_scale
    sb = torch.randn(B, 32, generator=g).to(DEV)
    return [(raw, 2, False), (feat[:, 0:128], 128, False), (cor, 256, False)], sb


def _standalone(B, N, srcs, sb, ca, cb):
    cls = torch.full((B, 1, N), float("nan"), device=DEV)
    q = torch.full((B * N, 32), float("nan"), device=DEV)
    F.pointwise(B * N, N, srcs[-1:], cb, cls, out_channels=1, channel_major=True)
    F.pointwise(B * N, N, srcs, ca, q, sample_bias=sb)
    return q, cls


@pytest.mark.parametrize("B,N", SHAPES)
def test_pair_is_the_two_standalone_launches(B, N):
    ca, cb = _chains(11)
    srcs, sb = _operands(B, N, 100 * B + N)
    q0, cls0 = _standalone(B, N, srcs, sb, ca, cb)
    q1 = torch.full((B * N, 32), float("nan"), device=DEV)
    cls1 = torch.full((B, 1, N), float("nan"), device=DEV)
    F.pointwise_pair(B * N, N, srcs, ca, q1, sb, cb, cls1, 1)
    torch.cuda.synchronize()
    assert torch.isfinite(q0).all() and torch.isfinite(cls0).all() and float(cls0.std()) > 0
    assert torch.equal(q1, q0), "chain A"
    assert torch.equal(cls1, cls0), "chain B"


def test_each_chain_keeps_its_own_position_scale():
    """f1 at 2^40, cor at 2^-40: chain A's position scale comes from f1, chain B's must come from cor alone -- under chain A's scale
    every piece of cor would vanish below fp16's range and chain B (no bias, no sigmoid here) would give zeros."""
    B, N = 8, 243
    ca, cb = _chains(12, plain_b=True)
    srcs, sb = _operands(B, N, 7, f1_scale=2.0 ** 40, cor_scale=2.0 ** -40)
    q0, cls0 = _standalone(B, N, srcs, sb, ca, cb)
    q1 = torch.full((B * N, 32), float("nan"), device=DEV)
    cls1 = torch.full((B, 1, N), float("nan"), device=DEV)
    F.pointwise_pair(B * N, N, srcs, ca, q1, sb, cb, cls1, 1)
    torch.cuda.synchronize()
    assert torch.isfinite(q0).all() and torch.isfinite(cls0).all()
    assert float(cls0.abs().max()) > 2.0 ** -48 and float((cls0 != 0).float().mean()) > 0.5
    assert torch.equal(q1, q0), "chain A"
    assert torch.equal(cls1, cls0), "chain B"


def test_nothing_is_written_outside_the_outputs():
    """Both outputs inside larger poisoned buffers: rows before and after, columns left and right of chain A's 32, samples before and
    after chain B's."""
    B, N = 3, 80
    ca, cb = _chains(13)
    srcs, sb = _operands(B, N, 9)
    q0, cls0 = _standalone(B, N, srcs, sb, ca, cb)
    qbuf = torch.full((B * N + 8, 48), 7.0, device=DEV)
    cbuf = torch.full((B + 2, 1, N), 7.0, device=DEV)
    F.pointwise_pair(B * N, N, srcs, ca, qbuf[4:4 + B * N, 8:40], sb, cb, cbuf[1:1 + B], 1)
    torch.cuda.synchronize()
    assert torch.equal(qbuf[4:4 + B * N, 8:40], q0) and torch.equal(cbuf[1:1 + B], cls0)
    assert torch.all(qbuf[:4] == 7.0) and torch.all(qbuf[4 + B * N:] == 7.0)
    assert torch.all(qbuf[:, :8] == 7.0) and torch.all(qbuf[:, 40:] == 7.0)
    assert torch.all(cbuf[0] == 7.0) and torch.all(cbuf[1 + B] == 7.0)
