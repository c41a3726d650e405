"""CPU: the host half of ratrack_amd/track_train.py -- the packed-gradient layout, the refusal of a captured sequence step, the native
surface (declared, bound, built for gfx950 and exported) and the constants the Python side restates."""
import ctypes
import os
import re

import pytest
import torch

import _track_train_util as U
from ratrack_amd import abi, build as B, tracker as T, track_train as TT
from ratrack_amd.track4d import Args, Track4D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ["rtk_affinity_train", "rtk_affinity_wgrad", "rtk_object_descriptors_bwd"]


def test_unpack_is_the_inverse_of_pack_affinity():
    net = Track4D(Args())
    packed = T.pack_affinity(net.affinity)
    assert packed.numel() == TT.WEIGHTS
    got = TT.unpack_affinity_grad(packed)
    named = list(net.affinity.named_parameters())
    assert len(got) == len(named) == 10
    for g, (name, p) in zip(got, named):
        assert g.shape == p.shape and torch.equal(g, p.detach()), name
    bwd = TT.pack_affinity_bwd(net.affinity)
    assert bwd.numel() == TT.WEIGHTS_BWD and torch.equal(bwd[:141 * 564].view(564, 141), named[0][1].detach())
    with pytest.raises(ValueError, match="packed Affinity image"):
        TT.unpack_affinity_grad(packed[:-1])


def test_a_captured_sequence_step_is_refused():
    with pytest.raises(ValueError, match="graph=True"):
        TT.SequenceTrainer(Track4D(Args()), streams=4, graph=True)


def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "rtk_train.h")).read()
    lib = ctypes.CDLL(B.build(verbose=False))
    for name in ENTRY:
        assert re.search(r"RTK_EXPORT int %s\(" % name, text), name
        assert hasattr(lib, name) and name in abi.SIGNATURES, name
    for name, value in (("RTK_AFF_TRAIN_ROW", TT.ROW), ("RTK_AFF_TRAIN_CHUNK", TT.CHUNK)):
        assert re.search(r"#define %s %d\b" % (name, value), text), name
    assert TT.ROW >= 141 + 564 + 282 + 70 + 35 + 564 + 282 + 70 + 35 + 1 + 1
    assert TT.workspace_floats(513) == 513 * TT.ROW + 2 * TT.WEIGHTS
    assert os.path.exists(os.path.join(ROOT, "ratrack_amd", "csrc", "track_train.hip"))


def test_the_torch_formulation_treats_undefined_streams_as_zero():
    """The arbiter itself: a stream that is not defined, or has no previous objects, adds nothing; the gradient of the rest is that of
    the scaled sum of the per-stream cross entropies."""
    case = U.pair_case("cpu")
    net = Track4D(Args())
    mlp = U.mlp_copy(net.affinity, torch.float64)
    desc = case["curr"].double().requires_grad_(True)
    total, losses = U.desc_term(mlp, desc, case["prev"].double(), case["m"], case["num_objects"], case["target"], (0, 1, 1, 1), case["scale"])
    total.backward()
    assert float(losses[0]) == 0.0 and float(losses[3]) == 0.0 and float(losses[1]) > 0
    assert not desc.grad[0].any() and not desc.grad[3].any() and desc.grad[1, :17].any() and not desc.grad[1, 17:].any()
    assert U.bound(torch.ones(3), torch.ones(3)) == 1e-6
