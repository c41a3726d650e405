"""CPU: the code objects of the per-point chain kernels (csrc/fused_pointwise.hip), compiled for gfx950 with the flags they are built
with (hipcc cross-compiles without a GPU).  Every chain and tap kernel instance -- the serial loops the default entries run (pointwise_mlp_kernel)
and the software-pipelined comparison loops, which hold the next group's rows in registers (pointwise_mlp_pipelined_kernel) -- must keep its state in registers (nothing in
scratch, no spilled vector or scalar register), stay within the 256 registers of the two workgroups per CU its launch bounds promise
(what other batches' kernels can co-reside with does not change), and keep the 32 KiB weight double buffer as its only LDS.

Figures of this tree (hipcc of ROCm 7.2; the tests print every instance's): all 32 pipelined and 48 serial chain instances and both
tap kernels have no scratch and no spill; the largest pipelined chain instance has 224 registers, the largest serial one 180, the
tap kernels 208 (pipelined) and 132 (serial).  Before the kernels read their arguments where they use them (pw_args_now) and formed
per-lane addresses inside the trip, 30 pipelined instances parked 8 - 49 scalar registers in vector lanes and the serial loops
62 - 663, nine of them with 12 - 308 bytes of scratch."""
import re

import pytest

from test_sa_code_object_cpu import compile_to_asm, kernels_metadata

LDS_BYTES = 32 * 1024           # 2 * PW_F fragments of 1 KiB
MAX_VGPRS = 512 // 2            # __launch_bounds__(256, 2): two waves per SIMD
KEYS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size")


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    text = compile_to_asm("fused_pointwise.hip", tmp_path_factory.mktemp("pw"))
    chains = dict(kernels_metadata(text, "pointwise_mlp_kernel"), **kernels_metadata(text, "pointwise_mlp_pipelined_kernel"))
    return chains, kernels_metadata(text, "pointwise_tap_kernel")


def short(name):
    return re.sub(r"^_Z\d+pointwise_|EEv\d+\w+Params$", "", name).replace("ELi", ",").replace("ELb", ";").replace("ILi", "<")


def check_all(mds):
    """Every instance of `mds`: printed, then asserted -- in registers, within the launch bounds' register count, the LDS unchanged."""
    bad = []
    print()
    for name, md in sorted(mds.items()):
        print("%-44s %s" % (short(name), " ".join("%s=%d" % (k.replace("_count", "").replace("_fixed_size", ""), md[k]) for k in KEYS)))
        if md["private_segment_fixed_size"] != 0 or md["vgpr_spill_count"] != 0 or md["sgpr_spill_count"] != 0 or \
                md["vgpr_count"] > MAX_VGPRS or md["group_segment_fixed_size"] != LDS_BYTES:
            bad.append(short(name))
    assert not bad, "%d of %d instances: %s" % (len(bad), len(mds), bad)


def pipelined(mds, flag):
    """the chain kernels: by name (pointwise_mlp_pipelined_kernel runs the pipelined loop); the tap kernel: by its last template argument"""
    return {n: md for n, md in mds.items() if ("pointwise_mlp_pipelined_kernel" in n or n.endswith("Lb1EEv9TapParams")) == flag}


def test_pipelined_chain_instances(metadata):
    mds = pipelined(metadata[0], True)
    assert len(mds) == 32, len(mds)             # twelve shapes x (interp, split) less the sixteen pw_has_pipe routes to the serial loop
    check_all(mds)


def test_serial_chain_instances(metadata):
    mds = pipelined(metadata[0], False)
    assert len(mds) == 48, len(mds)             # twelve shapes x (interp, split)
    check_all(mds)


def test_pipelined_tap_instance(metadata):
    mds = pipelined(metadata[1], True)
    assert len(mds) == 1
    check_all(mds)


def test_serial_tap_instance(metadata):
    mds = pipelined(metadata[1], False)
    assert len(mds) == 1
    check_all(mds)
