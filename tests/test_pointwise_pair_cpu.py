"""CPU: the code objects of the two per-point kernels this change adds (csrc/fused_pointwise.hip), compiled for gfx950 with the flags
the library is built with (hipcc cross-compiles without a GPU): pointwise_pair_kernel (the two readers of cor in one launch: 100
input registers next to the class head's layers) and the <12, 8> split instance with interpolation of pointwise_mlp_kernel (fp3 with
linear3 composed in: 128 interpolated + 64 skip channels).  Both must keep two waves per SIMD (at most 256 of the 512 vector
registers, __launch_bounds__(256, 2)), nothing in scratch, no spilled vector register, and the 32 KiB weight double buffer in LDS."""
import os
import shutil
import subprocess

import pytest

from test_cost_volume_consts_cpu import kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {
    "pair": "pointwise_pair_kernelILi25ELi2ELi16ELi8ELi4ELi2ELi1EE",
    "fp3 with linear3": "pointwise_mlp_kernelILi12ELi8ELi0ELi0ELi0ELb1ELb1EE",       # <12, 8, 0, 0, 0, INTERP, SPLIT>
}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    from ratrack_amd import build as B
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src, out = os.path.join(B.CSRC, "fused_pointwise.hip"), str(tmp_path_factory.mktemp("pw") / "fused_pointwise.s")
    cmd = [hipcc] + [f for f in B.flags_for(src) if f != "-fPIC"] + ["-I", os.path.join(ROOT, "include"), "-I", B.CSRC, "-S", "--cuda-device-only", "-o", out, src]
    assert subprocess.run(cmd, stderr=subprocess.DEVNULL).returncode == 0
    return open(out).read()


@pytest.mark.parametrize("which", sorted(KERNELS))
def test_two_waves_per_simd_and_no_scratch(asm, which):
    md = kernel_metadata(asm, KERNELS[which])
    assert md is not None, "%s not in the code object" % KERNELS[which]
    print("\n%s:" % which, {k: md[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "sgpr_spill_count", "group_segment_fixed_size")})
    assert md["vgpr_count"] + md["agpr_count"] <= 256                         # two waves of 256 lanes' registers per SIMD
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0
    assert md["group_segment_fixed_size"] == 32 * 1024
    assert md["max_flat_workgroup_size"] == 256
