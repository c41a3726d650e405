"""CPU: the code object of the patch aggregation's tile kernel (csrc/fused_patch.hip), compiled for gfx950 with the flags it is built
with (hipcc cross-compiles without a GPU): nothing in scratch, no spilled register, and a register count that lets at least two
waves share a SIMD (512 registers per lane and SIMD) -- the kernel is sized to run next to other kernels' workgroups."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_metadata(asm_text, name_part):
    """{key: int} of the .amdhsa metadata entry of the kernel whose mangled name holds `name_part`."""
    for entry in re.split(r"\n  - \.agpr_count:", asm_text)[1:]:
        entry = ".agpr_count:" + entry
        if re.search(r"\.name:\s+\S*%s" % re.escape(name_part), entry):
            return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*\n", entry)}
    return None


def test_tile_kernel_keeps_its_state_in_registers_and_two_waves_fit_a_simd(tmp_path):
    from ratrack_amd import build as B
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src, out = os.path.join(B.CSRC, "fused_patch.hip"), str(tmp_path / "fused_patch.s")
    cmd = [hipcc] + [f for f in B.flags_for(src) if f != "-fPIC"] + ["-I", os.path.join(ROOT, "include"), "-I", B.CSRC, "-S", "--cuda-device-only", "-o", out, src]
    assert subprocess.run(cmd, stderr=subprocess.DEVNULL).returncode == 0
    md = kernel_metadata(open(out).read(), "patch_cost_tile_kernel")
    assert md is not None, "patch_cost_tile_kernel not in the code object"
    print("\npatch_cost_tile_kernel:", {k: md[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size")})
    assert md["private_segment_fixed_size"] == 0
    assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0
    assert md["vgpr_count"] <= 256                       # unified count (vector + accumulation registers): 512 / 256 = two waves
    assert md["group_segment_fixed_size"] <= 40 * 1024   # four workgroups of it in a CU's 160 KiB
