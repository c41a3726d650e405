"""CPU: the code object of the forward cost volume on the 16-position tile (csrc/fused_split.hip, cost_volume_split_kernel16), compiled
for gfx950 with the flags it is built with (hipcc cross-compiles without a GPU).  The kernel exists to put TWO waves on a SIMD: at most
256 registers per lane in all (architectural + accumulation), nothing in scratch, no spilled vector or scalar register, eight waves per
workgroup, and the weight stream, the staged rows and the constants within a CU's 160 KiB of LDS."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "cost_volume_split_kernel16"


def kernel_metadata(asm_text, name_part):
    """{key: int} of the .amdhsa metadata entry of the kernel whose mangled name holds `name_part`."""
    for entry in re.split(r"\n  - \.agpr_count:", asm_text)[1:]:
        entry = ".agpr_count:" + entry
        if re.search(r"\.name:\s+\S*%s" % re.escape(name_part), entry):
            return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*\n", entry)}
    return None


def kernel_text(asm_text, name_part):
    """The instructions of the kernel whose mangled name holds `name_part`: from its label to the end of the function."""
    m = re.search(r"^_Z\w*%s\w*:[^\n]*\n(.*?)^\.Lfunc_end" % re.escape(name_part), asm_text, re.S | re.M)
    return m.group(1) if m else None


def test_tile16_kernel_fits_two_waves_per_simd(tmp_path):
    from ratrack_amd import build as B
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src, out = os.path.join(B.CSRC, "fused_split.hip"), str(tmp_path / "fused_split.s")
    cmd = [hipcc] + [f for f in B.flags_for(src) if f != "-fPIC"] + ["-I", os.path.join(ROOT, "include"), "-I", B.CSRC, "-S", "--cuda-device-only", "-o", out, src]
    assert subprocess.run(cmd, stderr=subprocess.DEVNULL).returncode == 0
    asm = open(out).read()
    md, text = kernel_metadata(asm, KERNEL), kernel_text(asm, KERNEL)
    assert md is not None and text is not None, "cost_volume_split_kernel16 not in the code object"
    print("\ncost_volume_split_kernel16:", {k: md[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count",
                                                                "private_segment_fixed_size", "group_segment_fixed_size", "max_flat_workgroup_size")})
    assert md["vgpr_count"] <= 256 and md["agpr_count"] <= 256      # (vgpr_count is the unified total on gfx950)
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0
    assert not re.search(r"^\s+scratch_", text, re.M)
    assert md["group_segment_fixed_size"] <= 163840
    assert md["max_flat_workgroup_size"] == 512
    # the text is the kernel's: the 16 x 16 x 32 fp16 instruction carries its layers, LDS-DMA its weight stream and row requests
    assert len(re.findall(r"^\s+v_mfma_f32_16x16x32_f16", text, re.M)) >= 2 * 64 * 6
    assert len(re.findall(r"^\s+v_mfma_f32_32x32", text, re.M)) == 0
    assert len(re.findall(r"^\s+global_load_lds_", text, re.M)) > 0
