"""CPU: the code object of the forward cost volume (csrc/fused_split.hip, cost_volume_split_kernel<false> with its constants in LDS),
compiled for gfx950 with the flags it is built with (hipcc cross-compiles without a GPU): nothing in scratch, no spilled vector
register, no more spilled scalar registers than before the constants moved (40), the three LDS regions within a CU's 160 KiB, and
the tile loop free of the global loads of constants (a read of the LDS image that the compiler could not prove to be one would be a flat
load: counted too) -- the kernel's text holds what a tile owns (its neighbour index, six coordinates,
two p1 slots, the optional per-sample term: at most 15 loads, once in the prologue and once in the loop) and the unrolled fill; with
the constants in global memory it held 158."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "cost_volume_split_kernelILb0ELb1EE"      # <SAVE = false, LDSC = true>


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


def test_forward_kernel_reads_its_constants_from_lds(tmp_path):
    from ratrack_amd import build as B
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src, out = os.path.join(B.CSRC, "fused_split.hip"), str(tmp_path / "fused_split.s")
    cmd = [hipcc] + [f for f in B.flags_for(src) if f != "-fPIC"] + ["-I", os.path.join(ROOT, "include"), "-I", B.CSRC, "-S", "--cuda-device-only", "-o", out, src]
    assert subprocess.run(cmd, stderr=subprocess.DEVNULL).returncode == 0
    asm = open(out).read()
    md, text = kernel_metadata(asm, KERNEL), kernel_text(asm, KERNEL)
    assert md is not None and text is not None, "cost_volume_split_kernel<false, true> not in the code object"
    loads = [l.split()[0] for l in text.split("\n") if re.match(r"\s+(global|flat|buffer|scratch)_load_(?!lds_)", l)]
    print("\ncost_volume_split_kernel<false>:", {k: md[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "sgpr_spill_count", "group_segment_fixed_size")},
          "vector global loads (not LDS-DMA):", len(loads))
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0
    assert md["group_segment_fixed_size"] <= 163840
    assert md["sgpr_spill_count"] <= 40
    assert len(loads) <= 64
    assert len(re.findall(r"^\s+global_load_lds_", text, re.M)) > 0      # (the text is the kernel's: its weight stream and row requests are there)
