"""CPU: the code objects of the set-abstraction scale kernels (csrc/fused_group.hip, csrc/fused_split.hip), compiled for gfx950 with
the flags they are built with (hipcc cross-compiles without a GPU).  Every sa_scale_kernel and sa_scale_split_kernel instance -- the
software-pipelined loops, which hold the next unit's rows in registers, and the serial comparison loops -- keeps its state in
registers (nothing in scratch, no spilled register), and the split instances stay within the register count of the occupancy their
launch bounds ask for: four waves per SIMD, 512 / 4 = 128 registers per lane (SA_SPLIT_WAVES, fused_split.hip)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT_WAVES = 4
SPLIT_VGPRS = 512 // SPLIT_WAVES


def kernels_metadata(asm_text, name_part):
    """{mangled name: {key: int}} of the .amdhsa metadata entries of the kernels whose name holds `name_part`."""
    found = {}
    for entry in re.split(r"\n  - \.agpr_count:", asm_text)[1:]:
        entry = ".agpr_count:" + entry
        m = re.search(r"\.name:\s+(\S*%s\S*)" % re.escape(name_part), entry)
        if m:
            found[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*\n", entry)}
    return found


def compile_to_asm(name, tmp_path):
    from ratrack_amd import build as B
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src, out = os.path.join(B.CSRC, name), str(tmp_path / (name[:-4] + ".s"))
    cmd = [hipcc] + [f for f in B.flags_for(src) if f != "-fPIC"] + ["-I", os.path.join(ROOT, "include"), "-I", B.CSRC, "-S", "--cuda-device-only", "-o", out, src]
    assert subprocess.run(cmd, stderr=subprocess.DEVNULL).returncode == 0
    return open(out).read()


def check_in_registers(name, md):
    print("%s: %s" % (name, {k: md[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size")}))
    assert md["private_segment_fixed_size"] == 0, name
    assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, name


def test_chain_kernel_instances_keep_their_state_in_registers(tmp_path):
    mds = kernels_metadata(compile_to_asm("fused_group.hip", tmp_path), "sa_scale_kernel")
    assert len(mds) == 12, sorted(mds)                     # six scales, pipelined and serial
    print()
    for name, md in sorted(mds.items()):
        check_in_registers(name, md)
        assert md["vgpr_count"] <= 128, name               # four waves per SIMD, what the launcher's grid gives


def test_split_kernel_instances_fit_four_waves_without_scratch(tmp_path):
    text = compile_to_asm("fused_split.hip", tmp_path)
    assert re.search(r"#define SA_SPLIT_WAVES %d\b" % SPLIT_WAVES, open(os.path.join(ROOT, "ratrack_amd", "csrc", "fused_split.hip")).read())
    mds = kernels_metadata(text, "sa_scale_split_kernel")
    assert len(mds) == 6, sorted(mds)                      # three shapes, pipelined and serial
    print()
    for name, md in sorted(mds.items()):
        check_in_registers(name, md)
        assert md["vgpr_count"] <= SPLIT_VGPRS, name
