"""CPU: the code objects of the set-abstraction scale kernels with the ball index requested one unit ahead (SA_INDEX_AHEAD = 1) and two
units ahead (SA_INDEX_AHEAD = 2; csrc/fused_group.hip, csrc/fused_split.hip), compiled for gfx950 with the flags they are built with.
The register, scratch and spill figures of all eighteen instances are printed for both settings; the setting that is the default build
keeps every instance in registers (0 scratch, 0 spilled registers) within 128 registers, four waves per SIMD."""
import os
import re

import pytest

from test_sa_code_object_cpu import ROOT, compile_to_asm, kernels_metadata

FILES = [("fused_group.hip", "sa_scale_kernel", 12), ("fused_split.hip", "sa_scale_split_kernel", 6)]
KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")


def default_ahead(name):
    m = re.search(r"#ifndef SA_INDEX_AHEAD\n#define SA_INDEX_AHEAD (\d)\n#endif", open(os.path.join(ROOT, "ratrack_amd", "csrc", name)).read())
    assert m, name
    return int(m.group(1))


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """{ahead: {file: {kernel: metadata}}}: the default setting from the build as it is (no -D), the other one set on the command line."""
    from ratrack_amd import build as B
    flags, out, default = list(B.FLAGS), {}, default_ahead("fused_split.hip")
    try:
        for ahead in (default, 3 - default):
            B.FLAGS = flags + (["-DSA_INDEX_AHEAD=%d" % ahead] if ahead != default else [])
            out[ahead] = {name: kernels_metadata(compile_to_asm(name, tmp_path_factory.mktemp("ahead%d" % ahead)), part) for name, part, _ in FILES}
    finally:
        B.FLAGS = flags
    return out


def test_both_files_have_the_same_default():
    assert default_ahead("fused_group.hip") == default_ahead("fused_split.hip") and default_ahead("fused_group.hip") in (1, 2)


def test_register_table_of_every_instance_with_the_macro_off_and_on(tables):
    print()
    for name, part, count in FILES:
        assert len(tables[1][name]) == count and sorted(tables[1][name]) == sorted(tables[2][name]), name
        for kernel in sorted(tables[1][name]):
            for ahead in (1, 2):
                md = tables[ahead][name][kernel]
                print("SA_INDEX_AHEAD=%d %s: %s" % (ahead, kernel, {k: md[k] for k in KEYS}))


def test_the_default_build_keeps_every_instance_in_registers(tables):
    for name, part, count in FILES:
        mds = tables[default_ahead(name)][name]
        assert len(mds) == count, sorted(mds)
        for kernel, md in sorted(mds.items()):
            assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, kernel
            assert md["vgpr_count"] <= 128, kernel
