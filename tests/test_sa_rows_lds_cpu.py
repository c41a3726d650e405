"""CPU: the code objects of the three sa_scale_split_kernel shapes whose pipelined loop takes the q rows through LDS (csrc/fused_split.hip,
SaRows), compiled for gfx950 with the flags they are built with.  The pipelined instances fit four workgroups on a CU's 160 KiB of LDS
(<= 40,960 bytes each), request rows with global_load_lds_dwordx4, and hold fewer global_load_dwordx4 than their serial partners, whose
loop fetches every row with four (C1 = 32) or eight (C1 = 64) of them.  The counts are printed."""
import re

import pytest

from test_sa_code_object_cpu import compile_to_asm, kernels_metadata

SHAPES = [(32, 64), (16, 64), (16, 32)]
LDS_PER_WORKGROUP = 160 * 1024 // 4


def body(text, name):
    """The instructions of kernel `name`: from its label to the end-of-function label."""
    m = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(name), text, re.M | re.S)
    assert m, name
    return m.group(0)


def count(asm, mnemonic):
    return len(re.findall(r"^\s+%s\s" % re.escape(mnemonic), asm, re.M))


@pytest.fixture(scope="module")
def code(tmp_path_factory):
    text = compile_to_asm("fused_split.hip", tmp_path_factory.mktemp("rows_lds"))
    return text, kernels_metadata(text, "sa_scale_split_kernel")


def instance(mds, ns, c1, pipe):
    names = [k for k in mds if "ILi%dELi%dELb%dEE" % (ns, c1, pipe) in k]
    assert len(names) == 1, (ns, c1, pipe, sorted(mds))
    return names[0]


@pytest.mark.parametrize("ns,c1", SHAPES)
def test_pipelined_instance_stages_rows_in_lds_and_fits_four_workgroups(code, ns, c1):
    text, mds = code
    pipe, serial = instance(mds, ns, c1, 1), instance(mds, ns, c1, 0)
    lds = mds[pipe]["group_segment_fixed_size"]
    a_pipe, a_serial = body(text, pipe), body(text, serial)
    dma = count(a_pipe, "global_load_lds_dwordx4")
    direct, direct_serial = count(a_pipe, "global_load_dwordx4"), count(a_serial, "global_load_dwordx4")
    print("\nns=%d c1=%d: pipelined %d bytes of LDS, %d global_load_lds_dwordx4, %d global_load_dwordx4; serial %d bytes, %d global_load_lds_dwordx4, "
          "%d global_load_dwordx4" % (ns, c1, lds, dma, direct, mds[serial]["group_segment_fixed_size"], count(a_serial, "global_load_lds_dwordx4"),
                                      direct_serial))
    assert lds <= LDS_PER_WORKGROUP
    assert dma > 0
    assert direct < direct_serial
