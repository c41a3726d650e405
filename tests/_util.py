"""Shared helpers for the parity tests (golden fixtures, deterministic weights, tolerances)."""
import collections
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from ratrack_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

EVAL_CASES = ["eval_b2_n256", "eval_b1_n242", "eval_b1_n1024", "eval_b1_n256_dups"]
# north_star tolerance: "within 1e-4 rel for scene-flow floats", defined per tensor as
# max|a-b| <= RTOL * max|b| (flows are ~0 for static points, element-wise relative
# error is meaningless there).
RTOL = 1e-4


def load_case(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))


def state_dict_spec():
    with open(os.path.join(GOLDEN, "state_dict_spec.json")) as f:
        return json.load(f)


def reference_state_dict(device="cpu"):
    """The reference's 361-entry state dict, values from the deterministic generator."""
    spec = state_dict_spec()["entries"]
    sd = {}
    for k, (shape, dtype) in spec.items():
        a = synth.tensor_for_key(k, tuple(shape), dtype_is_int=(dtype == "int64"))
        sd[k] = torch.from_numpy(np.ascontiguousarray(a)).reshape(shape).to(device)
    return sd


def inputs_of(case, device="cpu"):
    g = lambda k: torch.from_numpy(case["in_" + k]).to(device)
    return g("pc1"), g("pc2"), g("feature1"), g("feature2")


def rel_err(a, b):
    """max|a-b| / max|b| with a, b array-likes."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def assert_close(a, b, rtol=RTOL, what=""):
    e = rel_err(a, b)
    assert e <= rtol, "%s: rel-to-scale error %.3e > %.1e" % (what, e, rtol)


# ---- gradient records of the round-3 fixtures (tools/make_golden.py: grad_records) ----------------------------------------
REAL_CASES = ["real_549_1047", "real_1047_1201", "real_1201_549"]
GRAD_SAMPLE = 1024


def grad_stride(numel):
    s = -(-numel // GRAD_SAMPLE)
    return s | 1 if s > 1 else 1


def probe_vector(key, numel):
    return 2.0 * synth._uniform01("probe/" + key, numel, 77) - 1.0


def grad_sample(g):
    a = np.asarray(g, dtype=np.float64).ravel()
    return a[::grad_stride(a.size)]


def grad_report(case, grads, prefix=""):
    """grads: {parameter name: array or None}.  Compares with the fixture's gradient records (`prefix`grad/..., grad_norms,
    grad_probes, arb_*).  Returns a list of rows: e_ref = max|mine - reference fp32| over the sampled elements / the reference
    tensor's largest element, e_arb the same against the float64 arbiter (None without arbiter samples), floor = the fp32
    oracle's own distance from the arbiter.  Parameters whose EXACT gradient is zero -- a bias in front of a BatchNorm, the GRU
    under B = 1 batch statistics; recognised by a float64 norm below 1e-8 of the model's largest -- carry only rounding noise
    (1e-7 of the model's gradient scale in the reference too): for them the errors are measured against 1e-4 of the model's
    largest gradient element, i.e. `e <= 1` means "noise, as in the reference"."""
    names = [str(k) for k in case[prefix + "grad_names"]]
    norms = case[prefix + "grad_norms"]
    arb_norms = case[prefix + "arb_grad_norms"]
    gmax = max(float(np.abs(case[prefix + "grad/" + k]).max()) for k, n in zip(names, norms) if n >= 0)
    floor = case.get(prefix + "arb_fp32_oracle_relerr")
    rows = []
    for i, (k, n) in enumerate(zip(names, norms)):
        g = grads.get(k)
        if n < 0:
            assert g is None or float(np.abs(np.asarray(g)).max()) == 0.0, "%s: dead parameter has a gradient" % k
            continue
        assert g is not None, "%s: no gradient" % k
        zero = float(arb_norms[i]) <= 1e-8 * float(arb_norms.max())
        mine = grad_sample(g)
        ref = case[prefix + "grad/" + k].astype(np.float64)
        scale = 1e-4 * gmax if zero else float(np.abs(ref).max())
        e_ref = float(np.abs(mine - ref).max() / scale)
        e_arb = None
        ak = prefix + "arb_grad/" + k
        if ak in case:
            arb = case[ak].astype(np.float64)
            e_arb = float(np.abs(mine - arb).max() / (1e-4 * gmax if zero else float(np.abs(arb).max())))
        full = np.asarray(g, dtype=np.float64).ravel()
        probe = float((full * probe_vector(k, full.size)).sum())
        rows.append(dict(name=k, zero=zero, e_ref=e_ref, e_arb=e_arb, floor=None if floor is None or zero else float(floor[i]),
                         norm=float(np.sqrt((full * full).sum())), ref_norm=float(n), probe=probe,
                         ref_probe=float(case[prefix + "grad_probes"][i]), gmax=gmax))
    return rows


# ---- what a kernel file's gfx950 code object states ------------------------------------------------------------------------------
class KernelNotes(collections.namedtuple("KernelNotes", "private lds wavefront max_threads")):
    """The four fields, and beside them .vgpr (the .vgpr_count): an attribute, so that the tuple compares as it always did."""

    def __new__(cls, private, lds, wavefront, max_threads, vgpr):
        self = super().__new__(cls, private, lds, wavefront, max_threads)
        self.vgpr = vgpr
        return self


_NOTES = {}


def kernel_notes(src, tmp_path):
    """Compiles `src` for the device with the flags it is built with -> ({kernel symbol: KernelNotes}, the assembly text): the
    .private_segment_fixed_size (scratch), .group_segment_fixed_size (static LDS), .wavefront_size, .max_flat_workgroup_size and
    .vgpr_count of every kernel in the notes of the assembly.  A file is compiled once per test run.  Skips where there is no hipcc."""
    if src not in _NOTES:
        _NOTES[src] = _kernel_notes(src, tmp_path)
    return dict(_NOTES[src][0]), _NOTES[src][1]


def template_flags(symbol):
    """The bool template arguments of a mangled kernel symbol, in order: "_Z9ts_kernelILb1ELb0E...EEv..." -> (True, False, ...)."""
    return tuple(c == "1" for c in re.findall(r"Lb([01])E", symbol[:symbol.index("EEv") + 1]))


# the ten instantiations of csrc/track_score.hip's ts_kernel<LOG, MEM, PAIRS, CENTRE, BOX>, by the name of their variant
SCORE_VARIANTS = {"plain": (False, False, False, False, False), "memory": (False, True, False, False, False),
                  "logged": (True, False, False, False, False), "memory_logged": (True, True, False, False, False),
                  "pairs": (True, False, True, False, False), "pairs_memory": (True, True, True, False, False),
                  "centre": (True, False, True, True, False), "centre_memory": (True, True, True, True, False),
                  "box": (True, False, True, False, True), "box_memory": (True, True, True, False, True)}


def score_kernel_notes(tmp_path):
    """The scoring launch's one translation unit -> {variant name of SCORE_VARIANTS: KernelNotes}, after asserting that its code object
    holds exactly those ten ts_kernel instantiations and gt_objects_kernel, each a workgroup of 256 threads in waves of 64 without
    scratch and without static LDS."""
    from ratrack_amd import build as B
    found, _ = kernel_notes(os.path.join(B.CSRC, "track_score.hip"), tmp_path)
    ours = [n for n in found if re.match(r"_Z\d+ts_kernelI", n)]
    assert len(found) == 11 and [n for n in found if n not in ours] == ["_Z17gt_objects_kernel19rtk_gt_objects_in_t20rtk_gt_objects_out_t"], sorted(found)
    assert all((v.private, v.lds, v.wavefront, v.max_threads) == (0, 0, 64, 256) for v in found.values()), found
    by_flags = {template_flags(n): found[n] for n in ours}
    assert sorted(by_flags) == sorted(SCORE_VARIANTS.values()), sorted(by_flags)
    return {name: by_flags[flags] for name, flags in SCORE_VARIANTS.items()}


def _kernel_notes(src, tmp_path):
    from ratrack_amd import build as B
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path / (os.path.basename(src) + ".s"))
    cmd = [hipcc] + [f for f in B.flags_for(src) if f != "-fPIC"] + ["-I", os.path.join(ROOT, "include"), "-I", B.CSRC, "-S",
                                                                    "--cuda-device-only", "-o", out, src]
    subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
    asm = open(out).read()
    notes = asm[asm.index("amdhsa.kernels"):]
    found = {}
    for e in re.split(r"\n\s+- \.", notes):
        m = re.search(r"\.name:\s+(\S+)", e)
        v = [re.search(r"\.%s:\s+(\d+)" % k, e)
             for k in ("private_segment_fixed_size", "group_segment_fixed_size", "wavefront_size", "max_flat_workgroup_size", "vgpr_count")]
        if m and all(v):
            found[m.group(1)] = KernelNotes(*(int(x.group(1)) for x in v))
    return found, asm
