"""CPU: the batched tracker's native surface -- declared, built for gfx950 without scratch, arguments validated before any launch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ["rtk_dbscan_batched", "rtk_object_descriptors", "rtk_affinity_pairs", "rtk_associate_batched"]
KERNELS = ["dbscan_batched_kernel", "object_descriptors_kernel", "affinity_pairs_kernel", "associate_batched_kernel"]


def test_header_declares_the_batched_entry_points():
    text = open(os.path.join(ROOT, "include", "rtk_fused.h")).read()
    for name in ENTRY + ["rtk_track_max_objects"]:
        assert re.search(r"RTK_EXPORT int %s\(" % name, text), name
    assert "rtk_track_frame_t" in text and "rtk_bcn_view_t" in text


def test_kernels_build_for_gfx950_without_scratch(tmp_path):
    from ratrack_amd import build as B
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    # the batched kernels, and the B = 1 kernels that share their DBSCAN and log-OT code (assoc_common.h): kernel -> instantiations
    expect = {"track_batched.hip": {k: 1 for k in KERNELS}, "fused_misc.hip": {"dbscan_kernel": 2, "log_sinkhorn_kernel": 1}}
    for fname, kernels in expect.items():
        src = os.path.join(B.CSRC, fname)
        out = str(tmp_path / (fname + ".s"))
        cmd = [hipcc] + [f for f in B.flags_for(src) if f != "-fPIC"] + ["-I", os.path.join(ROOT, "include"), "-I", B.CSRC, "-S",
                                                                        "--cuda-device-only", "-o", out, src]
        subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
        asm = open(out).read()
        notes = asm[asm.index("amdhsa.kernels"):]
        entries = re.split(r"\n\s+- \.", notes)
        found = {}
        for e in entries:
            m = re.search(r"\.name:\s+(\S+)", e)
            p = re.search(r"\.private_segment_fixed_size:\s+(\d+)", e)
            if m and p:
                found[m.group(1)] = int(p.group(1))
        for k, count in kernels.items():
            hits = [v for name, v in found.items() if k in name]
            assert hits == [0] * count, (k, found)


def _call_fails(name, *args):
    from ratrack_amd import _lib, fused  # noqa: F401
    with pytest.raises(_lib.RtkError) as e:
        _lib.call(name, *args)
    return str(e.value)


def test_arguments_are_validated_before_any_launch():
    import ctypes
    import torch
    from ratrack_amd import _lib, tracker as T
    kmax = T.max_objects_limit()
    assert 128 <= kmax <= 256
    fake = 4096          # never dereferenced: the checks fail first
    # K beyond the LDS budget
    msg = _call_fails("rtk_associate_batched", 2, 16, kmax + 1, None, None, fake, fake, fake, fake, fake, 0.9, 500, fake, fake, fake,
                      fake, fake, fake, fake, fake, None, None)
    assert "K=%d" % (kmax + 1) in msg
    assert "K=0" in _call_fails("rtk_affinity_pairs", 2, 0, fake, fake, fake, None, fake, fake, fake, None)
    # null pointers
    assert "bad arguments" in _call_fails("rtk_associate_batched", 2, 16, 8, None, None, None, fake, fake, fake, fake, 0.9, 500, fake,
                                          fake, fake, fake, fake, fake, fake, fake, None, None)
    assert "bad arguments" in _call_fails("rtk_affinity_pairs", 2, 8, None, fake, fake, None, fake, fake, fake, None)
    assert "bad arguments" in _call_fails("rtk_dbscan_batched", None, 0.5, 1.5, 2, 8, fake, fake, fake, fake, None, 0, None)
    fr = T.TrackFrame(2, 16)                                         # views with null pointers
    assert "bad arguments" in _call_fails("rtk_dbscan_batched", ctypes.addressof(fr), 0.5, 1.5, 2, 8, fake, fake, fake, fake, None, 0, None)
    assert "bad arguments" in _call_fails("rtk_object_descriptors", ctypes.addressof(fr), 8, fake, fake, fake, fake, fake, None)
    v = T._View(fake, 1, 1, 1)
    fr = T.TrackFrame(2, 4000, v, v, v, v, v, None, None)            # tables beyond the LDS and no workspace
    assert "workspace" in _call_fails("rtk_dbscan_batched", ctypes.addressof(fr), 0.5, 1.5, 2, 8, fake, fake, fake, fake, None, 0, None)
    # n_valid beyond N (host tensors are checked before anything is queued; device ones by the kernels -> check() raises)
    with pytest.raises(ValueError, match="outside"):
        T.check_n_valid(torch.tensor([[10, 300], [10, 10]]), 256)
    with pytest.raises(ValueError, match="outside"):
        T.check_n_valid([[10, -1], [10, 10]], 256)
    T.check_n_valid(torch.tensor([[10, 256], [256, 3]]), 256)
    with pytest.raises(RuntimeError, match="stream 1 has an n_valid"):
        T.raise_on_flags([0, 2], 8)
    with pytest.raises(RuntimeError, match="stream 0 has more than max_objects=8"):
        T.raise_on_flags([1, 0], 8)


def test_tracker_refuses_bad_configurations():
    from ratrack_amd import tracker as T
    from ratrack_amd.track4d import Args, Track4D
    net = Track4D(Args()).eval()
    with pytest.raises(ValueError, match="max_objects"):
        T.BatchedTracker(net, streams=2, max_objects=T.max_objects_limit() + 1)
    with pytest.raises(ValueError, match="max_objects"):
        T.BatchedTracker(net, streams=2, max_objects=0)
    with pytest.raises(ValueError, match="eval"):
        T.BatchedTracker(net.train(), streams=2)
    w = T.pack_affinity(net.affinity)
    assert w.numel() == 141 * 564 + 564 + 564 * 282 + 282 + 282 * 70 + 70 + 70 * 35 + 35 + 35 + 1
