"""Oriented boxes for tracked objects: position, size and heading per object, fitted on the device.

    bx = object_boxes(out)                       # out: a tracker.StepResult; one launch, no synchronisation
    bx.box[b, j]                                 # (cx, cy, cz, l, w, h, yaw, area) float64 of object j of stream b, radar frame
    bx.valid[b, j], bx.cand[b, j]                # its point count (0: no object, -1: a coordinate was not finite), the winning candidate
    bx.check()                                   # synchronises: raises if an object was too large for the oriented search

The tracker's output is point clusters with track ids; the evaluators of the field (the KITTI tracking devkit, AB3DMOT, TrackEval's
KITTI loaders, the VoD devkit) read boxes.  The box of an object is the minimum-area rectangle around its points in the bird's-eye view
with the points' z range for its height: a search over the directions of all point pairs with a deterministic winner, stated in
include/rtk_fused.h ("Oriented boxes"), implemented in csrc/box_fit.h, one HIP launch for a whole step (rtk_object_boxes) or a whole
result log (rtk_result_log_boxes, `ResultLog.boxes` / `ResultLog.write_kitti`).  `BatchedTracker(boxes=True)` issues the launch
inside the step.  An object of more than MAX_POINTS points is fitted axis-aligned; `axis_only` marks it and `check()` says so.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from .abi import stream as _stream, view as _view
from .gt_device import _flag_bytes

MAX_POINTS = 128                       # RTK_BOX_MAX_POINTS
MAX_OBJECTS = 256                      # RTK_RESULT_MAX_OBJECTS
FLAG_AXIS, FLAG_OBJECTS = 1, 2         # RTK_BOX_FLAG_*
CX, CY, CZ, L, W, H, YAW, AREA = range(8)      # the words of a box


# ---- argument checks: no device is touched -----------------------------------------------------------------------------------------

def check_min_extent(min_extent):
    """-> float(min_extent); raises ValueError unless it is a finite number >= 0."""
    if isinstance(min_extent, bool) or not isinstance(min_extent, (int, float, np.integer, np.floating)) or \
            not math.isfinite(float(min_extent)) or float(min_extent) < 0.0:
        raise ValueError("min_extent=%r: a finite number >= 0 (the least length, width and height of a box, metres)" % (min_extent,))
    return float(min_extent)


def check_into(into, B, rows, dev):
    """`into` as the output buffers of B streams of `rows` boxes on device `dev`; raises ValueError."""
    want = (("box", (B, rows, 8), torch.float64), ("cand", (B, rows), torch.int32), ("valid", (B, rows), torch.int32), ("flags", (B,), torch.int32))
    for name, shape, dtype in want:
        t = getattr(into, name, None)
        if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != torch.device(dev):
            raise ValueError("into.%s must be a contiguous %s tensor of shape %s on %s, got %s" % (
                name, dtype, shape, dev, "%s %s on %s" % (t.dtype, tuple(t.shape), t.device) if torch.is_tensor(t) else type(t).__name__))
    return into


def flag_message(b, f, rows):
    """The first complaint about stream b's flags word f, or None."""
    if f & FLAG_OBJECTS:
        return "boxes: stream %d has a num_objects outside [0, max_objects=%d]: nothing of it was fitted" % (b, rows)
    if f & FLAG_AXIS:
        return "boxes: stream %d has an object of more than %d points: it was fitted axis-aligned (axis_only marks it)" % (b, MAX_POINTS)
    return None


class ObjectBoxes:
    """Device tensors: box (B,rows,8) float64 = cx, cy, cz, l, w, h, yaw, area (radar frame, yaw in [-pi/2, pi/2), area the rectangle's
    before min_extent); cand (B,rows) int32, the winning candidate (-1: no box); valid (B,rows) int32, the object's point count (0: no
    object, -1: a coordinate that is not finite); flags (B) int32, FLAG_AXIS | FLAG_OBJECTS.  rows: the step's max_objects, or the
    log's records (then only the rows below each stream's cursor are written)."""

    def __init__(self, box, cand, valid, flags):
        self.box, self.cand, self.valid, self.flags = box, cand, valid, flags

    @classmethod
    def empty(cls, B, rows, device):
        """Uninitialised buffers (what `into=` takes)."""
        i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=device)
        return cls(torch.empty(B, rows, 8, dtype=torch.float64, device=device), i32(B, rows), i32(B, rows), i32(B))

    @property
    def axis_only(self):
        """(B,rows) bool: the objects above MAX_POINTS points, fitted axis-aligned (a device tensor; no synchronisation)."""
        return self.valid > MAX_POINTS

    def check(self):
        """Synchronises; raises RuntimeError naming the stream for any flag."""
        rows = self.box.shape[1]
        for b, f in enumerate(self.flags.cpu().tolist()):
            msg = flag_message(b, int(f), rows)
            if msg:
                raise RuntimeError(msg)


# ---- the launches ---------------------------------------------------------------------------------------------------------------

def object_boxes_raw(pc1, obj, num_objects, max_objects, active=None, min_extent=0.0, into=None):
    """rtk_object_boxes for detections from anywhere.  pc1 (B,3,N) fp32 of any strides; obj (B,N) int32, the object of each column
    (outside [0, num_objects): none); num_objects (B) int32; active (B) or None.  -> ObjectBoxes of max_objects rows per stream."""
    min_extent = check_min_extent(min_extent)
    K = max_objects
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= K <= MAX_OBJECTS:
        raise ValueError("boxes: max_objects=%r must be an integer in [1, %d]" % (K, MAX_OBJECTS))
    if pc1.dim() != 3 or pc1.shape[1] != 3 or tuple(obj.shape) != (pc1.shape[0], pc1.shape[2]) or num_objects.numel() != pc1.shape[0]:
        raise ValueError("boxes: got pc1 %s, obj %s, num_objects %s" % (tuple(pc1.shape), tuple(obj.shape), tuple(num_objects.shape)))
    B, _, N = pc1.shape
    dev = pc1.device
    if into is not None:
        check_into(into, B, int(K), dev)
    out = into if into is not None else ObjectBoxes.empty(B, int(K), dev)
    obj = obj.to(device=dev, dtype=torch.int32).contiguous()
    num_objects = num_objects.to(device=dev, dtype=torch.int32).contiguous()
    act = _flag_bytes(active, B, dev)
    pv = _view(pc1.float())
    _lib.call("rtk_object_boxes", B, N, int(K), ctypes.addressof(pv), obj.data_ptr(), num_objects.data_ptr(), None if act is None else act.data_ptr(),
              min_extent, out.box.data_ptr(), out.cand.data_ptr(), out.valid.data_ptr(), out.flags.data_ptr(), _stream())
    return out


def object_boxes(out, min_extent=0.0, into=None):
    """The boxes of a `tracker.StepResult`'s objects: one launch on the current stream, no synchronisation.  Row j of stream b is the
    object `out.object_ids[b, j]`; rows past `out.num_objects[b]` and inactive streams hold no box (valid = 0).  into: an ObjectBoxes
    to write into (`ObjectBoxes.empty(B, out.max_objects, device)`): nothing is allocated, so the call can be captured in a graph."""
    return object_boxes_raw(out.pc1, out.obj, out.num_objects, out.max_objects, active=out.active, min_extent=min_extent, into=into)
