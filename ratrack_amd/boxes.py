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

    fb = log.filter_boxes(log.boxes(), filter=BoxFilter(smooth=1, size_rule=1))      # ResultLog; one launch, when the clip is over
    fb.box, fb.valid                             # a box per record in the same layout, from its whole track
    fb.vel[b, r]                                 # (vx, vy, vz, unwrapped yaw): the tracked object's velocity, metres per frame

A box fitted from one frame's two to ten radar points is a fraction of the object and its heading jumps by a quarter turn.
`BoxFilter` holds the parameters of a constant-velocity Kalman filter run along every track of a result log
(rtk_result_log_filter_boxes, csrc/track_box_filter.hip; the rule is stated in include/rtk_fused.h, "Filtered boxes"), with an optional
backward pass and an optional size from the whole track; `FilteredBoxes` is its result and goes wherever an `ObjectBoxes` goes.

    trk = BatchedTracker(net, streams=B, boxes=True, box_filter=BoxFilter(max_gap=3))      # the same filter, a frame at a time
    out.filtered_boxes[b, j], out.filtered_velocity[b, j]      # the track's box and velocity now, inside the step

`filter_step_raw` is that launch (rtk_track_box_filter_step, csrc/track_box_step.hip; the rule: include/rtk_fused.h, "Filtered boxes
inside the step"): the filter's state travels with the tracker's table and is advanced in place once per step; the forward pass with
the filter's own sizes only (`check_step_filter`), and for a measured object the bits `ResultLog.filter_boxes` gives its record.
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
FLAG_AXIS, FLAG_OBJECTS, FLAG_DUPLICATE, FLAG_TRACKS = 1, 2, 4, 8      # RTK_BOX_FLAG_*
FILTER_MAX_GAP = 64                    # RTK_BOX_FILTER_MAX_GAP
TRACKS = 2048                          # RTK_SCORE_SWEEP_TRACKS: track ids of one clip the filter can tell apart
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
    if f & FLAG_TRACKS:
        return "boxes: stream %d has a clip with more than %d track ids: it and the later clips were not filtered" % (b, TRACKS)
    if f & FLAG_DUPLICATE:
        return "boxes: stream %d has a frame with one track id on two records: the first was filtered, the others have no box" % b
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


# ---- filtered boxes ---------------------------------------------------------------------------------------------------------------

def _number(name, v, least, strict):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)) or \
            float(v) < least or (strict and float(v) == least):
        raise ValueError("BoxFilter: %s=%r must be a finite number %s %g" % (name, v, ">" if strict else ">=", least))
    return float(v)


def _integer(name, v, allowed, text):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) not in allowed:
        raise ValueError("BoxFilter: %s=%r must be %s" % (name, v, text))
    return int(v)


class BoxFilter:
    """The parameters of the track box filter (rtk_box_filter_t), checked on construction (ValueError; no device is touched).
    r_pos, r_yaw, r_size: measurement variances (> 0); q_pos, q_vel, q_yaw, q_size: process variances per frame (>= 0); p0, p0_vel: the
    initial variances (> 0).  symmetry: 2 (a box without a front) or 4 (without a front and a labelled side: fitted boxes).  max_gap:
    the frames between two members of a track beyond which the filter starts again (1 ... 64).  smooth: 1 adds the backward pass.
    size_rule: 0 the filter's sizes, 1 the reading of rank size_percent (0 ... 100) among each segment's readings.  The defaults are
    the values of the filter the tracker was modelled on, for fitted boxes; `reference()` is that filter itself."""

    def __init__(self, r_pos=1.0, r_yaw=1.0, r_size=1.0, q_pos=1.0, q_vel=0.01, q_yaw=1.0, q_size=1.0, p0=10.0, p0_vel=10000.0, symmetry=4,
                 max_gap=2, smooth=0, size_rule=0, size_percent=90):
        self.r_pos, self.r_yaw, self.r_size = (_number(n, v, 0.0, True) for n, v in (("r_pos", r_pos), ("r_yaw", r_yaw), ("r_size", r_size)))
        self.q_pos, self.q_vel, self.q_yaw, self.q_size = (_number(n, v, 0.0, False) for n, v in (("q_pos", q_pos), ("q_vel", q_vel),
                                                                                                  ("q_yaw", q_yaw), ("q_size", q_size)))
        self.p0, self.p0_vel = _number("p0", p0, 0.0, True), _number("p0_vel", p0_vel, 0.0, True)
        self.symmetry = _integer("symmetry", symmetry, (2, 4), "2 or 4")
        self.max_gap = _integer("max_gap", max_gap, range(1, FILTER_MAX_GAP + 1), "an integer in [1, %d]" % FILTER_MAX_GAP)
        self.smooth = _integer("smooth", smooth, (0, 1), "0 or 1")
        self.size_rule = _integer("size_rule", size_rule, (0, 1), "0 (the filter's sizes) or 1 (the extent rule)")
        self.size_percent = _integer("size_percent", size_percent, range(0, 101), "an integer in [0, 100]")

    @classmethod
    def reference(cls, **kw):
        """The ten-state filter with its shipped parameters: a half-turn symmetry, no gaps bridged beyond one frame."""
        return cls(**dict(dict(symmetry=2, max_gap=1), **kw))

    FIELDS = ("r_pos", "r_yaw", "r_size", "q_pos", "q_vel", "q_yaw", "q_size", "p0", "p0_vel", "symmetry", "max_gap", "smooth", "size_rule",
              "size_percent")

    def block(self):
        from .abi import BoxFilter as _Par
        return _Par(*(getattr(self, n) for n in self.FIELDS))

    def __repr__(self):
        return "BoxFilter(%s)" % ", ".join("%s=%r" % (n, getattr(self, n)) for n in self.FIELDS)


def check_filter(filter):
    """-> filter; raises ValueError unless it is a BoxFilter whose fields still pass its checks."""
    if not isinstance(filter, BoxFilter):
        raise ValueError("filter=%r: a boxes.BoxFilter" % (filter,))
    BoxFilter(**{n: getattr(filter, n) for n in BoxFilter.FIELDS})
    return filter


class FilteredBoxes(ObjectBoxes):
    """`ResultLog.filter_boxes`' result: box (B,R,8) float64, valid (B,R), flags (B) as an ObjectBoxes has them (box from the record's
    whole track; flags FLAG_DUPLICATE | FLAG_TRACKS), cand = the input boxes' cand tensor itself (the filter has no candidates of its
    own: `filter_boxes` sets the reference, the launch does not write it), and vel (B,R,4) float64 = vx, vy, vz per frame and the
    unwrapped yaw; state (B,R,16) float64 = the filtered mean (x, y, z, yaw, l, w, h, vx, vy, vz), P00, P01, P11, Pyaw, Psize, 0; aligned
    (B,R,4) float64 = the reading's yaw, l, w, h as the filter took them; link (B,R,4) int32 = previous member | gap | next member |
    the segment's first member (record indices, -1: none).  Written below each stream's records cursor only."""

    def __init__(self, box, cand, valid, flags, vel, state, aligned, link):
        ObjectBoxes.__init__(self, box, cand, valid, flags)
        self.vel, self.state, self.aligned, self.link = vel, state, aligned, link

    @classmethod
    def empty(cls, B, rows, device):
        """Uninitialised buffers (what `into=` takes)."""
        f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=device)
        i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=device)
        return cls(f64(B, rows, 8), i32(B, rows), i32(B, rows), i32(B), f64(B, rows, 4), f64(B, rows, 16), f64(B, rows, 4), i32(B, rows, 4))

    @classmethod
    def zeros(cls, B, rows, device):
        out = cls.empty(B, rows, device)
        for t in (out.box, out.cand, out.valid, out.flags, out.vel, out.state, out.aligned, out.link):
            t.zero_()
        return out


def check_filtered_into(into, B, rows, dev):
    """`into` as a FilteredBoxes of B streams of `rows` records on `dev`; raises ValueError."""
    check_into(into, B, rows, dev)
    for name, shape, dtype in (("vel", (B, rows, 4), torch.float64), ("state", (B, rows, 16), torch.float64),
                               ("aligned", (B, rows, 4), torch.float64), ("link", (B, rows, 4), torch.int32)):
        t = getattr(into, name, None)
        if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != torch.device(dev):
            raise ValueError("into.%s must be a contiguous %s tensor of shape %s on %s" % (name, dtype, shape, dev))
    return into


# ---- filtered boxes inside the step -------------------------------------------------------------------------------------------------

def check_step_filter(filter):
    """`check_filter` for the filter a tracker runs inside its step (rtk_track_box_filter_step): -> filter; raises ValueError also
    for smooth=1 or size_rule=1."""
    check_filter(filter)
    if filter.smooth or filter.size_rule:
        raise ValueError("box_filter: smooth=%d, size_rule=%d: neither is causal -- the backward pass and the extent rule look at a "
                         "track's later frames, which a step does not have; run them over the log when the clip is over "
                         "(ResultLog.filter_boxes)" % (filter.smooth, filter.size_rule))
    return filter


class StepBoxes:
    """`filter_step_raw`'s outputs (device tensors): box (B,K,8) float64 and valid (B,K) int32 in the layout of an ObjectBoxes' (the
    track's box now: filtered where the row was measured, predicted where it was carried; zeros, valid 0 elsewhere); vel (B,K,4) float64
    = vx, vy, vz per frame and the unwrapped yaw; aligned (B,K,4) float64 = the reading's yaw, l, w, h as the filter took them (zeros
    unless measured); gap (B,K) int32 = the frames since the track's previous measurement where the row continued it, else -1."""

    NAMES = (("box", 8, torch.float64), ("valid", 0, torch.int32), ("vel", 4, torch.float64), ("aligned", 4, torch.float64),
             ("gap", 0, torch.int32))

    def __init__(self, box, valid, vel, aligned, gap):
        self.box, self.valid, self.vel, self.aligned, self.gap = box, valid, vel, aligned, gap

    @classmethod
    def empty(cls, B, K, device):
        """Uninitialised buffers (what `into=` takes)."""
        return cls(*(torch.empty((B, K) + ((w,) if w else ()), dtype=dt, device=device) for _, w, dt in cls.NAMES))


def _check_tensor(what, t, shape, dtype, dev):
    if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != torch.device(dev):
        raise ValueError("filter_step: %s must be a contiguous %s tensor of shape %s on %s, got %s" % (
            what, dtype, shape, dev, "%s %s on %s" % (t.dtype, tuple(t.shape), t.device) if torch.is_tensor(t) else type(t).__name__))
    return t


def filter_step_raw(ids_prev, count_prev, ids_new, count_new, num_objects, box, valid, state, since, filter=None, active=None, reset=None,
                    into=None):
    """rtk_track_box_filter_step (include/rtk_fused.h, "Filtered boxes inside the step") for tables from anywhere: one launch on the
    current stream, no synchronisation.  ids_prev / ids_new (B,K) int32 and count_prev / count_new (B) int32: the previous table and
    the one this step wrote; num_objects (B) int32: the first rows of the new table that are this frame's detections; box (B,K,8)
    float64 and valid (B,K) int32: their boxes (an ObjectBoxes' fields); state (B,K,16) float64 and since (B,K) int32: the filter's
    state, ADVANCED IN PLACE (start from zeros and -1); active / reset (B) or None.  filter: a BoxFilter with smooth = size_rule = 0
    (None: its defaults).  -> StepBoxes; into: a StepBoxes to write into (`StepBoxes.empty(B, K, device)`) -- with it and device
    tensors for active and reset nothing is allocated and the call can be captured in a graph."""
    flt = check_step_filter(BoxFilter() if filter is None else filter)
    if not torch.is_tensor(ids_new) or ids_new.dim() != 2:
        raise ValueError("filter_step: ids_new must be a (B,K) int32 tensor")
    B, K = ids_new.shape
    if not 1 <= K <= MAX_OBJECTS:
        raise ValueError("filter_step: K=%d rows outside [1, %d]" % (K, MAX_OBJECTS))
    dev = ids_new.device
    for what, t, shape, dtype in (("ids_prev", ids_prev, (B, K), torch.int32), ("ids_new", ids_new, (B, K), torch.int32),
                                  ("count_prev", count_prev, (B,), torch.int32), ("count_new", count_new, (B,), torch.int32),
                                  ("num_objects", num_objects, (B,), torch.int32), ("box", box, (B, K, 8), torch.float64),
                                  ("valid", valid, (B, K), torch.int32), ("state", state, (B, K, 16), torch.float64),
                                  ("since", since, (B, K), torch.int32)):
        _check_tensor(what, t, shape, dtype, dev)
    if into is not None:
        for name, w, dt in StepBoxes.NAMES:
            _check_tensor("into." + name, getattr(into, name, None), (B, K) + ((w,) if w else ()), dt, dev)
        if into.box.data_ptr() == box.data_ptr() or into.valid.data_ptr() == valid.data_ptr():
            raise ValueError("filter_step: into must not share box or valid with the input boxes")
    out = into if into is not None else StepBoxes.empty(B, K, dev)
    act, rst = _flag_bytes(active, B, dev), _flag_bytes(reset, B, dev)
    par = flt.block()
    _lib.call("rtk_track_box_filter_step", B, K, None if act is None else act.data_ptr(), None if rst is None else rst.data_ptr(),
              ids_prev.data_ptr(), count_prev.data_ptr(), ids_new.data_ptr(), count_new.data_ptr(), num_objects.data_ptr(), box.data_ptr(),
              valid.data_ptr(), ctypes.addressof(par), state.data_ptr(), since.data_ptr(), out.box.data_ptr(), out.valid.data_ptr(),
              out.vel.data_ptr(), out.aligned.data_ptr(), out.gap.data_ptr(), _stream())
    return out
