"""Ground-truth objects, their matching to detections and the tracking score of a batch on the device (include/rtk_score.h,
csrc/track_score.hip).

    types  = pack_box_types(per_stream, max_boxes=32, device="cuda")     # (B,K) uint8, 1 = rider; pack_boxes' slot order, frame 1
    gobj   = gt_objects(pc1, boxes, types, n_valid=nv, min_obj_points=net.min_obj_points)                 # launch 1
    scorer = TrackScorer(streams=B, max_objects=trk.K, max_boxes=32, max_gt_tracks=1024)
    m      = scorer.update(out, gobj, reset=is_new_seq, active=has_frame)                                  # launch 2
    res    = scorer.result()                                                                               # the only download

Per stream, `gt_objects` computes what `vod_gt.filter_object_points` returns as `objs_combined` (elements 7 to 9 of its tuple: the
per-box point sets after the rider merge and the minimum object size) and `TrackScorer.update` what `vod_gt.map_gt_objects` returns
for the stream's detections, plus two things built on that matching:

  * `MatchResult.aff_target` (B,Kobj,Kobj): the 0/1 matrix `loss.affinity_loss` builds from the mappings of two consecutive frames,
    laid out like `StepResult.aff` (rows: the stream's previous active frame in that frame's object order; columns: this frame), with
    `aff_defined[b]` telling where that loss is not 0 by definition.  The reference's random negative keys of unmatched detections
    only make keys unequal: "-1 / no match" stands in for them.  Its `mapping_inv` is not reproduced (it stores the last ground-truth
    key of the inner loop and nothing reads it).
  * running counts per stream, all on the device: frames, gt, pred, tp, fp, fn, idsw and, per closed clip (`reset`), tracks and how
    many of them were mostly tracked (matched in > 80 % of the frames they were seen in), mostly lost (< 20 %) or partly tracked.

`TrackScorer.result()` turns the counts into mota = 1 - (fn + fp + idsw) / gt, moda = 1 - (fn + fp) / gt, recall, precision, the
mt / pt / ml fractions of tracks and the mean IoU of the matches.  These are CLEAR-MOT counts UNDER THE REFERENCE'S OWN POINT-IoU
MATCHING (best IoU, first come first served, no threshold) AT THE TRACKER'S OPERATING POINT.  They are not the sAMOTA / AMOTA table
of the reference's README: that one comes from a confidence-swept AB3DMOT variant the reference does not distribute.

Nothing here synchronises with the device except `GtObjects.check()`, `TrackScorer.check()` and `TrackScorer.result()`.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .abi import GtBoxes, GtObjectsIn, GtObjectsOut, ScoreIn, ScoreOut, ScoreState, stream as _stream, view as _view
from .gt_device import _flag_bytes, _n_valid

LDS_LIMIT = 65536                      # RTK_SCORE_LDS_LIMIT
MAX_BOXES = 64                         # RTK_SCORE_MAX_BOXES
MAX_OBJECTS = 256                      # RTK_SCORE_MAX_OBJECTS
MAX_POINTS = 32768                     # RTK_SCORE_MAX_POINTS
COUNTERS = ("frames", "gt", "pred", "tp", "fp", "fn", "idsw", "tracks", "mt", "pt", "ml")
FLAG_BOXES, FLAG_NVALID, FLAG_TRACKS, FLAG_OBJECTS = 1, 2, 4, 8


# ---- what fits -------------------------------------------------------------------------------------------------------------

def check_fit(max_boxes, points, max_objects=None):
    """Raises ValueError, stating the limit, for sizes whose per-stream tables do not fit one workgroup's LDS: those of `gt_objects`
    (max_boxes, points) and, with max_objects, those of `TrackScorer.update` as well.  Host only."""
    K, N = int(max_boxes), int(points)
    if not 1 <= K <= MAX_BOXES:
        raise ValueError("max_boxes=%d outside [1, %d] (a point's ground-truth objects are one 64-bit mask)" % (K, MAX_BOXES))
    if not 1 <= N <= MAX_POINTS:
        raise ValueError("N=%d points outside [1, %d]" % (N, MAX_POINTS))
    need = _lib._fn("rtk_gt_objects_lds_bytes")(K, N)
    if need < 0 or need > LDS_LIMIT:
        raise ValueError("gt_objects: max_boxes=%d and N=%d need %d bytes of LDS per stream, the limit is %d" % (K, N, need, LDS_LIMIT))
    if max_objects is None:
        return
    Kobj = int(max_objects)
    if not 1 <= Kobj <= MAX_OBJECTS:
        raise ValueError("max_objects=%d outside [1, %d]" % (Kobj, MAX_OBJECTS))
    need = _lib._fn("rtk_track_score_lds_bytes")(Kobj, K, N)
    if need < 0 or need > LDS_LIMIT:
        raise ValueError("TrackScorer: max_objects=%d, max_boxes=%d and N=%d need %d bytes of LDS per stream, the limit is %d"
                         % (Kobj, K, N, need, LDS_LIMIT))


# ---- launch 1 --------------------------------------------------------------------------------------------------------------

def pack_box_types(per_stream, max_boxes, device="cuda"):
    """per_stream as `gt_device.pack_boxes` takes it -> (B,K) uint8 on `device`: 1 where the frame-1 box in that slot has the label
    type "rider" (what `vod_gt.filter_object_points` tests), in pack_boxes' slot order."""
    B, K = len(per_stream), int(max_boxes)
    types = np.zeros((B, K), dtype=np.uint8)
    for b, item in enumerate(per_stream):
        if item is None:
            continue
        slots = {}
        for lab in item[0].values():          # pack_boxes' dict: a repeated id keeps its first slot and takes the later label
            slots[lab.id] = lab.type == "rider"
        if len(slots) > K:
            raise ValueError("stream %d, frame 1: %d boxes > max_boxes=%d" % (b, len(slots), K))
        types[b, :len(slots)] = list(slots.values())
    return torch.from_numpy(types).to(device)


class GtObjects:
    """The kept ground-truth objects of B frames, in label order (device tensors): count (B) int32; slot, label_id, size (B,K) int32
    (box slot as in `BoxBatch`, label id, number of points; -1 / -1 / 0 past count); members (B,K,ceil(N/32)) int32 holding uint32
    words, bit p & 31 of word p >> 5 = point p -- an object that received a rider keeps the FIRST column of each distinct coordinate
    triple (the host's torch.unique), so size is the number of set bits for every object; centre (B,K,3) float64, the mean of the
    points of the object's own box; flags (B) int32; n_valid (B) int32 or None."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def check(self):
        """Synchronises.  Raises RuntimeError naming the stream whose box count exceeded K or whose n_valid was out of range."""
        for b, f in enumerate(self.flags.cpu().tolist()):
            if f & FLAG_BOXES:
                raise RuntimeError("gt_objects: stream %d has a box count outside [0, max_boxes=%d]" % (b, self.max_boxes))
            if f & FLAG_NVALID:
                raise RuntimeError("gt_objects: stream %d has an n_valid outside [0, N]" % b)


def _nv_row(n_valid, B, dev):
    if n_valid is None:
        return None
    nv = torch.as_tensor(n_valid)
    return _n_valid(nv[0] if nv.dim() == 2 else nv, (B,), dev)


def gt_objects(pc1, boxes, types, n_valid=None, min_obj_points=2):
    """pc1 (B,3,N) fp32 device tensor of any strides, boxes a `gt_device.BoxBatch` (its frame-1 tables are read), types from
    `pack_box_types`, n_valid (B) int32 -- or the batch's (2,B), whose frame-1 row is taken -- or None.  One launch, no
    synchronisation.  -> GtObjects."""
    B, C, N = pc1.shape
    K = boxes.K
    if boxes.B != B or C != 3 or tuple(types.shape) != (B, K) or types.dtype != torch.uint8:
        raise ValueError("gt_objects: a %s cloud and %s %s types against the boxes of %d streams x %d slots"
                         % (tuple(pc1.shape), tuple(types.shape), types.dtype, boxes.B, K))
    check_fit(K, N)
    dev = pc1.device
    nv = _nv_row(n_valid, B, dev)
    types = types.to(dev).contiguous()
    W = (N + 31) // 32
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    slot, label_id, count, size, members, flags = i32(B, K), i32(B, K), i32(B), i32(B, K), i32(B, K, W), i32(B)
    centre = torch.empty(B, K, 3, dtype=torch.float64, device=dev)
    a = GtObjectsIn(B, N, K, _view(pc1), None if nv is None else nv.data_ptr(),
                    GtBoxes(boxes.boxes[0].data_ptr(), boxes.box_id[0].data_ptr(), boxes.count[0].data_ptr()), types.data_ptr(),
                    int(min_obj_points))
    o = GtObjectsOut(slot.data_ptr(), label_id.data_ptr(), count.data_ptr(), size.data_ptr(), members.data_ptr(), centre.data_ptr(),
                     flags.data_ptr())
    _lib.call("rtk_gt_objects", ctypes.addressof(a), ctypes.addressof(o), _stream())
    return GtObjects(slot=slot, label_id=label_id, count=count, size=size, members=members, centre=centre, flags=flags, n_valid=nv,
                     max_boxes=K, points=N)


# ---- launch 2 --------------------------------------------------------------------------------------------------------------

class MatchResult:
    """One frame's matching (device tensors): pred_gt_slot, pred_gt_id (B,Kobj) int32, the box slot and the label id detection i is
    matched to (-1: unmatched); gt_pred (B,K) int32, the detection kept ground-truth object j (GtObjects order) is matched to;
    iou (B,Kobj) float64 (0 when unmatched); aff_target (B,Kobj,Kobj) fp32; aff_defined (B) uint8.  Inactive streams: -1 / 0."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def values_from_counters(counters, iou_sum):
    """(..., 11) integer counts in COUNTERS order and (...) float64 IoU sums -> dict of float64 arrays: mota, moda, recall, precision,
    mt_fraction, pt_fraction, ml_fraction (of tracks; the counts keep the names mt, pt, ml) and mean_iou.  A ratio without a denominator is NaN."""
    c = np.asarray(counters, dtype=np.float64)
    g = lambda k: c[..., COUNTERS.index(k)]
    with np.errstate(divide="ignore", invalid="ignore"):
        return dict(mota=1.0 - (g("fn") + g("fp") + g("idsw")) / g("gt"), moda=1.0 - (g("fn") + g("fp")) / g("gt"),
                    recall=g("tp") / g("gt"), precision=g("tp") / g("pred"), mt_fraction=g("mt") / g("tracks"),
                    pt_fraction=g("pt") / g("tracks"), ml_fraction=g("ml") / g("tracks"), mean_iou=np.asarray(iou_sum, dtype=np.float64) / g("tp"))


def classify_tracks(seen, matched):
    """Frames seen / matched of ground-truth tracks -> (mt, pt, ml): matched / seen > 0.8 mostly tracked, < 0.2 mostly lost."""
    r = np.asarray(matched, dtype=np.float64) / np.asarray(seen, dtype=np.float64)
    mt, ml = int((r > 0.8).sum()), int((r < 0.2).sum())
    return mt, len(r) - mt - ml, ml


class TrackScorer:
    """Matches the detections of `streams` sequences to their ground-truth objects frame by frame and keeps the score on the device
    (see the module docstring).  State (device tensors): counters (B,11) int64 in COUNTERS order, iou_sum (B) float64, the table of
    open ground-truth tracks (table_key / table_last / table_seen / table_matched (B,max_gt_tracks) int32, table_used (B)), the
    previous active frame's record (prev_gt_id (B,Kobj), prev_count, prev_gt (B)) and sticky flags (B).  Whether the tables fit
    also depends on the clouds' size: `update` checks that (`check_fit`)."""

    def __init__(self, streams, max_objects=128, max_boxes=32, max_gt_tracks=1024, device="cuda"):
        self.B, self.Kobj, self.K, self.T = int(streams), int(max_objects), int(max_boxes), int(max_gt_tracks)
        if self.T < 1:
            raise ValueError("max_gt_tracks=%d must be at least 1" % self.T)
        check_fit(self.K, 1, self.Kobj)
        B, z = self.B, lambda *s: torch.zeros(*s, dtype=torch.int32, device=device)
        self.counters = torch.zeros(B, len(COUNTERS), dtype=torch.int64, device=device)
        self.iou_sum = torch.zeros(B, dtype=torch.float64, device=device)
        self.table_key, self.table_last, self.table_seen, self.table_matched = (z(B, self.T) for _ in range(4))
        self.table_used, self.prev_gt, self.flags = z(B), z(B), z(B)
        self.prev_gt_id = torch.full((B, self.Kobj), -1, dtype=torch.int32, device=device)
        self.prev_count = torch.full((B,), -1, dtype=torch.int32, device=device)

    def update(self, out, gobj, reset=None, active=None):
        """out: a `tracker.StepResult`; gobj: the GtObjects of the same frame (its n_valid is used).  active None: the mask the step
        ran with.  One launch, no synchronisation.  -> MatchResult."""
        if out.max_objects != self.Kobj:
            raise ValueError("TrackScorer(max_objects=%d) against a step with max_objects=%d" % (self.Kobj, out.max_objects))
        return self.update_raw(out.pc1, out.obj, out.num_objects, out.object_ids, gobj, gobj.n_valid, reset,
                               out.active if active is None else active)

    def update_raw(self, pc1, obj, num_objects, object_ids, gobj, n_valid=None, reset=None, active=None):
        """pc1 (B,3,N) fp32 of any strides; obj (B,N) int32, the detection each point belongs to (-1 none; detections are numbered in
        association order); num_objects (B) int32; object_ids (B,Kobj) int32 track ids; gobj from `gt_objects` on the same cloud;
        n_valid (B) / (2,B) / None; reset, active (B) masks or None."""
        B, C, N = pc1.shape
        if B != self.B or C != 3 or tuple(obj.shape) != (B, N) or tuple(object_ids.shape) != (B, self.Kobj) or num_objects.numel() != B:
            raise ValueError("TrackScorer(streams=%d, max_objects=%d): got pc1 %s, obj %s, object_ids %s"
                             % (self.B, self.Kobj, tuple(pc1.shape), tuple(obj.shape), tuple(object_ids.shape)))
        if gobj.max_boxes != self.K or gobj.points != N or gobj.count.numel() != B:
            raise ValueError("TrackScorer(max_boxes=%d): ground-truth objects of %d slots over %d points against %d points"
                             % (self.K, gobj.max_boxes, gobj.points, N))
        check_fit(self.K, N, self.Kobj)
        dev = pc1.device
        as32 = lambda x: x.to(device=dev, dtype=torch.int32).contiguous()
        obj, num_objects, object_ids = as32(obj), as32(num_objects), as32(object_ids)
        nv, rst, act = _nv_row(n_valid, B, dev), _flag_bytes(reset, B, dev), _flag_bytes(active, B, dev)
        Kobj, K = self.Kobj, self.K
        i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
        pred_gt_slot, pred_gt_id, gt_pred = i32(B, Kobj), i32(B, Kobj), i32(B, K)
        iou = torch.empty(B, Kobj, dtype=torch.float64, device=dev)
        aff_target = torch.empty(B, Kobj, Kobj, device=dev)
        aff_defined = torch.empty(B, dtype=torch.uint8, device=dev)
        ptr = lambda x: None if x is None else x.data_ptr()
        a = ScoreIn(B, N, Kobj, K, self.T, _view(pc1), obj.data_ptr(), num_objects.data_ptr(), object_ids.data_ptr(), ptr(nv),
                    gobj.slot.data_ptr(), gobj.label_id.data_ptr(), gobj.count.data_ptr(), gobj.size.data_ptr(), gobj.members.data_ptr(),
                    ptr(rst), ptr(act))
        s = ScoreState(self.counters.data_ptr(), self.iou_sum.data_ptr(), self.table_key.data_ptr(), self.table_last.data_ptr(),
                       self.table_seen.data_ptr(), self.table_matched.data_ptr(), self.table_used.data_ptr(), self.prev_gt_id.data_ptr(),
                       self.prev_count.data_ptr(), self.prev_gt.data_ptr(), self.flags.data_ptr())
        o = ScoreOut(pred_gt_slot.data_ptr(), pred_gt_id.data_ptr(), gt_pred.data_ptr(), iou.data_ptr(), aff_target.data_ptr(),
                     aff_defined.data_ptr())
        _lib.call("rtk_track_score", ctypes.addressof(a), ctypes.addressof(s), ctypes.addressof(o), _stream())
        return MatchResult(pred_gt_slot=pred_gt_slot, pred_gt_id=pred_gt_id, gt_pred=gt_pred, iou=iou, aff_target=aff_target,
                           aff_defined=aff_defined)

    def _raise_on_flags(self, flags):
        for b, f in enumerate(flags):
            if f & FLAG_TRACKS:
                raise RuntimeError("TrackScorer: stream %d saw more than max_gt_tracks=%d label ids in one clip (raise max_gt_tracks)"
                                   % (b, self.T))
            if f & FLAG_NVALID:
                raise RuntimeError("TrackScorer: stream %d has an n_valid outside [0, N]" % b)
            if f & FLAG_OBJECTS:
                raise RuntimeError("TrackScorer: stream %d has a num_objects outside [0, max_objects=%d]" % (b, self.Kobj))

    def check(self):
        """Synchronises.  Raises RuntimeError naming the stream whose track table overflowed or whose sizes were out of range."""
        self._raise_on_flags(self.flags.cpu().tolist())

    def result(self, check=True):
        """The only download; the device state is untouched.  Tracks of clips still open are classified on the downloaded copy.
        -> dict: `per_stream` {name: (B) array} and `overall` {name: number} with the COUNTERS, `iou_sum` and the values of
        `values_from_counters`; `flags` (B).  check: raise (naming the stream) if a stream's table overflowed or its sizes were out
        of range -- nothing is truncated silently."""
        B, T = self.B, self.T
        parts = [self.counters.reshape(-1), self.iou_sum.view(torch.int64), self.table_used.long(), self.flags.long(),
                 self.table_seen.reshape(-1).long(), self.table_matched.reshape(-1).long()]
        host = torch.cat(parts).cpu().numpy()
        nc = len(COUNTERS)
        counters = host[:B * nc].reshape(B, nc).copy()
        o = B * nc
        iou_sum = host[o:o + B].copy().view(np.float64)
        used, flags = host[o + B:o + 2 * B], host[o + 2 * B:o + 3 * B]
        seen = host[o + 3 * B:o + 3 * B + B * T].reshape(B, T)
        matched = host[o + 3 * B + B * T:].reshape(B, T)
        if check:
            self._raise_on_flags(flags.tolist())
        for b in range(B):
            u = int(used[b])
            if u:
                mt, pt, ml = classify_tracks(seen[b, :u], matched[b, :u])
                counters[b, COUNTERS.index("tracks"):] += (u, mt, pt, ml)
        total, total_iou = counters.sum(0), float(iou_sum.sum())
        per = {k: counters[:, i] for i, k in enumerate(COUNTERS)}
        per["iou_sum"] = iou_sum
        per.update(values_from_counters(counters, iou_sum))
        overall = {k: int(total[i]) for i, k in enumerate(COUNTERS)}
        overall["iou_sum"] = total_iou
        overall.update({k: float(v) for k, v in values_from_counters(total, total_iou).items()})
        return dict(per_stream=per, overall=overall, flags=flags.copy())
