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
mt / pt / ml fractions of tracks and the mean IoU of the matches: CLEAR-MOT counts under the reference's own point-IoU matching
(best IoU, first come first served, no threshold) at the tracker's operating point.

The confidence sweep.  `TrackScorer(..., sweep_frames=F, sweep_records=R)` makes the same launch append every active stream's
frame to a packed per-stream log on the device (at most F frames, R detection records and R kept-label entries per stream; a frame
that does not fit is not logged and raises FLAG_LOG), and `scorer.sweep(levels=40)` evaluates sAMOTA / AMOTA / AMOTP over it in a few
launches and one download:

    scorer = TrackScorer(streams=B, max_objects=trk.K, max_boxes=32, sweep_frames=512, sweep_records=16384)
    ...    scorer.update(out, gobj, ...)            # out.object_conf is logged with the match
    sw     = scorer.sweep()                         # SweepResult: amota, samota, amotp, best, per-level arrays

THESE ARE THE SWEEP METRICS OF WENG ET AL. ("3D Multi-Object Tracking: A Baseline and New Evaluation Metrics") APPLIED TO THIS
MODULE'S MATCHING RULE.  With L recall levels:

  * a clip is a stream's frames from one reset to the next; a track is a (stream, clip, track id), and its score the float64 sum
    of the fp32 `object_conf` of its logged detections in log order over their number;
  * the replay at threshold t walks every stream frame by frame without the detections whose track score is < t (equal stays); the
    others go through `update`'s rule in detection order -- the best object (largest IoU > 0, strict >, against all kept
    ground-truth objects: independent of the filter); already taken by a remaining detection: unmatched, no second choice; a
    removed detection takes nothing, so a later one can win an object it lost unfiltered -- and gt, pred, tp, fp, fn, idsw, iou_sum
    and the per-clip track table are counted as `update` counts them, open clips closed at the end; t = -inf reproduces
    `counters` / `iou_sum` bit for bit;
  * the thresholds are the KITTI walk over the track scores s[0..n) of the unfiltered replay's true positives, pooled and sorted
    descending, G the pooled gt count, cur = 0: for i in order, l = (i+1)/G, r = (i+2)/G if i < n-1 else l; if (r - cur) < (cur - l)
    and i < n-1, i is skipped; otherwise s[i] is the next threshold and cur += 1/L.  The first (recall 0) is dropped, the k-th
    remaining one belongs to recall level r_k = k/L; levels the walk never reaches contribute 0 to every average;
  * MOTA_k = 1 - (FP+FN+IDSW)/G, sMOTA_k = max(0, 1 - (FP+FN+IDSW - (1-r_k) G)/(r_k G)), MOTP_k = iou_sum/TP; AMOTA, sAMOTA, AMOTP
    are each the sum over the reached levels divided by L; `best` is the level of the largest MOTA_k (the lowest k among equals).

The device delivers integers and fixed-order IoU sums; every ratio is float64 host arithmetic (`sweep_values`).  They are still NOT
the numbers of the reference's README table: its evaluator (a confidence-swept AB3DMOT variant) is not distributed, and the IoU and
the thresholds it uses are unknown.

Track memory.  Behind a `BatchedTracker(max_age=...)` the previous table is taller than the previous frame's detections: coasted
tracks follow them, and `StepResult.aff` has a row for each.  `TrackScorer(..., track_memory=True)` keeps its record by the tracker's
table (`StepResult.table_ids` / `table_count`), one launch per frame as before (rtk_track_score_memory, rules in
include/rtk_score.h): `prev_gt_id` then holds the label id of EVERY row of the record, `row_track` its track id, and a coasted row
keeps the label id its track last had -- so row i of `aff_target` is row i of `aff`, and a coasted row whose object is detected
again has a 1 in that detection's column.  Two rows may carry one label id (a lost track still coasts while its object came back
under a fresh ID); both get the 1, on purpose: both rows are that object.  `aff_defined` = prev_count > 0 and P > 0 and G > 0 and
(prev_gt > 0 or labelled_coasted > 0): the plain rule wherever nothing coasts, and a frame stays defined when the previous frame had
no kept ground-truth object but a coasted row remembers one.  A plain `TrackScorer` may still score a memory tracker -- its counters
are right -- but its target has no row for a coasted track.

HOTA.  `scorer.hota(alphas=19)` evaluates HOTA with its parts DetA, AssA and LocA (Luiten et al., "HOTA: A Higher Order Metric for
Evaluating Multi-Object Tracking") over the same log, in one launch and one download -- two launches with `threshold=`, for instance
`scorer.hota(threshold=sw.best["threshold"])`, which removes the detections the sweep removes at that threshold:

    ho = scorer.hota()                              # HotaResult: hota, deta_mean, assa_mean, loca_mean, per-alpha arrays

AssA is the share of a trajectory that carries one track id: what CLEAR-MOT's single `idsw` integer cannot say and what track memory
is there to raise.  THIS IS HOTA UNDER THIS MODULE'S MATCHING RULE AND THE REFERENCE'S POINT IoU: per level alpha (a / (A + 1)), a
remaining detection is a candidate when its pre-greedy best object has IoU >= alpha; candidates take their best object in detection
order, first come first served, and a detection below alpha takes nothing (threshold first, then match).  TrackEval's own numbers use
a Hungarian assignment on box IoU and are not these.  The definitions are in include/rtk_score.h; the device delivers integers and
four fixed-order float64 sums, `hota_values` is the arithmetic.

Identity.  `scorer.identity(alphas=(0.5,))` evaluates IDF1, IDP and IDR (Ristani et al., "Performance Measures and a Data Set for
Multi-Target, Multi-Camera Tracking") over the same log, in one launch and one download -- two launches with `threshold=`:

    idn = scorer.identity()                         # IdentityResult: idf1, idr, idp, idtp, idfn, idfp per level

IDF1 is the share of all detections that sit under the single best identity of their object.  Per level alpha every remaining
detection whose best object is one of the frame's kept labels with IoU >= alpha is a candidate -- there is no greedy pass, two
detections of a frame may share a label --; per clip n[g,t] counts the frames in which a candidate of track t had label g, and when
the clip closes idtp gains the weight of a MAXIMUM-WEIGHT ONE-TO-ONE MATCHING of the clip's labels and track ids under n, solved
exactly on the device (csrc/lds_assignment.h).  That is TrackEval's `Identity` arrangement (every pair above the threshold, one global
assignment), but under this module's log -- a detection's best object only -- and the reference's point IoU: TrackEval's own numbers
use box IoU at 0.5 and are not these.  The definitions are in include/rtk_score.h; the device delivers integers, `identity_values`
is the arithmetic.

Optimal matching.  Everything above rests on `update`'s rule (best object, first come first served, no threshold).  The KITTI /
AB3DMOT evaluation matches otherwise: per frame ONE ASSIGNMENT of detections to ground-truth objects that refuses pairs below an IoU
threshold.  `TrackScorer(..., sweep_pairs=Q)` makes the scoring launch also log every (detection, kept object) pair with a common
point (at most Q per stream; a frame whose pairs do not fit is in neither log and raises FLAG_LOG), and then

    sw  = scorer.sweep(matching="optimal", min_iou=0.25)      # SweepResult, with frag and iou_q
    op  = scorer.clear_optimal(min_iou=0.25, threshold=sw.best["threshold"])

replay the log under that scheme: per frame the remaining detections and the kept objects are matched by an exact maximum-weight
assignment (csrc/lds_assignment.h) over the pairs with IoU >= min_iou, weight 2^23 + floor(IoU * 65536) -- most matches first, then
the largest quantised IoU sum --; idsw, the per-clip track table and MT / PT / ML are counted as `update` counts them, and frag counts
an object matched again after a frame in which it was seen but unmatched.  tp, fp, fn and iou_q are unique; where several matchings
are optimal the solver's documented choice (rows in order, ties to the smaller column) is taken.  `min_iou` has no default: the
threshold of the reference's evaluation is not known.  THIS IS THE KITTI / AB3DMOT MATCHING SCHEME ON THE REFERENCE'S POINT IoU AT A
THRESHOLD THE CALLER CHOOSES; it is still not a reproduction of the reference README's numbers, whose threshold and evaluator are not
distributed.  The greedy path is untouched: without `sweep_pairs` the scorer issues the launches it always issued.

HOTA and Identity under TrackEval's matching.  With the pair log,

    ho  = scorer.hota(matching="optimal")           # HotaResult, .matching == "optimal"
    idn = scorer.identity(pairs="all")              # IdentityResult, .pair_mode == "all"

follow TrackEval's arrangement (definitions in include/rtk_score.h, at the end).  HOTA: per clip an alignment pass gives every (label,
track) its global alignment score A -- a Jaccard of the pair's accumulated normalised overlap --, every frame is matched ONCE by an
exact assignment over similarity x A (csrc/lds_assignment.h, the float64 score truncated to 28 bits so that the optimum is an
integer), and the matched pairs are thresholded at each alpha afterwards; A is what makes HOTA prefer the track that follows an object
through the clip over a one-frame intruder with a slightly larger IoU.  Identity: every (detection, object) pair above the level
counts, not only a detection's best object.  `threshold=` removes detections before anything else, the alignment pass included.  WHAT
NOW AGREES WITH TrackEval is the arrangement of both metrics and, under `similarity="centre"` (below), the similarity as well; WHAT
STILL DOES NOT is the 28-bit weights and, under "centre", the positions, which are point centroids rather than label-box centres.
Under the default `similarity="iou"` the similarity is the reference's point IoU.  TrackEval's other similarity is a box IoU:
`similarity="box"` / `"box_bev"` (below) write the pair log under the oriented-box IoU of the detections' fitted boxes
(ratrack_amd/boxes.py) and the label boxes.  The defaults (`matching="greedy"`, `pairs="best"`) are the calls above with their
launches and bits.

The centre-distance similarity.  `TrackScorer(..., sweep_pairs=Q, similarity="centre", zero_distance=2.0)` writes the pair log under
TrackEval's similarity for detections that are positions (`_calculate_euclidean_similarity`): s = max(0, 1 - |c - g| / zero_distance),
c the float64 centroid of the detection's points (column order), g the kept object's `GtObjects.centre`.  A pair is logged iff s > 0,
whatever its common point count -- the point IoU is harsh on radar clusters of two to five points, this asks whether the detection sits
on its object.  Everything else `update` does is bit for bit what it does under "iou" (rtk_track_score_pairs_centre), and

    sw  = scorer.sweep(matching="optimal", min_iou=0.5)       # min_iou: the minimum similarity
    op  = scorer.clear_optimal(min_iou=0.5)
    ho  = scorer.hota(matching="optimal")
    idn = scorer.identity(pairs="all")

replay that log unchanged in every other respect, with "IoU" read as s (the *_sim entry points: the same kernels' bodies on the log's
own similarity).  `similarity_distance(s, zero_distance)` turns motp, amotp and LocA back into metres.  The greedy calls read only the
main log and are the same under either similarity; a log has one similarity: build two scorers for both.

The box IoU.  `TrackScorer(..., sweep_pairs=Q, similarity="box")` writes the pair log under the three-dimensional IoU of each
detection's fitted box (`BatchedTracker(boxes=True, box_min_extent=...)`, or `boxes.object_boxes_raw`) and each kept object's label
box -- entry `GtObjects.slot` of `GtObjects.boxes`, the frame-1 table `pack_boxes` makes --, `similarity="box_bev"` under the IoU of
their footprints in the bird's-eye view: what the KITTI devkit, AB3DMOT, TrackEval's loaders and the VoD devkit match by.  A pair is
logged iff its IoU is > 0, whatever its common point count; everything else `update` does is bit for bit what it does under "iou"
(rtk_track_score_pairs_box, the same single launch), and the four calls above replay the log unchanged with "IoU" read as the box IoU.
Definitions in include/rtk_score.h, the last section.  WHAT STILL DEPARTS FROM TrackEval: the 28-bit assignment weights; the label box
is read UPRIGHT in the radar frame (heading from its first axis, footprint and z range from its centre and half-extents), which drops
the radar-lidar calibration's tilt of about half a degree, and its centre's z is whatever `vod_gt.box_in_radar_frame` takes it to be --
one reason "box_bev" exists; and the detections' boxes are fitted from their points.  A detection without a box has no pairs: a cluster
of two points, or of collinear points, fitted with min_extent = 0 has width 0 -- give `box_min_extent` a positive value.

Nothing here synchronises with the device except `GtObjects.check()`, `TrackScorer.check()`, `TrackScorer.result()`,
`TrackScorer.sweep()`, `TrackScorer.hota()`, `TrackScorer.identity()` and `TrackScorer.clear_optimal()`.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .abi import GtBoxes, GtObjectsIn, GtObjectsOut, ScoreIn, ScoreLog, ScoreMemory, ScoreOut, ScorePairs, ScoreState, stream as _stream, view as _view
from .gt_device import _flag_bytes, _n_valid

LDS_LIMIT = 65536                      # RTK_SCORE_LDS_LIMIT
MAX_BOXES = 64                         # RTK_SCORE_MAX_BOXES
MAX_OBJECTS = 256                      # RTK_SCORE_MAX_OBJECTS
MAX_POINTS = 32768                     # RTK_SCORE_MAX_POINTS
COUNTERS = ("frames", "gt", "pred", "tp", "fp", "fn", "idsw", "tracks", "mt", "pt", "ml")
FLAG_BOXES, FLAG_NVALID, FLAG_TRACKS, FLAG_OBJECTS = 1, 2, 4, 8
FLAG_LOG, FLAG_SWEEP = 16, 32          # RTK_SCORE_FLAG_LOG, RTK_SCORE_FLAG_SWEEP
FLAG_TABLE = 64                        # RTK_SCORE_FLAG_TABLE
SWEEP_TRACKS = 2048                    # RTK_SCORE_SWEEP_TRACKS
FLAG_HOTA = 128                        # RTK_SCORE_FLAG_HOTA
HOTA_COUNTERS = ("frames", "clips", "gt", "pred", "tp", "pairs")
HOTA_SUMS = ("ass", "ass_re", "ass_pr", "loc")
HOTA_PAIRS = 1024                      # RTK_SCORE_HOTA_PAIRS
FLAG_IDENTITY = 256                    # RTK_SCORE_FLAG_IDENTITY
IDENTITY_COUNTERS = ("frames", "clips", "gt", "pred", "idtp", "pairs")
IDENTITY_PAIRS = 1024                  # RTK_SCORE_ID_PAIRS
FLAG_OPTIMAL = 512                     # RTK_SCORE_FLAG_OPTIMAL
OPTIMAL_COUNTERS = ("frames", "gt", "pred", "tp", "fp", "fn", "idsw", "frag", "tracks", "mt", "pt", "ml")
PAIR_EDGES = 2048                      # RTK_SCORE_PAIR_EDGES
ALIGN_PAIRS = 1024                     # RTK_SCORE_ALIGN_PAIRS


# ---- the similarity of the pair log ----------------------------------------------------------------------------------------

SIMILARITIES = ("iou", "centre", "box", "box_bev")
ZERO_DISTANCE = 2.0                    # TrackEval's default zero_distance
BOX_MODES = {"box": 0, "box_bev": 1}   # RTK_SCORE_BOX_3D, RTK_SCORE_BOX_BEV


def check_similarity(similarity="iou", zero_distance=None, sweep_pairs=None):
    """The checks of the two similarities that need no boxes, host only -> (similarity, zero_distance as a float, or None under
    "iou").  "iou": the point IoU of the logged integers, today's scorer; a zero_distance given with it is an error.  "centre":
    TrackEval's centre-distance similarity, which lives in the pair log and so needs sweep_pairs; zero_distance None means 2.0, any
    other value must be a finite number > 0.  Anything else is refused here, the box similarities included: this function is what it
    was before they came (tests/test_track_centre_cpu.py holds it to that); `check_pair_similarity` takes all four."""
    if similarity not in ("iou", "centre"):
        raise ValueError("TrackScorer: similarity=%r is neither \"iou\" nor \"centre\"" % (similarity,))
    if similarity == "iou":
        if zero_distance is not None:
            raise ValueError("TrackScorer: zero_distance=%r goes with similarity=\"centre\"; the point IoU has no distance scale" % (zero_distance,))
        return "iou", None
    if sweep_pairs is None:
        raise ValueError("TrackScorer: similarity=\"centre\" lives in the pair log (give sweep_pairs, with sweep_frames and sweep_records)")
    if zero_distance is None:
        return "centre", ZERO_DISTANCE
    try:
        z = float(zero_distance)
    except (TypeError, ValueError):
        raise ValueError("TrackScorer: zero_distance=%r is not a number" % (zero_distance,))
    if not (np.isfinite(z) and z > 0.0):
        raise ValueError("TrackScorer: zero_distance=%r must be finite and above 0" % (zero_distance,))
    return "centre", z


def check_pair_similarity(similarity="iou", zero_distance=None, sweep_pairs=None):
    """The checks of `TrackScorer(similarity=..., zero_distance=..., sweep_pairs=...)`, host only and before anything is allocated
    -> (similarity, zero_distance as a float or None).  "iou" and "centre": `check_similarity`'s.  "box" / "box_bev": the oriented-box
    IoU in three dimensions / in the bird's-eye view, which lives in the pair log and so needs sweep_pairs; it has no distance scale,
    so a zero_distance given with it is an error.  Any other value is a ValueError that names the four."""
    if not isinstance(similarity, str) or similarity not in SIMILARITIES:
        raise ValueError("TrackScorer: similarity=%r is none of \"iou\", \"centre\", \"box\", \"box_bev\"" % (similarity,))
    if similarity not in BOX_MODES:
        return check_similarity(similarity, zero_distance, sweep_pairs)
    if zero_distance is not None:
        raise ValueError("TrackScorer: zero_distance=%r goes with similarity=\"centre\"; a box IoU has no distance scale" % (zero_distance,))
    if sweep_pairs is None:
        raise ValueError("TrackScorer: similarity=\"%s\" lives in the pair log (give sweep_pairs, with sweep_frames and sweep_records)" % similarity)
    return similarity, None


def similarity_distance(s, zero_distance):
    """The distance a centre-distance similarity stands for, (1 - s) * zero_distance in float64: motp, amotp and LocA in metres."""
    return (1.0 - np.asarray(s, dtype=np.float64)) * float(zero_distance)


# ---- what fits -------------------------------------------------------------------------------------------------------------

def check_fit(max_boxes, points, max_objects=None, track_memory=False, centre=False, box=False):
    """Raises ValueError, stating the limit, for sizes whose per-stream tables do not fit one workgroup's LDS: those of `gt_objects`
    (max_boxes, points) and, with max_objects, those of `TrackScorer.update` as well (track_memory: of its memory variant, which
    keeps max_objects more words; centre: of the centre-similarity variant, which keeps the kept objects' positions; box: of the
    box-IoU variant, which keeps their upright boxes).  Host only."""
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
    memory = 1 if track_memory else 0
    if box:
        name, args = "rtk_track_score_box_lds_bytes", (Kobj, K, N, memory)
    elif centre:
        name, args = "rtk_track_score_centre_lds_bytes", (Kobj, K, N, memory)
    elif track_memory:
        name, args = "rtk_track_score_memory_lds_bytes", (Kobj, K, N)
    else:
        name, args = "rtk_track_score_lds_bytes", (Kobj, K, N)
    need = _lib._fn(name)(*args)
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
    points of the object's own box; boxes (B,K,16) float64, the frame-1 box table `gt_objects` was given (a reference, not a copy: entry
    slot[b][j] is kept object j's label box); flags (B) int32; n_valid (B) int32 or None."""

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
    return GtObjects(slot=slot, label_id=label_id, count=count, size=size, members=members, centre=centre, boxes=boxes.boxes[0], flags=flags,
                     n_valid=nv, max_boxes=K, points=N)


# ---- launch 2 --------------------------------------------------------------------------------------------------------------

class MatchResult:
    """One frame's matching (device tensors): pred_gt_slot, pred_gt_id (B,Kobj) int32, the box slot and the label id detection i is
    matched to (-1: unmatched); gt_pred (B,K) int32, the detection kept ground-truth object j (GtObjects order) is matched to;
    iou (B,Kobj) float64 (0 when unmatched); aff_target (B,Kobj,Kobj) fp32; aff_defined (B) uint8.  Inactive streams: -1 / 0."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _clear_values(names, counters, iou_sum, iou_key):
    """The CLEAR-MOT ratios of (..., len(names)) integer counts in `names` order and (...) float64 IoU sums, iou_sum / tp under `iou_key`."""
    c = np.asarray(counters, dtype=np.float64)
    g = lambda k: c[..., names.index(k)]
    with np.errstate(divide="ignore", invalid="ignore"):
        val = dict(mota=1.0 - (g("fn") + g("fp") + g("idsw")) / g("gt"), moda=1.0 - (g("fn") + g("fp")) / g("gt"),
                   recall=g("tp") / g("gt"), precision=g("tp") / g("pred"), mt_fraction=g("mt") / g("tracks"),
                   pt_fraction=g("pt") / g("tracks"), ml_fraction=g("ml") / g("tracks"))
        val[iou_key] = np.asarray(iou_sum, dtype=np.float64) / g("tp")
    return val


def values_from_counters(counters, iou_sum):
    """(..., 11) integer counts in COUNTERS order and (...) float64 IoU sums -> dict of float64 arrays: mota, moda, recall, precision,
    mt_fraction, pt_fraction, ml_fraction (of tracks; the counts keep the names mt, pt, ml) and mean_iou.  A ratio without a denominator is NaN."""
    return _clear_values(COUNTERS, counters, iou_sum, "mean_iou")


def classify_tracks(seen, matched):
    """Frames seen / matched of ground-truth tracks -> (mt, pt, ml): matched / seen > 0.8 mostly tracked, < 0.2 mostly lost."""
    r = np.asarray(matched, dtype=np.float64) / np.asarray(seen, dtype=np.float64)
    mt, ml = int((r > 0.8).sum()), int((r < 0.2).sum())
    return mt, len(r) - mt - ml, ml


class SweepResult:
    """What `TrackScorer.sweep` returns (host values; see the module docstring for the definitions).  `levels` L; `reached`, the
    number of recall levels the walk reached; `thresholds` (L+1) float64: [0] = -inf (the unfiltered replay), [k] the threshold of
    level k, +inf past `reached`.  Per-level arrays of length L+1, index k = recall level k (index 0: unfiltered, levels past
    `reached`: 0 for counts, NaN for ratios): tp, fp, fn, idsw, gt, pred, tracks, mt, pt, ml (pooled over the streams) and mota,
    smota (NaN at index 0), motp, moda, recall, precision.  amota, samota, amotp.  `best`: dict of the level of the largest MOTA
    (level, threshold, mota, moda, recall, precision, mt_fraction, pt_fraction, ml_fraction and the raw counts), None when no level
    was reached.  `unfiltered`: the pooled index-0 counts and iou_sum.  `counters` (L+1,B,11) int64 and `iou_sums` (L+1,B) float64 per
    stream; `flags` (B).  `matching` "greedy" or "optimal" and `min_iou` (None for greedy); `similarity` and `zero_distance` of the
    scorer's pair log ("iou" and None, "centre" and its distance scale, or "box" / "box_bev" and None: the IoU sums are then sums of s).  Under the optimal matching also `frag`
    (L+1) int64, the pooled fragmentations per level, and `iou_q` (L+1) int64, the pooled sums of the matches' IoUs quantised to
    1/65536 (both 0 past `reached`), with `frag_streams` and `iou_q_streams` (L+1,B) per stream; under the greedy rule they are
    None.  MOTP is iou_sum / tp under either."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def sweep_values(counters, iou_sums, thresholds, reached, levels):
    """The sweep's arithmetic, host only: counters (levels+1,B,11) integer counts in COUNTERS order and iou_sums (levels+1,B)
    float64 of the replays (index 0: unfiltered, index k: recall level k), thresholds (levels+1), reached -> dict with the fields of
    `SweepResult` except flags.  Counts are pooled over the streams (the IoU sums added in stream order); float64 throughout.  A
    reached level without a true positive has MOTP NaN and adds nothing to AMOTP (the divisor stays `levels`); AMOTA and sAMOTA take
    every reached level."""
    L, reached = int(levels), int(reached)
    c = np.asarray(counters, dtype=np.int64).reshape(L + 1, -1, len(COUNTERS))
    q = np.asarray(iou_sums, dtype=np.float64).reshape(L + 1, -1)
    if not 0 <= reached <= L:
        raise ValueError("reached=%d outside [0, levels=%d]" % (reached, L))
    pooled = c.sum(axis=1)
    iou = np.cumsum(q, axis=1)[:, -1] if q.shape[1] else np.zeros(L + 1)          # cumsum: one addition after the other
    live = np.arange(L + 1) <= reached
    pooled[~live] = 0
    iou = np.where(live, iou, 0.0)
    g = lambda k: pooled[:, COUNTERS.index(k)].astype(np.float64)
    G, err = g("gt"), g("fp") + g("fn") + g("idsw")
    rk = np.arange(L + 1, dtype=np.float64) / float(L)
    nan = np.full(L + 1, np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        mota = np.where(live, 1.0 - err / G, nan)
        moda = np.where(live, 1.0 - (g("fp") + g("fn")) / G, nan)
        smota = np.where(live, np.maximum(0.0, 1.0 - (err - (1.0 - rk) * G) / (rk * G)), nan)
        smota[0] = np.nan
        motp = np.where(live, iou / g("tp"), nan)
        recall, precision = np.where(live, g("tp") / G, nan), np.where(live, g("tp") / g("pred"), nan)
    amota = samota = amotp = 0.0
    for k in range(1, reached + 1):                                                  # in level order: fixed bits
        amota += mota[k]
        samota += smota[k]
        if pooled[k, COUNTERS.index("tp")] > 0:
            amotp += motp[k]
    out = dict(levels=L, reached=reached, thresholds=np.asarray(thresholds, dtype=np.float64).copy(), counters=c, iou_sums=q,
               mota=mota, smota=smota, motp=motp, moda=moda, recall=recall, precision=precision, iou_sum=iou,
               amota=amota / L, samota=samota / L, amotp=amotp / L)
    for k in COUNTERS[1:]:
        out[k] = pooled[:, COUNTERS.index(k)].copy()
    counts = lambda k: dict({n: int(pooled[k, i]) for i, n in enumerate(COUNTERS)}, iou_sum=float(iou[k]))
    out["unfiltered"] = counts(0)
    best = None
    for k in range(1, reached + 1):
        if best is None or mota[k] > mota[best]:                                    # strict >: the lowest level among equals
            best = k
    if best is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            tr = np.float64(pooled[best, COUNTERS.index("tracks")])
            frac = {n + "_fraction": float(np.float64(pooled[best, COUNTERS.index(n)]) / tr) for n in ("mt", "pt", "ml")}
        best = dict(counts(best), level=best, threshold=float(out["thresholds"][best]), mota=float(mota[best]), moda=float(moda[best]),
                    smota=float(smota[best]), motp=float(motp[best]), recall=float(recall[best]), precision=float(precision[best]), **frac)
    out["best"] = best
    return out


def optimal_values(counters, iou_sum):
    """(..., 12) integer counts in OPTIMAL_COUNTERS order and (...) float64 IoU sums -> dict of float64 arrays: mota, moda, recall,
    precision, motp (iou_sum / tp) and the mt / pt / ml fractions of tracks.  A ratio without a denominator is NaN."""
    return _clear_values(OPTIMAL_COUNTERS, counters, iou_sum, "motp")


def optimal_sweep_values(counters, iou_q, iou_sums, thresholds, reached, levels):
    """The sweep's arithmetic under the optimal matching, host only: counters (levels+1,B,12) in OPTIMAL_COUNTERS order, iou_q
    (levels+1,B) int64 and iou_sums (levels+1,B) float64 -> `sweep_values` of the eleven shared counters (the same formulas: MOTP is
    iou_sum / tp) plus frag and iou_q pooled per level (0 past `reached`) and per stream."""
    L = int(levels)
    c12 = np.asarray(counters, dtype=np.int64).reshape(L + 1, -1, len(OPTIMAL_COUNTERS))
    iq = np.asarray(iou_q, dtype=np.int64).reshape(L + 1, -1)
    out = sweep_values(c12[:, :, [OPTIMAL_COUNTERS.index(k) for k in COUNTERS]], iou_sums, thresholds, reached, L)
    live = np.arange(L + 1) <= int(reached)
    frag_streams = c12[:, :, OPTIMAL_COUNTERS.index("frag")].copy()
    out.update(frag=np.where(live, frag_streams.sum(axis=1), 0), iou_q=np.where(live, iq.sum(axis=1), 0), frag_streams=frag_streams,
               iou_q_streams=iq.copy())
    if out["best"] is not None:
        out["best"].update(frag=int(out["frag"][out["best"]["level"]]), iou_q=int(out["iou_q"][out["best"]["level"]]))
    out["unfiltered"].update(frag=int(out["frag"][0]), iou_q=int(out["iou_q"][0]))
    return out


class HotaResult:
    """What `TrackScorer.hota` returns (host values; definitions in include/rtk_score.h).  `alphas` A and `alpha` (A) float64, the
    levels a / (A + 1).  Per-level arrays of length A, pooled over the streams: tp, fn, fp, gt, pred, pairs (integers) and deta, detre,
    detpr, assa, assre, asspr, loca, hota_alpha (NaN where the denominator is 0).  Scalars, each the sum over the levels of the
    non-NaN terms divided by A: hota, deta_mean, assa_mean, detre_mean, detpr_mean, assre_mean, asspr_mean, loca_mean.  `counters`
    (A,B,6) int64 in HOTA_COUNTERS order and `sums` (A,B,4) float64 in HOTA_SUMS order per stream; `flags` (B); `threshold` (None
    or the float the detections were filtered with); `matching` "greedy" or "optimal"; `similarity` and `zero_distance` of the scorer's
    pair log ("iou" and None, or "centre" and its distance scale)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def hota_values(counters, sums):
    """HOTA's arithmetic, host only: counters (A,S,6) integer counts in HOTA_COUNTERS order and sums (A,S,4) float64 in HOTA_SUMS order
    of A levels and any number S of streams -> dict with the fields of `HotaResult` except flags and threshold.  Counts are pooled over
    the streams and the sums added in stream order; float64 throughout.  A level without a denominator is NaN and adds nothing to the
    means, whose divisor stays A."""
    c = np.asarray(counters, dtype=np.int64)
    q = np.asarray(sums, dtype=np.float64)
    if c.ndim != 3 or c.shape[2] != len(HOTA_COUNTERS) or q.shape != c.shape[:2] + (len(HOTA_SUMS),) or c.shape[0] < 1:
        raise ValueError("hota_values: counters %s and sums %s are not (A,S,%d) and (A,S,%d)" % (c.shape, q.shape, len(HOTA_COUNTERS), len(HOTA_SUMS)))
    A = c.shape[0]
    pooled = c.sum(axis=1)
    qs = np.cumsum(q, axis=1)[:, -1] if q.shape[1] else np.zeros((A, len(HOTA_SUMS)))       # cumsum: one addition after the other
    g = lambda k: pooled[:, HOTA_COUNTERS.index(k)].astype(np.float64)
    tp, fn, fp = g("tp"), g("gt") - g("tp"), g("pred") - g("tp")
    with np.errstate(divide="ignore", invalid="ignore"):
        val = dict(deta=tp / (tp + fn + fp), detre=tp / (tp + fn), detpr=tp / (tp + fp), assa=qs[:, 0] / tp, assre=qs[:, 1] / tp,
                   asspr=qs[:, 2] / tp, loca=qs[:, 3] / tp)
        val["hota_alpha"] = np.sqrt(val["deta"] * val["assa"])
    out = dict(alphas=A, alpha=np.arange(1, A + 1, dtype=np.float64) / float(A + 1), counters=c, sums=q, **val)
    for k in ("tp", "gt", "pred", "pairs"):
        out[k] = pooled[:, HOTA_COUNTERS.index(k)].copy()
    out["fn"], out["fp"] = out["gt"] - out["tp"], out["pred"] - out["tp"]
    for k, name in (("hota_alpha", "hota"),) + tuple((n, n + "_mean") for n in ("deta", "assa", "detre", "detpr", "assre", "asspr", "loca")):
        acc = 0.0
        for v in val[k]:                                                                 # in level order: fixed bits
            if not np.isnan(v):
                acc += float(v)
        out[name] = acc / A
    return out


class IdentityResult:
    """What `TrackScorer.identity` returns (host values; definitions in include/rtk_score.h).  `alpha` (A) float64, the levels as
    given.  Per-level arrays of length A, pooled over the streams: idtp, idfn, idfp, gt, pred, pairs (integers) and idf1, idr, idp
    (NaN where the denominator is 0).  `counters` (A,B,6) int64 in IDENTITY_COUNTERS order per stream; `flags` (B); `threshold` (None
    or the float the detections were filtered with); `pair_mode` "best" or "all": what `identity(pairs=...)` was given (the field
    `pairs` is the count); `similarity` and `zero_distance` of the scorer's pair log ("iou" and None, or "centre" and its distance scale)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def identity_values(counters, alpha):
    """The identity metrics' arithmetic, host only: counters (A,S,6) integer counts in IDENTITY_COUNTERS order of A levels and any
    number S of streams, alpha the A levels -> dict with the fields of `IdentityResult` except flags and threshold.  Counts are pooled
    over the streams; float64 throughout: IDR = idtp / gt, IDP = idtp / pred, IDF1 = 2 idtp / (gt + pred), NaN without a denominator."""
    c = np.asarray(counters, dtype=np.int64)
    al = np.asarray(alpha, dtype=np.float64).reshape(-1)
    if c.ndim != 3 or c.shape[2] != len(IDENTITY_COUNTERS) or c.shape[0] < 1 or al.shape[0] != c.shape[0]:
        raise ValueError("identity_values: counters %s and alpha %s are not (A,S,%d) and (A)" % (c.shape, al.shape, len(IDENTITY_COUNTERS)))
    pooled = c.sum(axis=1)
    g = lambda k: pooled[:, IDENTITY_COUNTERS.index(k)]
    idtp, gt, pred = g("idtp").astype(np.float64), g("gt").astype(np.float64), g("pred").astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        val = dict(idr=idtp / gt, idp=idtp / pred, idf1=2.0 * idtp / (gt + pred))
    out = dict(alpha=al.copy(), counters=c, **val)
    for k in ("idtp", "gt", "pred", "pairs"):
        out[k] = g(k).copy()
    out["idfn"], out["idfp"] = out["gt"] - out["idtp"], out["pred"] - out["idtp"]
    return out


def _download(tensors):
    """Device tensors of 8-byte elements (int64, float64; a narrower integer is widened by the caller) -> host arrays of the same
    shapes and dtypes, through one concatenation and one `.cpu()`: the one synchronising copy of a call."""
    host = torch.cat([x.reshape(-1).view(torch.int64) for x in tensors]).cpu().numpy()
    out, o = [], 0
    for x in tensors:
        a = host[o:o + x.numel()].copy()
        out.append((a.view(np.float64) if x.dtype == torch.float64 else a).reshape(tuple(x.shape)))
        o += x.numel()
    return out


class TrackScorer:
    """Matches the detections of `streams` sequences to their ground-truth objects frame by frame and keeps the score on the device
    (see the module docstring).  State (device tensors): counters (B,11) int64 in COUNTERS order, iou_sum (B) float64, the table of
    open ground-truth tracks (table_key / table_last / table_seen / table_matched (B,max_gt_tracks) int32, table_used (B)), the
    previous active frame's record (prev_gt_id (B,Kobj), prev_count, prev_gt (B)) and sticky flags (B).  Whether the tables fit
    also depends on the clouds' size: `update` checks that (`check_fit`).

    sweep_frames, sweep_records: both None (today's object and launch), or both given: `update` / `update_raw` then also append
    every active stream's frame to its log for `sweep` -- at most sweep_frames frames, sweep_records detection records and
    sweep_records kept-label entries per stream, about 24 bytes per record.  The log (device tensors, all cursors included):
    log_cursor (B,4) int32 frames | records | label entries logged; log_frame (B,F,4) int32 first record | first label entry |
    detections + 65536 * began a clip | kept objects; log_label (B,R); log_track, log_best (B,R) int32, log_conf (B,R) fp32,
    log_iou (B,R) float64.

    track_memory: False (today's object, launches and bits, also behind a tracker with track memory), or True: the record follows
    the table of a `BatchedTracker(max_age=...)` (module docstring).  prev_gt_id (B,Kobj) is then the label id of every row of the
    record and prev_count its row count; two more state tensors sit next to them: row_track (B,Kobj) int32, the track id of every
    row of the record (-1 past prev_count), and labelled_coasted (B) int32, the record's rows past its frame's detections that carry
    a label id.  `update` takes the table from the StepResult, `update_raw` as table_ids= / table_count=.

    sweep_pairs: None (today's object and launches), or Q, which needs sweep_frames / sweep_records: `update` / `update_raw` then
    also append every (detection, kept object) pair with a common point to the pair log, at most Q per stream (rtk_track_score_pairs,
    with and without track_memory), for `sweep(matching="optimal")` and `clear_optimal`.  A frame whose pairs do not fit is logged in
    neither log (FLAG_LOG).  The pair log (device tensors): pair_cursor (B) int32; pair_frame (B,F,2) int32 first pair | pair count;
    pair_key (B,Q) int32 detection index << 8 | kept-object index; pair_common (B,Q) int32; log_size, log_label_size (B,R) int32, the
    point counts of the logged detections and kept objects.

    similarity: "iou" (today's object, launches and bits) or "centre", which needs sweep_pairs: the pair log then holds every pair
    with centre-distance similarity s = 1 - |c - g| / zero_distance > 0 (module docstring; rtk_track_score_pairs_centre), pair_common
    may be 0, and pair_sim (B,Q) float64 holds s.  zero_distance: None (2.0 under "centre") or a finite number > 0; only with
    "centre".  `update` / `update_raw` then read `gobj.centre`; `sweep(matching="optimal")`, `clear_optimal`, `hota(matching="optimal")`
    and `identity(pairs="all")` replay the log on s (min_iou: the minimum similarity).  "box" / "box_bev", which need sweep_pairs as
    well: the pair log holds every pair whose oriented-box IoU -- in three dimensions / in the bird's-eye view -- between the
    detection's fitted box and the kept object's label box, read upright, is > 0 (module docstring; rtk_track_score_pairs_box);
    pair_common may be 0 and pair_sim (B,Q) float64 holds the IoU.  `update` then reads `out.object_boxes` / `out.object_box_valid`
    (`BatchedTracker(boxes=True)`), `update_raw` takes det_boxes= / det_box_valid=, both read `gobj.boxes`.  A DETECTION WITHOUT A BOX
    HAS NO PAIRS: a cluster of two points, or of collinear points, fitted with min_extent = 0 has width 0 and therefore none -- build
    the tracker with `BatchedTracker(box_min_extent=...)` above 0 (or give `object_boxes_raw` a positive min_extent)."""

    def __init__(self, streams, max_objects=128, max_boxes=32, max_gt_tracks=1024, device="cuda", sweep_frames=None, sweep_records=None,
                 track_memory=False, sweep_pairs=None, similarity="iou", zero_distance=None):
        self.similarity, self.zero_distance = check_pair_similarity(similarity, zero_distance, sweep_pairs)
        self.centre = self.similarity == "centre"
        self.box = self.similarity in BOX_MODES
        self.B, self.Kobj, self.K, self.T = int(streams), int(max_objects), int(max_boxes), int(max_gt_tracks)
        if self.T < 1:
            raise ValueError("max_gt_tracks=%d must be at least 1" % self.T)
        if (sweep_frames is None) != (sweep_records is None):
            raise ValueError("TrackScorer: sweep_frames=%r and sweep_records=%r must be given together" % (sweep_frames, sweep_records))
        self.logging = sweep_frames is not None
        if self.logging:
            self.F, self.R = int(sweep_frames), int(sweep_records)
            if self.F < 1 or self.R < 1 or self.B * max(self.F * 4, self.R) >= 2 ** 31:
                raise ValueError("TrackScorer: sweep_frames=%d, sweep_records=%d must be at least 1 (and the log below 2^31 entries)"
                                 % (self.F, self.R))
        self.pairs = sweep_pairs is not None
        if self.pairs:
            if not self.logging:
                raise ValueError("TrackScorer: sweep_pairs=%r needs the log (give sweep_frames and sweep_records)" % (sweep_pairs,))
            self.Q = int(sweep_pairs)
            if self.Q < 1 or self.B * self.Q >= 2 ** 31:
                raise ValueError("TrackScorer: sweep_pairs=%d must be at least 1 (and the pair log below 2^31 entries)" % self.Q)
        self.track_memory = bool(track_memory)
        check_fit(self.K, 1, self.Kobj, self.track_memory, self.centre, self.box)
        B, z = self.B, lambda *s: torch.zeros(*s, dtype=torch.int32, device=device)
        self.counters = torch.zeros(B, len(COUNTERS), dtype=torch.int64, device=device)
        self.iou_sum = torch.zeros(B, dtype=torch.float64, device=device)
        self.table_key, self.table_last, self.table_seen, self.table_matched = (z(B, self.T) for _ in range(4))
        self.table_used, self.prev_gt, self.flags = z(B), z(B), z(B)
        self.prev_gt_id = torch.full((B, self.Kobj), -1, dtype=torch.int32, device=device)
        self.prev_count = torch.full((B,), -1, dtype=torch.int32, device=device)
        if self.track_memory:
            self.row_track = torch.full((B, self.Kobj), -1, dtype=torch.int32, device=device)
            self.labelled_coasted = z(B)
        if self.logging:
            self.log_cursor, self.log_frame = z(B, 4), z(B, self.F, 4)
            self.log_label, self.log_track, self.log_best = z(B, self.R), z(B, self.R), z(B, self.R)
            self.log_conf = torch.zeros(B, self.R, dtype=torch.float32, device=device)
            self.log_iou = torch.zeros(B, self.R, dtype=torch.float64, device=device)
        if self.pairs:
            self.pair_cursor, self.pair_frame = z(B), z(B, self.F, 2)
            self.pair_key, self.pair_common = z(B, self.Q), z(B, self.Q)
            self.log_size, self.log_label_size = z(B, self.R), z(B, self.R)
        if self.centre or self.box:          # a log that carries its similarity: the replays go to the *_sim entry points
            self.pair_sim = torch.zeros(B, self.Q, dtype=torch.float64, device=device)
        self.has_sim = self.centre or self.box

    def _log_block(self, object_conf=None):
        return ScoreLog(self.F, self.R, object_conf, self.log_cursor.data_ptr(), self.log_frame.data_ptr(), self.log_label.data_ptr(),
                        self.log_track.data_ptr(), self.log_best.data_ptr(), self.log_conf.data_ptr(), self.log_iou.data_ptr())

    def _pair_block(self):
        return ScorePairs(self.Q, self.pair_cursor.data_ptr(), self.pair_frame.data_ptr(), self.pair_key.data_ptr(), self.pair_common.data_ptr(),
                          self.log_size.data_ptr(), self.log_label_size.data_ptr())

    def update(self, out, gobj, reset=None, active=None):
        """out: a `tracker.StepResult`; gobj: the GtObjects of the same frame (its n_valid is used).  active None: the mask the step
        ran with.  With logging on, out.object_conf is logged; with track_memory, out.table_ids / out.table_count are the table;
        under similarity "box" / "box_bev", out.object_boxes / out.object_box_valid are the detections' boxes.  One launch, no
        synchronisation.  -> MatchResult."""
        if out.max_objects != self.Kobj:
            raise ValueError("TrackScorer(max_objects=%d) against a step with max_objects=%d" % (self.Kobj, out.max_objects))
        table = {}
        if self.track_memory:
            if getattr(out, "table_ids", None) is None or getattr(out, "table_count", None) is None:
                raise ValueError("TrackScorer(track_memory=True) keeps its record by the tracker's table, and this step has none: "
                                 "build the tracker with max_age (0 or more)")
            table = dict(table_ids=out.table_ids, table_count=out.table_count)
        if self.box:
            if getattr(out, "object_boxes", None) is None or getattr(out, "object_box_valid", None) is None:
                raise ValueError("TrackScorer(similarity=\"%s\") scores the detections' boxes, and this step has none: build the tracker with "
                                 "BatchedTracker(boxes=True)" % self.similarity)
            table.update(det_boxes=out.object_boxes, det_box_valid=out.object_box_valid)
        return self.update_raw(out.pc1, out.obj, out.num_objects, out.object_ids, gobj, gobj.n_valid, reset,
                               out.active if active is None else active, object_conf=out.object_conf if self.logging else None, **table)

    def update_raw(self, pc1, obj, num_objects, object_ids, gobj, n_valid=None, reset=None, active=None, object_conf=None, table_ids=None,
                   table_count=None, det_boxes=None, det_box_valid=None):
        """pc1 (B,3,N) fp32 of any strides; obj (B,N) int32, the detection each point belongs to (-1 none; detections are numbered in
        association order); num_objects (B) int32; object_ids (B,Kobj) int32 track ids; gobj from `gt_objects` on the same cloud;
        n_valid (B) / (2,B) / None; reset, active (B) masks or None; object_conf (B,Kobj) fp32, the confidence of each detection:
        required when the scorer logs for `sweep`, ignored otherwise; table_ids (B,Kobj) int32 and table_count (B) int32: the
        tracker's NEW table (the one this frame's association wrote: its first num_objects rows are this frame's detections),
        required with track_memory, ignored otherwise; det_boxes (B,Kobj,8) float64 and det_box_valid (B,Kobj) int32: the detections'
        boxes as `boxes.object_boxes` / `object_boxes_raw` return them (`.box`, `.valid`) for the same step, required under
        similarity "box" / "box_bev" (with `gobj.boxes`, the frame-1 box table), ignored otherwise."""
        B, C, N = pc1.shape
        if B != self.B or C != 3 or tuple(obj.shape) != (B, N) or tuple(object_ids.shape) != (B, self.Kobj) or num_objects.numel() != B:
            raise ValueError("TrackScorer(streams=%d, max_objects=%d): got pc1 %s, obj %s, object_ids %s"
                             % (self.B, self.Kobj, tuple(pc1.shape), tuple(obj.shape), tuple(object_ids.shape)))
        if gobj.max_boxes != self.K or gobj.points != N or gobj.count.numel() != B:
            raise ValueError("TrackScorer(max_boxes=%d): ground-truth objects of %d slots over %d points against %d points"
                             % (self.K, gobj.max_boxes, gobj.points, N))
        check_fit(self.K, N, self.Kobj, self.track_memory, self.centre, self.box)
        dev = pc1.device
        gt_boxes = None
        if self.box:
            gt_boxes = getattr(gobj, "boxes", None)
            if gt_boxes is None or tuple(gt_boxes.shape) != (B, self.K, 16) or gt_boxes.dtype != torch.float64:
                raise ValueError("TrackScorer(similarity=\"%s\"): gobj.boxes must be the (%d,%d,16) float64 frame-1 box table, got %s"
                                 % (self.similarity, B, self.K, None if gt_boxes is None else (tuple(gt_boxes.shape), gt_boxes.dtype)))
            if det_boxes is None or det_box_valid is None or tuple(det_boxes.shape) != (B, self.Kobj, 8) or det_boxes.dtype != torch.float64 or \
                    tuple(det_box_valid.shape) != (B, self.Kobj):
                raise ValueError("TrackScorer(similarity=\"%s\"): update_raw needs the detections' boxes, det_boxes (%d,%d,8) float64 and "
                                 "det_box_valid (%d,%d), got %s and %s"
                                 % (self.similarity, B, self.Kobj, B, self.Kobj, None if det_boxes is None else (tuple(det_boxes.shape), det_boxes.dtype),
                                    None if det_box_valid is None else tuple(det_box_valid.shape)))
            gt_boxes, det_boxes = gt_boxes.to(dev).contiguous(), det_boxes.to(dev).contiguous()
            det_box_valid = det_box_valid.to(device=dev, dtype=torch.int32).contiguous()
        gt_centre = None
        if self.centre:
            gt_centre = getattr(gobj, "centre", None)
            if gt_centre is None or tuple(gt_centre.shape) != (B, self.K, 3) or gt_centre.dtype != torch.float64:
                raise ValueError("TrackScorer(similarity=\"centre\"): gobj.centre must be (%d,%d,3) float64, got %s"
                                 % (B, self.K, None if gt_centre is None else (tuple(gt_centre.shape), gt_centre.dtype)))
            gt_centre = gt_centre.to(dev).contiguous()
        if self.track_memory and (table_ids is None or table_count is None or tuple(table_ids.shape) != (B, self.Kobj) or table_count.numel() != B):
            raise ValueError("TrackScorer(track_memory=True): update_raw needs the tracker's table, table_ids (%d,%d) and table_count (%d), got %s and %s"
                             % (B, self.Kobj, B, None if table_ids is None else tuple(table_ids.shape),
                                None if table_count is None else tuple(table_count.shape)))
        if self.logging:
            if object_conf is None or tuple(object_conf.shape) != (B, self.Kobj):
                raise ValueError("TrackScorer(sweep_frames=%d, sweep_records=%d) logs for the sweep: update_raw needs object_conf (%d,%d), got %s"
                                 % (self.F, self.R, B, self.Kobj, None if object_conf is None else tuple(object_conf.shape)))
            object_conf = object_conf.to(device=dev, dtype=torch.float32).contiguous()
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
        lg = self._log_block(object_conf.data_ptr()) if self.logging else None
        pr = self._pair_block() if self.pairs else None
        mm = None
        if self.track_memory:
            table_ids, table_count = as32(table_ids), as32(table_count)
            mm = ScoreMemory(table_ids.data_ptr(), table_count.data_ptr(), self.row_track.data_ptr(), self.labelled_coasted.data_ptr())
        lgp, prp, mmp = (None if x is None else ctypes.addressof(x) for x in (lg, pr, mm))
        # the one launch: the entry point of the scorer's mode and what it takes behind the in, state and out blocks
        if self.box:
            name, extra = "rtk_track_score_pairs_box", (lgp, mmp, prp, self.pair_sim.data_ptr(), det_boxes.data_ptr(), det_box_valid.data_ptr(),
                                                        gt_boxes.data_ptr(), BOX_MODES[self.similarity])
        elif self.centre:
            name, extra = "rtk_track_score_pairs_centre", (lgp, mmp, prp, self.pair_sim.data_ptr(), gt_centre.data_ptr(), self.zero_distance)
        elif self.pairs:
            name, extra = "rtk_track_score_pairs", (lgp, mmp, prp)
        elif self.track_memory:
            name, extra = "rtk_track_score_memory", (lgp, mmp)
        elif self.logging:
            name, extra = "rtk_track_score_logged", (lgp,)
        else:
            name, extra = "rtk_track_score", ()
        _lib.call(name, ctypes.addressof(a), ctypes.addressof(s), ctypes.addressof(o), *extra, _stream())
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
            if f & FLAG_TABLE:
                raise RuntimeError("TrackScorer: stream %d has a table_count outside [num_objects, max_objects=%d]" % (b, self.Kobj))
            if f & FLAG_LOG:
                raise RuntimeError("TrackScorer: stream %d has a frame that did not fit its log of sweep_frames=%d frames and "
                                   "sweep_records=%d records%s and was not logged (raise them)"
                                   % (b, self.F, self.R, " or its pair log of sweep_pairs=%d pairs" % self.Q if self.pairs else ""))
            if f & FLAG_SWEEP:
                raise RuntimeError("TrackScorer.sweep: stream %d has more than %d track ids in one clip" % (b, SWEEP_TRACKS))
            if f & FLAG_HOTA:
                raise RuntimeError("TrackScorer.hota: stream %d has a clip with more than max_gt_tracks=%d label ids, %d track ids or %d "
                                   "(label id, track id) pairs" % (b, self.T, SWEEP_TRACKS, HOTA_PAIRS))
            if f & FLAG_IDENTITY:
                raise RuntimeError("TrackScorer.identity: stream %d has a clip with more than max_gt_tracks=%d label ids, %d track ids or "
                                   "%d (label id, track id) pairs" % (b, self.T, SWEEP_TRACKS, IDENTITY_PAIRS))
            if f & FLAG_OPTIMAL:
                raise RuntimeError("TrackScorer: stream %d has a frame with more than %d candidate (detection, object) pairs for the optimal "
                                   "matching" % (b, PAIR_EDGES))

    def check(self):
        """Synchronises.  Raises RuntimeError naming the stream whose track table overflowed or whose sizes were out of range."""
        self._raise_on_flags(self.flags.cpu().tolist())

    def result(self, check=True):
        """The only download; the device state is untouched.  Tracks of clips still open are classified on the downloaded copy.
        -> dict: `per_stream` {name: (B) array} and `overall` {name: number} with the COUNTERS, `iou_sum` and the values of
        `values_from_counters`; `flags` (B).  check: raise (naming the stream) if a stream's table overflowed or its sizes were out
        of range -- nothing is truncated silently."""
        B = self.B
        counters, iou_sum, used, flags, seen, matched = _download([self.counters, self.iou_sum, self.table_used.long(), self.flags.long(),
                                                                   self.table_seen.long(), self.table_matched.long()])
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
        return dict(per_stream=per, overall=overall, flags=flags)

    def _optimal_args(self, what, min_iou):
        """The checks `sweep(matching="optimal")` and `clear_optimal` share -> min_iou as a float."""
        if not self.pairs:
            raise RuntimeError("TrackScorer.%s: the optimal matching needs the pair log (give sweep_pairs)" % what)
        if min_iou is None:
            raise ValueError("TrackScorer.%s: the optimal matching needs an explicit min_iou in (0, 1]: the threshold of the reference's "
                             "evaluation is not known, so there is no default" % what)
        m = float(min_iou)
        if not (np.isfinite(m) and 0.0 < m <= 1.0):
            raise ValueError("TrackScorer.%s: min_iou=%r outside (0, 1]" % (what, min_iou))
        need = _lib._fn("rtk_score_optimal_lds_bytes")(self.T)
        if need < 0 or need > LDS_LIMIT:
            raise ValueError("TrackScorer.%s: max_gt_tracks=%d needs %d bytes of LDS per stream for the optimal matching, the limit is %d"
                             % (what, self.T, need, LDS_LIMIT))
        return m

    def sweep(self, levels=40, check=True, matching="greedy", min_iou=None):
        """sAMOTA / AMOTA / AMOTP over the log (module docstring): track scores, the unfiltered replay, a sort of the true
        positives' scores, the threshold walk and the replay at every threshold on the device -- five launches of this library plus
        torch's sort -- then one download.  The running state and the log are only read: scoring may go on.  check: raise (naming the
        stream) on any sticky flag, a frame that did not fit the log among them.  matching "greedy": `update`'s rule, today's call.
        "optimal": both replays match every frame by an exact assignment over the logged pairs with IoU >= min_iou (module docstring;
        under similarity="centre" min_iou is the minimum similarity s);
        it needs the pair log (sweep_pairs) and an explicit min_iou in (0, 1] -- there is no default.  -> SweepResult."""
        if matching not in ("greedy", "optimal"):
            raise ValueError("TrackScorer.sweep: matching=%r is neither \"greedy\" nor \"optimal\"" % (matching,))
        if not self.logging:
            raise RuntimeError("TrackScorer.sweep: the scorer keeps no log (give sweep_frames and sweep_records)")
        L = int(levels)
        if not 1 <= L <= 65534:
            raise ValueError("levels=%d outside [1, 65534]" % L)
        if matching == "optimal":
            m = self._optimal_args("sweep", min_iou)
            pr = self._pair_block()
            prp = ctypes.addressof(pr)
            replay = lambda lgp, score, thr, reached, count, mask, flags, st: self._replay_optimal(lgp, prp, score, thr, reached, count, m, mask,
                                                                                                  flags, st)
            fl, val = self._sweep(L, check, replay, OPTIMAL_COUNTERS, optimal_sweep_values)
            return SweepResult(flags=fl, matching="optimal", min_iou=m, similarity=self.similarity, zero_distance=self.zero_distance, **val)
        if min_iou is not None:
            raise ValueError("TrackScorer.sweep: min_iou=%r goes with matching=\"optimal\"; the greedy rule has no threshold" % (min_iou,))
        fl, val = self._sweep(L, check, self._replay_greedy, COUNTERS, sweep_values)
        return SweepResult(flags=fl, matching="greedy", min_iou=None, frag=None, iou_q=None, frag_streams=None, iou_q_streams=None,
                           similarity=self.similarity, zero_distance=self.zero_distance, **val)

    def _sweep(self, L, check, replay, names, values):
        """The sweep under either matching: track means, the unfiltered replay with the mask, the sort, the threshold walk and the
        replay at the thresholds; one download.  replay(lgp, score, thr, reached, count, mask, flags, st) -> the replay's device
        outputs, the counters (count,B,len(names)) first; values(*those on the host, thresholds, reached, L) -> the result's fields.
        -> (flags, fields)."""
        B, dev = self.B, self.counters.device
        lg = self._log_block()
        lgp, st = ctypes.addressof(lg), _stream()
        score = torch.zeros(B, self.R, dtype=torch.float64, device=dev)
        flags = self.flags.clone()
        _lib.call("rtk_score_track_means", B, lgp, score.data_ptr(), flags.data_ptr(), st)
        mask = torch.zeros(B, self.R, dtype=torch.uint8, device=dev)
        minus = torch.full((1,), float("-inf"), dtype=torch.float64, device=dev)
        c0 = replay(lgp, score, minus, None, 1, mask, flags, st)[0]
        ordered = torch.where(mask.bool(), score, minus).reshape(-1).sort(descending=True).values
        n, gt = mask.sum(dtype=torch.int64).reshape(1), c0[0, :, names.index("gt")].sum().reshape(1)
        thr = torch.empty(L + 1, dtype=torch.float64, device=dev)
        reached = torch.empty(1, dtype=torch.int32, device=dev)
        _lib.call("rtk_score_thresholds", ordered.data_ptr(), n.data_ptr(), gt.data_ptr(), L, thr.data_ptr(), reached.data_ptr(), st)
        outs = replay(lgp, score, thr, reached, L + 1, None, flags, st)
        *outs, thresholds, k, fl = _download(list(outs) + [thr, reached.long(), flags.long()])
        if check:
            self._raise_on_flags(fl.tolist())
        return fl, values(*outs, thresholds, int(k[0]), L)

    def _replay_greedy(self, lgp, score, thr, reached, count, mask, flags, st):
        B, dev = self.B, self.counters.device
        c = torch.empty(count, B, len(COUNTERS), dtype=torch.int64, device=dev)
        q = torch.empty(count, B, dtype=torch.float64, device=dev)
        _lib.call("rtk_score_replay", B, self.T, lgp, score.data_ptr(), thr.data_ptr(), None if reached is None else reached.data_ptr(), count,
                  c.data_ptr(), q.data_ptr(), None if mask is None else mask.data_ptr(), st)
        return c, q

    def _replay_optimal(self, lgp, prp, score, thr, reached, count, min_iou, mask, flags, st):
        B, dev = self.B, self.counters.device
        c = torch.empty(count, B, len(OPTIMAL_COUNTERS), dtype=torch.int64, device=dev)
        iq = torch.empty(count, B, dtype=torch.int64, device=dev)
        q = torch.empty(count, B, dtype=torch.float64, device=dev)
        tail = (score.data_ptr(), thr.data_ptr(), None if reached is None else reached.data_ptr(), count, min_iou, c.data_ptr(), iq.data_ptr(),
                q.data_ptr(), None if mask is None else mask.data_ptr(), flags.data_ptr(), st)
        self._call_on_pairs("rtk_score_replay_optimal", (B, self.T, lgp, prp), *tail)
        return c, iq, q

    def _call_on_pairs(self, name, head, *tail):
        """A replay of the pair log: `name(*head, *tail)`, head ending in the pair block -- or, where the log carries its similarity,
        the `_sim` twin with pair_sim right behind the pair block."""
        if self.has_sim:
            _lib.call(name + "_sim", *head, self.pair_sim.data_ptr(), *tail)
        else:
            _lib.call(name, *head, *tail)

    def _threshold_scores(self, threshold, lgp, flags, st):
        """The prologue of a call that may filter by track score.  threshold None: (None, None), no launch.  A float or a 0-dim
        tensor: (the threshold (1) and the track scores (B,R) on the device), one launch (rtk_score_track_means)."""
        if threshold is None:
            return None, None
        dev = self.counters.device
        thr = torch.as_tensor(threshold, dtype=torch.float64).reshape(1).to(dev)
        score = torch.zeros(self.B, self.R, dtype=torch.float64, device=dev)
        _lib.call("rtk_score_track_means", self.B, lgp, score.data_ptr(), flags.data_ptr(), st)
        return thr, score

    def clear_optimal(self, min_iou, threshold=None, check=True):
        """The one operating point under the optimal matching (module docstring): every logged detection (threshold None, one launch)
        or those whose track score is not below `threshold` (a float or a 0-dim tensor, two launches), matched frame by frame by an
        exact assignment over the logged pairs with IoU >= min_iou (explicit, in (0, 1]).  Then one download; the running state and
        the logs are only read.  -> dict: `per_stream` {name: (B) array} and `overall` {name: number} with the OPTIMAL_COUNTERS,
        iou_q, iou_sum and the ratios mota, moda, recall, precision, motp (iou_sum / tp), mt_fraction, pt_fraction, ml_fraction (NaN
        without a denominator); `flags` (B); `min_iou`, `threshold`."""
        m = self._optimal_args("clear_optimal", min_iou)
        B, dev = self.B, self.counters.device
        lg, pr = self._log_block(), self._pair_block()
        lgp, prp, st = ctypes.addressof(lg), ctypes.addressof(pr), _stream()
        flags = self.flags.clone()
        thr, score = self._threshold_scores(threshold, lgp, flags, st)
        if thr is None:          # nothing is removed: the scores are not read past the comparison with -inf
            thr = torch.full((1,), float("-inf"), dtype=torch.float64, device=dev)
            score = torch.zeros(B, self.R, dtype=torch.float64, device=dev)
        c, iq, q = self._replay_optimal(lgp, prp, score, thr, None, 1, m, None, flags, st)
        (counters,), (iou_q,), (iou_sum,), (tau,), fl = _download([c, iq, q, thr, flags.long()])
        if check:
            self._raise_on_flags(fl.tolist())
        per = {k: counters[:, i] for i, k in enumerate(OPTIMAL_COUNTERS)}
        per.update(iou_q=iou_q, iou_sum=iou_sum, **optimal_values(counters, iou_sum))
        total = counters.sum(0)
        total_iou = float(np.cumsum(iou_sum)[-1]) if B else 0.0          # cumsum: one addition after the other, in stream order
        overall = {k: int(total[i]) for i, k in enumerate(OPTIMAL_COUNTERS)}
        overall.update(iou_q=int(iou_q.sum()), iou_sum=total_iou, **{k: float(v) for k, v in optimal_values(total, total_iou).items()})
        return dict(per_stream=per, overall=overall, flags=fl, min_iou=m, threshold=None if threshold is None else float(tau),
                    similarity=self.similarity, zero_distance=self.zero_distance)

    def _pair_log_args(self, what, keyword, value, choices):
        """The checks `hota(matching=...)` and `identity(pairs=...)` share: the keyword's value, and the pair log for the second choice."""
        if value not in choices:
            raise ValueError("TrackScorer.%s: %s=%r is neither \"%s\" nor \"%s\"" % (what, keyword, value, choices[0], choices[1]))
        if value == choices[1] and not self.pairs:
            raise RuntimeError("TrackScorer.%s: the optimal matching needs the pair log (give sweep_pairs)" % what)

    def hota(self, alphas=19, threshold=None, check=True, matching="greedy"):
        """HOTA, DetA, AssA and LocA over the log (module docstring; definitions in include/rtk_score.h) at `alphas` levels
        a / (alphas + 1).  threshold None: every logged detection counts, one launch.  A float or a 0-dim tensor (for instance
        `sweep().best["threshold"]`): the detections whose track score is below it are removed as the sweep removes them, two
        launches (track scores, then HOTA).  Then one download.  The running state and the log are only read: scoring may go on.
        check: raise (naming the stream) on any sticky flag and on a clip that overflowed HOTA's tables; check=False returns the
        other streams' numbers (`flags` tells which to leave out).  matching "greedy": `update`'s rule at every level, today's call.
        "optimal": TrackEval's arrangement over the pair log (sweep_pairs) -- the alignment pass, then one exact assignment per frame
        for all levels (module docstring) --, one launch more; a clip beyond the alignment pass's tables raises FLAG_HOTA, a frame with
        more than PAIR_EDGES valid pairs FLAG_OPTIMAL.  -> HotaResult."""
        self._pair_log_args("hota", "matching", matching, ("greedy", "optimal"))
        if not self.logging:
            raise RuntimeError("TrackScorer.hota: the scorer keeps no log (give sweep_frames and sweep_records)")
        A = int(alphas)
        if not 1 <= A <= 63:
            raise ValueError("alphas=%d outside [1, 63]" % A)
        B, dev = self.B, self.counters.device
        if matching == "optimal":
            need = _lib._fn("rtk_score_alignment_lds_bytes")(self.T)
            if need < 0 or need > LDS_LIMIT:
                raise ValueError("TrackScorer.hota: max_gt_tracks=%d needs %d bytes of LDS per stream for the alignment pass, the limit is %d"
                                 % (self.T, need, LDS_LIMIT))
        lg = self._log_block()
        lgp, st = ctypes.addressof(lg), _stream()
        flags = self.flags.clone()
        thr, score = self._threshold_scores(threshold, lgp, flags, st)
        c = torch.empty(A, B, len(HOTA_COUNTERS), dtype=torch.int64, device=dev)
        q = torch.empty(A, B, len(HOTA_SUMS), dtype=torch.float64, device=dev)
        sp, tp = None if score is None else score.data_ptr(), None if thr is None else thr.data_ptr()
        if matching == "optimal":
            pr = self._pair_block()
            prp = ctypes.addressof(pr)
            pair_a = torch.empty(B, self.Q, dtype=torch.float64, device=dev)
            pair_index, clip_cg, clip_ct = (torch.empty(B, self.Q, dtype=torch.int32, device=dev) for _ in range(3))
            tables = (pair_a.data_ptr(), pair_index.data_ptr(), clip_cg.data_ptr(), clip_ct.data_ptr())
            self._call_on_pairs("rtk_score_alignment", (B, self.T, lgp, prp), sp, tp, *tables, flags.data_ptr(), st)
            self._call_on_pairs("rtk_score_hota_optimal", (B, lgp, prp), sp, tp, A, *tables, c.data_ptr(), q.data_ptr(), flags.data_ptr(), st)
        else:
            _lib.call("rtk_score_hota", B, self.T, lgp, sp, tp, A, c.data_ptr(), q.data_ptr(), flags.data_ptr(), st)
        counters, sums, fl, *tau = _download([c, q, flags.long()] + ([] if thr is None else [thr]))
        tau = float(tau[0][0]) if tau else None
        if check:
            self._raise_on_flags(fl.tolist())
        return HotaResult(flags=fl, threshold=tau, matching=matching, similarity=self.similarity, zero_distance=self.zero_distance,
                          **hota_values(counters, sums))

    def identity(self, alphas=(0.5,), threshold=None, check=True, pairs="best"):
        """IDF1, IDP and IDR over the log (module docstring; definitions in include/rtk_score.h).  alphas: a float or a sequence of
        1..63 floats, each finite and in (0, 1]: the IoU levels.  threshold as in `hota`: None, one launch; a float or a 0-dim
        tensor, the detections whose track score is below it are removed, two launches (track scores, then the walk).  Then one
        download.  The running state and the log are only read: scoring may go on.  check: raise (naming the stream) on any sticky
        flag and on a clip that overflowed the tables; check=False returns the other streams' numbers (`flags` tells which to leave
        out).  pairs "best": a detection counts for its best object only, today's call.  "all": every (detection, object) pair of the
        pair log (sweep_pairs) at or above the level counts, as TrackEval counts them (module docstring); the same number of
        launches.  -> IdentityResult."""
        self._pair_log_args("identity", "pairs", pairs, ("best", "all"))
        if not self.logging:
            raise RuntimeError("TrackScorer.identity: the scorer keeps no log (give sweep_frames and sweep_records)")
        al = np.atleast_1d(np.asarray(alphas, dtype=np.float64))
        if al.ndim != 1 or not 1 <= al.shape[0] <= 63:
            raise ValueError("alphas=%r must be a float or a sequence of 1 to 63 floats" % (alphas,))
        if not (np.isfinite(al) & (al > 0.0) & (al <= 1.0)).all():
            raise ValueError("alphas=%r: every level must be finite and in (0, 1]" % (alphas,))
        A, B, dev = al.shape[0], self.B, self.counters.device
        lg = self._log_block()
        lgp, st = ctypes.addressof(lg), _stream()
        flags = self.flags.clone()
        thr, score = self._threshold_scores(threshold, lgp, flags, st)
        levels = torch.from_numpy(al.copy()).to(dev)
        c = torch.empty(A, B, len(IDENTITY_COUNTERS), dtype=torch.int64, device=dev)
        sp, tp = None if score is None else score.data_ptr(), None if thr is None else thr.data_ptr()
        if pairs == "all":
            pr = self._pair_block()
            self._call_on_pairs("rtk_score_identity_pairs", (B, self.T, lgp, ctypes.addressof(pr)), sp, tp, levels.data_ptr(), A, c.data_ptr(),
                                flags.data_ptr(), st)
        else:
            _lib.call("rtk_score_identity", B, self.T, lgp, sp, tp, levels.data_ptr(), A, c.data_ptr(), flags.data_ptr(), st)
        counters, fl, *tau = _download([c, flags.long()] + ([] if thr is None else [thr]))
        tau = float(tau[0][0]) if tau else None
        if check:
            self._raise_on_flags(fl.tolist())
        return IdentityResult(flags=fl, threshold=tau, pair_mode=pairs, similarity=self.similarity, zero_distance=self.zero_distance,
                              **identity_values(counters, al))
