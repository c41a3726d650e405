"""Many sequences at once: B independent radar sequences tracked in lockstep, one batched step per frame.

    trk = BatchedTracker(net, streams=B, max_objects=128)      # net: an eval-mode Track4D; the Affinity weights are read here
    out = trk.step(pc1, pc2, feature1, feature2, n_valid=None, reset=None, active=None)

Per stream, `step()` computes what `Track4D.forward` computes for that stream run alone (models/track4d.py:49-65): the backbone on
the fused engine for the whole batch, then detection and association as four HIP launches for the whole batch
(csrc/track_batched.hip) -- no host synchronisation between the backbone and the track IDs.  State between steps (h, the previous
objects' descriptors, IDs and count, the next-ID counter) lives on the device; this frame's descriptors and IDs become the previous
ones by a buffer swap -- or, with `static_state=True`, by one device copy at the start of the next step, so that the state's
addresses never change and the whole step can be captured in a hipGraph and replayed (`graph=True`; several independent groups of
streams in flight at once: `TrackerPipeline`).

  * reset (B,) bool: the reference's is_new_seq (main_utils.py:70-74): the stream's h goes to zero and its previous objects are
    dropped; its ID counter keeps counting (the reference's max_id across clips).
  * active (B,) bool: a stream that sits the frame out keeps h, previous objects and counter exactly as they were and reports no
    objects (clips of different lengths).  reset only acts on an active stream.

Outputs stay on the device; `StepResult.objects(b)`, `aff_mat(b)`, `indices1(b)` and `BatchedTracker.write_results` synchronise
when they are called.  More than `max_objects` objects in a stream is an error, never a truncation: the kernels flag it on the
device and `objects`, `write_results` and `check()` raise.

Track memory (`max_age`, off by default): the reference's rule is that the previous objects of a frame are the detections of the
stream's last active frame and nothing else -- an object missed for one frame comes back with a fresh ID.  With
`BatchedTracker(..., max_age=A)` the previous table of a stream is its last active frame's detections (its first `n_det` rows)
followed by the tracks that were not matched for up to A active frames, each holding its last descriptor (no motion model unless `motion` asks for one, below); the
association kernels see one table of `count` rows and need not know which is which.  A fifth launch (rtk_track_memory, rules in
include/rtk_fused.h) advances that table on the device; `StepResult.object_hits`, `object_gap`, `num_coasted` and `prev_age` report
the lifecycle.  Detections plus coasted tracks beyond `max_objects` rows drop the last coasted tracks and set a flag: `check()`
raises, `objects` and `write_results` do not (what they report is complete).

Motion (`motion="flow"`, off by default, needs `max_age`): every row of the table also carries a velocity -- the object's displacement
per frame in the sensor frame, its mean predicted scene flow (descriptor channels 134..136; the flow includes the ego motion, so no
pose is needed), smoothed along the track by `motion_beta` -- and a coasted row's centre (channels 0..2) is advanced by it every
frame it coasts, so that the Affinity MLP sees one frame of motion in `desc_cur - desc_prev` however long the track was lost.  The
fifth launch is then rtk_track_memory_motion (csrc/track_motion.hip) instead of rtk_track_memory; `StepResult.object_velocity` and
`table_velocity` report the estimate.  Without `motion` a coasted track holds its last descriptor, as above.
"""
import ctypes
import os

import torch

from . import _lib
from .captured import CapturedStep, capture_graph, signature
from .abi import TrackFrame, View as _View, stream, view as _view  # noqa: F401  (_View: tests and tools take it from here)

DESC = 141
DBSCAN_POINT_BYTES = 48          # RTK_DBSCAN_POINT_BYTES
DBSCAN_LDS_BYTES = 128 * 1024
_FLAG_OVERFLOW, _FLAG_NVALID, _FLAG_TRUNCATED = 1, 2, 4


def max_objects_limit():
    """The largest max_objects the batched association accepts (its per-stream table in one workgroup's LDS)."""
    return _lib.load().rtk_track_max_objects()


def pack_affinity(affinity):
    """Affinity.affinity (Linear 141-564-282-70-35-1) -> the packed fp32 image of rtk_affinity_pairs: per layer W^T (Cin, Cout), b."""
    lins = [m for m in affinity.affinity if isinstance(m, torch.nn.Linear)]
    dims = [(l.in_features, l.out_features) for l in lins]
    if dims != [(141, 564), (564, 282), (282, 70), (70, 35), (35, 1)]:
        raise ValueError("rtk_affinity_pairs is built for the 141-564-282-70-35-1 Affinity MLP, got %s" % (dims,))
    parts = []
    for l in lins:
        parts += [l.weight.detach().float().t().reshape(-1), l.bias.detach().float().reshape(-1)]
    return torch.cat(parts).contiguous()


def _mask(x, B, default, dev):
    if x is None:
        return torch.full((B,), int(default), dtype=torch.uint8, device=dev)
    t = torch.as_tensor(x).to(device=dev).reshape(-1)
    if t.numel() != B:
        raise ValueError("a per-stream mask needs %d entries, got %d" % (B, t.numel()))
    return (t != 0).to(torch.uint8)


def check_n_valid(n_valid, N):
    """Host-side sizes check of a (2,B) n_valid (a device tensor is checked by the kernels: flag -> check() raises)."""
    if n_valid is not None and not (torch.is_tensor(n_valid) and n_valid.is_cuda):
        nv = torch.as_tensor(n_valid)
        if nv.dim() != 2 or nv.shape[0] != 2:
            raise ValueError("n_valid must be (2, B), got %s" % (tuple(nv.shape),))
        if bool((nv > N).any()) or bool((nv < 0).any()):
            raise ValueError("n_valid %s outside [0, N=%d]" % (nv.tolist(), N))


def device_n_valid(n_valid, B, N, dev):
    """`check_n_valid`, then n_valid as a contiguous (2,B) int32 tensor on `dev` (None stays None)."""
    check_n_valid(n_valid, N)
    return None if n_valid is None else torch.as_tensor(n_valid).to(device=dev, dtype=torch.int32).reshape(2, B).contiguous()


def reset_h(h, reset):
    """h (5,B,128) with the state of the streams that `reset` (B,) marks zeroed."""
    return torch.where((reset != 0).view(1, -1, 1), 0.0, h)


def keep_h(active, h_new, h_old):
    """The new h of the streams that `active` (B,) marks, the old h of those that sit the frame out."""
    return torch.where((active != 0).view(1, -1, 1), h_new, h_old)


class StepResult:
    """One step's outputs (device tensors): flow (B,3,N), cls (B,N), h (5,B,128), point_track_id (B,N) int32, num_objects (B,),
    object_ids / object_conf (B,K), aff (B,K,K) (only [:m_b, :n_b] meaningful), indices1() (B,K) int32 (-1: no match);
    descriptors / desc_prev (B,K,141): this frame's and the previous objects' descriptors (the tracker's own buffers: the next
    step but one overwrites them; with `static_state=True` the NEXT step does, as it advances the state in place).
    From a `BatchedTracker(graph=True)` every tensor here is a static output of the captured graph: the next step overwrites all of
    them in place, so clone what must outlive it.  Each step hands back a new StepResult, so the host-side copy that `objects`,
    `aff_mat`, `indices1(b)` and `check` keep belongs to that step alone.
    With track memory (`BatchedTracker(max_age=...)`, else None): object_hits (B,K) int32: how many frames object j's track has been
    detected in, this one included (0 past num_objects); object_gap (B,K) int32: the age of the row object j inherited its ID from --
    0: seen last frame, g: re-acquired after g missed frames, -1: a fresh ID or past num_objects; num_coasted (B,) int32: the rows of
    the new table that are coasted tracks; prev_age (B,K) int32: the ages of the previous table's rows, aligned with the rows of `aff`
    (0: a detection of the last active frame; the first `num_prev` are meaningful); table_ids (B,K) int32 and table_count (B) int32:
    the table this step wrote -- the track id of every row, this frame's detections first and the coasted tracks after them, and its
    row count (the tracker's own buffers, overwritten like `descriptors`): what `TrackScorer(track_memory=True)` keeps its record
    by.
    With `BatchedTracker(motion="flow")` (else None): object_velocity (B,K,3): the velocity of object j's track after this frame's
    measurement, metres per frame in the sensor frame (0 past num_objects and on an inactive stream); table_velocity (B,K,3): the
    velocity of every row of the table this step wrote, aligned with `table_ids` (0 past `table_count`) -- a view of the tracker's
    own buffer, overwritten when `table_ids` is.
    With `BatchedTracker(assign="optimal")` (else None): assign_total (B,) int64: the weight of the stream's matching, the sum of
    (int)(aff * 2^28) over its matched pairs; 0 where nothing was associated (no previous or no current objects); an inactive stream
    keeps the value of its last active frame (0 before the first) -- the tracker's own buffer, overwritten by the next step.
    With `BatchedTracker(boxes=True)` (else None): object_boxes (B,K,8) float64: the oriented box of object j, (cx, cy, cz, l, w, h,
    yaw, area) in the sensor frame (ratrack_amd/boxes.py; zeros past num_objects and on an inactive stream); object_box_valid (B,K)
    int32: the object's point count (0: no object, -1: a coordinate that is not finite); object_box_cand (B,K) int32: the winning
    candidate of the search (-1: no box); object_box_flags (B) int32: boxes.FLAG_AXIS where an object above boxes.MAX_POINTS points was
    fitted axis-aligned.
    With `BatchedTracker(box_filter=BoxFilter(...))` (else None): the boxes of the TRACKS in the table this step wrote, from a Kalman
    filter advanced inside the step (include/rtk_fused.h, "Filtered boxes inside the step").  Rows j < num_objects[b] are the objects,
    in the order of `object_ids`; with `max_age` the rows up to table_count[b] are the coasted tracks, aligned with `table_ids`.
    filtered_boxes (B,K,8) float64 and filtered_valid (B,K) int32 in the layout of object_boxes / object_box_valid (they go to
    `TrackScorer.update_raw(det_boxes=, det_box_valid=)` as they are): the filtered box where the row was measured this frame, the
    predicted box (filtered_valid 0) where its track was carried, zeros where the row has no filter; filtered_velocity (B,K,4) float64:
    vx, vy, vz in metres per frame and the unwrapped yaw; filtered_aligned (B,K,4) float64: the reading's yaw, l, w, h as the filter
    took them; filtered_gap (B,K) int32: k where the row continued a track measured k frames ago, else -1; filtered_since (B,K) int32
    (-1: no filter, 0: measured this frame, s: frames since the last measurement) and filtered_state (B,K,16) float64 (the mean x, y,
    z, yaw, l, w, h, vx, vy, vz, then P00, P01, P11, Pyaw, Psize, 0): the tracker's own buffers `box_since` / `box_state`, advanced in
    place -- valid until the next step, as `desc_prev` is under static_state."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def fresh(self):
        """A new wrapper around the same tensors: the host-side cache of an earlier step never answers for this one."""
        return StepResult(**dict(self.__dict__, _cache=None))

    def indices1(self, b=None):
        """b None: the (B,K) int32 device tensor.  b: the reference's indices1 of stream b, (1,n_b) int64, or None when there was
        nothing to associate (no previous or no current objects), as Track4D.forward returns it."""
        if b is None:
            return self._indices1
        m, n = self._sizes(b)
        if m == 0 or n == 0:
            return None
        return self._indices1[b, :n].long().unsqueeze(0)

    def _host(self):
        if self._cache is None:
            self._cache = dict(num=self.num_objects.cpu().tolist(), prev=self.num_prev.cpu().tolist(), flags=self.flags.cpu().tolist(),
                               active=self.active.cpu().tolist())
        return self._cache

    def _sizes(self, b):
        h = self._host()
        return h["prev"][b], h["num"][b]

    def check(self):
        raise_on_flags(self._host()["flags"], self.max_objects)

    def aff_mat(self, b):
        """(1, m_b, n_b) affinities of stream b (previous x current), as Track4D.forward returns them."""
        m, n = self._sizes(b)
        if m == 0 or n == 0:
            return torch.zeros(1, m, n, device=self.aff.device)
        return self.aff[b, :m, :n].unsqueeze(0)

    def objects(self, b):
        """(objects, confs) of stream b in the structure of Track4D.forward: {track id: (1,139,n_i) tensor} in association order,
        confs aligned with it (0 for a fresh track, the 0-dim affinity tensor for an inherited one)."""
        raise_on_flags(self._host()["flags"], self.max_objects, only=b, truncation=False)
        m, n = self._sizes(b)
        if n == 0:
            return dict(), []
        ids = self.object_ids[b, :n].cpu().tolist()
        idx = self._indices1[b, :n].cpu().tolist()
        conf = self.object_conf[b, :n].cpu().tolist()
        N = self.pc1.shape[2]
        pf = torch.cat((self.pc1[b] + self.flow[b], self.pc1[b], self.flow[b], self.feature1[b], self.prop[b]), dim=0)   # (139, N)
        obj = self.obj[b].long()
        order = torch.argsort(obj * N + torch.arange(N, device=obj.device))       # objects in order, points in column order inside
        sizes = torch.bincount(obj[obj >= 0], minlength=n).cpu().tolist()
        npts = sum(sizes)
        order = order[N - npts:]                                                   # (the -1 keys sort first)
        parts = torch.split(pf.index_select(1, order).unsqueeze(0), sizes, dim=2)
        objects, confs = dict(), []
        for j in range(n):
            objects[ids[j]] = parts[j]
            confs.append(0 if conf[j] == 0.0 else self.aff[b, idx[j], j])      # an inherited ID has conf >= 0.01
        return objects, confs


def raise_on_flags(flags, K, only=None, truncation=True):
    """truncation=False: dropped coasted tracks do not raise (for a caller whose output is complete without them)."""
    for b, f in enumerate(flags):
        if only is not None and b != only:
            continue
        if f & _FLAG_OVERFLOW:
            raise RuntimeError("BatchedTracker: stream %d has more than max_objects=%d objects (raise max_objects)" % (b, K))
        if f & _FLAG_NVALID:
            raise RuntimeError("BatchedTracker: stream %d has an n_valid outside [0, N]" % b)
        if truncation and f & _FLAG_TRUNCATED:
            raise RuntimeError("BatchedTracker: stream %d dropped coasted tracks: its detections and the lost tracks within max_age "
                               "exceed max_objects=%d rows (raise max_objects)" % (b, K))


def check_motion(motion, motion_beta, memory, memory_name):
    """The `motion` / `motion_beta` keywords of a tracker whose track memory is switched on by the keyword `memory_name` (value
    `memory`, None = off): raises ValueError on a combination that means nothing."""
    if motion not in (None, "flow"):
        raise ValueError("motion=%r: None (a coasted track holds its last descriptor) or \"flow\" (it moves with its track's velocity, "
                         "the mean predicted scene flow)" % (motion,))
    ok = isinstance(motion_beta, (int, float)) and not isinstance(motion_beta, bool) and 0.0 < float(motion_beta) <= 1.0
    if not ok:
        raise ValueError("motion_beta=%r: a number in (0, 1] (the weight of a frame's measured flow in its track's velocity)" % (motion_beta,))
    if motion is not None and memory is None:
        raise ValueError("motion=%r needs %s: only a track that is kept while it is lost can coast" % (motion, memory_name))
    if motion is None and float(motion_beta) != 1.0:
        raise ValueError("motion_beta=%r without motion: there is no velocity to smooth (give motion=\"flow\")" % (motion_beta,))


def check_assign(assign, min_affinity):
    """The `assign` / `min_affinity` keywords of a tracker: raises ValueError on a value or a combination that means nothing."""
    if assign not in ("sinkhorn", "optimal"):
        raise ValueError("assign=%r: \"sinkhorn\" (the reference's decision: log-Sinkhorn, then the mutual best match) or \"optimal\" "
                         "(an exact maximum-weight one-to-one assignment of the affinities at or above min_affinity)" % (assign,))
    ok = isinstance(min_affinity, (int, float)) and not isinstance(min_affinity, bool) and 0.01 <= float(min_affinity) <= 1.0
    if not ok:
        raise ValueError("min_affinity=%r: a number in [0.01, 1] (0.01 is the reference's confidence threshold)" % (min_affinity,))
    if assign == "sinkhorn" and float(min_affinity) != 0.01:
        raise ValueError("min_affinity=%r without assign=\"optimal\": the reference's decision has the one threshold 0.01" % (min_affinity,))


class BatchedTracker:
    """Tracks `streams` independent sequences in lockstep (see the module docstring)."""

    def __init__(self, net, streams, max_objects=128, iters=500, alpha=0.9, eps=1.5, threshold=0.5, train_mode=False,
                 static_state=False, graph=False, graph_warmup=2, engine=None, max_age=None, motion=None, motion_beta=1.0,
                 assign="sinkhorn", min_affinity=0.01, boxes=False, box_min_extent=0.0, box_filter=None):
        """train_mode: accept a train-mode net -- for a caller that runs the backbone itself and uses `associate` and the state only
        (track_train.SequenceTrainer); `step()` stays the eval-mode path.
        static_state: this frame's objects are always written to slot 0 of `desc` / `ids` / `count` and the previous objects read
        from slot 1; `associate` begins by copying slot 0 to slot 1 on the device (one rtk_copy_multi launch) instead of swapping
        references afterwards, and `h` is updated in place.  Same results bit for bit; nothing is rebound, so a captured graph can
        replay the step.  `StepResult.h`, `descriptors` and `desc_prev` are then valid until the next step only.
        graph (implies static_state): the first `graph_warmup` steps of a key -- the shapes and dtypes of pc1, pc2, feature1,
        feature2 and whether n_valid was given -- run eagerly (real steps: they advance the state); the next one captures the whole
        step into one hipGraph, and it and every later step copy their inputs into static buffers and replay.  reset / active /
        n_valid live in static device buffers (None: all streams active, none reset), so they never re-capture.  The outputs are the
        graph's static tensors: the next step overwrites them in place.  A new key captures again.  The captured graph keeps the
        weights it was captured with -- the backbone engine's packed images and the packed Affinity image -- as `fused.GraphPipeline`
        does: build a new tracker after changing weights.
        engine: the `fused.FusedBackbone` that `step()` runs (default: `net._fused_engine()`, looked up every step).
        max_age: None (default): the reference's rule, the tracker as it is without track memory -- no further launch or buffer, the
        four lifecycle fields of `StepResult` are None.  An integer A >= 0: a track that is not matched stays in the stream's table
        for up to A active frames (module docstring); 0 keeps the bookkeeping (hits, gap) and lets nothing coast.  A launch constant:
        a captured step replays it as it was.
        motion: None (default): a coasted track holds its last descriptor -- the tracker as it is without the keyword: the same
        launches, no further buffer, `StepResult.object_velocity` and `table_velocity` are None.  "flow" (needs max_age): every
        row carries a velocity taken from its object's mean predicted scene flow and a coasted row's centre moves by it every frame
        (module docstring; rules in include/rtk_fused.h, rtk_track_memory_motion, which replaces rtk_track_memory).
        motion_beta in (0, 1]: the weight of this frame's measured flow in an inherited track's velocity, v + beta (flow - v); a
        fresh track starts at its flow.  The default 1.0 makes the velocity the last measured mean flow: tracking quality has not
        been measured on real sequences here, so no smoothing default can be justified.  A launch constant, like max_age.
        assign: "sinkhorn" (default): the reference's decision -- `iters` log-Sinkhorn iterations with dustbin `alpha`, then the
        mutual best match (rtk_associate_batched): the tracker as it is without the keyword, the same buffers and launches;
        `StepResult.assign_total` is None.  "optimal": rtk_associate_optimal in its place (csrc/track_assign.hip; rules in
        include/rtk_fused.h) -- previous rows and current objects are matched one to one so that the affinities of the matched pairs,
        each quantised to (int)(aff * 2^28), have the largest sum any one-to-one matching of the pairs with aff >= min_affinity can
        have; `iters` and `alpha` are ignored.  The same number of launches, the same outputs: graph, static_state, max_age, motion,
        TrackerPipeline and write_results work unchanged.  `StepResult.assign_total` (B,) int64 is that sum per stream.
        min_affinity in [0.01, 1] (needs assign="optimal"): the gate below which a pair is never matched; the default 0.01 is the
        reference's confidence threshold.  Both are launch constants, like max_age.
        boxes: False (default): the tracker as it is without the keyword, the same launches and outputs; `StepResult.object_boxes`,
        `object_box_valid`, `object_box_cand` and `object_box_flags` are None.  True: one more launch after the association
        (rtk_object_boxes, ratrack_amd/boxes.py; inside the captured graph under `graph=True`) fits every object's oriented box:
        `StepResult.object_boxes` (B,K,8) float64, `boxes.object_boxes(out)`'s.  box_min_extent: the least length, width and height
        of a box, a finite number >= 0 (needs boxes=True to be anything but 0).  A launch constant, like max_age.
        box_filter: None (default): the tracker as it is without the keyword, the same launches, buffers and bits; the `filtered_*`
        fields of `StepResult` are None.  A boxes.BoxFilter with smooth = 0 and size_rule = 0 (needs boxes=True): one more launch after
        rtk_object_boxes (rtk_track_box_filter_step; inside the captured graph under `graph=True`) runs the constant-velocity Kalman
        filter of `ResultLog.filter_boxes` along every track, a frame at a time: its state lives in `box_state` (B,K,16) float64 and
        `box_since` (B,K) int32, single buffers advanced in place, and follows a track's id through the table -- through coasting
        with `max_age`, both association modes, reset and inactive streams.  A measured object's `filtered_boxes` row holds the bits
        `ResultLog.filter_boxes` gives its record with the same filter.  The association does not use the prediction.  Launch
        constants, like max_age."""
        from .boxes import check_min_extent, check_step_filter
        self.boxes, self.box_min_extent = bool(boxes), check_min_extent(box_min_extent)
        if not self.boxes and self.box_min_extent != 0.0:
            raise ValueError("box_min_extent=%r without boxes=True: there is no box to pad" % (box_min_extent,))
        self.box_filter = None if box_filter is None else check_step_filter(box_filter)
        if self.box_filter is not None and not self.boxes:
            raise ValueError("box_filter=%r without boxes=True: there is no box to filter" % (box_filter,))
        if max_age is not None and (isinstance(max_age, bool) or not isinstance(max_age, int) or max_age < 0):
            raise ValueError("max_age=%r: None (no track memory) or an integer >= 0 (frames a lost track is kept)" % (max_age,))
        check_motion(motion, motion_beta, max_age, "max_age")
        check_assign(assign, min_affinity)
        self.assign, self.min_affinity = assign, float(min_affinity)
        if net.training and not train_mode:
            raise ValueError("BatchedTracker runs the eval-mode (fused) backbone: call net.eval() first")
        kmax = max_objects_limit()
        if not 1 <= max_objects <= kmax:
            raise ValueError("max_objects=%d outside [1, %d] (the per-stream association table must fit one workgroup's LDS)"
                             % (max_objects, kmax))
        self.net, self.B, self.K = net, int(streams), int(max_objects)
        self.iters, self.alpha, self.eps, self.threshold = int(iters), float(alpha), float(eps), float(threshold)
        self.min_samples = int(net.min_obj_points)
        dev = next(net.parameters()).device
        self.dev = dev
        self.weights = pack_affinity(net.affinity).to(dev)
        B, K = self.B, self.K
        self.h = torch.zeros(5, B, 128, device=dev)
        # double-buffered: [cur] written, [1 - cur] = previous objects (static_state: cur is always 0)
        self.desc = torch.zeros(2, B, K, DESC, device=dev)
        self.ids = torch.full((2, B, K), -1, dtype=torch.int32, device=dev)
        self.count = torch.zeros(2, B, dtype=torch.int32, device=dev)
        self.counter = torch.zeros(B, dtype=torch.int32, device=dev)
        self.max_age = max_age
        self.age = self.hits = self.n_det = None
        if max_age is not None:        # the lifecycle of every row of the table, double-buffered like the table itself
            self.age = torch.zeros(2, B, K, dtype=torch.int32, device=dev)
            self.hits = torch.zeros(2, B, K, dtype=torch.int32, device=dev)
            self.n_det = torch.zeros(2, B, dtype=torch.int32, device=dev)
        self.motion, self.motion_beta = motion, float(motion_beta)
        self.vel = None
        if motion is not None:         # every row's velocity, metres per frame
            self.vel = torch.zeros(2, B, K, 3, device=dev)
        # the weight of every stream's matching (assign="optimal"): the kernel leaves an inactive stream's word as it is
        self.assign_total = torch.zeros(B, dtype=torch.int64, device=dev) if assign == "optimal" else None
        self.box_state = self.box_since = None
        if self.box_filter is not None:      # the filter of every row of the table: ONE buffer each, advanced in place by its launch
            self.box_state = torch.zeros(B, K, 16, dtype=torch.float64, device=dev)
            self.box_since = torch.full((B, K), -1, dtype=torch.int32, device=dev)
        self.cur = 0
        self._work = None
        self.last = None
        self.graph = bool(graph)
        self.static_state = bool(static_state) or self.graph
        self.engine = engine
        if self.graph:
            from .fused import _copy_inputs
            self._graphed = CapturedStep(graph_warmup, _copy_inputs)     # the inputs and n_valid: ONE rtk_copy_multi launch
            self._reset_s = torch.zeros(B, dtype=torch.uint8, device=dev)
            self._active_s = torch.ones(B, dtype=torch.uint8, device=dev)
            self._reset_default = self._active_default = True       # the static masks hold their defaults: a None needs no copy

    @property
    def captured(self):
        """Whether the last step() was the replay of a captured graph."""
        return self.graph and self._graphed.captured

    # ---- one frame --------------------------------------------------------------------------------
    def step(self, pc1, pc2, feature1, feature2, n_valid=None, reset=None, active=None):
        B, _, N = pc1.shape
        if B != self.B or pc2.shape[2] != N:
            raise ValueError("step(): expected (%d,3,N) clouds of one padded size, got %s and %s" % (self.B, tuple(pc1.shape), tuple(pc2.shape)))
        dev = self.dev
        nv = device_n_valid(n_valid, B, N, dev)
        if self.graph:
            return self._graph_step(pc1, pc2, feature1, feature2, nv, reset, active)
        reset_d, active_d = _mask(reset, B, False, dev), _mask(active, B, True, dev)
        return self._body(pc1, pc2, feature1, feature2, nv, reset_d, active_d)

    def _body(self, pc1, pc2, feature1, feature2, nv, reset_d, active_d):
        """Everything of a step that runs on the device: the h reset, the backbone, the h keep of inactive streams, `associate`."""
        h_in = reset_h(self.h, reset_d)
        eng = self.engine if self.engine is not None else self.net._fused_engine()
        with torch.no_grad():
            flow, h_out, cls, _, _, _, prop = eng.backbone(pc1, pc2, feature1, feature2, h_in, n_valid=nv)
        if self.static_state:
            self.h.copy_(keep_h(active_d, h_out, self.h))
        else:
            self.h = keep_h(active_d, h_out, self.h)
        return self.associate(pc1, feature1, flow, cls, prop, nv, reset_d, active_d)

    def _set_mask(self, static, x, default, is_default):
        """A step's reset / active into its static buffer; -> whether the buffer now holds the default."""
        if x is None:
            if not is_default:
                static.fill_(int(default))
            return True
        static.copy_(_mask(x, self.B, default, self.dev))
        return False

    def _graph_step(self, pc1, pc2, feature1, feature2, nv, reset, active):
        """Warm-up / capture / replay (captured.CapturedStep) keyed by the shapes and dtypes of the inputs and of nv (or its absence)."""
        args = [pc1, pc2, feature1, feature2, nv]
        self._reset_default = self._set_mask(self._reset_s, reset, False, self._reset_default)
        self._active_default = self._set_mask(self._active_s, active, True, self._active_default)
        out = self._graphed(signature(args), args, lambda a: self._body(*a, self._reset_s, self._active_s), self._capture_step)
        self.last = out = out.fresh()
        return out

    def _capture_step(self, static):
        self._workspace(static[0].shape[2])                # the DBSCAN workspace of a large N: allocated before the capture
        if self.engine is None:
            self.net._fused_engine()                       # (folding and packing synchronise: not inside the capture either)
        torch.cuda.synchronize()
        g, out = capture_graph(lambda: self._body(*static, self._reset_s, self._active_s))      # records the launches, executes nothing
        return out, g.replay

    def _workspace(self, N):
        """(address, bytes) of the workspace in which streams whose DBSCAN tables exceed the LDS cluster; (None, 0) for a small N."""
        need = N * DBSCAN_POINT_BYTES
        if need <= DBSCAN_LDS_BYTES:
            return None, 0
        if self._work is None or self._work.numel() < self.B * need:
            self._work = torch.empty(self.B * need, dtype=torch.uint8, device=self.dev)
        return self._work.data_ptr(), self._work.numel()

    def associate(self, pc1, feature1, flow, cls, prop, n_valid, reset, active):
        """The post-backbone half of step(): four launches, the state swap (static_state: the state advance first, five launches);
        with max_age one more, rtk_track_memory (with motion: rtk_track_memory_motion in its place); with boxes rtk_object_boxes and with
        box_filter rtk_track_box_filter_step behind it; no host synchronisation.  reset / active (B,) uint8 and n_valid (2,B) int32 (or
        None) are device tensors."""
        B, K = self.B, self.K
        N = pc1.shape[2]
        dev = self.dev
        st = stream()
        if self.static_state:
            # last frame's objects (slot 0) become the previous objects (slot 1).  Here and not at the end of the last step: its
            # caller may still have read desc_prev (the training backward does).  An inactive stream's kernels carried slot 1 over
            # into slot 0, so the copy leaves it as it was; a reset stream's previous objects are ignored.
            from .fused import copy_multi
            cur, prev = 0, 1
            state = [self.desc, self.ids, self.count] + ([] if self.max_age is None else [self.age, self.hits, self.n_det])
            state += [] if self.vel is None else [self.vel]                # seven of the launch's eight jobs
            copy_multi([(t[1], t[0]) for t in state])
        else:
            cur, prev = self.cur, 1 - self.cur
        i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
        labels, obj, num, flags = i32(B, N), i32(B, N), i32(B), i32(B)
        fr = TrackFrame(B, N, _view(pc1), _view(flow), _view(feature1), _view(prop), _view(cls),
                        None if n_valid is None else n_valid.data_ptr(), active.data_ptr())
        work, work_bytes = self._workspace(N)      # a stream whose tables exceed the LDS clusters in its slice of this workspace
        _lib.call("rtk_dbscan_batched", ctypes.addressof(fr), self.threshold, self.eps, self.min_samples, K, labels.data_ptr(),
                  obj.data_ptr(), num.data_ptr(), flags.data_ptr(), work, work_bytes, st)
        desc_prev, desc = self.desc[prev], self.desc[cur]
        _lib.call("rtk_object_descriptors", ctypes.addressof(fr), K, obj.data_ptr(), num.data_ptr(), self.count[prev].data_ptr(),
                  desc_prev.data_ptr(), desc.data_ptr(), st)
        aff = torch.empty(B, K, K, device=dev)
        _lib.call("rtk_affinity_pairs", B, K, self.weights.data_ptr(), desc_prev.data_ptr(), self.count[prev].data_ptr(), reset.data_ptr(),
                  desc.data_ptr(), num.data_ptr(), aff.data_ptr(), st)
        object_ids, object_conf, indices1, num_prev, point_track_id = i32(B, K), torch.empty(B, K, device=dev), i32(B, K), i32(B), i32(B, N)
        assign_total = self.assign_total
        if self.assign == "optimal":
            _lib.call("rtk_associate_optimal", B, N, K, active.data_ptr(), reset.data_ptr(), aff.data_ptr(), num.data_ptr(), obj.data_ptr(),
                      self.ids[prev].data_ptr(), self.count[prev].data_ptr(), self.min_affinity, self.counter.data_ptr(),
                      self.ids[cur].data_ptr(), self.count[cur].data_ptr(), object_ids.data_ptr(), object_conf.data_ptr(),
                      indices1.data_ptr(), num_prev.data_ptr(), point_track_id.data_ptr(), assign_total.data_ptr(), st)
        else:
            _lib.call("rtk_associate_batched", B, N, K, active.data_ptr(), reset.data_ptr(), aff.data_ptr(), num.data_ptr(), obj.data_ptr(),
                      self.ids[prev].data_ptr(), self.count[prev].data_ptr(), self.alpha, self.iters, self.counter.data_ptr(),
                      self.ids[cur].data_ptr(), self.count[cur].data_ptr(), object_ids.data_ptr(), object_conf.data_ptr(), indices1.data_ptr(),
                      num_prev.data_ptr(), point_track_id.data_ptr(), None, st)
        memory = dict(object_hits=None, object_gap=None, num_coasted=None, prev_age=None, table_ids=None, table_count=None,
                      object_velocity=None, table_velocity=None)
        if self.motion is not None:
            # the next table as below, its rows' velocities, and the survivors' centres moved on by one frame
            memory.update(object_hits=i32(B, K), object_gap=i32(B, K), num_coasted=i32(B), prev_age=self.age[prev],
                          table_ids=self.ids[cur], table_count=self.count[cur], object_velocity=torch.empty(B, K, 3, device=dev),
                          table_velocity=self.vel[cur])
            _lib.call("rtk_track_memory_motion", B, K, self.max_age, self.motion_beta, active.data_ptr(), reset.data_ptr(), num.data_ptr(),
                      indices1.data_ptr(), object_conf.data_ptr(), self.ids[prev].data_ptr(), self.age[prev].data_ptr(),
                      self.hits[prev].data_ptr(), self.n_det[prev].data_ptr(), self.count[prev].data_ptr(), desc_prev.data_ptr(),
                      self.vel[prev].data_ptr(), self.ids[cur].data_ptr(), self.age[cur].data_ptr(), self.hits[cur].data_ptr(),
                      self.n_det[cur].data_ptr(), self.count[cur].data_ptr(), desc.data_ptr(), self.vel[cur].data_ptr(), flags.data_ptr(),
                      memory["object_hits"].data_ptr(), memory["object_gap"].data_ptr(), memory["num_coasted"].data_ptr(),
                      memory["object_velocity"].data_ptr(), st)
        elif self.max_age is not None:
            # the next table: this frame's detections, then the unmatched previous rows that are still young enough
            memory.update(object_hits=i32(B, K), object_gap=i32(B, K), num_coasted=i32(B), prev_age=self.age[prev],
                          table_ids=self.ids[cur], table_count=self.count[cur])
            _lib.call("rtk_track_memory",B, K, self.max_age, active.data_ptr(), reset.data_ptr(), num.data_ptr(), indices1.data_ptr(),
                      object_conf.data_ptr(), self.ids[prev].data_ptr(), self.age[prev].data_ptr(), self.hits[prev].data_ptr(),
                      self.n_det[prev].data_ptr(), self.count[prev].data_ptr(), desc_prev.data_ptr(), self.ids[cur].data_ptr(),
                      self.age[cur].data_ptr(), self.hits[cur].data_ptr(), self.n_det[cur].data_ptr(), self.count[cur].data_ptr(),
                      desc.data_ptr(), flags.data_ptr(), memory["object_hits"].data_ptr(), memory["object_gap"].data_ptr(),
                      memory["num_coasted"].data_ptr(), st)
        fitted = dict(object_boxes=None, object_box_valid=None, object_box_cand=None, object_box_flags=None)
        if self.boxes:
            from .boxes import object_boxes_raw
            bx = object_boxes_raw(pc1, obj, num, K, active=active, min_extent=self.box_min_extent)
            fitted.update(object_boxes=bx.box, object_box_valid=bx.valid, object_box_cand=bx.cand, object_box_flags=bx.flags)
        fitted.update(filtered_boxes=None, filtered_valid=None, filtered_velocity=None, filtered_aligned=None, filtered_gap=None,
                      filtered_since=None, filtered_state=None)
        if self.box_filter is not None:
            from .boxes import filter_step_raw
            fb = filter_step_raw(self.ids[prev], self.count[prev], self.ids[cur], self.count[cur], num, bx.box, bx.valid, self.box_state,
                                 self.box_since, filter=self.box_filter, active=active, reset=reset)
            fitted.update(filtered_boxes=fb.box, filtered_valid=fb.valid, filtered_velocity=fb.vel, filtered_aligned=fb.aligned,
                          filtered_gap=fb.gap, filtered_since=self.box_since, filtered_state=self.box_state)
        if not self.static_state:
            self.cur = prev                # this frame's objects are the next frame's previous objects: a swap, not a copy
        out = StepResult(flow=flow, cls=cls, h=self.h, point_track_id=point_track_id, num_objects=num, object_ids=object_ids,
                         object_conf=object_conf, _indices1=indices1, aff=aff, num_prev=num_prev, flags=flags, labels=labels, obj=obj,
                         descriptors=desc, desc_prev=desc_prev, active=active, pc1=pc1, feature1=feature1, prop=prop, max_objects=K, _cache=None,
                         assign_total=assign_total, **memory, **fitted)
        self.last = out
        return out

    def check(self, out=None):
        """Raises RuntimeError naming the stream if the last step (or `out`) overflowed max_objects, had a bad n_valid or (track
        memory) dropped coasted tracks that did not fit max_objects rows."""
        out = out if out is not None else self.last
        if out is not None:
            out.check()

    # ---- result files ------------------------------------------------------------------------------
    def write_results(self, root, seqs, indices, out, min_hits=1):
        """One result file per active stream, <root>/<seqs[b]>/<indices[b]:05d>.txt, byte-identical to
        vod_io.write_track_results(root, seqs[b], indices[b], *out.objects(b)); one device->host copy for the whole batch.
        min_hits (track memory only): objects whose track has been detected in fewer frames (`object_hits` < min_hits) are left out
        of the file -- confirmed tracks only.  Returns the paths written."""
        if isinstance(min_hits, bool) or not isinstance(min_hits, int) or min_hits < 1:
            raise ValueError("min_hits=%r: an integer >= 1" % (min_hits,))
        if min_hits > 1 and out.object_hits is None:
            raise ValueError("min_hits=%d needs the hit counts of track memory: build the tracker with max_age (0 or more)" % min_hits)
        B, K = self.B, self.K
        N = out.pc1.shape[2]
        pc1 = out.pc1.float()
        flat = [out.num_objects, out.flags, out.active.to(torch.int32), out.object_ids.reshape(-1), out.object_conf.reshape(-1).view(torch.int32),
                out.obj.reshape(-1), pc1.contiguous().reshape(-1).view(torch.int32)]
        if min_hits > 1:
            flat.append(out.object_hits.reshape(-1))
        host = torch.cat([t.reshape(-1) for t in flat]).cpu()
        o = 0

        def take(count):
            nonlocal o
            r = host[o:o + count]
            o += count
            return r
        num, flags, act = take(B).tolist(), take(B).tolist(), take(B).tolist()
        ids, conf = take(B * K).view(B, K), take(B * K).view(torch.float32).view(B, K)
        obj, xyz = take(B * N).view(B, N), take(B * 3 * N).view(torch.float32).view(B, 3, N)
        hits = take(B * K).view(B, K) if min_hits > 1 else None
        raise_on_flags([f if a else 0 for f, a in zip(flags, act)], K, truncation=False)
        paths = []
        for b in range(B):
            if not act[b]:
                continue
            d = os.path.join(root, str(seqs[b]))
            os.makedirs(d, exist_ok=True)
            path = os.path.join(d, str(int(indices[b])).zfill(5) + ".txt")
            ob = obj[b].tolist()
            members = [[] for _ in range(num[b])]
            for p, k in enumerate(ob):
                if k >= 0:
                    members[k].append(p)
            xb = xyz[b].numpy()
            with open(path, "w+") as f:
                for j in range(num[b]):
                    if hits is not None and int(hits[b, j]) < min_hits:
                        continue
                    parts = ["NA", "1", "-1", "-1", str(float(conf[b, j])), str(int(ids[b, j]))]
                    for p in members[j]:
                        parts += [str(float(xb[0, p])), str(float(xb[1, p])), str(float(xb[2, p]))]
                    f.write(" ".join(parts) + "\n")
            paths.append(path)
        return paths


class TrackerPipeline:
    """`groups` independent groups of `streams` sequences each, every group a `BatchedTracker(graph=True)` on its own HIP stream:

        pipe = TrackerPipeline(net, groups=2, streams=32)
        out0 = pipe.submit(0, pc1, pc2, feature1, feature2, n_valid=None, reset=None, active=None)
        out1 = pipe.submit(1, ...)
        pipe.drain()

    Three of the four association launches run one workgroup per stream and leave most of the device idle; replays of different
    groups overlap them (and the backbones' latency-bound phases, as `fused.GraphPipeline` does for the backbone alone).  State is
    sequential within a group: concurrency comes from different groups only.  Every group has its own copy of the backbone engine
    (packed weights shared, per-engine state separate); beyond two groups the engines run their geometry kernels on their own
    stream and the cost volume on a share of the CUs, as in `GraphPipeline`.  The weights are those at construction.
    Every other keyword of `BatchedTracker` (max_age, motion, assign, boxes, box_filter, ...) is forwarded to every group's tracker.
    `submit` returns group g's `StepResult`, enqueued on group g's stream: its tensors and host accessors (`objects`, `aff_mat`,
    `indices1(b)`, `check`, `write_results`) are valid after `drain()` or under `pipe.streams[g]`, and until group g's next submit.
    Inputs are read on group g's stream after everything the current stream held at the time of the submit."""

    MAX_GROUPS = 4

    def __init__(self, net, groups, streams, max_objects=128, **tracker_kw):
        groups = int(groups)
        if not 1 <= groups <= self.MAX_GROUPS:
            raise ValueError("TrackerPipeline: groups=%d outside [1, %d]: one group per hardware queue -- a fifth stream shares one of "
                             "the four queues, the arrangement that cost 20-30 %% whenever it was measured (DESIGN.md: forked "
                             "geometry streams beyond depth 2, forked MSG scales 102.6 -> 74-83 k pairs/s)" % (groups, self.MAX_GROUPS))
        for k in ("graph", "static_state", "engine"):
            if k in tracker_kw:
                raise ValueError("TrackerPipeline sets %s itself" % k)
        base = net._fused_engine()
        self.engines = []
        for _ in range(groups):
            e = base.clone()                # packed weights shared, per-engine state its own
            if groups > 2:
                e.use_side_stream, e.cv_shared = False, True
            self.engines.append(e)
        self.trackers = [BatchedTracker(net, streams, max_objects=max_objects, graph=True, engine=e, **tracker_kw) for e in self.engines]
        self.streams = [torch.cuda.Stream(device=self.trackers[0].dev) for _ in range(groups)]
        self.groups = groups

    def submit(self, g, pc1, pc2, feature1, feature2, n_valid=None, reset=None, active=None):
        """Group g's next step on group g's stream -> its StepResult (see the class docstring for when it may be read)."""
        s = self.streams[g]
        s.wait_stream(torch.cuda.current_stream())
        for t in (pc1, pc2, feature1, feature2, n_valid, reset, active):
            if torch.is_tensor(t) and t.is_cuda:
                t.record_stream(s)          # the caller may drop its inputs before group g's stream has read them
        with torch.cuda.stream(s):
            return self.trackers[g].step(pc1, pc2, feature1, feature2, n_valid=n_valid, reset=reset, active=active)

    def drain(self):
        """Join every group's stream into the current stream."""
        cur = torch.cuda.current_stream()
        for s in self.streams:
            cur.wait_stream(s)
