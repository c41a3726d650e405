"""The tracking term of the loss for B sequences in lockstep (include/rtk_train.h, csrc/track_train.hip).

    trainer = SequenceTrainer(net, streams=B, max_objects=128, max_boxes=32)
    for every frame:
        gt   = gt_device.ground_truth(pc1, pc2, boxes, n_valid=nv)                  # gt_warp, gt_cls
        gobj = track_score.gt_objects(pc1, boxes, types, n_valid=nv, min_obj_points=net.min_obj_points)
        items, h, out, match = trainer.step(pc1, pc2, f1, f2, gt.gt_warp, gt.gt_cls, gobj, h, n_valid=nv, reset=is_new_seq, active=has_frame)

`Trainer.step` optimises 0.5 L_sf + L_seg; the reference's third term, 0.5 affinity_loss (losses/loss.py:22,48-72), is the only thing
that trains the Affinity MLP.  Here it is `affinity_term`: per stream the binary cross entropy of the live block of `StepResult.aff`
against `MatchResult.aff_target`, with a backward in HIP through the MLP (input and weight gradients), the descriptor differences and
the descriptors down to `flow` (through the mean) and `prop_features` (through the max).  The previous frame's objects are detached,
as in the reference (main_utils.py:158-160).  No host synchronisation, a fixed number of launches, no floating-point atomics: the
term is reproducible bit for bit.

Re-acquisition.  With `SequenceTrainer(..., reacquire=A)` the trainer's tracker keeps lost tracks for up to A frames
(`BatchedTracker(max_age=A)`) and its scorer keeps a record of the whole table (`TrackScorer(track_memory=True)`): `out.num_prev`
counts the coasted rows too, `aff_target` has a row for each, and the term trains the MLP to give a coasted track the detection
of the object it last was.  The training kernels need no change: they take m_b = `out.num_prev` rows, and a taller table is just
more live pairs.  `motion="flow"` (with `reacquire`) is forwarded to the tracker: the coasted rows then move with their tracks'
velocities.

A batch with more live pairs than `max_pairs` (the workspace holds 8 KiB per pair) leaves the streams beyond the cap out of the term
and flags them; `check()` raises naming them -- nothing is truncated silently.
"""
import ctypes

import torch

from . import _lib, tracker as T
from .abi import TrackFrame, ptr as _ptr, stream as _stream, view as _view
from .track_score import GtObjects, TrackScorer
from .train import Trainer

DIMS = ((141, 564), (564, 282), (282, 70), (70, 35), (35, 1))
WEIGHTS = sum(i * o + o for i, o in DIMS)            # RTK_AFFINITY_WEIGHTS
WEIGHTS_BWD = sum(i * o for i, o in DIMS)            # RTK_AFFINITY_WEIGHTS_BWD
ROW = 2048                                           # RTK_AFF_TRAIN_ROW: floats of workspace per live pair (8192 bytes)
CHUNK = 512                                          # RTK_AFF_TRAIN_CHUNK
MAX_PAIRS_LIMIT = 1 << 20
DEFAULT_MAX_PAIRS = 1 << 15                          # 256 MiB of rows


def unpack_affinity_grad(packed):
    """The inverse of `tracker.pack_affinity`'s layout: a packed image (or its gradient, as rtk_affinity_wgrad writes it) -> the ten
    tensors in `named_parameters` order, weight (Cout, Cin) then bias (Cout) of each of the five Linear layers.  Views of `packed`."""
    packed = packed.reshape(-1)
    if packed.numel() != WEIGHTS:
        raise ValueError("a packed Affinity image has %d floats, got %d" % (WEIGHTS, packed.numel()))
    out, o = [], 0
    for cin, cout in DIMS:
        out.append(packed[o:o + cin * cout].view(cin, cout).t())
        o += cin * cout
        out.append(packed[o:o + cout])
        o += cout
    return out


def workspace_floats(max_pairs):
    """Floats of workspace rtk_affinity_train / rtk_affinity_wgrad need: the pairs' rows and the chunks' partial weight images."""
    return max_pairs * ROW + -(-max_pairs // CHUNK) * WEIGHTS


def default_max_pairs(B, K):
    return min(B * K * K, DEFAULT_MAX_PAIRS)


_WORKSPACE = {}


def workspace(dev, max_pairs):
    """The cached device workspace of rtk_affinity_train / rtk_affinity_wgrad (layout: include/rtk_train.h), grown on demand."""
    ws = _WORKSPACE.get(dev)
    if ws is None or ws.numel() < workspace_floats(max_pairs):
        ws = _WORKSPACE[dev] = torch.empty(workspace_floats(max_pairs), dtype=torch.float32, device=dev)
    return ws


def _linears(affinity):
    lins = [m for m in affinity.affinity if isinstance(m, torch.nn.Linear)]
    if tuple((l.in_features, l.out_features) for l in lins) != DIMS:
        raise ValueError("the tracking term is built for the 141-564-282-70-35-1 Affinity MLP")
    return lins


def pack_affinity_bwd(affinity):
    """The second weight image of rtk_affinity_train: the five layers' weights as nn.Linear keeps them, (Cout, Cin), no biases."""
    return torch.cat([l.weight.detach().float().reshape(-1) for l in _linears(affinity)])


def affinity_loss_only(aff, aff_target, aff_defined, prev_count, num_objects, reset=None, active=None, max_pairs=None):
    """rtk_affinity_train without a scale: -> (loss (B,), flags (B,) int32), the loss read off `aff` (B,K,K).  Two launches."""
    B, K = aff.shape[0], aff.shape[1]
    max_pairs = default_max_pairs(B, K) if max_pairs is None else int(max_pairs)
    dev = aff.device
    loss = torch.empty(B, dtype=torch.float32, device=dev)
    pair_offset = torch.empty(B + 1, dtype=torch.int32, device=dev)
    flags = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.call("rtk_affinity_train", B, K, None, None, None, prev_count.data_ptr(), _ptr(reset), _ptr(active), None, num_objects.data_ptr(),
              aff.data_ptr(), aff_target.data_ptr(), aff_defined.data_ptr(), None, max_pairs, loss.data_ptr(), None,
              pair_offset.data_ptr(), flags.data_ptr(), None, 0, _stream())
    return loss, flags


def affinity_backward(weights, weights_bwd, desc_prev, prev_count, desc, num_objects, aff_target, aff_defined, scale, reset=None,
                      active=None, max_pairs=None):
    """rtk_affinity_train with a scale, then rtk_affinity_wgrad: -> (loss (B,), d_desc (B,K,141), d_weights (packed layout),
    flags (B,) int32).  weights / weights_bwd: `tracker.pack_affinity` / `pack_affinity_bwd`; desc_prev, desc (B,K,141) contiguous;
    prev_count, num_objects (B,) int32; aff_target (B,K,K); aff_defined, reset, active (B,) uint8; scale (B,) fp32.  Five launches."""
    B, K = desc.shape[0], desc.shape[1]
    max_pairs = default_max_pairs(B, K) if max_pairs is None else int(max_pairs)
    dev = desc.device
    ws = workspace(dev, max_pairs)
    loss = torch.empty(B, dtype=torch.float32, device=dev)
    pair_offset = torch.empty(B + 1, dtype=torch.int32, device=dev)
    flags = torch.empty(B, dtype=torch.int32, device=dev)
    d_desc = torch.empty(B, K, T.DESC, dtype=torch.float32, device=dev)
    d_weights = torch.empty(WEIGHTS, dtype=torch.float32, device=dev)
    _lib.call("rtk_affinity_train", B, K, weights.data_ptr(), weights_bwd.data_ptr(), desc_prev.data_ptr(), prev_count.data_ptr(),
              _ptr(reset), _ptr(active), desc.data_ptr(), num_objects.data_ptr(), None, aff_target.data_ptr(), aff_defined.data_ptr(),
              scale.data_ptr(), max_pairs, loss.data_ptr(), d_desc.data_ptr(), pair_offset.data_ptr(), flags.data_ptr(), ws.data_ptr(),
              ws.numel(), _stream())
    _lib.call("rtk_affinity_wgrad", B, max_pairs, pair_offset.data_ptr(), ws.data_ptr(), ws.numel(), d_weights.data_ptr(), _stream())
    return loss, d_desc, d_weights, flags


def descriptors_backward(out, d_desc):
    """rtk_object_descriptors_bwd on the frame of a `tracker.StepResult`: d_desc (B,K,141) -> (d_flow (B,3,N), d_prop (B,128,N)),
    contiguous.  Two launches.  (The padding columns carry obj = -1: no n_valid is needed.)"""
    B, K = out.aff.shape[0], out.aff.shape[1]
    N = out.obj.shape[1]
    dev = d_desc.device
    d_flow = torch.empty(B, 3, N, dtype=torch.float32, device=dev)
    d_prop = torch.empty(B, 128, N, dtype=torch.float32, device=dev)
    arg_ws = torch.empty(B * K * 129, dtype=torch.int32, device=dev)
    fr = TrackFrame(B, N, _view(out.pc1), _view(out.flow), _view(out.feature1), _view(out.prop), _view(out.cls), None, out.active.data_ptr())
    _lib.call("rtk_object_descriptors_bwd", ctypes.addressof(fr), K, out.obj.data_ptr(), out.num_objects.data_ptr(), d_desc.data_ptr(),
              d_flow.data_ptr(), d_prop.data_ptr(), arg_ws.data_ptr(), _stream())
    return d_flow, d_prop


class _AffinityTerm(torch.autograd.Function):
    # num_prev is the tracker's m_b -- 0 on a reset or inactive stream -- so it stands in for (prev_count, reset) here

    @staticmethod
    def forward(ctx, flow, prop, cfg, *params):
        out, match, max_pairs = cfg
        loss, flags = affinity_loss_only(out.aff, match.aff_target, match.aff_defined, out.num_prev, out.num_objects, None, out.active,
                                         max_pairs)
        out.pair_flags, out.max_pairs = flags, max_pairs
        ctx.cfg, ctx.params = cfg, params
        return loss

    @staticmethod
    def backward(ctx, g):
        out, match, max_pairs = ctx.cfg
        params = ctx.params
        with torch.no_grad():
            weights = torch.cat([t for w, b in zip(params[0::2], params[1::2]) for t in (w.float().t().reshape(-1), b.float().reshape(-1))])
            weights_bwd = torch.cat([w.float().reshape(-1) for w in params[0::2]])
        _, d_desc, d_weights, _ = affinity_backward(weights, weights_bwd, out.desc_prev, out.num_prev, out.descriptors, out.num_objects,
                                                    match.aff_target, match.aff_defined, g.contiguous().float(), None, out.active, max_pairs)
        d_flow = d_prop = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            d_flow, d_prop = descriptors_backward(out, d_desc)
        grads = [t.contiguous().view_as(p) for t, p in zip(unpack_affinity_grad(d_weights), params)]
        return (d_flow if ctx.needs_input_grad[0] else None, d_prop if ctx.needs_input_grad[1] else None, None) + tuple(grads)


def affinity_term(affinity, out, match, flow, prop, max_pairs=None):
    """loss (B,): per stream the mean binary cross entropy of the live block of `out.aff` against `match.aff_target`; 0 for a stream
    without live pairs, with `aff_defined == 0`, reset or inactive.  out: the `tracker.StepResult` of `associate` on the DETACHED
    `flow` / `prop` (B,3,N) / (B,128,N) handed in here with their graph; match: the `track_score.MatchResult` of the same frame.
    Backward: gradients of `flow`, `prop` (contiguous) and the ten Affinity parameters (always tensors: zeros when no stream is
    defined): three entry points, seven launches, the weight-gradient launch pair once.  Under torch.no_grad() only the value is formed (two launches).
    `check(out)` raises if streams fell beyond `max_pairs` (default: min(B K K, 32768))."""
    B, K = out.aff.shape[0], out.aff.shape[1]
    max_pairs = default_max_pairs(B, K) if max_pairs is None else int(max_pairs)
    if not 1 <= max_pairs <= MAX_PAIRS_LIMIT:
        raise ValueError("max_pairs=%d outside [1, %d]" % (max_pairs, MAX_PAIRS_LIMIT))
    params = [p for l in _linears(affinity) for p in (l.weight, l.bias)]
    return _AffinityTerm.apply(flow, prop, (out, match, max_pairs), *params)


def check(out):
    """Synchronises.  Raises RuntimeError naming the streams whose pairs fell beyond max_pairs in the last `affinity_term` on `out`."""
    flags = getattr(out, "pair_flags", None)
    if flags is None:
        return
    bad = [b for b, f in enumerate(flags.cpu().tolist()) if f]
    if bad:
        raise RuntimeError("affinity_term: the live pairs of stream%s %s fell beyond max_pairs=%d and took no part in the tracking term "
                           "(raise max_pairs)" % ("s" if len(bad) > 1 else "", ", ".join(map(str, bad)), out.max_pairs))


class _TrainTracker(T.BatchedTracker):
    """BatchedTracker's state and `associate` behind a train-mode backbone that the trainer runs itself."""

    def __init__(self, net, streams, max_objects, static_state=False, max_age=None, motion=None, motion_beta=1.0):
        super().__init__(net, streams, max_objects=max_objects, train_mode=True, static_state=static_state, max_age=max_age,
                         motion=motion, motion_beta=motion_beta)

    def step(self, *a, **k):
        raise RuntimeError("SequenceTrainer runs the train-mode backbone itself: use SequenceTrainer.step")


class SequenceTrainer(Trainer):
    """`Trainer` with the tracking term: B sequences trained in lockstep, total = 0.5 L_sf + L_seg + 0.5 L_trk with L_trk the mean over
    the B streams of `affinity_term` (undefined streams count 0, the batch convention of `loss.backbone_loss`).  Owns the tracker
    state (`.tracker`) and a `TrackScorer` (`.scorer`).
    graph=True (with `graph_warmup`, `split_graph`, ... of `Trainer`): after the warm-up steps of a key the whole step -- the h reset,
    the train-mode backbone, the pack of the live Affinity weights, `associate`, `scorer.update`, both losses, the backward, the
    gradient pack, the h keep of inactive streams and (one process) Adam -- is one hipGraph that every later step replays.  The tracker
    then keeps its state in place (`BatchedTracker(static_state=True)`); it and the scorer's state are advanced by the replay.  reset
    and active always live in static device buffers, so they never re-capture; h=None / a tensor, n_valid=None / a tensor, pretrain
    and the shapes do.  `items`, `h`, `out` and `match` are the graph's static outputs, as with `Trainer(graph=True)`: the next step
    overwrites them in place (`out` is a new wrapper every step, so its host-side accessors never answer from an earlier step).
    reacquire: None (default): the trainer's tracker follows the reference's rule (previous objects = the last active frame's
    detections), the object and the launches as they are without it.  An integer A >= 0: the tracker is built with max_age=A and
    the scorer with track_memory=True, so that the term also covers the coasted rows of the previous table (module docstring);
    the tracker's lifecycle state and the scorer's record live at fixed addresses, and graph=True replays advance them.
    `max_age` other than None is refused: a plain scorer's `aff_target` is defined against the previous frame's detections only
    and has no target for a coasted row -- `reacquire` is the keyword that changes the scorer with the tracker.
    motion, motion_beta (need reacquire): forwarded to the tracker (`BatchedTracker(motion="flow")`): the coasted rows of
    `out.desc_prev` then hold centres moved on by their tracks' velocities, so the MLP is trained on the difference it will see when
    it tracks with the same setting.  Nothing else changes: `out.desc_prev` stays detached, the training kernels take whatever rows
    the table holds, and the scorer's record is keyed by track id."""

    N_GOBJ = ("slot", "label_id", "size", "count", "members", "centre", "n_valid")

    def __init__(self, model, streams, max_objects=128, max_boxes=32, max_gt_tracks=1024, max_pairs=None, max_age=None, reacquire=None,
                 motion=None, motion_beta=1.0, **trainer_kw):
        if max_age is not None:
            raise ValueError("SequenceTrainer: max_age=%r: the tracking term trains against the previous frame's detections only "
                             "(track_score's aff_target has no target for a coasted track); to train with track memory give "
                             "reacquire=%r, which builds the tracker with that max_age and a scorer that has such a target"
                             % (max_age, max_age))
        if reacquire is not None and (isinstance(reacquire, bool) or not isinstance(reacquire, int) or reacquire < 0):
            raise ValueError("reacquire=%r: None (no track memory) or an integer >= 0 (frames a lost track is kept)" % (reacquire,))
        T.check_motion(motion, motion_beta, reacquire, "reacquire")
        if trainer_kw.get("graph") and next(model.parameters()).device.type != "cuda":
            raise ValueError("SequenceTrainer: graph=True captures the sequence step in a hipGraph and needs the model on the GPU")
        super().__init__(model, **trainer_kw)
        if self._dev.type != "cuda":
            raise ValueError("SequenceTrainer needs a model on the GPU (the tracker, the scorer and the tracking term are HIP only)")
        model.train()
        self.reacquire = reacquire
        if reacquire is None:
            self.tracker = _TrainTracker(model, streams, max_objects, static_state=bool(self.graph))
            self.scorer = TrackScorer(streams=streams, max_objects=max_objects, max_boxes=max_boxes, max_gt_tracks=max_gt_tracks, device=self._dev)
        else:
            self.tracker = _TrainTracker(model, streams, max_objects, static_state=bool(self.graph), max_age=reacquire, motion=motion,
                                         motion_beta=motion_beta)
            self.scorer = TrackScorer(streams=streams, max_objects=max_objects, max_boxes=max_boxes, max_gt_tracks=max_gt_tracks,
                                      device=self._dev, track_memory=True)
        self.max_pairs = default_max_pairs(int(streams), int(max_objects)) if max_pairs is None else int(max_pairs)
        self.last = None
        self._default_masks = None

    def _forward_backward_impl(self, pc1, pc2, feature1, feature2, gt_warp, gt_cls, gobj, h, n_valid, pretrain, reset, active):
        from . import train_ops
        self.opt.zero_grad(set_to_none=True)
        train_ops.arena_begin_step(self._dev)
        flow, h_out, cls, _, _, _, prop = self.model.backbone(pc1, pc2, feature1, feature2, h, n_valid=n_valid)
        trk = self.tracker
        trk.weights = T.pack_affinity(self.model.affinity)              # the live parameters, every step
        out = trk.associate(pc1, feature1, flow.detach(), cls.detach(), prop.detach(), n_valid, reset, active)
        match = self.scorer.update(out, gobj, reset=reset, active=active)
        total, items = train_ops.backbone_loss(pc1, flow, cls, gt_warp, gt_cls, pretrain=pretrain,
                                               n_valid=None if n_valid is None else n_valid[0].contiguous())
        B = pc1.shape[0]
        if pretrain:                # weight 0: the value alone, no backward launches
            with torch.no_grad():
                term = affinity_term(self.model.affinity, out, match, flow, prop, self.max_pairs).sum() / B
        else:
            term = affinity_term(self.model.affinity, out, match, flow, prop, self.max_pairs).sum() / B
            total = total + 0.5 * term
        items = dict(items, Loss=total, TrackingLoss=term)
        self.opt.zero_grad(set_to_none=True)
        train_ops.begin_deferred_wgrads()
        try:
            total.backward(gradient=self._one)
        except BaseException:
            train_ops.drop_deferred_wgrads()
            raise
        train_ops.flush_deferred_wgrads()
        train_ops.arena_end_step(self._dev)
        self.reducer.pack()
        self.last = out
        return {k: v.detach() for k, v in items.items()}, h_out.detach(), out, match

    def step(self, pc1, pc2, feature1, feature2, gt_warp, gt_cls, gobj, h=None, pretrain=False, n_valid=None, reset=None, active=None):
        """One optimisation step on B streams' current frames.  gobj: `track_score.gt_objects` of the same frame.  reset / active (B,):
        as for `BatchedTracker.step` and `TrackScorer.update` -- a reset stream's h goes to zero and its previous objects are dropped
        (no tracking term for it this frame); an inactive stream keeps h, tracker and scorer state and adds nothing to the term.
        -> (items, h, out, match): the loss items (`TrackingLoss` the term, `Loss` including 0.5 of it unless pretrain), the GRU
        state, the step's `StepResult` and `MatchResult`.  No host synchronisation; `check()` afterwards."""
        self.model.train()
        B, N = pc1.shape[0], pc1.shape[2]
        if B != self.tracker.B:
            raise ValueError("step(): expected %d streams, got %s" % (self.tracker.B, tuple(pc1.shape)))
        nv = T.device_n_valid(n_valid, B, N, self._dev)
        if self.graph and self._default_masks is None:       # built once: the captured step only ever copies from them
            self._default_masks = (T._mask(None, B, False, self._dev), T._mask(None, B, True, self._dev))
        dm = self._default_masks
        reset_d = dm[0] if (dm is not None and reset is None) else T._mask(reset, B, False, self._dev)
        active_d = dm[1] if (dm is not None and active is None) else T._mask(active, B, True, self._dev)
        if not self.graph:
            h_in = h
            if h is not None and reset is not None:
                h_in = T.reset_h(h, reset_d)
            items, h_out, out, match = self._forward_backward(pc1, pc2, feature1, feature2, gt_warp, gt_cls, gobj, h_in, nv, pretrain,
                                                               reset_d, active_d)
            if active is not None:
                h_out = T.keep_h(active_d, h_out, torch.zeros_like(h_out) if h_in is None else h_in)
            self.reducer.all_reduce()
            self._optimize()
            return items, h_out, out, match
        self._gobj_meta = (gobj.max_boxes, gobj.points)
        flat = [pc1, pc2, feature1, feature2, gt_warp, gt_cls, h, nv] + [getattr(gobj, k) for k in self.N_GOBJ] + [reset_d, active_d]
        return self._run(flat, pretrain)

    # ---- the captured step (Trainer._run: warm-up, key, capture, replay) ----------------------------------------------------------
    def _body(self, flat, pretrain):
        """The step up to the all-reduce on the flat list of static tensors; the two masks are always tensors here, so the h reset
        and the h keep are part of it (with no stream reset / every stream active they change no bit)."""
        pc1, pc2, feature1, feature2, gt_warp, gt_cls, h, nv = flat[:8]
        reset_d, active_d = flat[-2:]
        gobj = GtObjects(max_boxes=self._gobj_meta[0], points=self._gobj_meta[1], flags=None, **dict(zip(self.N_GOBJ, flat[8:-2])))
        h_in = None if h is None else T.reset_h(h, reset_d)
        items, h_out, out, match = self._forward_backward(pc1, pc2, feature1, feature2, gt_warp, gt_cls, gobj, h_in, nv, pretrain, reset_d,
                                                           active_d)
        h_out = T.keep_h(active_d, h_out, torch.zeros_like(h_out) if h_in is None else h_in)
        return items, h_out, out, match

    def _result(self, res):
        items, h_out, out, match = res
        self.last = out = out.fresh()
        return items, h_out, out, match

    @staticmethod
    def _copy_statics(pairs):
        from .fused import _copy_inputs
        word = [p for p in pairs if p[0].element_size() == 4]          # one launch per eight 4-byte tensors
        rest = [p for p in pairs if p[0].element_size() != 4]
        _copy_inputs(word)
        if rest:
            torch._foreach_copy_([p[0] for p in rest], [p[1] for p in rest])

    def check(self, out=None):
        """Synchronises.  Raises RuntimeError naming the stream that overflowed max_objects, max_gt_tracks or max_pairs."""
        out = out if out is not None else self.last
        if out is not None:
            out.check()
            check(out)
        self.scorer.check()
