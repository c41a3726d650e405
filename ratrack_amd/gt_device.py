"""Ground truth and scoring of a batch of frame pairs on the device (include/rtk_gt.h, csrc/gt_eval.hip).

    boxes = pack_boxes(per_stream, max_boxes=32, device="cuda")     # host: labels -> box tables, ONE upload for the batch
    gt = ground_truth(pc1, pc2, boxes, n_valid=nv)                   # one launch: gt.gt_warp, gt.gt_cls are what Trainer.step takes
    fm = frame_metrics(pc1, pc1 + flow, gt.gt_warp, mask, cls, gt.gt_cls, n_valid=nv, active=active)     # one launch
    acc = MetricAccumulator(streams=B); acc.update(fm); ...; acc.result()                                # the only download

Per stream, `ground_truth` computes what `vod_gt.filter_object_points` (membership, motion-segmentation labels, the id each
point carries) and `vod_gt.gt_scene_flow` compute on the host for that stream's valid slice, and `frame_metrics` what
`metrics.eval_scene_flow` / `metrics.eval_motion_seg` return for it -- each stream with its OWN mask row (the host function's
`mask[0]` is an artefact of the reference's B = 1).  Nothing here synchronises with the device except `GroundTruth.check()`,
`FrameMetrics.stream()` and `MetricAccumulator.result()`.

Not covered here: the rider merge and the minimum object size (`objs_combined`), `map_gt_objects` and the target of the tracking
loss are `ratrack_amd.track_score` (two more launches over the same `BoxBatch`); training the tracking term and label-file parsing
stay host code.
"""
import ctypes

import numpy as np
import torch

from . import _lib, vod_gt
from .abi import EvalIn, GtBoxes, GtIn, GtOut, stream as _stream, view as _view

MAX_BOXES = 256                        # RTK_GT_MAX_BOXES
KEYS = ("rne", "50-50 rne", "mov_rne", "stat_rne", "sas", "ras", "epe", "acc", "sen", "miou")
SUM_KEYS = ("points", "error", "rn_error", "rn_error_moving", "moving", "rn_error_static", "static", "sas", "ras", "tp", "tn", "fp", "fn")
_FLAG_BOXES, _FLAG_NVALID = 1, 2


# ---- box tables ----------------------------------------------------------------------------------------------------------

class BoxBatch:
    """The box tables of B frame pairs on `device` (views of one uploaded buffer): boxes (2,B,K,16) float64 = centre | R row-major |
    half-extent | pad per box, frame 1 then frame 2; box_id (2,B,K) int32 (-1 past count); count (2,B) int32; pair (B,K) int32;
    motion (B,K,12) float32; ego (B,12) float64 or None.  `host`: the same arrays as numpy, before the upload."""

    def __init__(self, B, K, host, dev):
        self.B, self.K, self.host = B, K, host
        self.__dict__.update(dev)


def _box_row(box):
    return np.concatenate([box.center, box.R.reshape(-1), box.extent / 2, [0.0]])


def pack_boxes(per_stream, max_boxes, device="cuda"):
    """per_stream[b]: (labels1, tf1, labels2, tf2) or (labels1, tf1, labels2, tf2, ego_motion) -- {id: Label} and FrameTransforms of
    the two frames as `vod_gt.filter_object_points` takes them, frame 1 being the frame of pc1, and optionally the 4x4
    `vod_gt.ego_motion` of the pair -- or None for a stream without boxes.  Boxes are `vod_gt.box_in_radar_frame`'s in label
    order; motion[b][k] is `gt_scene_flow`'s matrix (float64 product of the box poses, cast to fp32) for every frame-1 box whose
    id is also in frame 2.  A stream without an ego matrix is not compensated (identity) when another stream has one; with no ego
    matrix at all `ego` is None and `ground_truth` takes pc1_comp from its caller.  Raises ValueError when a frame has more than
    max_boxes boxes."""
    B, K = len(per_stream), int(max_boxes)
    if not 1 <= K <= MAX_BOXES:
        raise ValueError("max_boxes=%d outside [1, %d] (both frames' tables of a stream must fit one workgroup's LDS)" % (K, MAX_BOXES))
    boxes = np.zeros((2, B, K, 16), dtype=np.float64)
    box_id = np.full((2, B, K), -1, dtype=np.int32)
    count = np.zeros((2, B), dtype=np.int32)
    pair = np.full((B, K), -1, dtype=np.int32)
    motion = np.zeros((B, K, 12), dtype=np.float32)
    ego = np.tile(np.eye(4)[:3].reshape(-1), (B, 1))
    has_ego = False
    for b, item in enumerate(per_stream):
        if item is None:
            continue
        frames = []
        for f, (labels, tf) in enumerate(((item[0], item[1]), (item[2], item[3]))):
            bx = {lab.id: vod_gt.box_in_radar_frame(lab, tf) for lab in labels.values()}
            if len(bx) > K:
                raise ValueError("stream %d, frame %d: %d boxes > max_boxes=%d" % (b, f + 1, len(bx), K))
            for k, (obj_id, box) in enumerate(bx.items()):
                boxes[f, b, k] = _box_row(box)
                box_id[f, b, k] = obj_id
            count[f, b] = len(bx)
            frames.append(bx)
        slot2 = {obj_id: k for k, obj_id in enumerate(frames[1])}
        for k, (obj_id, box) in enumerate(frames[0].items()):
            if obj_id in slot2:
                pair[b, k] = slot2[obj_id]
                t = np.dot(vod_gt.box_transform(frames[1][obj_id]), np.linalg.inv(vod_gt.box_transform(box)))
                motion[b, k] = t.astype(np.float32)[:3].reshape(-1)
        if len(item) > 4 and item[4] is not None:
            has_ego = True
            ego[b] = np.linalg.inv(np.asarray(item[4]).T).T[:3].reshape(-1)      # vod_io.compensate_ego_motion's matrix, transposed
    host = dict(boxes=boxes, box_id=box_id, count=count, pair=pair, motion=motion, ego=ego if has_ego else None)
    # one buffer, one upload: the float64 sections first (every view starts on a multiple of its element size)
    parts = [("boxes", boxes), ("ego", ego), ("motion", motion), ("box_id", box_id), ("count", count), ("pair", pair)]
    buf = torch.from_numpy(np.concatenate([np.ascontiguousarray(a).reshape(-1).view(np.uint8) for _, a in parts])).to(device)
    dev, o = {}, 0
    for name, a in parts:
        dev[name] = buf[o:o + a.nbytes].view(torch.from_numpy(a[:0]).dtype).view(a.shape)
        o += a.nbytes
    if not has_ego:
        dev["ego"] = None
    dev["_buffer"] = buf
    return BoxBatch(B, K, host, dev)


# ---- ground truth --------------------------------------------------------------------------------------------------------

class GroundTruth:
    """Device tensors: gt_cls (B,N) bool, box_index (B,N) int32 (slot of the point's frame-1 box, -1 none), obj_id (B,N) int32 (its
    label id), gt_warp (B,3,N), pc1_comp (B,3,N), counts1 / counts2 (B,K) int32 (valid points inside each box), flags (B) int32."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def check(self):
        """Synchronises.  Raises RuntimeError naming the stream whose box count exceeded K or whose n_valid was out of range."""
        for b, f in enumerate(self.flags.cpu().tolist()):
            if f & _FLAG_BOXES:
                raise RuntimeError("ground_truth: stream %d has a box count outside [0, max_boxes=%d]" % (b, self.max_boxes))
            if f & _FLAG_NVALID:
                raise RuntimeError("ground_truth: stream %d has an n_valid outside [0, N]" % b)


def _n_valid(n_valid, shape, dev):
    if n_valid is None:
        return None
    nv = torch.as_tensor(n_valid).to(device=dev, dtype=torch.int32)
    if tuple(nv.shape) != shape:
        raise ValueError("n_valid must be %s, got %s" % (shape, tuple(nv.shape)))
    return nv.contiguous()


def ground_truth(pc1, pc2, boxes, n_valid=None, pc1_comp=None):
    """pc1 (B,3,N), pc2 (B,3,N2) fp32 device tensors (any strides), boxes a BoxBatch, n_valid (2,B) int32 or None.  pc1_comp (B,3,N):
    the ego-motion compensated frame 1 when the caller already has it (it then replaces the BoxBatch's ego matrices); with neither,
    frame 1 is taken as compensated.  One launch, no synchronisation."""
    B, _, N = pc1.shape
    if boxes.B != B or pc2.shape[0] != B or pc1.shape[1] != 3 or pc2.shape[1] != 3:
        raise ValueError("ground_truth: %s / %s clouds against the boxes of %d streams" % (tuple(pc1.shape), tuple(pc2.shape), boxes.B))
    dev, K = pc1.device, boxes.K
    nv = _n_valid(n_valid, (2, B), dev)
    ego = None
    if pc1_comp is not None:
        if tuple(pc1_comp.shape) != (B, 3, N):
            raise ValueError("pc1_comp must be %s, got %s" % ((B, 3, N), tuple(pc1_comp.shape)))
        comp = pc1_comp.to(torch.float32).contiguous()
    elif boxes.ego is not None:
        comp, ego = torch.empty(B, 3, N, device=dev), boxes.ego
    else:
        comp = pc1.to(torch.float32).contiguous()
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    cls8 = torch.empty(B, N, dtype=torch.uint8, device=dev)
    box_index, obj_id, counts1, counts2, flags = i32(B, N), i32(B, N), i32(B, K), i32(B, K), i32(B)
    gt_warp = torch.empty(B, 3, N, device=dev)
    a = GtIn(B, N, pc2.shape[2], K, _view(pc1), _view(pc2), None if nv is None else nv.data_ptr(),
             GtBoxes(boxes.boxes[0].data_ptr(), boxes.box_id[0].data_ptr(), boxes.count[0].data_ptr()),
             GtBoxes(boxes.boxes[1].data_ptr(), boxes.box_id[1].data_ptr(), boxes.count[1].data_ptr()),
             boxes.pair.data_ptr(), boxes.motion.data_ptr(), None if ego is None else ego.data_ptr())
    o = GtOut(cls8.data_ptr(), box_index.data_ptr(), obj_id.data_ptr(), gt_warp.data_ptr(), comp.data_ptr(), counts1.data_ptr(),
              counts2.data_ptr(), flags.data_ptr())
    _lib.call("rtk_gt_labels", ctypes.addressof(a), ctypes.addressof(o), _stream())
    return GroundTruth(gt_cls=cls8.view(torch.bool), box_index=box_index, obj_id=obj_id, gt_warp=gt_warp, pc1_comp=comp, counts1=counts1,
                       counts2=counts2, flags=flags, max_boxes=K)


# ---- metrics -------------------------------------------------------------------------------------------------------------

def values_from_sums(sums):
    """(..., 13) float64 sums -> (..., 10) values in KEYS order: the reference's formulae (main_utils.py:342-389), as the kernel
    evaluates them per stream."""
    s = np.asarray(sums, dtype=np.float64)
    g = lambda i: s[..., i]
    with np.errstate(divide="ignore", invalid="ignore"):
        mov, stat = g(3) / (g(4) + 1e-6), g(5) / g(6)
        tp, tn, fp, fn = g(9) + 1e-20, g(10) + 1e-20, g(11) + 1e-20, g(12) + 1e-20
        out = [g(2) / g(0), (mov + stat) / 2, mov, stat, g(7) / g(0), g(8) / g(0), g(1) / g(0), (tp + tn) / (tp + tn + fp + fn),
               tp / (tp + fn), 0.5 * (tp / (tp + fp + fn + 1e-4) + tn / (tn + fp + fn + 1e-4))]
    return np.stack(out, axis=-1)


class FrameMetrics:
    """values (B,10) float64 in `keys` order, sums (B,13) float64 in `sum_keys` order (device tensors); active (B) uint8 or None."""
    keys, sum_keys = KEYS, SUM_KEYS

    def __init__(self, values, sums, active):
        self.values, self.sums, self.active = values, sums, active

    def stream(self, b):
        """Synchronises: stream b's values as the dict the host functions return (scene flow and segmentation together)."""
        return dict(zip(KEYS, self.values[b].cpu().tolist()))


def _flag_bytes(x, B, dev):
    if x is None:
        return None
    t = torch.as_tensor(x).to(device=dev).reshape(-1)
    if t.numel() != B:
        raise ValueError("a per-stream mask needs %d entries, got %d" % (B, t.numel()))
    return t.view(torch.uint8) if t.dtype == torch.bool else (t if t.dtype == torch.uint8 else (t != 0).to(torch.uint8))


def frame_metrics(pc1, warp, gt_warp, mask, cls, gt_cls, n_valid=None, active=None, threshold=0.5):
    """pc1, warp (= pc1 + flow), gt_warp (B,3,N) fp32 device tensors of any strides; mask (B,N): 1 static, 0 moving (the epoch loop's
    1 - gt_cls); cls (B,1,N) or (B,N) scores, moving iff cls > threshold; gt_cls (B,N) bool / uint8.  n_valid (B) int32 -- or the
    batch's (2,B), whose frame-1 row is taken -- and active (B) select the columns and the streams that are scored.
    One launch, no synchronisation."""
    B, _, N = pc1.shape
    dev = pc1.device
    if n_valid is not None:
        nv = torch.as_tensor(n_valid)
        nv = _n_valid(nv[0] if nv.dim() == 2 else nv, (B,), dev)
    else:
        nv = None
    act = _flag_bytes(active, B, dev)
    mask32 = mask.to(device=dev, dtype=torch.float32).reshape(B, N).contiguous()
    g = gt_cls.reshape(B, N)
    g8 = (g.view(torch.uint8) if g.dtype == torch.bool else (g if g.dtype == torch.uint8 else (g == 1).to(torch.uint8))).contiguous()
    if cls.dim() == 3 and cls.shape[1] != 1:
        raise ValueError("cls must be (B,1,N) or (B,N), got %s" % (tuple(cls.shape),))
    sums = torch.empty(B, len(SUM_KEYS), dtype=torch.float64, device=dev)
    values = torch.empty(B, len(KEYS), dtype=torch.float64, device=dev)
    a = EvalIn(B, N, _view(pc1), _view(warp), _view(gt_warp), _view(cls), mask32.data_ptr(), g8.data_ptr(), float(threshold),
               None if nv is None else nv.data_ptr(), None if act is None else act.data_ptr())
    _lib.call("rtk_eval_frame", ctypes.addressof(a), sums.data_ptr(), values.data_ptr(), _stream())
    return FrameMetrics(values, sums, act)


class MetricAccumulator:
    """Sums FrameMetrics over the frames of `streams` sequences on the device.  `update` adds the frame of every active stream;
    `result` downloads once."""

    def __init__(self, streams, device="cuda"):
        self.B = int(streams)
        self.value_sum = torch.zeros(self.B, len(KEYS), dtype=torch.float64, device=device)
        self.raw_sum = torch.zeros(self.B, len(SUM_KEYS), dtype=torch.float64, device=device)
        self.frames = torch.zeros(self.B, dtype=torch.int64, device=device)

    def update(self, fm, active=None):
        """active (B) overrides the mask the frame was scored with (fm.active); None and no such mask: every stream counts."""
        act = fm.active if active is None else _flag_bytes(active, self.B, self.frames.device)
        if act is None:
            self.value_sum += fm.values
            self.raw_sum += fm.sums
            self.frames += 1
            return
        on = (act != 0)
        self.value_sum += torch.where(on.unsqueeze(1), fm.values, 0.0)
        self.raw_sum += torch.where(on.unsqueeze(1), fm.sums, 0.0)
        self.frames += on.to(torch.int64)

    def result(self):
        """The only download.  -> dict: `frames` (B) int; `per_stream` {key: (B) array} = each stream's mean over its frames of the
        per-frame values and `overall` {key: float} = the mean over all frames of all streams (what the reference's epoch loop
        accumulates, main_utils.py:131-146); `pooled` / `pooled_per_stream`: the values recomputed from the raw sums of all points;
        `sums` (B,13)."""
        flat = torch.cat([self.value_sum.reshape(-1), self.raw_sum.reshape(-1), self.frames.to(torch.float64)]).cpu().numpy()
        nk, ns = len(KEYS), len(SUM_KEYS)
        vs = flat[:self.B * nk].reshape(self.B, nk)
        rs = flat[self.B * nk:self.B * (nk + ns)].reshape(self.B, ns)
        frames = flat[self.B * (nk + ns):]
        with np.errstate(divide="ignore", invalid="ignore"):
            per = vs / frames[:, None]
            overall = vs.sum(0) / frames.sum()
        pooled, pooled_per = values_from_sums(rs.sum(0)), values_from_sums(rs)
        return dict(frames=frames.astype(np.int64), per_stream={k: per[:, i] for i, k in enumerate(KEYS)},
                    overall={k: float(overall[i]) for i, k in enumerate(KEYS)}, pooled={k: float(pooled[i]) for i, k in enumerate(KEYS)},
                    pooled_per_stream={k: pooled_per[:, i] for i, k in enumerate(KEYS)}, sums=rs)
