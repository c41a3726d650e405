"""The batched tracker's result files without a host round trip per step: a result log on the device, one selection pass, one download.

    log = ResultLog(streams=B, max_objects=trk.K, frames=F, records=R, points=P, device="cuda")
    for t in range(T):
        out = trk.step(pc1, pc2, f1, f2, n_valid=nv, reset=is_new_seq, active=has_frame)
        log.append(out, seq=seq_no, index=frame_no, reset=is_new_seq)       # one launch, no synchronisation
    sel   = log.select(threshold=sw.best["threshold"], min_hits=1, min_track_frames=3)       # one launch
    paths = log.write(root, names, threshold=..., min_hits=..., min_track_frames=...)        # the only downloads
    log.clear()

`BatchedTracker.write_results` downloads a whole step and writes its B files, every step.  `append` (rtk_result_log_append,
csrc/track_results.hip; the rules are stated in include/rtk_fused.h, "The result log") keeps what those files hold on the device
instead: per stream a packed list of frames, of records (track id, confidence, hits, size) and of points grouped by object in the
file's order, behind cursors that live on the device, so that a captured append replays correctly.  With no filter, `write` produces
the files `write_results` would have produced, byte for byte.

What the per-step writer cannot do is decide by something that is only known when the clip is over.  `select`
(rtk_result_log_select) computes for every record the score of its track -- the mean object_conf of its (stream, clip, track id), the
score `TrackScorer.sweep` reports its operating point in, the same bits -- and the track's length, and keeps a record iff
`!(score < threshold)`, `rec_hits >= min_hits` (from 2 on; 1 asks nothing, as in `write_results`) and
`length >= min_track_frames`: files at the sweep's operating point, and short tracks dropped whole, their first frames included.

`boxes` (rtk_result_log_boxes, ratrack_amd/boxes.py) fits every record's oriented box in one launch, and `write_kitti` writes them, for
the records a selection keeps, as KITTI tracking result files, one per sequence: the format the evaluators of the field read.
`filter_boxes` (rtk_result_log_filter_boxes, `boxes.BoxFilter`) turns those per-frame boxes into the boxes of each track -- a Kalman
filter along every (stream, clip, track id), optionally smoothed, optionally with a size from the whole track -- in one more launch, and
`write_kitti(filter=...)` writes them instead.

Only `write`, `write_kitti`, `frames`, `check`, `download` and `select(check=True)` synchronise.  `seq` / `index` given as host values cost one small
host-to-device copy per append; given as (B,) int32 device tensors they are read at launch time and cost nothing.

With a `TrackerPipeline` use one ResultLog per group and append under `torch.cuda.stream(pipe.streams[g])` before group g's next
submit: the step's outputs are the graph's static tensors, and the next replay overwrites them.
"""
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib
from .abi import ResultLog as _Block, stream as _stream, view as _view
from .gt_device import _flag_bytes

MAX_OBJECTS = 256                      # RTK_RESULT_MAX_OBJECTS (= RTK_SCORE_MAX_OBJECTS)
TRACKS = 2048                          # RTK_SCORE_SWEEP_TRACKS: track ids of one clip `select` can tell apart
FLAG_OBJECTS, FLAG_STEP, FLAG_FULL, FLAG_TRACKS = 1, 2, 4, 8      # RTK_RESULT_FLAG_*


# ---- argument checks: no device is touched -----------------------------------------------------------------------------------------

def check_sizes(streams, max_objects, frames, records, points):
    """The constructor's sizes; raises ValueError."""
    for name, v in (("streams", streams), ("max_objects", max_objects), ("frames", frames), ("records", records), ("points", points)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError("ResultLog: %s=%r must be an integer >= 1" % (name, v))
    if max_objects > MAX_OBJECTS:
        raise ValueError("ResultLog: max_objects=%d above %d (the frame word's count and the append kernel's scan)" % (max_objects, MAX_OBJECTS))
    if streams * max(4 * frames, records, 3 * points) >= 2 ** 31:
        raise ValueError("ResultLog: streams=%d x max(4 frames=%d, records=%d, 3 points=%d) must stay below 2^31 words"
                         % (streams, frames, records, points))


def check_filters(threshold, min_hits, min_track_frames, hits_logged=True):
    """The filters of `select` / `write`; -> whether any of them can remove a record.  hits_logged: every logged frame came with hit
    counts.  Raises ValueError."""
    for name, v in (("min_hits", min_hits), ("min_track_frames", min_track_frames)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError("%s=%r: an integer >= 1" % (name, v))
    if min_hits > 1 and not hits_logged:
        raise ValueError("min_hits=%d needs the hit counts of track memory, and a logged frame came without them: build the tracker with "
                         "max_age (0 or more)" % min_hits)
    if torch.is_tensor(threshold):
        if threshold.numel() != 1 or threshold.dim() > 1 or not threshold.dtype.is_floating_point:
            raise ValueError("threshold: a float or a 0-dim floating-point tensor, got a %s tensor of shape %s" % (threshold.dtype, tuple(threshold.shape)))
    elif threshold is not None:
        if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)) or math.isnan(float(threshold)):
            raise ValueError("threshold=%r: None, a number (not NaN) or a 0-dim tensor" % (threshold,))
    return threshold is not None or min_hits > 1 or min_track_frames > 1


def flag_message(b, f, max_objects):
    """The first complaint about stream b's flags word f, or None."""
    if f & FLAG_OBJECTS:
        return "ResultLog: stream %d had a frame with num_objects outside [0, max_objects=%d]: it was not logged" % (b, max_objects)
    if f & FLAG_STEP:
        return "ResultLog: stream %d had a frame whose step overflowed max_objects or had an n_valid outside [0, N]: it was not logged" % b
    if f & FLAG_FULL:
        return "ResultLog: stream %d had a frame that did not fit what was left of its log (frames, records or points): it was not logged" % b
    if f & FLAG_TRACKS:
        return "ResultLog: stream %d has a clip with more than %d track ids: no selection for it" % (b, TRACKS)
    return None


def raise_on_flags(flags, max_objects):
    for b, f in enumerate(flags):
        msg = flag_message(b, int(f), max_objects)
        if msg:
            raise RuntimeError(msg)


# ---- the host half: a dict of numpy arrays -> files ----------------------------------------------------------------------------
# host: cursor (B,4) int32, frame / tag (B,>=frames,4) int32, rec_track / rec_size (B,>=records) int32, rec_conf (B,>=records) fp32,
# points (B,>=points,3) fp32 (and rec_hits, which the files do not need): the live prefix of the log's tensors.

def format_values(x):
    """fp32 values -> their text in a result file: str(float(x)) of each, as vod_io.format_track_line writes them (the shortest text
    that reads back as the double the fp32 value widens to).  One conversion for the whole array instead of one per number."""
    return [repr(v) for v in np.asarray(x, dtype=np.float32).astype(np.float64).reshape(-1).tolist()]


def _streams_of(host, streams):
    return range(host["cursor"].shape[0]) if streams is None else streams


def logged_frames(host, streams=None):
    """[(stream, frame slot, seq, index)] of every logged frame, stream after stream."""
    out = []
    for b in _streams_of(host, streams):
        tag = host["tag"][b]
        out += [(b, f, int(tag[f, 0]), int(tag[f, 1])) for f in range(int(host["cursor"][b, 0]))]
    return out


def frame_path(root, names, seq, index):
    return os.path.join(root, str(names[seq]), str(int(index)).zfill(5) + ".txt")


def check_paths(root, names, host, streams=None):
    """[(stream, frame slot, path)]; two logged frames with one (seq, index) raise ValueError naming both."""
    seen, out = {}, []
    for b, f, seq, index in logged_frames(host, streams):
        if (seq, index) in seen:
            raise ValueError("ResultLog: frame %d of stream %d and frame %d of stream %d are both (seq=%d, index=%d): one file for two frames"
                             % (seen[(seq, index)][1], seen[(seq, index)][0], f, b, seq, index))
        seen[(seq, index)] = (b, f)
        out.append((b, f, frame_path(root, names, seq, index)))
    return out


def render_frames(host, keep=None, streams=None):
    """{(stream, frame slot): the text of its file}: one line per kept record, `NA 1 -1 -1 conf id x y z x y z ...`."""
    texts = {}
    for b in _streams_of(host, streams):
        frames, records, points = (int(v) for v in host["cursor"][b, :3])
        conf = format_values(host["rec_conf"][b, :records])
        xyz = format_values(host["points"][b, :points])
        ids, sizes = host["rec_track"][b, :records].tolist(), host["rec_size"][b, :records].tolist()
        kept = None if keep is None else np.asarray(keep)[b, :records].tolist()
        fw = host["frame"][b, :frames].tolist()
        for f in range(frames):
            rec, at, count = fw[f][0], 3 * fw[f][1], fw[f][2] & 0xffff
            lines = []
            for r in range(rec, rec + count):
                end = at + 3 * sizes[r]
                if kept is None or kept[r]:
                    lines.append(" ".join(["NA", "1", "-1", "-1", conf[r], str(ids[r])] + xyz[at:end]) + "\n")
                at = end
            texts[(b, f)] = "".join(lines)
    return texts


def write_frames(root, names, host, keep=None, streams=None):
    """One file <root>/<names[seq]>/<index:05d>.txt per logged frame of `host` with its kept records (keep (B,>=records), None: all;
    a frame without a kept record gets an empty file); streams: the streams to write (None: all).  Two frames with one (seq, index)
    raise ValueError before anything is written.  Returns the paths."""
    where = check_paths(root, names, host, streams)
    texts = render_frames(host, keep, streams)
    paths = []
    for b, f, path in where:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w+") as fh:
            fh.write(texts[(b, f)])
        paths.append(path)
    return paths


def host_frames(host, b, keep=None):
    """[(seq, index, [(track id, conf, points (n,3) float64), ...]), ...] of stream b: per frame what vod_io.read_track_results
    returns for its file."""
    frames = int(host["cursor"][b, 0])
    out = []
    for f in range(frames):
        rec, at, word = (int(v) for v in host["frame"][b, f, :3])
        objects = []
        for r in range(rec, rec + (word & 0xffff)):
            n = int(host["rec_size"][b, r])
            if keep is None or keep[b, r]:
                objects.append((int(host["rec_track"][b, r]), float(host["rec_conf"][b, r]), host["points"][b, at:at + n].astype(np.float64)))
            at += n
        out.append((int(host["tag"][b, f, 0]), int(host["tag"][b, f, 1]), objects))
    return out


def check_transforms(host, transforms, streams=None):
    """Every logged frame of `host` has its entry in `transforms` ((seq, index) -> vod_gt.FrameTransforms; None asks nothing);
    raises ValueError naming the first that has not."""
    if transforms is None:
        return
    for b, f, seq, index in logged_frames(host, streams):
        if (seq, index) not in transforms:
            raise ValueError("ResultLog: frame %d of stream %d is (seq=%d, index=%d), and transforms has no entry for it" % (f, b, seq, index))


def kitti_rows(host, keep=None, transforms=None, obj_type="Car", streams=None):
    """{seq: [(frame index, track id, obj_type, vod_io.KittiFields, score), ...]}: the lines of every sequence's KITTI tracking result
    file, in (index, record) order -- one per kept record that has a box (host["box_valid"] > 0), its score the record's confidence.
    host: `download(boxes=...)`'s dict.  transforms: None (radar-frame values, ry = yaw) or (seq, index) -> FrameTransforms.  Raises
    ValueError before anything is rendered for two logged frames with one (seq, index) or a frame that `transforms` misses."""
    from . import vod_io
    seen = {}
    for b, f, seq, index in logged_frames(host, streams):
        if (seq, index) in seen:
            raise ValueError("ResultLog: frame %d of stream %d and frame %d of stream %d are both (seq=%d, index=%d): one frame number for "
                             "two frames" % (seen[(seq, index)][1], seen[(seq, index)][0], f, b, seq, index))
        seen[(seq, index)] = (b, f)
    check_transforms(host, transforms, streams)
    rows = {}
    for (seq, index), (b, f) in sorted(seen.items(), key=lambda kv: (kv[0][0], kv[0][1])):
        out = rows.setdefault(seq, [])
        rec, count = int(host["frame"][b, f, 0]), int(host["frame"][b, f, 2]) & 0xffff
        tf = None if transforms is None else transforms[(seq, index)]
        for r in range(rec, rec + count):
            if (keep is not None and not keep[b, r]) or host["box_valid"][b, r] <= 0:
                continue
            fields = vod_io.box_label_fields(host["box"][b, r, :7], tf)
            out.append((index, int(host["rec_track"][b, r]), obj_type, fields, float(host["rec_conf"][b, r])))
    return rows


def kitti_path(root, names, seq):
    return os.path.join(root, str(names[seq]) + ".txt")


# ---- the device half ------------------------------------------------------------------------------------------------------------

class Selection:
    """`ResultLog.select`'s outputs (device tensors, meaningful below each stream's records cursor): keep (B,R) uint8, track_score
    (B,R) float64, track_frames (B,R) int32; flags (B) int32: FLAG_TRACKS where a clip has more track ids than the table holds."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _stream_words(values, B, dev):
    """seq / index -> (B,) int32 device tensors.  Device tensors are taken as they are (read at launch time); host values (an int or
    B ints each) travel together in one host-to-device copy."""
    out, host = [None] * len(values), []
    for k, (name, x) in enumerate(values):
        if torch.is_tensor(x) and x.is_cuda:
            if x.numel() != B or x.dtype.is_floating_point:
                raise ValueError("ResultLog: %s must hold %d integers, got %s of %s" % (name, B, tuple(x.shape), x.dtype))
            out[k] = x.reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
            continue
        a = np.asarray(x.cpu() if torch.is_tensor(x) else x)
        if a.dtype.kind not in "iu" or a.size not in (1, B):
            raise ValueError("ResultLog: %s must be an int or %d ints, got %r" % (name, B, x))
        a = np.broadcast_to(a.reshape(-1).astype(np.int64), (B,))
        if a.min() < -2 ** 31 or a.max() >= 2 ** 31:
            raise ValueError("ResultLog: %s=%r does not fit an int32" % (name, x))
        host.append((k, a.astype(np.int32)))
    if host:
        dev_rows = torch.from_numpy(np.stack([a for _, a in host])).to(dev)
        for row, (k, _) in enumerate(host):
            out[k] = dev_rows[row]
    return out


class ResultLog:
    """The result log of `streams` sequences (module docstring).  State, all device tensors, zero-initialised, written by `append`
    only: cursor (B,4) int32 frames | records | points logged | unused; frame (B,F,4) int32 first record | first point | objects +
    65536 * (the frame began a clip) | 0 (the scorer's frame word); tag (B,F,4) int32 seq | index | points of the frame | the step's
    flags word; rec_track (B,R) int32, rec_conf (B,R) fp32, rec_hits (B,R) int32 (0 when the step has none), rec_size (B,R) int32;
    points (B,P,3) fp32; flags (B) int32, sticky (FLAG_OBJECTS | FLAG_STEP | FLAG_FULL)."""

    def __init__(self, streams, max_objects, frames, records, points, device="cuda"):
        check_sizes(streams, max_objects, frames, records, points)
        self.B, self.K, self.F, self.R, self.P = int(streams), int(max_objects), int(frames), int(records), int(points)
        B, z = self.B, lambda *s: torch.zeros(*s, dtype=torch.int32, device=device)
        self.cursor, self.frame, self.tag = z(B, 4), z(B, self.F, 4), z(B, self.F, 4)
        self.rec_track, self.rec_hits, self.rec_size = z(B, self.R), z(B, self.R), z(B, self.R)
        self.rec_conf = torch.zeros(B, self.R, dtype=torch.float32, device=device)
        self.points = torch.zeros(B, self.P, 3, dtype=torch.float32, device=device)
        self.flags = z(B)
        self.hits_logged = True         # every frame appended since the last clear() came with hit counts

    def _block(self):
        return _Block(self.F, self.R, self.P, *(t.data_ptr() for t in (self.cursor, self.frame, self.tag, self.rec_track, self.rec_conf,
                                                                        self.rec_hits, self.rec_size, self.points, self.flags)))

    # ---- append ------------------------------------------------------------------------------------------------------------------
    def append(self, out, seq, index, reset=None, active=None):
        """A `tracker.StepResult`'s frame into the log: one launch on the current stream, no synchronisation.  seq, index: an int, B
        ints or a (B,) int32 device tensor each (a device tensor is read at launch time); reset (B) or None: the streams whose frame
        begins a clip; active None: the mask the step ran with."""
        if out.max_objects != self.K:
            raise ValueError("ResultLog(max_objects=%d) against a step with max_objects=%d" % (self.K, out.max_objects))
        return self.append_raw(out.pc1, out.obj, out.num_objects, out.object_ids, out.object_conf, seq, index,
                               object_hits=getattr(out, "object_hits", None), step_flags=out.flags, reset=reset,
                               active=out.active if active is None else active)

    def append_raw(self, pc1, obj, num_objects, object_ids, object_conf, seq, index, object_hits=None, step_flags=None, reset=None, active=None):
        """The same launch for detections from elsewhere.  pc1 (B,3,N) fp32 of any strides; obj (B,N) int32, the object of each column
        (outside [0, num_objects): none); num_objects (B) int32; object_ids (B,K) int32; object_conf (B,K) fp32; object_hits (B,K) int32
        or None (hits are logged as 0); step_flags (B) int32 or None: a word with bit 0 or 1 set refuses the frame."""
        B, K = self.B, self.K
        if pc1.dim() != 3 or pc1.shape[0] != B or pc1.shape[1] != 3 or tuple(obj.shape) != (B, pc1.shape[2]) or num_objects.numel() != B or \
                tuple(object_ids.shape) != (B, K) or tuple(object_conf.shape) != (B, K):
            raise ValueError("ResultLog(streams=%d, max_objects=%d): got pc1 %s, obj %s, num_objects %s, object_ids %s, object_conf %s"
                             % (B, K, tuple(pc1.shape), tuple(obj.shape), tuple(num_objects.shape), tuple(object_ids.shape), tuple(object_conf.shape)))
        if object_hits is not None and tuple(object_hits.shape) != (B, K):
            raise ValueError("ResultLog: object_hits must be (%d,%d), got %s" % (B, K, tuple(object_hits.shape)))
        if step_flags is not None and step_flags.numel() != B:
            raise ValueError("ResultLog: step_flags must hold %d words, got %s" % (B, tuple(step_flags.shape)))
        N, dev = pc1.shape[2], self.cursor.device
        as32 = lambda x: None if x is None else x.to(device=dev, dtype=torch.int32).contiguous()
        obj, num_objects, object_ids, object_hits, step_flags = (as32(x) for x in (obj, num_objects, object_ids, object_hits, step_flags))
        object_conf = object_conf.to(device=dev, dtype=torch.float32).contiguous()
        seq_d, index_d = _stream_words((("seq", seq), ("index", index)), B, dev)
        rst, act = _flag_bytes(reset, B, dev), _flag_bytes(active, B, dev)
        ptr = lambda x: None if x is None else x.data_ptr()
        pv, lg = _view(pc1.float()), self._block()
        _lib.call("rtk_result_log_append", B, N, K, ctypes.addressof(pv), obj.data_ptr(), num_objects.data_ptr(), object_ids.data_ptr(),
                  object_conf.data_ptr(), ptr(object_hits), ptr(step_flags), seq_d.data_ptr(), index_d.data_ptr(), ptr(rst), ptr(act),
                  ctypes.addressof(lg), _stream())
        if object_hits is None:
            self.hits_logged = False

    # ---- select ------------------------------------------------------------------------------------------------------------------
    def select(self, threshold=None, min_hits=1, min_track_frames=1, check=True):
        """Which records the files keep (module docstring): one launch, -> Selection.  threshold: None (keeps every score, as
        -infinity does), a float, or a 0-dim device tensor (read on the device).  check: download the selection's flags and raise
        RuntimeError for a stream with more than 2048 track ids in a clip (the one synchronisation; check=False: none)."""
        check_filters(threshold, min_hits, min_track_frames, self.hits_logged)
        B, dev = self.B, self.cursor.device
        thr, value = None, float("-inf")
        if torch.is_tensor(threshold):
            thr = threshold.detach().to(device=dev, dtype=torch.float64).reshape(1)
        elif threshold is not None:
            value = float(threshold)
        keep = torch.zeros(B, self.R, dtype=torch.uint8, device=dev)
        score = torch.zeros(B, self.R, dtype=torch.float64, device=dev)
        length = torch.zeros(B, self.R, dtype=torch.int32, device=dev)
        flags = torch.zeros(B, dtype=torch.int32, device=dev)
        lg = self._block()
        _lib.call("rtk_result_log_select", B, ctypes.addressof(lg), None if thr is None else thr.data_ptr(), value, int(min_hits),
                  int(min_track_frames), keep.data_ptr(), score.data_ptr(), length.data_ptr(), flags.data_ptr(), _stream())
        sel = Selection(keep=keep, track_score=score, track_frames=length, flags=flags, threshold=threshold, min_hits=int(min_hits),
                        min_track_frames=int(min_track_frames))
        if check:
            raise_on_flags(flags.cpu().tolist(), self.K)
        return sel

    # ---- the way out ----------------------------------------------------------------------------------------------------------------
    def download(self, selection=None, boxes=None):
        """-> (host, keep, flags): the live prefix of the log as a dict of numpy arrays (`write_frames`' argument), the selection's keep
        (B,records) uint8 or None, and the sticky flags or-ed with the selection's.  Two transfers whatever the frame count: the
        cursors and flags, then everything below the largest cursors in one concatenation.  boxes (`boxes()`'s result): its rows
        travel in the same two transfers and join host as box (B,records,8) float64, box_cand, box_valid (B,records) int32 and
        box_flags (B) int32 (kept apart from `flags`: a box flag refuses no frame); `filter_boxes()`'s result goes the same way and
        adds box_vel (B,records,4) float64."""
        head = [self.cursor.reshape(-1), self.flags] + ([] if selection is None else [selection.flags]) + ([] if boxes is None else [boxes.flags])
        head = torch.cat(head).cpu().numpy()
        B = self.B
        cursor, flags = head[:4 * B].reshape(B, 4).copy(), head[4 * B:5 * B].copy()
        if selection is not None:
            flags |= head[5 * B:6 * B]
        f, r, p = (int(min(cursor[:, k].max(), cap)) if B else 0 for k, cap in enumerate((self.F, self.R, self.P)))
        parts = [("frame", self.frame[:, :f]), ("tag", self.tag[:, :f]), ("rec_track", self.rec_track[:, :r]), ("rec_size", self.rec_size[:, :r]),
                 ("rec_hits", self.rec_hits[:, :r]), ("rec_conf", self.rec_conf[:, :r].view(torch.int32)),
                 ("points", self.points[:, :p].reshape(B, -1).view(torch.int32))]
        if selection is not None:
            parts.append(("keep", selection.keep[:, :r].to(torch.int32)))
        if boxes is not None:
            parts += [("box", boxes.box[:, :r].reshape(B, -1).view(torch.int32)), ("box_cand", boxes.cand[:, :r]), ("box_valid", boxes.valid[:, :r])]
            if hasattr(boxes, "vel"):      # a FilteredBoxes: the velocity rows travel too
                parts.append(("box_vel", boxes.vel[:, :r].reshape(B, -1).view(torch.int32)))
        flat = torch.cat([t.reshape(-1) for _, t in parts]).cpu().numpy()
        host, o = dict(cursor=cursor), 0
        for name, t in parts:
            host[name] = flat[o:o + t.numel()].reshape(tuple(t.shape)).copy()
            o += t.numel()
        host["rec_conf"] = host["rec_conf"].view(np.float32)
        host["points"] = host["points"].view(np.float32).reshape(B, p, 3)
        keep = host.pop("keep").astype(np.uint8) if selection is not None else None
        if boxes is not None:
            host["box"] = host["box"].view(np.float64).reshape(B, r, 8)
            if "box_vel" in host:
                host["box_vel"] = host["box_vel"].view(np.float64).reshape(B, r, 4)
            host["box_flags"] = head[-B:].copy() if B else head[:0].copy()
        return host, keep, flags

    def _selected(self, threshold, min_hits, min_track_frames):
        if check_filters(threshold, min_hits, min_track_frames, self.hits_logged):
            return self.select(threshold, min_hits, min_track_frames, check=False)
        return None

    def write(self, root, names, threshold=None, min_hits=1, min_track_frames=1, check=True):
        """One file <root>/<names[seq]>/<index:05d>.txt per logged frame, with the kept records only (`select` runs when a filter is
        given).  check=True raises RuntimeError naming the stream for any flag before anything is written; check=False writes the
        streams without a flag.  Returns the paths."""
        host, keep, flags = self.download(self._selected(threshold, min_hits, min_track_frames))
        if check:
            raise_on_flags(flags.tolist(), self.K)
        return write_frames(root, names, host, keep, [b for b in range(self.B) if not flags[b]])

    # ---- boxes ------------------------------------------------------------------------------------------------------------------
    def boxes(self, keep=None, min_extent=0.0, into=None):
        """The oriented box of every logged record (ratrack_amd/boxes.py; rtk_result_log_boxes): one launch, no synchronisation,
        -> boxes.ObjectBoxes with one row per record slot, written below each stream's records cursor only (zero elsewhere).  keep:
        None, a `Selection` or its (B,R) uint8 `keep`: the records it does not mark get no box (valid = 0).  into: an ObjectBoxes of
        (B,R) rows to write into instead of new buffers (nothing is allocated: the call can be captured)."""
        from . import boxes as _boxes
        min_extent = _boxes.check_min_extent(min_extent)
        keep = getattr(keep, "keep", keep)
        dev = self.cursor.device
        if keep is not None:
            if not torch.is_tensor(keep) or tuple(keep.shape) != (self.B, self.R) or keep.dtype not in (torch.uint8, torch.bool):
                raise ValueError("ResultLog.boxes: keep must be a (%d,%d) uint8 tensor (Selection.keep)" % (self.B, self.R))
            keep = keep.to(device=dev).contiguous()
            keep = keep.view(torch.uint8) if keep.dtype == torch.bool else keep
        if into is not None:
            out = _boxes.check_into(into, self.B, self.R, dev)
        else:
            out = _boxes.ObjectBoxes(torch.zeros(self.B, self.R, 8, dtype=torch.float64, device=dev),
                                     torch.zeros(self.B, self.R, dtype=torch.int32, device=dev),
                                     torch.zeros(self.B, self.R, dtype=torch.int32, device=dev), torch.zeros(self.B, dtype=torch.int32, device=dev))
        lg = self._block()
        _lib.call("rtk_result_log_boxes", self.B, ctypes.addressof(lg), None if keep is None else keep.data_ptr(), min_extent,
                  out.box.data_ptr(), out.cand.data_ptr(), out.valid.data_ptr(), out.flags.data_ptr(), _stream())
        return out

    def filter_boxes(self, boxes, keep=None, filter=None, into=None):
        """The boxes of every track instead of every frame (ratrack_amd/boxes.py, `BoxFilter`; rtk_result_log_filter_boxes): one
        launch over the log when the clip is over, no synchronisation, -> boxes.FilteredBoxes with one row per record slot, written
        below each stream's records cursor only (zero elsewhere).  boxes: `boxes()`'s result, or an ObjectBoxes of (B,R) rows from
        anywhere; it is only read.  keep: None, a `Selection` or its (B,R) uint8 `keep`: the records it does not mark belong to no
        track and get no box.  filter: a boxes.BoxFilter (None: its defaults).  into: a FilteredBoxes of (B,R) rows to write into
        (`FilteredBoxes.empty(B, R, device)`; nothing is allocated: the call can be captured)."""
        from . import boxes as _boxes
        flt = _boxes.check_filter(_boxes.BoxFilter() if filter is None else filter)
        keep = getattr(keep, "keep", keep)
        dev = self.cursor.device
        if keep is not None:
            if not torch.is_tensor(keep) or tuple(keep.shape) != (self.B, self.R) or keep.dtype not in (torch.uint8, torch.bool):
                raise ValueError("ResultLog.filter_boxes: keep must be a (%d,%d) uint8 tensor (Selection.keep)" % (self.B, self.R))
        try:
            _boxes.check_into(boxes, self.B, self.R, dev)
        except ValueError as e:
            raise ValueError("ResultLog.filter_boxes: boxes: " + str(e).replace("into.", "")) from None
        if into is not None:
            out = _boxes.check_filtered_into(into, self.B, self.R, dev)
            if out.box.data_ptr() == boxes.box.data_ptr() or out.valid.data_ptr() == boxes.valid.data_ptr():
                raise ValueError("ResultLog.filter_boxes: into must not share box or valid with the input boxes")
        else:
            out = _boxes.FilteredBoxes.zeros(self.B, self.R, dev)
        if keep is not None:
            keep = keep.to(device=dev).contiguous()
            keep = keep.view(torch.uint8) if keep.dtype == torch.bool else keep
        out.cand = boxes.cand
        lg, par = self._block(), flt.block()
        _lib.call("rtk_result_log_filter_boxes", self.B, ctypes.addressof(lg), None if keep is None else keep.data_ptr(), boxes.box.data_ptr(),
                  boxes.valid.data_ptr(), ctypes.addressof(par), out.box.data_ptr(), out.valid.data_ptr(), out.vel.data_ptr(),
                  out.state.data_ptr(), out.aligned.data_ptr(), out.link.data_ptr(), out.flags.data_ptr(), _stream())
        return out

    def write_kitti(self, root, names, transforms=None, obj_type="Car", threshold=None, min_hits=1, min_track_frames=1, min_extent=0.0,
                    check=True, filter=None):
        """KITTI tracking result files (vod_io.format_kitti_track_line), one per sequence: <root>/<names[seq]>.txt with one line per
        kept record that has a box, in (index, record) order; the frame number is the frame's index, the score the record's confidence.
        `select` runs with the given filters (when one is given), `boxes` on what it keeps, then everything is downloaded once.
        transforms: None -- the radar-frame values as they are, ry = yaw -- or a mapping (seq, index) -> vod_gt.FrameTransforms: the
        label fields of the camera frame (vod_io.box_label_fields); a logged frame without an entry raises ValueError before any file
        is written.  check=True raises RuntimeError naming the stream for any flag of the log or of the selection before anything is
        written; check=False writes the streams without one.  A stream with an object above boxes.MAX_POINTS points is written, its
        box axis-aligned, with a warning.  filter: None, or a boxes.BoxFilter: the files hold `filter_boxes`' boxes of the kept
        records instead of the per-frame ones (one more launch; the fit's warning still comes from the per-frame boxes, and a stream
        whose filter raised a flag is written with a warning too).  Returns the paths."""
        import warnings
        from . import boxes as _boxes, vod_io
        _boxes.check_min_extent(min_extent)
        if filter is not None:
            _boxes.check_filter(filter)
        sel = self._selected(threshold, min_hits, min_track_frames)
        fitted = self.boxes(sel, min_extent)
        if filter is not None:
            filtered = self.filter_boxes(fitted, sel, filter)
            filtered.flags = filtered.flags | fitted.flags
            fitted = filtered
        host, keep, flags = self.download(sel, boxes=fitted)
        if check:
            raise_on_flags(flags.tolist(), self.K)
        streams = [b for b in range(self.B) if not flags[b]]
        rows = kitti_rows(host, keep, transforms, obj_type, streams)
        for b in streams:
            if host["box_flags"][b]:
                warnings.warn(_boxes.flag_message(b, int(host["box_flags"][b]), self.R))
        return [vod_io.write_kitti_tracks(kitti_path(root, names, seq), rows[seq]) for seq in sorted(rows)]

    def frames(self, b, threshold=None, min_hits=1, min_track_frames=1):
        """[(seq, index, [(track id, conf, points (n,3) float64), ...]), ...] of stream b: per logged frame what
        vod_io.read_track_results returns for its file."""
        host, keep, _ = self.download(self._selected(threshold, min_hits, min_track_frames))
        return host_frames(host, b, keep)

    def check(self):
        """Raises RuntimeError naming the stream for any sticky flag (a frame that was refused)."""
        raise_on_flags(self.flags.cpu().tolist(), self.K)

    def clear(self):
        """Zeroes cursors and flags: the log is empty (what lies behind the cursors is never read)."""
        self.cursor.zero_()
        self.flags.zero_()
        self.hits_logged = True
