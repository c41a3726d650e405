"""A host statement of the result log (include/rtk_fused.h, "The result log"): plain numpy / Python loops written from the rules --
append (the stable grouping, the refusals, the flags), select (float64 sums in log order) and the text of a result file.  The tests
compare the kernels and ratrack_amd.result_log's host half with it, bit for bit."""
import os

import numpy as np

FLAG_OBJECTS, FLAG_STEP, FLAG_FULL, FLAG_TRACKS = 1, 2, 4, 8
TRACKS = 2048
TABLES = ("cursor", "frame", "tag", "rec_track", "rec_conf", "rec_hits", "rec_size", "points", "flags")
POISON = 0x5a5a5a5a       # a word no append writes in these tests (as fp32: 1.5e16)


class HostLog:
    """The log's tensors as numpy arrays of the device's shapes and dtypes.  poison: every word but cursors and flags starts as POISON
    instead of 0, so that a word an append should not have touched is told from one it wrote."""

    def __init__(self, streams, max_objects, frames, records, points, poison=False):
        self.B, self.K, self.F, self.R, self.P = streams, max_objects, frames, records, points
        B, fill = streams, (POISON if poison else 0)
        word = lambda *s: np.full(s, fill, dtype=np.int32)
        self.cursor, self.flags = np.zeros((B, 4), np.int32), np.zeros(B, np.int32)
        self.frame, self.tag = word(B, frames, 4), word(B, frames, 4)
        self.rec_track, self.rec_hits, self.rec_size = word(B, records), word(B, records), word(B, records)
        self.rec_conf = word(B, records).view(np.float32)
        self.points = word(B, points, 3).view(np.float32)

    def tables(self):
        return {n: getattr(self, n) for n in TABLES}

    def append(self, pc1, obj, num_objects, object_ids, object_conf, seq, index, object_hits=None, step_flags=None, reset=None, active=None):
        """pc1 (B,3,N) fp32, obj (B,N), num_objects (B), object_ids / object_conf (B,K), seq / index (B): one frame per active stream."""
        for b in range(self.B):
            if active is not None and not active[b]:
                continue
            pf, sf = int(num_objects[b]), 0 if step_flags is None else int(step_flags[b])
            bad = (FLAG_OBJECTS if (pf < 0 or pf > self.K) else 0) | (FLAG_STEP if sf & 3 else 0)
            if bad:
                self.flags[b] |= bad
                continue
            members = [[] for _ in range(pf)]
            for p, o in enumerate(obj[b].tolist()):
                if 0 <= o < pf:
                    members[o].append(p)
            total = sum(len(m) for m in members)
            cf, cr, cp = (int(v) for v in self.cursor[b, :3])
            if cf + 1 > self.F or cr + pf > self.R or cp + total > self.P:
                self.flags[b] |= FLAG_FULL
                continue
            at = cp
            for j in range(pf):
                self.rec_track[b, cr + j] = object_ids[b, j]
                self.rec_conf[b, cr + j] = object_conf[b, j]
                self.rec_hits[b, cr + j] = 0 if object_hits is None else object_hits[b, j]
                self.rec_size[b, cr + j] = len(members[j])
                for p in members[j]:
                    self.points[b, at] = pc1[b, :, p]
                    at += 1
            mark = 65536 if (reset is not None and reset[b]) else 0
            self.frame[b, cf] = (cr, cp, pf + mark, 0)
            self.tag[b, cf] = (int(seq[b]), int(index[b]), total, sf)
            self.cursor[b, :3] = (cf + 1, cr + pf, cp + total)


def clips(frame_words):
    """The logged frames [(first record, objects, mark)] of one stream -> [[frame slot, ...], ...]: a clip is a maximal run of frames in
    which only the first may carry the mark."""
    out = []
    for f, (_, _, mark) in enumerate(frame_words):
        if f == 0 or mark:
            out.append([])
        out[-1].append(f)
    return out


def select(tables, threshold=None, min_hits=1, min_track_frames=1):
    """-> keep (B,R) uint8, track_score (B,R) float64, track_frames (B,R) int32, flags (B) int32; zeros where nothing is written."""
    B, R = tables["rec_track"].shape
    keep, score, length = np.zeros((B, R), np.uint8), np.zeros((B, R), np.float64), np.zeros((B, R), np.int32)
    flags = np.zeros(B, np.int32)
    tau = float("-inf") if threshold is None else float(threshold)
    for b in range(B):
        words = [(int(w[0]), int(w[2]) & 0xffff, (int(w[2]) >> 16) & 1) for w in tables["frame"][b, :int(tables["cursor"][b, 0])]]
        for clip in clips(words):
            recs = [r for f in clip for r in range(words[f][0], words[f][0] + words[f][1])]      # log order
            sums, counts = {}, {}
            for r in recs:
                t = int(tables["rec_track"][b, r])
                sums[t] = sums.get(t, np.float64(0.0)) + np.float64(tables["rec_conf"][b, r])
                counts[t] = counts.get(t, 0) + 1
            if len(sums) > TRACKS:
                flags[b] |= FLAG_TRACKS
            if flags[b]:
                continue                      # this clip and the later ones are not written
            for r in recs:
                t = int(tables["rec_track"][b, r])
                s = sums[t] / np.float64(counts[t])
                score[b, r], length[b, r] = s, counts[t]
                hits = min_hits <= 1 or tables["rec_hits"][b, r] >= min_hits      # (1 asks nothing: a frame without hit counts holds 0)
                keep[b, r] = (not (s < tau)) and hits and counts[t] >= min_track_frames
    return keep, score, length, flags


def file_texts(tables, keep=None):
    """{(seq, index): the text of the frame's result file}: per kept record `NA 1 -1 -1 conf id x y z ...`, every number str(float(x))
    of the fp32 value (vod_io.format_track_line)."""
    out = {}
    for b in range(tables["cursor"].shape[0]):
        for f in range(int(tables["cursor"][b, 0])):
            rec, at, word, _ = (int(v) for v in tables["frame"][b, f])
            text = ""
            for r in range(rec, rec + (word & 0xffff)):
                n = int(tables["rec_size"][b, r])
                if keep is None or keep[b, r]:
                    parts = ["NA", "1", "-1", "-1", str(float(tables["rec_conf"][b, r])), str(int(tables["rec_track"][b, r]))]
                    for q in range(at, at + n):
                        parts += [str(float(v)) for v in tables["points"][b, q]]
                    text += " ".join(parts) + "\n"
                at += n
            out[(int(tables["tag"][b, f, 0]), int(tables["tag"][b, f, 1]))] = text
    return out


def pack_frames(frames, max_objects=None):
    """[(seq, index, [(track id, conf, points (n,3)), ...]), ...] -> the tables of a one-stream host log holding exactly these frames
    (every frame goes through HostLog.append as a cloud whose columns are the objects' points in file order)."""
    objs = max([len(o) for _, _, o in frames] + [1])
    pts = max([sum(len(p) for _, _, p in o) for _, _, o in frames] + [1])
    K = max_objects or objs
    log = HostLog(1, K, len(frames), objs * len(frames), pts * len(frames))
    for seq, index, objects in frames:
        xyz = np.zeros((1, 3, pts), np.float32)
        obj = np.full((1, pts), -1, np.int32)
        ids, conf = np.zeros((1, K), np.int32), np.zeros((1, K), np.float32)
        at = 0
        for j, (tid, c, p) in enumerate(objects):
            ids[0, j], conf[0, j] = tid, c
            xyz[0, :, at:at + len(p)] = np.asarray(p, np.float32).reshape(-1, 3).T
            obj[0, at:at + len(p)] = j
            at += len(p)
        log.append(xyz, obj, [len(objects)], ids, conf, [seq], [index])
    return log.tables()


def read_tree(root):
    """{relative path: bytes} of every file under root."""
    out = {}
    for d, _, files in os.walk(root):
        for n in files:
            p = os.path.join(d, n)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out
