"""Shared by tests/test_track_score_cpu.py and tests/test_track_score_gpu.py: the host statement of ratrack_amd/track_score.py
(vod_gt.filter_object_points, vod_gt.map_gt_objects, the target list of loss.affinity_loss, a counter loop written from the
definitions in include/rtk_score.h), run per stream on the valid slice, and the seeded synthetic sequence with its census of the
situations it has to contain."""
import functools
import random

import numpy as np
import torch

import _gt_util as U
from ratrack_amd import vod_gt

Q = 1.0 / 64           # every coordinate is a multiple of Q (exact in fp32): two points are bit-identical or at least Q apart
MIN_PTS = 2
_RNG = random.Random(1)      # map_gt_objects' negative keys of unmatched detections: one generator, so that no two calls repeat a key
COUNTERS = ("frames", "gt", "pred", "tp", "fp", "fn", "idsw", "tracks", "mt", "pt", "ml")


# ---- host path, one stream and frame ---------------------------------------------------------------------------------------------
def host_gt_objects(item, pc_b, n, min_pts=MIN_PTS):
    """vod_gt.filter_object_points on the stream's valid slice -> its 10-tuple (elements 7..9: objs_combined, idx, centres)."""
    a = torch.from_numpy(np.ascontiguousarray(pc_b[:, :n])).unsqueeze(0)
    labels, tf = (item[0], item[1]) if item is not None else ({}, U.IDENTITY_TF)
    return vod_gt.filter_object_points(min_pts, labels, a, tf)


def objects_dict(pc_b, obj_b, ids_b, num):
    """The `objects` of StepResult.objects from obj / object_ids: {track id: (1,6,n_i)} in association order, points in column
    order, rows 3:6 the un-warped coordinates (all map_gt_objects reads)."""
    out = {}
    for i in range(num):
        cols = np.nonzero(obj_b == i)[0]
        xyz = torch.from_numpy(np.ascontiguousarray(pc_b[:, cols]))
        out[int(ids_b[i])] = torch.cat((xyz, xyz), dim=0).unsqueeze(0)
    assert len(out) == num, "track ids of one frame must be distinct"
    return out


def host_match(r, objects):
    """vod_gt.map_gt_objects -> (the mapping as loss.affinity_loss takes it, per detection: label id or -1, float64 IoU or 0)."""
    mapping, _ = vod_gt.map_gt_objects(r[9], r[7], objects, rng=_RNG)
    keys = list(mapping.keys())
    gt_id, iou = [], []
    for key, (track, pts) in zip(keys, objects.items()):
        assert mapping[key] == track
        gt_id.append(key if key >= 0 else -1)
        iou.append(float(vod_gt.iou_points(pts[0].numpy().T, r[7][key][0].numpy().T)) if key >= 0 else 0.0)
    if not keys:
        gt_id, iou = [-1] * len(objects), [0.0] * len(objects)
    return mapping, gt_id, iou


def host_target(mapping_prev, mapping_curr):
    """The target of loss.affinity_loss (loss.py:44), or None where that loss is 0 by definition."""
    if len(mapping_prev) == 0 or len(mapping_curr) == 0:
        return None
    prev, curr = list(mapping_prev.keys()), list(mapping_curr.keys())
    gt = torch.tensor([1.0 if m == n else 0.0 for m in prev for n in curr])
    return gt.reshape(len(prev), len(curr)).numpy()


class HostScorer:
    """The counters of include/rtk_score.h for one stream, from the definitions."""

    def __init__(self):
        self.c = dict.fromkeys(COUNTERS, 0)
        self.iou_sum = 0.0
        self.table = {}           # label id -> [last matched track id or None, frames seen, frames matched]
        self.prev = None          # the mapping of the last active frame

    @staticmethod
    def classify(entries):
        mt = sum(1 for _, seen, matched in entries if matched / seen > 0.8)
        ml = sum(1 for _, seen, matched in entries if matched / seen < 0.2)
        return len(entries), mt, len(entries) - mt - ml, ml

    def close(self):
        for k, v in zip(("tracks", "mt", "pt", "ml"), self.classify(list(self.table.values()))):
            self.c[k] += v
        self.table = {}
        self.prev = None

    def frame(self, gt_labels, track_ids, gt_id, iou, mapping, reset):
        """gt_labels: kept label ids; per detection its track id, matched label id (-1) and IoU.  -> (target or None, switches)."""
        if reset:
            self.close()
        c = self.c
        matched = {g: t for g, t in zip(gt_id, track_ids) if g >= 0}
        M = len(matched)
        c["frames"] += 1
        c["gt"] += len(gt_labels)
        c["pred"] += len(track_ids)
        c["tp"] += M
        c["fp"] += len(track_ids) - M
        c["fn"] += len(gt_labels) - M
        for g, v in zip(gt_id, iou):
            if g >= 0:
                self.iou_sum += v
        sw = 0
        for lab in gt_labels:
            if lab not in self.table:
                self.table[lab] = [None, 0, 0]
            e = self.table[lab]
            e[1] += 1
            if lab in matched:
                if e[0] is not None and e[0] != matched[lab]:
                    sw += 1
                e[0] = matched[lab]
                e[2] += 1
        c["idsw"] += sw
        target = host_target(self.prev, mapping) if self.prev is not None else None
        self.prev = mapping
        return target, sw

    def final(self):
        """Counters with the still-open tracks classified (TrackScorer.result)."""
        out = dict(self.c)
        for k, v in zip(("tracks", "mt", "pt", "ml"), self.classify(list(self.table.values()))):
            out[k] += v
        return out


# ---- the synthetic sequence --------------------------------------------------------------------------------------------------------
def _label(kind, obj_id, c, ry):
    return vod_gt.Label(kind, obj_id, 0, 0, 0, 0, 0, 0, 2.0, 2.0, 2.0, float(c[0]), float(c[1]), float(c[2]), float(ry))


def _q(a):
    return np.round(np.asarray(a, dtype=np.float64) / Q) * Q + 0.0        # + 0.0: no -0.0


def _local_points(rng, k):
    """k distinct offsets inside 0.8 of a 2 m box's half extents, multiples of Q."""
    pts = set()
    while len(pts) < k:
        pts.add(tuple(int(v) for v in rng.integers(-51, 52, 3)))
    return np.array(sorted(pts), dtype=np.float64) * Q


# spec of one ground-truth object: kind, id, start offset from the stream's origin, points, rotation, plan
#   plan: "mt" always detected exactly | "ml" never detected | "mix" a cycle of exact / drop / add / split / gap | "merge": detected
#   together with the next object as ONE detection | "sw": exact, the track id changes at frame 5 and 9
def _scene(kind):
    car, rider = "Car", "rider"
    if kind == 0:      # plain: an overlapping pair, a rotated car, a one-point box, a car that is never detected
        return [(car, 3, (0, 0, 0), 8, 0, "sw"), (car, 7, (1.0, 0, 0), 8, 0, "mix"), (car, 5, (8, 0, 0), 9, 0.3, "mt"),
                (car, 9, (16, 0, 0), 1, 0, "ml"), (car, 11, (24, 0, 0), 7, 0, "ml")]
    if kind == 1:      # rider + bicycle sharing points (and a duplicated point), a car
        return [("Cyclist", 4, (0, 0, 0), 8, 0, "mt"), (rider, 2, (0.5, 0, 0), 6, 0, "mix"), (car, 6, (12, 0, 0), 8, 0, "mix")]
    if kind == 2:      # two riders into one target
        return [(rider, 8, (-2.5, 0, 0), 5, 0, "mix"), ("Cyclist", 1, (0, 0, 0), 7, 0, "sw"), (rider, 12, (2.5, 0, 0), 5, 0, "mt"),
                (car, 6, (14, 0, 0), 8, 0, "mix")]
    if kind == 3:      # a rider merged into a rider (both go), a car far away
        return [(rider, 21, (0, 0, 0), 6, 0, "mix"), (rider, 20, (2.5, 0, 0), 6, 0, "mix"), (car, 22, (20, 0, 0), 8, 0, "mt")]
    if kind == 4:      # a rider alone
        return [(rider, 30, (0, 0, 0), 8, 0.3, "mix")]
    if kind == 5:      # no labels at all
        return None
    if kind == 6:      # two cars of equal size detected as one (an exact IoU tie), a split car
        return [(car, 40, (0, 0, 0), 8, 0, "merge"), (car, 41, (4, 0, 0), 8, 0, "merged"), (car, 42, (12, 0, 0), 10, 0, "split")]
    return [(car, 50, (0, 0, 0), 8, 0, "mix"), (car, 51, (6, 0, 0), 8, 0.3, "sw"), (rider, 52, (6.5, 1.0, 0), 4, 0, "mt"),
            (car, 53, (14, 0, 0), 6, 0, "ml")]


_MIX = ("exact", "drop", "add", "exact", "split", "gap", "exact")


@functools.lru_cache(maxsize=4)
def synthetic_sequence(B=64, N=256, K=32, frames=12, seed=20250117):
    """Seeded.  -> dict(frames=[per frame: per_stream, pc1 (B,3,N) float32, n_valid (B), obj (B,N) int32, num (B), ids (B,K) int32,
    active (B), reset (B)], B, N, K).  Ground truth: persistent label ids on boxes that move a little every frame (their points move
    with them); detections are made from the ground-truth point sets (exact, a point dropped, clutter added, split in two, two
    merged into one), plus spurious clusters of clutter; track ids with planned switches and gaps; padded and None streams; a
    changing `active` mask; a reset at frame 0 and, for a third of the streams, at frame 6."""
    rng = np.random.default_rng(seed)
    scenes = []
    for b in range(B):
        spec = _scene(b % 8)
        origin = _q([rng.integers(0, 10), rng.integers(-10, 10), 0.0])
        objs = []
        for (kind, oid, off, k, rot, plan) in (spec or []):
            objs.append(dict(kind=kind, id=oid, off=np.array(off, dtype=np.float64), local=_local_points(rng, k), rot=rot, plan=plan))
        if b % 8 == 1 and b >= 8:      # the cyclist's first point twice in the cloud
            objs[0]["dup"] = True
        clutter = set()
        while len(clutter) < N:
            clutter.add((int(rng.integers(-4000, -2000)), int(rng.integers(-1000, 1000)), int(rng.integers(-64, 64))))
        scenes.append(dict(origin=origin, objs=objs, clutter=np.array(sorted(clutter), dtype=np.float64) * Q,
                           vel=_q([rng.integers(8, 40) * Q, rng.integers(-16, 16) * Q, 0.0])))
    out = []
    for f in range(frames):
        pc1 = np.zeros((B, 3, N), dtype=np.float32)
        n_valid = np.zeros(B, dtype=np.int32)
        obj = np.full((B, N), -1, dtype=np.int32)
        num = np.zeros(B, dtype=np.int32)
        ids = np.full((B, K), -1, dtype=np.int32)
        active = np.ones(B, dtype=np.uint8)
        reset = np.zeros(B, dtype=np.uint8)
        per_stream = []
        for b, sc in enumerate(scenes):
            active[b] = 0 if (b % 5 == 2 and f in (3, 4)) or (b % 7 == 3 and f % 4 == 1) else 1
            reset[b] = 1 if f == 0 or (f == 6 and b % 3 == 0) else 0
            cols, labels, members = [], {}, []
            for o in sc["objs"]:
                centre = sc["origin"] + o["off"] + f * sc["vel"]              # a multiple of Q; the box centre is half a Q further
                rz = vod_gt.rot_z(o["rot"])
                pts = _q(centre + o["local"] @ rz.T)
                if o.get("dup"):
                    pts = np.concatenate([pts, pts[:1]])
                labels[o["id"]] = _label(o["kind"], o["id"], centre + Q / 2, -(o["rot"] + np.pi / 2))
                members.append(list(range(len(cols), len(cols) + len(pts))))
                cols += [tuple(p) for p in pts]
            # points of different objects may coincide (overlapping boxes): that is allowed, they are bit-identical
            nobj = len(cols)
            fill = N - nobj if b % 4 == 0 else 40 + (b * 7 + f) % 30
            cl = sc["clutter"][:fill]
            pts = np.concatenate([np.array(cols, dtype=np.float64).reshape(-1, 3), cl])
            perm = rng.permutation(len(pts))                                   # objects are not contiguous runs of columns
            where = np.empty(len(pts), dtype=np.int64)
            where[perm] = np.arange(len(pts))
            n = len(pts)
            pc1[b, :, :n] = pts[perm].T.astype(np.float32)
            pc1[b, :, n:] = pc1[b, :, :1]
            n_valid[b] = n
            per_stream.append(None if sc["objs"] == [] and b % 16 == 5 else (labels, U.IDENTITY_TF, labels, U.IDENTITY_TF))
            # ---- detections ----
            preds, taken = [], set()
            clutter_cols = [int(where[nobj + i]) for i in range(len(cl))]
            nxt = iter(clutter_cols)

            def own(i):
                c = [int(where[m]) for m in members[i] if int(where[m]) not in taken]
                taken.update(c)
                return c
            for i, o in enumerate(sc["objs"]):
                plan, tid = o["plan"], 10 + o["id"]
                mode = plan if plan not in ("mix", "sw", "mt", "ml") else {"mt": "exact", "ml": "gap", "sw": "exact"}.get(plan)
                if plan == "mix":
                    mode = _MIX[(i * 3 + f * 2 + b) % len(_MIX)]
                if plan == "sw":
                    tid += 1000 * int(f >= 5) + 1000 * int(f >= 9)
                if mode == "gap" or mode == "merged":
                    continue
                c = own(i)
                if mode == "merge":
                    c += own(i + 1)
                if mode == "drop":
                    c = c[:-1]
                if mode == "add":
                    c += [next(nxt), next(nxt)]
                if mode == "split":
                    h = len(c) // 2
                    preds.append((tid + 500, c[h:]))
                    c = c[:h]
                if c:
                    preds.append((tid, c))
            for s in range((b + f) % 3):                                       # spurious clusters
                preds.append((9000 + 10 * s + f % 2, [next(nxt), next(nxt), next(nxt)]))
            if b % 8 == 4 and f in (2, 7):                                     # no detection at all
                preds = []
            if f % 2:
                preds.reverse()
            preds = [p for p in preds if p[1]]
            for i, (tid, c) in enumerate(preds):
                obj[b, c] = i
                ids[b, i] = tid
            num[b] = len(preds)
        out.append(dict(per_stream=per_stream, pc1=pc1, n_valid=n_valid, obj=obj, num=num, ids=ids, active=active, reset=reset))
    return dict(frames=out, B=B, N=N, K=K)


def input_conditions(seq):
    """The conditions under which the host's fp32 decisions and the kernel's float64 ones coincide, measured on the CPU:
    -> dict(rider_gap: smallest relative gap between a rider's nearest and second nearest centre distance, point_gap: smallest
    non-zero distance between two valid points of a stream, face_margin, negative_zero: count)."""
    rider_gap, point_gap, margin, negz = np.inf, np.inf, np.inf, 0
    for fr in seq["frames"][::3]:
        pc, nv = fr["pc1"], fr["n_valid"]
        negz += int((np.signbit(pc) & (pc == 0)).sum())
        margin = min(margin, U.face_margin(fr["per_stream"], pc, pc, np.stack([nv, nv])))
        for b, item in enumerate(fr["per_stream"]):
            p = pc[b, :, :nv[b]].astype(np.float64).T
            d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))
            if (d > 0).any():
                point_gap = min(point_gap, float(d[d > 0].min()))
            if item is None:
                continue
            r = host_gt_objects(item, pc[b], nv[b])
            centres = {k: v[0].double().numpy() for k, v in r[4].items()}
            for k, c in centres.items():
                if item[0][k].type != "rider" or len(centres) < 3:
                    continue
                ds = sorted(float(np.linalg.norm(c - o)) for j, o in centres.items() if j != k)
                rider_gap = min(rider_gap, (ds[1] - ds[0]) / ds[1])
    return dict(rider_gap=rider_gap, point_gap=point_gap, face_margin=margin, negative_zero=negz)


@functools.lru_cache(maxsize=4)
def host_sequence(B=64, N=256, K=32, frames=12):
    """The host path over `synthetic_sequence`, computed once: -> (per frame {b: dict(r, labels, slots, mapping, gt_id, iou, target,
    defined)}, [HostScorer], census of the situations met)."""
    seq = synthetic_sequence(B, N, K, frames)
    scorers = [HostScorer() for _ in range(B)]
    census = dict.fromkeys(("iou_tie", "same_best", "rider_merged", "rider_alone", "rider_into_rider", "two_riders_one_target",
                            "min_size", "merged_duplicates", "shared_point", "g0_p", "p0_g", "idsw", "mt", "ml", "defined0", "defined1"), 0)
    ref = []
    for fr in seq["frames"]:
        row = {}
        for b in range(B):
            if not fr["active"][b]:
                continue
            item, n = fr["per_stream"][b], int(fr["n_valid"][b])
            r = host_gt_objects(item, fr["pc1"][b], n)
            objects = objects_dict(fr["pc1"][b], fr["obj"][b, :n], fr["ids"][b], int(fr["num"][b]))
            mapping, gt_id, iou = host_match(r, objects)
            labels = list(r[7].keys())
            target, sw = scorers[b].frame(labels, list(objects.keys()), gt_id, iou, mapping, bool(fr["reset"][b]))
            row[b] = dict(r=r, labels=labels, mapping=mapping, gt_id=gt_id, iou=iou, target=target, tracks=list(objects.keys()))
            _census(census, item, r, objects, sw, target)
        ref.append(row)
    for s in scorers:
        fin = s.final()
        census["mt"] += fin["mt"]
        census["ml"] += fin["ml"]
    return ref, scorers, census


def _census(census, item, r, objects, sw, target):
    objs, centres, kept = r[2], r[4], r[7]
    labels = item[0] if item is not None else {}
    census["idsw"] += sw
    census["defined1" if target is not None else "defined0"] += 1
    census["g0_p"] += int(len(kept) == 0 and len(objects) > 0)
    census["p0_g"] += int(len(kept) > 0 and len(objects) == 0)
    idx = [set(v.tolist()) for v in r[3].values()]
    census["shared_point"] += sum(len(a & b) for i, a in enumerate(idx) for b in idx[i + 1:])
    # the rider loop, restated to see which of its branches ran
    targets, dropped, pairs = [], set(), []
    for k, c in centres.items():
        if labels[k].type != "rider":
            continue
        others = [(float((c - o).pow(2).sum().sqrt()), j) for j, o in centres.items() if j != k]
        if not others:
            census["rider_alone"] += 1
            continue
        near = min(others, key=lambda t: t[0])[1]
        census["rider_merged"] += 1
        census["rider_into_rider"] += int(labels[near].type == "rider")
        targets.append(near)
        pairs.append((k, near))
        dropped.add(k)
    census["two_riders_one_target"] += sum(1 for t in set(targets) if targets.count(t) > 1)
    for t in set(targets) - dropped:
        columns = set(r[3][t].tolist()).union(*[set(r[3][k].tolist()) for k, tt in pairs if tt == t])
        census["merged_duplicates"] += int(objs[t].size(2) < len(columns))      # distinct columns with one coordinate triple
    census["min_size"] += sum(1 for k, o in objs.items() if k not in dropped and o.size(2) < MIN_PTS)
    best = []
    for pts in objects.values():
        ious = [vod_gt.iou_points(pts[0].numpy().T, g[0].numpy().T) for g in kept.values()]
        top = max(ious) if ious else 0
        if top > 0:
            census["iou_tie"] += int(ious.count(top) > 1)
            best.append(ious.index(top))
    census["same_best"] += sum(1 for j in set(best) if best.count(j) > 1)
