"""Shared by tests/test_gt_device_cpu.py and tests/test_gt_device_gpu.py: the shipped radar frames as `pack_boxes` streams, the
seeded synthetic batch, and the host references (vod_gt / metrics run per stream on the valid slice)."""
import os
import types

import numpy as np
import torch

from _util import GOLDEN
from ratrack_amd import vod_gt, vod_io

EX = os.path.join(GOLDEN, "vod_example")
REAL_PAIRS = [("01047", "01201"), ("00549", "01047"), ("01201", "00549")]      # (later = frame 1, earlier = frame 2)


def tf_of(f):
    return vod_gt.FrameTransforms(os.path.join(EX, "radar_calib_%s.txt" % f), os.path.join(EX, "lidar_calib_%s.txt" % f),
                                  os.path.join(EX, "pose_%s.json" % f))


def moving_labels(f):
    det = open(os.path.join(EX, "label_%s.txt" % f)).read().splitlines()
    tracking = []
    for i, line in enumerate(det):
        t = line.split(" ")
        tracking.append(" ".join([t[0], str(i)] + t[2:15]))
    return vod_gt.filter_moving_labels(det, vod_gt.parse_tracking_labels(tracking))


def scan_of(f):
    return vod_io.load_radar_bin(os.path.join(EX, "radar_%s.bin" % f))


def real_streams():
    """-> (per_stream for pack_boxes, [frame_pair_tensors], [ego 4x4]) of REAL_PAIRS."""
    per_stream, pairs, egos = [], [], []
    for later, earlier in REAL_PAIRS:
        tf1, tf2 = tf_of(later), tf_of(earlier)
        ego = vod_gt.ego_motion(tf1, tf2)
        per_stream.append((moving_labels(later), tf1, moving_labels(earlier), tf2, ego))
        pairs.append(vod_io.frame_pair_tensors(scan_of(later), scan_of(earlier)))
        egos.append(ego)
    return per_stream, pairs, egos


# ---- the synthetic batch ---------------------------------------------------------------------------------------------------
IDENTITY_TF = types.SimpleNamespace(t_radar_camera=np.eye(4), t_radar_lidar=np.eye(4))      # camera frame = radar frame


def _label(obj_id, x, y, z, l, w, h, ry):
    return vod_gt.Label("Car", obj_id, 0, 0, 0, 0, 0, 0, float(h), float(w), float(l), float(x), float(y), float(z), float(ry))


def synthetic_batch(B=64, N=256, K=32, seed=20240607):
    """Seeded.  Per stream: clouds of n1, n2 <= N valid points (padded with copies of point 0), up to K boxes per frame.  Contains
    overlapping boxes, boxes whose partner in frame 2 is empty, boxes without a partner, ids in frame 2 only, streams with no box
    (empty dicts and None), and padded streams whose point 0 (hence every padding column) lies inside a box.
    -> dict(per_stream, pc1, pc2 (B,3,N) float32 numpy, n_valid (2,B) int32, ego [4x4])."""
    rng = np.random.default_rng(seed)
    per_stream, egos = [], []
    pc1 = np.zeros((B, 3, N), dtype=np.float32)
    pc2 = np.zeros((B, 3, N), dtype=np.float32)
    n_valid = np.zeros((2, B), dtype=np.int32)

    def cloud(n):
        p = np.stack([rng.uniform(-20, 20, n), rng.uniform(-20, 20, n), rng.uniform(-2, 2, n)]).astype(np.float32)
        return p

    for b in range(B):
        n1 = N if b % 4 == 0 else int(rng.integers(60, N))
        n2 = N if b % 4 == 1 else int(rng.integers(60, N + 1))
        a, c = cloud(n1), cloud(n2)
        kind = b % 8
        nbox = 0 if kind in (5, 6) else (K if b % 16 == 0 else int(rng.integers(3, K + 1)))
        labels1, labels2 = {}, {}
        for k in range(nbox):
            obj_id = 100 + 3 * k
            if k % 5 == 1 and k > 0:          # overlaps the previous box: same place, a little shifted
                prev = labels1[100 + 3 * (k - 1)]
                x, y, z = prev.x + rng.uniform(-0.5, 0.5), prev.y + rng.uniform(-0.5, 0.5), prev.z
            else:
                x, y, z = rng.uniform(-18, 18), rng.uniform(-18, 18), rng.uniform(-1, 1)
            l, w, h, ry = rng.uniform(3, 9), rng.uniform(2, 6), rng.uniform(1.5, 4), rng.uniform(-np.pi, np.pi)
            labels1[obj_id] = _label(obj_id, x, y, z, l, w, h, ry)
            if k % 7 == 3:
                continue                      # no partner in frame 2
            if k % 7 == 5:                    # the partner exists but holds no point of frame 2
                labels2[obj_id] = _label(obj_id, 500.0 + k, 500.0, 0.0, l, w, h, ry + 0.1)
            else:
                labels2[obj_id] = _label(obj_id, x + rng.uniform(-1, 1), y + rng.uniform(-1, 1), z, l, w, h, ry + rng.uniform(-0.2, 0.2))
        for k in range(min(nbox // 4, K - len(labels2))):      # ids of frame 2 only, listed between the partners below
            labels2[7000 + k] = _label(7000 + k, rng.uniform(-18, 18), rng.uniform(-18, 18), 0.0, 5.0, 3.0, 2.0, rng.uniform(-3, 3))
        if nbox:
            labels2 = dict(sorted(labels2.items(), key=lambda kv: (kv[0] * 7919) % 101))      # frame 2 lists them in another order
        if kind == 3 and nbox:                # point 0 inside box 0 of a padded stream
            first = next(iter(labels1.values()))
            a[:, 0] = np.array([first.x + 0.25, first.y - 0.25, first.z + 0.125], dtype=np.float32)
            n1 = min(n1, N - 17)
            a = a[:, :n1]
        pc1[b, :, :n1], pc1[b, :, n1:] = a, a[:, :1]
        pc2[b, :, :n2], pc2[b, :, n2:] = c, c[:, :1]
        n_valid[:, b] = (n1, n2)
        ang = rng.uniform(-0.05, 0.05)
        ego = np.eye(4)
        ego[:3, :3] = vod_gt.rot_z(ang)
        ego[:3, 3] = rng.uniform(-1, 1, 3)
        egos.append(ego)
        per_stream.append(None if kind == 6 else (labels1, IDENTITY_TF, labels2, IDENTITY_TF, ego))
    return dict(per_stream=per_stream, pc1=pc1, pc2=pc2, n_valid=n_valid, ego=egos)


def face_margin(per_stream, pc1, pc2, n_valid):
    """The smallest | |(p - c) . axis_k| - half_k | over every (stream, frame, box, valid point, axis), float64 on the host."""
    best = np.inf
    for b, item in enumerate(per_stream):
        if item is None:
            continue
        for labels, tf, pc, n in ((item[0], item[1], pc1[b], n_valid[0, b]), (item[2], item[3], pc2[b], n_valid[1, b])):
            pts = np.asarray(pc, dtype=np.float64)[:, :n].T
            for lab in labels.values():
                box = vod_gt.box_in_radar_frame(lab, tf)
                proj = (pts - box.center) @ box.R
                best = min(best, float(np.abs(np.abs(proj) - box.extent / 2).min()))
    return best


def host_ground_truth(item, pc1_b, pc2_b, n1, n2, ego):
    """The host path on one stream's valid slice: vod_gt.filter_object_points on both frames, vod_io.compensate_ego_motion,
    vod_gt.gt_scene_flow.  -> dict of numpy arrays over the n1 valid points (+ per-box counts by label id)."""
    a = torch.from_numpy(np.ascontiguousarray(pc1_b[:, :n1])).unsqueeze(0)
    c = torch.from_numpy(np.ascontiguousarray(pc2_b[:, :n2])).unsqueeze(0)
    labels1, tf1, labels2, tf2 = item[:4] if item is not None else ({}, IDENTITY_TF, {}, IDENTITY_TF)
    r1 = vod_gt.filter_object_points(2, labels1, a, tf1)
    r2 = vod_gt.filter_object_points(2, labels2, c, tf2)
    comp64 = vod_io.compensate_ego_motion(a[0].numpy().T, ego)[:, :3].T if ego is not None else a[0].numpy().astype(np.float64)
    comp = torch.from_numpy(np.ascontiguousarray(comp64.astype(np.float32))).unsqueeze(0)
    gt = vod_gt.gt_scene_flow(r2[4], r1[1], r1[5], a, comp, r1[6], r2[6])
    return dict(cls=r1[1].numpy(), obj_id=r1[5].numpy(), gt=gt[0].numpy(), comp=comp[0].numpy(), comp64=comp64,
                counts1={k: len(v) for k, v in r1[3].items()}, counts2={k: len(v) for k, v in r2[3].items()},
                boxes1=r1[6], boxes2=r2[6], moving_ids=set(r2[4].keys()))
