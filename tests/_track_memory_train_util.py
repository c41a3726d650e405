"""Shared by tests/test_track_memory_train_cpu.py and tests/test_track_memory_train_gpu.py: the host statement of the record that
rtk_track_score_memory keeps (include/rtk_score.h) -- plain Python over lists, written from the rules in the header -- and the scenes
of the tests that know their answer by construction.  No GPU is needed to import this module."""
import torch

import _gt_util as GU
import _track_memory_util as U
from ratrack_amd import vod_gt

FLAG_TABLE = 64


# ---- the host statement -------------------------------------------------------------------------------------------------------------
def empty_record():
    """One stream's record before its first frame (prev_count = -1)."""
    return dict(count=-1, track=[], label=[], gt=0, labelled=0)


def host_score_memory(rec, object_ids, det_labels, G, table_ids, table_count, K, reset=False, active=True):
    """One frame of one stream.  rec: its record (`empty_record`'s keys; track / label: one entry per row).  object_ids: the track ids
    of this frame's P detections, det_labels their matched label ids (-1: unmatched), G its kept ground-truth objects; table_ids
    (K-long) and table_count: the tracker's NEW table.
    -> (new record, target (K x K nested lists of 0 / 1), aff_defined, flag: RTK_SCORE_FLAG_TABLE or 0)."""
    zeros = [[0] * K for _ in range(K)]
    if not active:
        return rec, zeros, 0, 0
    if reset:
        rec = empty_record()
    P = len(det_labels)
    assert len(object_ids) == P <= K
    target = [[1 if i < len(rec["label"]) and j < P and rec["label"][i] >= 0 and rec["label"][i] == det_labels[j] else 0
               for j in range(K)] for i in range(K)]
    defined = int(rec["count"] > 0 and P > 0 and G > 0 and (rec["gt"] > 0 or rec["labelled"] > 0))
    R = max(min(max(table_count, 0), K), P)
    track, label = list(object_ids), list(det_labels)
    for r in range(P, R):
        found = [i for i in range(len(rec["track"])) if rec["track"][i] == table_ids[r]]
        track.append(table_ids[r])
        label.append(rec["label"][found[0]] if found else -1)
    new = dict(count=R, track=track, label=label, gt=G, labelled=sum(1 for v in label[P:] if v >= 0))
    return new, target, defined, (FLAG_TABLE if R != table_count else 0)


def ones(target):
    """[(i, j)] of the target's ones."""
    return [(i, j) for i, row in enumerate(target) for j, v in enumerate(row) if v]


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
def car_labels(centres, count=None):
    """One `Car` label per object (label id = its index), its 3 x 4 x 6 box around the object's centre -> the per-stream item of
    `gt_device.pack_boxes` with identity transforms (the pattern of tests/test_track_memory_gpu.py `scored`)."""
    c = torch.as_tensor(centres, dtype=torch.float32).tolist()
    count = len(c) if count is None else count
    labels = {k: vod_gt.Label("Car", k, 0, 0, 0, 0, 0, 0, 3.0, 4.0, 6.0, c[k][0], c[k][1], c[k][2], 0.0) for k in range(count)}
    return (labels, GU.IDENTITY_TF, labels, GU.IDENTITY_TF)


def scenario_centres(t, count=3):
    """The centres of tests/test_track_memory_gpu.py `scenario` at frame t: a lattice moving 0.2 m per frame along x."""
    return U.lattice(count) + torch.tensor([0.2 * t, 0.0, 0.0])


def scenario(g, frames=None):
    """`scenario(g)` of tests/test_track_memory_gpu.py with its boxes: three objects moving 0.2 m per frame; object A (index 0) is
    hidden in frames 2 .. 2 + g - 1 and back in frame 2 + g.  -> [(blob_stream dict, per-stream item)] per frame."""
    total = 2 + g + 2 if frames is None else frames
    out = []
    for t in range(total):
        visible = [not 2 <= t < 2 + g, True, True]
        c = scenario_centres(t)
        out.append((U.blob_stream(c, visible, 32, points=3, seed=100 + t), car_labels(c)))
    return out


def single_object(frames=4, hidden=(1,), unlabelled=()):
    """One object alone in its scene, hidden in the frames of `hidden`; the frames of `unlabelled` carry no label at all (None)."""
    out = []
    for t in range(frames):
        c = scenario_centres(t, 1)
        out.append((U.blob_stream(c, [t not in hidden], 32, points=3, seed=400 + t), None if t in unlabelled else car_labels(c)))
    return out


def duplicate_label():
    """Object A (index 0) of three: seen in frames 0 and 1, hidden in frame 2, back in frame 3 displaced by 3 m along y -- under
    `distance_affinity(4, 4)` its affinity to its coasting track is below sigmoid(4 - 12) = 3e-4, and below 0.01 the association hands
    out a fresh ID; the box follows it -- and 0.2 m further in frame 4.  Its old track still coasts in frame 3 (max_age = 2)."""
    out = []
    for t in range(5):
        c = scenario_centres(t)
        if t >= 3:
            c[0, 1] += 3.0
        out.append((U.blob_stream(c, [t != 2, True, True], 32, points=3, seed=500 + t), car_labels(c)))
    return out


def with_clutter(centres, visible, N, points, seed, where=(-30.0, -30.0, 0.0)):
    """A `blob_stream` frame with one more object than `centres`, a blob at `where` (outside every box): its columns come after the
    others', so the objects' order is unchanged."""
    c = torch.cat([torch.as_tensor(centres, dtype=torch.float32), torch.tensor([list(where)])])
    return U.blob_stream(c, list(visible) + [True], N, points=points, seed=seed)
