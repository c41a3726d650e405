"""CPU: the host half of the device ground-truth path (ratrack_amd/gt_device.py): `pack_boxes` on the three shipped radar frames
against vod_gt.box_in_radar_frame and gt_scene_flow's motion matrix, the pairing of label ids across frames, the box limit, and the
generator of the synthetic GPU batch (tests/test_gt_device_gpu.py) keeping every point away from every box face."""
import numpy as np
import pytest
import torch

import _gt_util as U
from ratrack_amd import gt_device as G
from ratrack_amd import vod_gt


def test_pack_boxes_tables_are_the_host_paths_boxes_and_motion_bit_for_bit():
    per_stream, pairs, egos = U.real_streams()
    bb = G.pack_boxes(per_stream, max_boxes=16, device="cpu")
    assert bb.B == 3 and bb.K == 16 and bb.boxes.shape == (2, 3, 16, 16) and bb.boxes.dtype == torch.float64
    assert bb.motion.shape == (3, 16, 12) and bb.motion.dtype == torch.float32 and bb.pair.dtype == torch.int32
    # the device views are the host arrays (one buffer, one upload)
    for name in ("boxes", "box_id", "count", "pair", "motion", "ego"):
        assert np.array_equal(getattr(bb, name).numpy(), bb.host[name]), name
        assert getattr(bb, name).untyped_storage().data_ptr() == bb._buffer.untyped_storage().data_ptr(), name
    for b, (labels1, tf1, labels2, tf2, ego) in enumerate(per_stream):
        for f, (labels, tf) in enumerate(((labels1, tf1), (labels2, tf2))):
            assert int(bb.count[f, b]) == len(labels)
            assert bb.box_id[f, b, :len(labels)].tolist() == [lab.id for lab in labels.values()]
            assert (bb.box_id[f, b, len(labels):] == -1).all()
            for k, lab in enumerate(labels.values()):
                box = vod_gt.box_in_radar_frame(lab, tf)
                row = bb.boxes[f, b, k].numpy()
                assert np.array_equal(row[:3], box.center) and np.array_equal(row[3:12].reshape(3, 3), box.R)
                assert np.array_equal(row[12:15], box.extent / 2) and row[15] == 0.0
        boxes1 = {lab.id: vod_gt.box_in_radar_frame(lab, tf1) for lab in labels1.values()}
        boxes2 = {lab.id: vod_gt.box_in_radar_frame(lab, tf2) for lab in labels2.values()}
        ids2 = list(boxes2)
        npaired = 0
        for k, obj_id in enumerate(boxes1):
            if obj_id not in boxes2:
                assert int(bb.pair[b, k]) == -1
                continue
            npaired += 1
            assert int(bb.pair[b, k]) == ids2.index(obj_id)
            # gt_scene_flow's matrix, as it builds it (float64 product, then a float32 tensor)
            t = np.dot(vod_gt.box_transform(boxes2[obj_id]), np.linalg.inv(vod_gt.box_transform(boxes1[obj_id])))
            t32 = torch.tensor(t, dtype=torch.float32).numpy()
            assert np.array_equal(bb.motion[b, k].numpy().view(np.uint32), t32[:3].reshape(-1).view(np.uint32)), (b, k)
        assert npaired >= 1
        # the ego rows are vod_io.compensate_ego_motion's matrix: [x y z 1] . inv(ego^T)
        m = np.linalg.inv(ego.T)
        assert np.array_equal(bb.ego[b].numpy().reshape(3, 4), m.T[:3])


def test_pair_and_count_when_ids_exist_in_one_frame_only():
    L = lambda i, x: U._label(i, x, 0.0, 0.0, 4.0, 2.0, 1.5, 0.3)
    labels1 = {7: L(7, 1.0), 3: L(3, 5.0), 9: L(9, 9.0), 4: L(4, 13.0)}
    labels2 = {5: L(5, 2.0), 9: L(9, 9.5), 7: L(7, 1.5)}
    bb = G.pack_boxes([(labels1, U.IDENTITY_TF, labels2, U.IDENTITY_TF), None, ({}, U.IDENTITY_TF, labels2, U.IDENTITY_TF)], 4, device="cpu")
    assert bb.ego is None and bb.host["ego"] is None
    assert bb.count.tolist() == [[4, 0, 0], [3, 0, 3]]
    assert bb.box_id[0, 0].tolist() == [7, 3, 9, 4] and bb.box_id[1, 0].tolist() == [5, 9, 7, -1]
    assert bb.pair[0].tolist() == [2, -1, 1, -1]
    assert bb.pair[1].tolist() == [-1] * 4 and bb.pair[2].tolist() == [-1] * 4
    assert (bb.motion[0, 1] == 0).all() and (bb.motion[0, 3] == 0).all() and (bb.motion[0, 0] != 0).any()
    # the unpaired rows of a paired stream and every row of an empty stream are zero tables
    assert (bb.boxes[:, 1] == 0).all() and (bb.boxes[0, 2] == 0).all()


def test_more_boxes_than_max_boxes_raises():
    L = lambda i: U._label(i, float(i), 0.0, 0.0, 4.0, 2.0, 1.5, 0.0)
    five = {i: L(i) for i in range(5)}
    with pytest.raises(ValueError, match="stream 1, frame 2: 5 boxes > max_boxes=4"):
        G.pack_boxes([None, ({}, U.IDENTITY_TF, five, U.IDENTITY_TF)], 4, device="cpu")
    G.pack_boxes([(five, U.IDENTITY_TF, five, U.IDENTITY_TF)], 5, device="cpu")
    with pytest.raises(ValueError):
        G.pack_boxes([None], G.MAX_BOXES + 1, device="cpu")


def test_synthetic_batch_keeps_every_point_off_every_face_and_holds_every_case():
    """The GPU test compares membership EXACTLY: the host's BLAS projection and the kernel's written-out one may differ in the last
    bits of a float64, so no point may sit within 1e-9 of a face.  And the batch must really contain the cases it is there for."""
    d = U.synthetic_batch()
    assert U.face_margin(d["per_stream"], d["pc1"], d["pc2"], d["n_valid"]) >= 1e-9
    overlap = fallback_empty = fallback_alone = moved = padded_inside = empty = 0
    for b, item in enumerate(d["per_stream"]):
        n1, n2 = d["n_valid"][:, b]
        h = U.host_ground_truth(item, d["pc1"][b], d["pc2"][b], n1, n2, d["ego"][b])
        if item is None or not item[0]:
            empty += 1
            assert not h["cls"].any()
            continue
        pts = d["pc1"][b].astype(np.float64).T
        inside = np.stack([np.isin(np.arange(len(pts)), vod_gt.points_in_box(bx, pts)) for bx in h["boxes1"].values()])
        overlap += int((inside[:, :n1].sum(0) > 1).sum())
        padded_inside += int(n1 < len(pts) and inside[:, 0].any())
        for obj_id in np.unique(h["obj_id"][h["cls"]]):
            if obj_id not in h["boxes2"]:
                fallback_alone += 1
            elif obj_id not in h["moving_ids"]:
                fallback_empty += 1
            else:
                moved += 1
    assert overlap >= 10 and fallback_empty >= 10 and fallback_alone >= 10 and moved >= 50 and padded_inside >= 3 and empty >= 8, \
        (overlap, fallback_empty, fallback_alone, moved, padded_inside, empty)


def test_values_from_sums_restates_the_host_metrics():
    """gt_device.values_from_sums (the pooled values of MetricAccumulator.result) on hand-made sums against the formulae of
    metrics.eval_scene_flow / eval_motion_seg evaluated by hand."""
    s = np.array([100.0, 25.0, 40.0, 30.0, 20.0, 10.0, 80.0, 60.0, 75.0, 15.0, 70.0, 10.0, 5.0])
    v = dict(zip(G.KEYS, G.values_from_sums(s)))
    assert v["rne"] == 0.4 and v["epe"] == 0.25 and v["sas"] == 0.6 and v["ras"] == 0.75
    assert v["mov_rne"] == 30.0 / (20.0 + 1e-6) and v["stat_rne"] == 0.125 and v["50-50 rne"] == (v["mov_rne"] + 0.125) / 2
    assert abs(v["acc"] - 0.85) < 1e-15 and abs(v["sen"] - 0.75) < 1e-15
    assert abs(v["miou"] - 0.5 * (15 / (30 + 1e-4) + 70 / (85 + 1e-4))) < 1e-15
    s[6] = s[5] = 0.0
    assert np.isnan(G.values_from_sums(s)[3])
