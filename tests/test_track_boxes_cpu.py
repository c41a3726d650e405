"""CPU: the box fitting rule (include/rtk_fused.h, "Oriented boxes") as tests/_box_fit_util.py states it, on hand-checked cases; the
KITTI box I/O of ratrack_amd/vod_io.py against `vod_gt.box_in_radar_frame` on the shipped example frames; and the host-side refusals
of ratrack_amd/boxes.py and the result log's KITTI writer, none of which touches a device."""
import math
import os
import types

import numpy as np
import pytest
import torch

import _box_fit_util as F
import _result_log_util as U
from _gt_util import EX, tf_of
from ratrack_amd import boxes as BX, result_log as RL, vod_gt, vod_io

CX, CY, CZ, L, W, H, YAW, AREA = range(8)


def rank(n, i, j):
    """The candidate of pair i < j among n points."""
    return 1 + i * (2 * n - i - 1) // 2 + j - i - 1


def rotated(points, degrees, shift=(0.0, 0.0)):
    a = math.radians(degrees)
    c, s = math.cos(a), math.sin(a)
    return [(c * x - s * y + shift[0], s * x + c * y + shift[1], z) for x, y, z in points]


# ---- the statement on hand-checked cases ----------------------------------------------------------------------------------------
def test_no_point_and_a_coordinate_that_is_not_finite():
    box, cand, valid, _ = F.fit(np.zeros((0, 3)))
    assert box.tolist() == [0.0] * 8 and (cand, valid) == (-1, 0)
    for bad in (float("nan"), float("inf"), -float("inf")):
        for axis in range(3):
            pts = [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]
            pts[1][axis] = bad
            box, cand, valid, _ = F.fit(pts)
            assert box.tolist() == [0.0] * 8 and (cand, valid) == (-1, -1)


def test_one_point():
    box, cand, valid, runner = F.fit([[3.0, -2.0, 0.5]])
    assert box.tolist() == [3.0, -2.0, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0] and (cand, valid) == (0, 1) and runner == F.INF
    box, _, _, _ = F.fit([[3.0, -2.0, 0.5]], min_extent=0.25)
    assert box.tolist() == [3.0, -2.0, 0.5, 0.25, 0.25, 0.25, 0.0, 0.0]


def test_two_points_along_an_axis_tie_with_candidate_0():
    box, cand, valid, _ = F.fit([[1.0, 2.0, 0.0], [5.0, 2.0, 1.0]])
    assert (cand, valid) == (0, 2) and box.tolist() == [3.0, 2.0, 0.5, 4.0, 0.0, 1.0, 0.0, 0.0]
    # along y: candidate 0 again (area 0 on both), and the longer side is t: the swap turns yaw to pi/2, the wrap to -pi/2
    box, cand, valid, _ = F.fit([[1.0, 2.0, 0.0], [1.0, 8.0, 0.0]])
    assert (cand, valid) == (0, 2) and box.tolist() == [1.0, 5.0, 0.0, 6.0, 0.0, 0.0, -F.PI / 2.0, 0.0]


def test_two_oblique_points():
    box, cand, valid, runner = F.fit([[0.0, 0.0, 0.0], [3.0, 4.0, 2.0]])
    assert (cand, valid) == (1, 2) and runner == 12.0                    # the axis-aligned box is 3 x 4
    assert box[[CX, CY, CZ, L, W, H, AREA]].tolist() == [1.5, 2.0, 1.0, 5.0, 0.0, 2.0, 0.0]
    assert box[YAW] == math.atan2(4.0, 3.0)
    # the same pair listed the other way round points at -180 + 53 degrees: the wrap brings it back
    box2, cand2, _, _ = F.fit([[3.0, 4.0, 2.0], [0.0, 0.0, 0.0]])
    assert cand2 == 1 and math.atan2(-4.0, -3.0) < -F.PI / 2.0 and abs(box2[YAW] - box[YAW]) < 1e-15
    assert box2[[CX, CY, CZ, L, W, H, AREA]].tolist() == box[[CX, CY, CZ, L, W, H, AREA]].tolist()


def test_three_collinear_points():
    box, cand, valid, _ = F.fit([[0.0, 0.0, 0.0], [2.0, 2.0, 0.0], [1.0, 1.0, 0.0]])
    assert (cand, valid) == (1, 3)                                         # every pair gives area 0: the first wins
    assert box[[CX, CY, L, W, AREA]].tolist() == [1.0, 1.0, 8.0 / math.sqrt(8.0), 0.0, 0.0] and box[YAW] == math.atan2(2.0, 2.0)


def test_coincident_points_are_skipped_and_keep_their_index():
    # points 0, 1 and 2 coincide: pairs (0,1), (0,2), (1,2) = candidates 1, 2, 4 have q == 0; the first live oblique pair is (0,3) = 3
    pts = [[1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [4.0, 5.0, 0.0]]
    assert [c[0] for c in F.candidates([p[0] for p in pts], [p[1] for p in pts])] == [0, 3, 5, 6]
    box, cand, valid, _ = F.fit(pts)
    assert (cand, valid) == (3, 4) and rank(4, 0, 3) == 3 and box[[L, W, AREA]].tolist() == [5.0, 0.0, 0.0]
    # all coincident: candidate 0 is all there is
    box, cand, valid, runner = F.fit([[2.0, 3.0, 1.0]] * 5)
    assert (cand, valid) == (0, 5) and runner == F.INF and box.tolist() == [2.0, 3.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]


def test_an_integer_rectangle_is_an_exact_tie_and_candidate_0_wins():
    corners = [[1.0, 1.0, 0.0], [7.0, 1.0, 0.5], [7.0, 4.0, 0.0], [1.0, 4.0, 2.0]]
    xs, ys = [p[0] for p in corners], [p[1] for p in corners]
    areas = {c[0]: c[4] for c in F.candidates(xs, ys)}
    assert areas[0] == areas[rank(4, 0, 1)] == areas[rank(4, 1, 2)] == areas[rank(4, 2, 3)] == areas[rank(4, 0, 3)] == 18.0
    assert areas[rank(4, 0, 2)] > 18.0 and areas[rank(4, 1, 3)] > 18.0            # the diagonals
    box, cand, valid, runner = F.fit(corners)
    assert (cand, valid) == (0, 4) and box.tolist() == [4.0, 2.5, 1.0, 6.0, 3.0, 2.0, 0.0, 18.0] and runner == areas[rank(4, 0, 2)]
    # a negative zero among the extremes (t = d_x y - d_y x of a point on an axis) shows in no bit
    box, cand, _, _ = F.fit([[0.0, 0.0, -0.0], [-2.0, 0.0, 0.0], [-2.0, -1.0, 0.0], [0.0, -1.0, 0.0]])
    assert cand == 0 and [v.hex() for v in box.tolist()] == [v.hex() for v in [-1.0, -0.5, 0.0, 2.0, 1.0, 0.0, 0.0, 2.0]]


# two shapes whose minimum rectangle is flush with the edge AB alone (AB on the bottom; no other pair is parallel or perpendicular to
# it, and every other candidate's area is more than 1 % larger).  LONG: a pentagon with one point each at the left, right and top
# extremes, AB along the long side (4.5 x 2); TALL: AB is the whole short side (2.5 x 4.5).
LONG = [(0.0, 0.0, 0.0), (4.0, 0.0, 1.0), (4.25, 1.0, 0.0), (-0.25, 1.25, 0.0), (2.0, 2.0, 0.0), (1.0, 0.75, 0.5), (3.0, 1.5, 0.25)]
TALL = [(0.0, 0.0, 0.0), (2.5, 0.0, 1.0), (1.25, 4.5, 0.0), (1.875, 4.125, 0.0), (1.5, 2.375, 0.0), (0.75, 4.25, 0.5), (1.0, 3.625, 0.25)]


@pytest.mark.parametrize("shape,flip,l,w,yaw_deg,swapped,wrapped", [
    (LONG, False, 4.5, 2.0, 30.0, False, False),
    (LONG, True, 4.5, 2.0, 30.0, False, True),          # B listed before A: d points at 210 degrees, the wrap adds pi
    (TALL, False, 4.5, 2.5, -60.0, True, True),         # d along the short side: swapped, 30 + 90 = 120 degrees, the wrap takes pi
    (TALL, True, 4.5, 2.5, -60.0, True, False),         # 210 - 360 + 90 = -60 degrees as it is
])
def test_a_rotated_shape_whose_winner_is_one_hull_edge(shape, flip, l, w, yaw_deg, swapped, wrapped):
    pts = rotated(shape, 30.0, shift=(10.0, -5.0))
    if flip:
        pts[0], pts[1] = pts[1], pts[0]
    box, cand, valid, runner = F.fit(pts)
    assert (cand, valid) == (rank(7, 0, 1), 7)                            # the pair (A, B), an edge of the hull
    assert runner > box[AREA] * 1.01                                       # no other candidate comes near
    assert abs(box[L] - l) < 1e-5 and abs(box[W] - w) < 1e-5 and abs(box[AREA] - l * w) < 1e-4 and box[L] >= box[W]
    assert abs(box[YAW] - math.radians(yaw_deg)) < 1e-6 and -F.PI / 2.0 <= box[YAW] < F.PI / 2.0
    p32 = np.asarray(pts, np.float32).astype(np.float64)
    d = p32[1, :2] - p32[0, :2]
    raw = math.atan2(d[1], d[0])
    assert swapped == (abs(math.hypot(*d) - l) > 1.0)                      # the pair lies along the shorter side
    assert wrapped == (not -F.PI / 2.0 <= raw + (F.PI / 2.0 if swapped else 0.0) < F.PI / 2.0)
    # the centre is the rectangle's: rotate the unrotated rectangle's centre
    centre = {4.5 * 2.0: (2.0, 1.0), 4.5 * 2.5: (1.25, 2.25)}[l * w]
    want = rotated([centre + (0.0,)], 30.0, shift=(10.0, -5.0))[0]
    assert abs(box[CX] - want[0]) < 1e-5 and abs(box[CY] - want[1]) < 1e-5 and box[CZ] == 0.5 and box[H] == 1.0


def test_above_the_cap_only_candidate_0_is_taken():
    rng = np.random.default_rng(3)
    pts = rotated([(x, y, 0.0) for x, y in zip(rng.uniform(-4, 4, 129), rng.uniform(-1, 1, 129))], 40.0)
    box, cand, valid, _ = F.fit(pts)
    p32 = np.asarray(pts, np.float32).astype(np.float64)
    assert (cand, valid) == (0, 129) and box[YAW] == (-F.PI / 2.0 if np.ptp(p32[:, 1]) > np.ptp(p32[:, 0]) else 0.0)
    assert box[L] == max(np.ptp(p32[:, 0]), np.ptp(p32[:, 1])) and box[AREA] == np.ptp(p32[:, 0]) * np.ptp(p32[:, 1])
    _, cand128, _, _ = F.fit(pts[:128])
    assert cand128 > 0                                                     # at the cap the search runs


def test_the_side_by_side_statement_is_the_plain_one_bit_for_bit():
    rng = np.random.default_rng(4)
    clouds = [(rng.normal(size=(40, 2)) * [3.0, 0.5] + [20.0, -7.0]).astype(np.float32).astype(np.float64),
              rng.integers(-3, 4, size=(30, 2)).astype(np.float64)]                  # coincident points, exact ties, zeros of both signs
    for xy in clouds:
        xs, ys = xy[:, 0].tolist(), xy[:, 1].tolist()
        plain, fast = F.candidates(xs, ys), F.candidates_side_by_side(xs, ys)
        flat = lambda cands: [(c[0],) + tuple(v.hex() for v in c[1:5] + c[5]) for c in cands]
        assert flat(plain) == flat(fast) and len(plain) > 300


# ---- vod_io: label fields and files --------------------------------------------------------------------------------------------------
def example_labels(f):
    det = open(os.path.join(EX, "label_%s.txt" % f)).read().splitlines()
    return vod_gt.parse_tracking_labels([" ".join([line.split(" ")[0], str(i)] + line.split(" ")[2:15]) for i, line in enumerate(det)])


def test_box_label_fields_inverts_box_in_radar_frame():
    """Measured on the three shipped frames (float64 on float32-valued matrices): over 62 labels the centre comes back within
    7.2e-15 m and the direction of the rebuilt box's first axis within 8.9e-16 rad of yaw modulo pi; the bounds asserted are 1e-9."""
    count, worst_c, worst_a = 0, 0.0, 0.0
    for f in ("00549", "01047", "01201"):
        tf = tf_of(f)
        assert abs(tf.t_radar_lidar[2, 0]) > 1e-4 or abs(tf.t_radar_lidar[0, 2]) > 1e-4           # the extrinsics carry a tilt
        for lab in example_labels(f).values():
            box = vod_gt.box_in_radar_frame(lab, tf)
            yaw = math.atan2(box.R[1, 0], box.R[0, 0])
            fields = vod_io.box_label_fields(list(box.center) + list(box.extent) + [yaw], tf)
            assert (fields.l, fields.w, fields.h) == (lab.l, lab.w, lab.h) and -math.pi <= fields.ry < math.pi
            again = vod_gt.box_in_radar_frame(lab._replace(**fields._asdict()), tf)
            worst_c = max(worst_c, float(np.abs(again.center - box.center).max()))
            off = (math.atan2(again.R[1, 0], again.R[0, 0]) - yaw) % math.pi
            worst_a = max(worst_a, min(off, math.pi - off))
            count += 1
    print("box_label_fields: %d labels, centre %.3g m, direction %.3g rad" % (count, worst_c, worst_a))
    assert count > 30 and worst_c < 1e-9 and worst_a < 1e-9
    # without transforms the radar-frame values pass through
    assert vod_io.box_label_fields([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 0.25]) == vod_io.KittiFields(6.0, 5.0, 4.0, 1.0, 2.0, 3.0, 0.25)


def test_the_line_format_column_for_column():
    fields = vod_io.KittiFields(h=1.5, w=0.1, l=4.25, x=-7.5, y=1e-7, z=42.0, ry=-1.0 / 3.0)
    line = vod_io.format_kitti_track_line(17, 3, "Car", fields, 0.5)
    assert line == "17 3 Car -1 -1 -10 -1 -1 -1 -1 1.5 0.1 4.25 -7.5 1e-07 42.0 -0.3333333333333333 0.5\n"
    tok = line.split()
    assert len(tok) == 18 and tok[3:10] == ["-1", "-1", "-10", "-1", "-1", "-1", "-1"]      # truncated occluded alpha, the image box
    with pytest.raises(ValueError, match="one word"):
        vod_io.format_kitti_track_line(0, 0, "Car park", fields, 0.0)


def test_read_kitti_tracks_returns_every_field_with_its_bits(tmp_path):
    rng = np.random.default_rng(5)
    rows = []
    for k in range(200):
        vals = (rng.normal(size=8) * 10.0 ** rng.integers(-12, 12, size=8)).tolist()
        rows.append((int(rng.integers(0, 10 ** 5)), int(rng.integers(0, 10 ** 6)), ["Car", "Pedestrian", "Cyclist"][k % 3],
                     vod_io.KittiFields(*vals[:7]), vals[7]))
    rows.append((0, 0, "Car", vod_io.KittiFields(0.0, -0.0, 5e-324, 1.7976931348623157e308, math.pi, -math.pi / 2, 0.1), 1.0))
    path = vod_io.write_kitti_tracks(str(tmp_path / "deep" / "seq.txt"), rows)
    got = vod_io.read_kitti_tracks(path)
    assert len(got) == len(rows)
    for g, w in zip(got, rows):
        assert g[:3] == w[:3] and [v.hex() for v in g[3]] == [v.hex() for v in w[3]] and g[4].hex() == w[4].hex()
    assert open(path).read() == "".join(vod_io.format_kitti_track_line(*r) for r in rows)


# ---- refusals: no device is touched ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [-1.0, -1e-300, float("nan"), float("inf"), "0.5", None, True])
def test_a_bad_min_extent_is_refused(bad):
    with pytest.raises(ValueError, match="min_extent"):
        BX.check_min_extent(bad)
    step = types.SimpleNamespace(pc1=torch.zeros(2, 3, 8), obj=torch.zeros(2, 8, dtype=torch.int32), num_objects=torch.zeros(2, dtype=torch.int32),
                                 max_objects=4, active=None)
    with pytest.raises(ValueError, match="min_extent"):
        BX.object_boxes(step, min_extent=bad)
    assert BX.check_min_extent(0) == 0.0 and BX.check_min_extent(np.float32(0.5)) == 0.5


def test_the_tracker_refuses_a_bad_box_keyword_before_it_looks_at_the_net():
    from ratrack_amd import tracker as T
    with pytest.raises(ValueError, match="min_extent"):
        T.BatchedTracker(None, streams=2, boxes=True, box_min_extent=-0.5)
    with pytest.raises(ValueError, match="without boxes=True"):
        T.BatchedTracker(None, streams=2, box_min_extent=0.5)


def test_bad_into_buffers_are_refused():
    B, K = 2, 4
    step = types.SimpleNamespace(pc1=torch.zeros(B, 3, 8), obj=torch.zeros(B, 8, dtype=torch.int32), num_objects=torch.zeros(B, dtype=torch.int32),
                                 max_objects=K, active=None)
    good = lambda: BX.ObjectBoxes.empty(B, K, "cpu")
    BX.check_into(good(), B, K, "cpu")
    cases = {"box": [torch.zeros(B, K, 7, dtype=torch.float64), torch.zeros(B, K, 8), torch.zeros(B, 8, K, dtype=torch.float64).transpose(1, 2)],
             "cand": [torch.zeros(B, K + 1, dtype=torch.int32), torch.zeros(B, K, dtype=torch.int64)],
             "valid": [torch.zeros(K, B, dtype=torch.int32), torch.zeros(B, K)],
             "flags": [torch.zeros(B, 1, dtype=torch.int32), torch.zeros(B, dtype=torch.uint8), None]}
    for name, bads in cases.items():
        for bad in bads:
            into = good()
            setattr(into, name, bad)
            with pytest.raises(ValueError, match="into.%s" % name):
                BX.object_boxes(step, into=into)
    with pytest.raises(ValueError, match="into.box"):
        BX.object_boxes(step, into=object())
    with pytest.raises(ValueError, match="max_objects"):
        BX.object_boxes_raw(step.pc1, step.obj, step.num_objects, 257)
    with pytest.raises(ValueError, match="got pc1"):
        BX.object_boxes_raw(step.pc1, step.obj[:, :5], step.num_objects, K)


def host_log_with_boxes():
    """A two-stream host log of three frames and the statement's boxes for it, as `ResultLog.download(boxes=...)` hands them over."""
    rng = np.random.default_rng(6)
    B, N, K = 2, 24, 3
    host = U.HostLog(B, K, 3, 9, 3 * N)
    for t in range(3):
        obj = np.stack([rng.integers(-1, K, size=N) for _ in range(B)]).astype(np.int32)
        host.append((rng.normal(size=(B, 3, N)) * 5.0).astype(np.float32), obj, np.array([K, K - 1], np.int32),
                    rng.integers(0, 50, size=(B, K)).astype(np.int32), rng.uniform(0, 1, size=(B, K)).astype(np.float32), seq=[0, 1], index=[10 + t] * B)
    tables = host.tables()
    box, cand, valid, flags, _ = F.log_boxes(tables)
    return dict(tables, box=box, box_cand=cand, box_valid=valid, box_flags=flags)


def test_a_transforms_mapping_that_misses_a_logged_frame_is_refused():
    host = host_log_with_boxes()
    tf = tf_of("00549")
    full = {(s, 10 + t): tf for s in range(2) for t in range(3)}
    rows = RL.kitti_rows(host, transforms=full)
    assert sorted(rows) == [0, 1] and len(rows[0]) == 9 and len(rows[1]) == 6
    assert [r[0] for r in rows[0]] == [10] * 3 + [11] * 3 + [12] * 3
    missing = dict(full)
    del missing[(1, 11)]
    with pytest.raises(ValueError, match=r"stream 1 is \(seq=1, index=11\)"):
        RL.kitti_rows(host, transforms=missing)
    with pytest.raises(ValueError, match="transforms"):
        RL.check_transforms(host, {})
    RL.check_transforms(host, None)


def test_the_host_rendering_is_the_statements(tmp_path):
    host = host_log_with_boxes()
    keep = np.ones((2, 9), np.uint8)
    keep[0, 4], keep[1, 0] = 0, 0
    host["box_valid"][0, 7] = 0                        # a record without a box gets no line
    tf = tf_of("01047")
    transforms = {(s, 10 + t): tf for s in range(2) for t in range(3)}
    for tfs in (None, transforms):
        rows = RL.kitti_rows(host, keep, tfs, "Cyclist")
        want = F.kitti_text(host, host["box"], host["box_valid"], keep, tfs, "Cyclist")
        assert {s: "".join(vod_io.format_kitti_track_line(*r) for r in rs) for s, rs in rows.items()} == want
        assert len(rows[0]) == 7 and len(rows[1]) == 5
    # in the radar frame a line carries the box's own words
    r = RL.kitti_rows(host)[0][0]
    assert r[3] == vod_io.KittiFields(*(float(host["box"][0, 0, k]) for k in (H, W, L, CX, CY, CZ, YAW))) and r[1] == int(host["rec_track"][0, 0])
    # two frames with one (seq, index)
    host["tag"][1, 1, :2] = host["tag"][0, 2, :2]
    with pytest.raises(ValueError, match="both"):
        RL.kitti_rows(host)
    assert RL.kitti_path("root", ["a", "b"], 1) == os.path.join("root", "b.txt")
