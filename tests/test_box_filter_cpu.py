"""CPU: the track box filter's rule (include/rtk_fused.h, "Filtered boxes") as tests/_box_filter_util.py states it -- against the dense
ten-state filter, on hand-built tracks and logs, and on the synthetic track it was designed on -- and the argument checks of
ratrack_amd/boxes.py and ResultLog.filter_boxes, which touch no device."""
import math

import numpy as np
import pytest
import torch

import _box_filter_util as K
import _box_fit_util as F
import _track_box_util as TB
from ratrack_amd import boxes as BX, result_log as RL

PI = math.pi
MODES = [(sm, sz) for sm in (0, 1) for sz in (0, 1)]
DENSE_SEEDS = (1, 2, 3, 4)
DENSE_MEASURED = 1.1e-13              # the largest difference measured over this file's own cases, rounded up (see the test)
QUALITY_SEEDS = tuple(range(12))


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def run(boxes, frames=None, **par):
    """One track of per-frame boxes through the statement -> its output dict with the stream axis dropped."""
    tables, box, valid = K.track_tables(boxes, frames)
    out = K.filter_log(tables, box, valid, par=K.Par(**par))
    return {n: v[0] for n, v in out.items()}


# ---- the decomposition against the dense filter ------------------------------------------------------------------------------------------
def dense_case(seed, n=60):
    """A gap-free track whose heading moves slowly (never a correction): coordinates up to 60."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = rng.uniform(-20, 20) + 0.6 * t + rng.normal(size=n) * 0.5
    y = rng.uniform(-20, 20) - 0.5 * t + rng.normal(size=n) * 0.5
    z = rng.normal(size=n) * 0.2
    yaw = 0.2 + 0.01 * t + rng.normal(size=n) * 0.05
    l, w, h = 4.0 + rng.normal(size=n) * 0.3, 1.8 + rng.normal(size=n) * 0.2, 1.5 + rng.normal(size=n) * 0.1
    assert np.abs(x).max() < 60 and np.abs(y).max() < 60 and np.abs(yaw).max() < 1.2
    return np.column_stack([x, y, z, l, w, h, yaw, l * w])


def dense_difference(seed, smooth):
    boxes = dense_case(seed)
    p = K.Par(symmetry=2, max_gap=1, smooth=smooth)
    zs = [K.measurement(b) for b in boxes]
    rows = K.run_segment(zs, [-1] + [1] * (len(zs) - 1), list(range(len(zs))), p)
    want = K.dense_track(zs, p, smooth)
    if smooth:      # the smoothed mean: x, y, z, l, w, h through the box (l >= w throughout, so no swap), yaw and v through vel
        got = np.array([[r["box"][0], r["box"][1], r["box"][2], r["vel"][3], r["box"][3], r["box"][4], r["box"][5]] + r["vel"][:3] for r in rows])
    else:
        got = np.array([r["state"][:10] for r in rows])
    return float(np.abs(got - want).max())


def test_the_decomposed_filter_is_the_dense_ten_state_filter():
    """Reference parameters, symmetry 2, gap-free tracks of 60 frames, filtered and smoothed, against 10 x 10 matrices with the Joseph
    form and dense RTS.  Largest absolute difference measured over these eight cases (seeds 1 ... 4, filtered and smoothed, all ten
    words of every mean): 1.07e-13; the bound is 16 x that, rounded up: 16 x 1.1e-13 = 1.76e-12."""
    worst = 0.0
    for seed in DENSE_SEEDS:
        for smooth in (0, 1):
            d = dense_difference(seed, smooth)
            print("   seed %d smooth %d: %.3g" % (seed, smooth, d))
            worst = max(worst, d)
    assert worst <= 16 * DENSE_MEASURED, worst


# ---- hand-built tracks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symmetry", [2, 4])
@pytest.mark.parametrize("smooth,size_rule", MODES)
def test_a_constant_track_comes_out_as_it_went_in(symmetry, smooth, size_rule):
    row = [3.0, -2.0, 0.5, 4.0, 1.75, 1.5, 0.3, 7.0]
    out = run([row] * 9, frames=[0, 1, 2, 4, 5, 6, 8, 9, 10], symmetry=symmetry, smooth=smooth, size_rule=size_rule, size_percent=50)
    assert (bits(out["box"]) == bits([row] * 9)).all()
    assert (out["vel"][:, :3] == 0).all() and (bits(out["vel"][:, 3]) == bits(0.3)).all() and out["valid"].tolist() == [1] * 9
    assert out["link"][:, 1].tolist() == [-1, 1, 1, 2, 1, 1, 2, 1, 1] and (out["link"][:, 3] == 0).all()


@pytest.mark.parametrize("symmetry", [2, 4])
@pytest.mark.parametrize("smooth", [0, 1])
def test_headings_on_either_side_of_the_wrap_stay_at_the_wrap(symmetry, smooth):
    rows = [[1.0 * i, 2.0, 0.0, 4.0, 1.8, 1.5, 1.55 if i % 2 == 0 else -1.56, 7.2] for i in range(12)]
    out = run(rows, symmetry=symmetry, smooth=smooth)
    yaw = out["box"][:, 6]
    assert (np.abs(np.abs(yaw) - PI / 2.0) < 0.05).all(), yaw
    assert ((yaw >= -PI / 2.0) & (yaw < PI / 2.0)).all()
    assert (np.abs(out["vel"][:, 3] - 1.55) < 0.05).all()                  # the filter's own heading never left the first reading's side
    assert (np.abs(out["aligned"][1::2, 0] - (PI - 1.56)) < 1e-12).all()   # -1.56 was read as pi - 1.56


def test_a_quarter_turn_swaps_the_sides_and_keeps_the_heading():
    """A 2.0 x 1.9 box whose fitted rectangle comes out along either side in turn."""
    rows = [[0.5 * i, 1.0, 0.0, 2.0, 1.9, 1.0, 0.3 if i % 2 == 0 else 0.3 - PI / 2.0, 3.8] for i in range(10)]
    out = run(rows, symmetry=4)
    assert (np.abs(out["vel"][:, 3] - 0.3) < 1e-12).all()
    assert (bits(out["aligned"][0::2, 1:3]) == bits([[2.0, 1.9]] * 5)).all() and (bits(out["aligned"][1::2, 1:3]) == bits([[1.9, 2.0]] * 5)).all()
    assert (np.abs(out["aligned"][:, 0] - 0.3) < 1e-12).all()
    # every output box is the same rectangle: its long side along 0.3 or its short side along 0.3 - pi/2
    yaw = out["box"][:, 6]
    assert ((np.abs(yaw - 0.3) < 1e-9) | (np.abs(yaw - (0.3 - PI / 2.0)) < 1e-9)).all() and (out["box"][:, 3] >= out["box"][:, 4]).all()
    # read with a half-turn symmetry the same track loses its heading
    half = run(rows, symmetry=2)
    assert np.abs(half["vel"][-1, 3] - 0.3) > 0.3 and (half["aligned"][1::2, 1] == 2.0).all()


def test_gaps():
    """max_gap = 3: gaps of 1, 2 and 3 stay in the segment; 4, 0 and -1 start one, whose first box is its measurement."""
    rng = np.random.default_rng(5)
    rows = K.random_boxes(rng, 1, 7)[0]
    frames = [0, 1, 3, 6, 10, 10, 9]
    for smooth, size_rule in MODES:
        out = run(rows, frames=frames, max_gap=3, smooth=smooth, size_rule=size_rule, size_percent=100)
        assert out["link"].tolist() == [[-1, -1, 1, 0], [0, 1, 2, 0], [1, 2, 3, 0], [2, 3, -1, 0], [-1, -1, -1, 4], [-1, -1, -1, 5], [-1, -1, -1, 6]]
        for r in (0, 4, 5, 6):
            assert (bits(out["state"][r, :7]) == bits(K.measurement(rows[r]))).all() and (out["state"][r, 7:10] == 0).all()
            assert out["state"][r, 10:].tolist() == [10.0, 0.0, 10000.0, 10.0, 10.0, 0.0]
        for r in (4, 5, 6):      # a segment of one: the box itself
            assert (bits(out["box"][r]) == bits(rows[r])).all(), (smooth, size_rule, r)
    # the gap enters the prediction: two frames on, the mean has moved twice
    a = run(rows[:3], frames=[0, 1, 3], max_gap=3)
    b = run(rows[:3], frames=[0, 1, 2], max_gap=3)
    assert (a["state"][1] == b["state"][1]).all() and (a["state"][2, :3] != b["state"][2, :3]).all()
    s = K.State(K.measurement(rows[0]), K.Par())
    K.predict(s, K.Par())
    K.update(s, K.align(s, K.measurement(rows[1]), K.Par()), K.Par())
    K.predict(s, K.Par())
    K.predict(s, K.Par())
    K.update(s, K.align(s, K.measurement(rows[2]), K.Par()), K.Par())
    assert (bits(a["state"][2]) == bits(s.words())).all()


def membership_log():
    """Stream 0: a clip of three frames and a clip of two that reuses id 5; stream 1: one frame."""
    log = K.ids_log([[(0, True, [5, 5, 6]), (1, False, [6, 5, 5, 7]), (2, False, [5, 6]), (3, True, [5, 8]), (4, False, [8, 5])],
                     [(0, True, [1, 2])]])
    tables = log.tables()
    assert tables["cursor"][:, 1].tolist() == [13, 2]
    valid = np.ones((2, tables["rec_track"].shape[1]), np.int32)
    valid[0, 3] = -1                  # id 6 in frame 1: a box that is not finite
    valid[0, 4] = 0                   # the first of the two 5s in frame 1: no box, so the second is the member and no duplicate
    return tables, K.random_boxes(np.random.default_rng(6), 2, valid.shape[1]), valid


def test_membership():
    tables, box, valid = membership_log()
    out = K.filter_log(tables, box, valid, par=K.Par(max_gap=2))
    assert out["flags"].tolist() == [K.FLAG_DUPLICATE, 0]
    #          record:  0  1  2 | 3  4  5  6 | 7  8 | 9 10 | 11 12
    assert out["valid"][0, :13].tolist() == [1, 0, 1, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1]
    link = out["link"][0, :13].tolist()
    assert link[0] == [-1, -1, 5, 0] and link[5] == [0, 1, 7, 0] and link[7] == [5, 1, -1, 0]              # id 5 of the first clip
    assert link[2] == [-1, -1, 8, 2] and link[8] == [2, 2, -1, 2]                                          # id 6 skips frame 1
    assert link[1] == link[3] == link[4] == [-1] * 4 and link[6] == [-1, -1, -1, 6]
    assert link[9] == [-1, -1, 12, 9] and link[12] == [9, 1, -1, 9] and link[10] == [-1, -1, 11, 10]       # the second clip starts anew
    assert (out["box"][0, [1, 3, 4]] == 0).all() and (out["state"][0, [1, 3, 4]] == 0).all()
    assert out["link"][1, :2].tolist() == [[-1, -1, -1, 0], [-1, -1, -1, 1]] and (out["valid"][:, 13:] == 0).all() and (out["link"][0, 13:] == 0).all()
    # a keep mask: record 0 is not kept, so its duplicate, record 1, becomes id 5's member of frame 0
    keep = np.ones_like(valid, dtype=np.uint8)
    keep[0, 0] = 0
    masked = K.filter_log(tables, box, valid, keep=keep, par=K.Par(max_gap=2))
    assert masked["flags"].tolist() == [0, 0] and masked["valid"][0, :2].tolist() == [0, 1] and masked["link"][0, 1].tolist() == [-1, -1, 5, 1]
    assert (bits(masked["state"][0, 1, :7]) == bits(K.measurement(box[0, 1]))).all()
    # more ids in a clip than the table holds: that clip and the later one come out empty, the earlier one does not
    big = K.ids_log([[(0, True, [1, 2]), (1, True, list(range(256))), (2, False, list(range(256, 512)))] +
                     [(3 + i, False, list(range(512 + 256 * i, 768 + 256 * i))) for i in range(7)] + [(10, True, [1])]])
    tb = big.tables()
    n = int(tb["cursor"][0, 1])
    assert n == 2 + 9 * 256 + 1
    o = K.filter_log(tb, K.random_boxes(np.random.default_rng(7), 1, tb["rec_track"].shape[1]), np.ones((1, tb["rec_track"].shape[1]), np.int32))
    assert o["flags"].tolist() == [K.FLAG_TRACKS] and o["valid"][0, :2].tolist() == [1, 1] and (o["valid"][0, 2:] == 0).all()
    assert (o["link"][0, 2:n] == -1).all() and (o["box"][0, 2:] == 0).all()


def test_the_extent_rank():
    assert [K.extent_rank(1, q) for q in (0, 50, 90, 100)] == [0, 0, 0, 0]
    assert [K.extent_rank(2, q) for q in (0, 50, 90, 100)] == [0, 0, 0, 1]
    assert [K.extent_rank(11, q) for q in (0, 50, 90, 100)] == [0, 5, 9, 10]
    rng = np.random.default_rng(8)
    for n in (1, 2, 11):
        rows = K.random_boxes(rng, 1, n)[0]
        rows[:, 6] = 0.1                                     # one heading: no swap, the readings are the measurements
        for q in (0, 50, 90, 100):
            for smooth in (0, 1):
                out = run(rows, size_rule=1, size_percent=q, smooth=smooth)
                for word in (3, 4, 5):      # (every row has l >= w, so the order statistics have too: the output swaps nothing)
                    want = np.sort(rows[:, word])[K.extent_rank(n, q)]
                    assert (bits(out["box"][:, word]) == bits(want)).all() and want in rows[:, word], (n, q, word)
                # everything but the sizes is the size_rule 0 result
                plain = run(rows, size_rule=0, smooth=smooth)
                assert (bits(out["box"][:, :3]) == bits(plain["box"][:, :3])).all() and (bits(out["vel"]) == bits(plain["vel"])).all()
                assert (bits(out["state"]) == bits(plain["state"])).all()
    # equal values are ordered by record index, so the choice is one of them whatever the order
    rows = K.random_boxes(rng, 1, 4)[0]
    rows[:, 3:6], rows[:, 6] = [4.0, 2.0, 1.0], 0.0
    assert (run(rows, size_rule=1, size_percent=50)["box"][:, 3:6] == [4.0, 2.0, 1.0]).all()


# ---- quality ------------------------------------------------------------------------------------------------------------------------------
def bev_iou(a, b):
    """Rows (x, y, ., l, w, ., yaw): the IoU of their footprints by _track_box_util's clipping, in float."""
    ra = TB._rect(a[0], a[1], math.cos(a[6]), math.sin(a[6]), a[3] / 2.0, a[4] / 2.0)
    rb = TB._rect(b[0], b[1], math.cos(b[6]), math.sin(b[6]), b[3] / 2.0, b[4] / 2.0)
    inter = float(TB._area(TB._clip_polygon(ra, rb)))
    return inter / (a[3] * a[4] + b[3] * b[4] - inter)


def quality(seed, points=(3, 8)):
    """-> (mean BEV IoU of the per-frame boxes, of the filtered boxes) against the true box of the synthetic track."""
    track = K.arc_track(seed, points=points)
    fitted = np.array([F.fit(pts, min_extent=0.2)[0] for _, pts, _ in track])
    out = run(fitted, frames=[t for t, _, _ in track], smooth=1, size_rule=1, size_percent=90)
    truth = [(x, y, z, l, w, h, yaw) for _, _, (x, y, z, l, w, h, yaw) in track]
    per_frame = np.mean([bev_iou(fitted[i], truth[i]) for i in range(len(track))])
    filtered = np.mean([bev_iou(out["box"][i], truth[i]) for i in range(len(track))])
    return float(per_frame), float(filtered)


@pytest.mark.parametrize("seed", QUALITY_SEEDS)
def test_filtered_boxes_are_better_than_per_frame_boxes(seed):
    """A 4.0 x 1.8 x 1.5 m box along an arc for 40 frames, 3-8 interior points per frame, a fifth of the frames dropped, min_extent 0.2;
    smooth = 1, size_rule = 1, size_percent = 90, everything else at its default.  Seeds 0 ... 11 as first chosen."""
    per_frame, filtered = quality(seed)
    print("   seed %d: per-frame %.3f, filtered %.3f" % (seed, per_frame, filtered))
    assert filtered > per_frame


# ---- arguments: no device is touched ---------------------------------------------------------------------------------------------------
BAD = [dict(r_pos=0.0), dict(r_yaw=-1.0), dict(r_size=float("nan")), dict(r_pos=float("inf")), dict(q_pos=-1e-9), dict(q_vel=float("nan")),
       dict(q_yaw=float("inf")), dict(q_size="1"), dict(p0=0.0), dict(p0_vel=-1.0), dict(p0=True), dict(symmetry=3), dict(symmetry=2.0),
       dict(max_gap=0), dict(max_gap=65), dict(max_gap=1.5), dict(smooth=2), dict(smooth=True), dict(size_rule=-1), dict(size_rule=2),
       dict(size_percent=-1), dict(size_percent=101), dict(size_percent=50.0)]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: "%s=%r" % next(iter(d.items())))
def test_a_bad_parameter_is_refused(bad):
    name = next(iter(bad))
    with pytest.raises(ValueError, match=name):
        BX.BoxFilter(**bad)
    good = BX.BoxFilter()
    setattr(good, name, bad[name])
    log = RL.ResultLog(2, 4, 3, 8, 16, device="cpu")
    with pytest.raises(ValueError, match=name):
        log.filter_boxes(BX.ObjectBoxes.empty(2, 8, "cpu"), filter=good)
    with pytest.raises(ValueError, match=name):
        log.write_kitti("/nonexistent", ["a"], filter=good)


def test_the_defaults_and_the_reference():
    d, r = BX.BoxFilter(), BX.BoxFilter.reference()
    assert [getattr(d, n) for n in BX.BoxFilter.FIELDS] == [1.0, 1.0, 1.0, 1.0, 0.01, 1.0, 1.0, 10.0, 10000.0, 4, 2, 0, 0, 90]
    assert (r.symmetry, r.max_gap) == (2, 1) and [getattr(r, n) for n in BX.BoxFilter.FIELDS[:9]] == [getattr(d, n) for n in BX.BoxFilter.FIELDS[:9]]
    assert BX.BoxFilter.reference(smooth=1).smooth == 1 and K.Par().kwargs() == {n: getattr(d, n) for n in BX.BoxFilter.FIELDS}
    blk = BX.BoxFilter(q_vel=0.5, max_gap=7, size_percent=33).block()
    assert (blk.q_vel, blk.max_gap, blk.size_percent, blk.p0_vel, blk.symmetry) == (0.5, 7, 33, 10000.0, 4)
    assert (BX.FLAG_DUPLICATE, BX.FLAG_TRACKS, BX.FILTER_MAX_GAP) == (K.FLAG_DUPLICATE, K.FLAG_TRACKS, K.MAX_GAP)


def test_bad_buffers_are_refused():
    B, R = 2, 8
    log = RL.ResultLog(B, 4, 3, R, 16, device="cpu")
    boxes = BX.ObjectBoxes.empty(B, R, "cpu")
    with pytest.raises(ValueError, match="BoxFilter"):
        log.filter_boxes(boxes, filter=dict(smooth=1))
    with pytest.raises(ValueError, match="boxes: box"):
        log.filter_boxes(BX.ObjectBoxes.empty(B, R + 1, "cpu"))
    with pytest.raises(ValueError, match="keep"):
        log.filter_boxes(boxes, keep=torch.zeros(B, R - 1, dtype=torch.uint8))
    good = lambda: BX.FilteredBoxes.empty(B, R, "cpu")
    BX.check_filtered_into(good(), B, R, "cpu")
    cases = {"box": torch.zeros(B, R, 7, dtype=torch.float64), "valid": torch.zeros(B, R), "flags": None, "vel": torch.zeros(B, R, 3, dtype=torch.float64),
             "state": torch.zeros(B, R, 16), "aligned": torch.zeros(B, 4, R, dtype=torch.float64).transpose(1, 2),
             "link": torch.zeros(B, R, 4, dtype=torch.int64)}
    for name, bad in cases.items():
        into = good()
        setattr(into, name, bad)
        with pytest.raises(ValueError, match="into.%s" % name):
            log.filter_boxes(boxes, into=into)
    into = good()
    into.box = boxes.box
    with pytest.raises(ValueError, match="share"):
        log.filter_boxes(boxes, into=into)
    with pytest.raises(ValueError, match="into.box"):
        log.filter_boxes(boxes, into=object())
