"""GPU: the scorer's per-frame log and the confidence sweep over it (ratrack_amd/track_score.py `TrackScorer.sweep`,
csrc/track_score.hip `rtk_track_score_logged`, csrc/track_sweep.hip) against the host statement of tests/_track_sweep_util.py.
The device delivers integers and fixed-order float64 sums and the host does the same arithmetic on them, so everything is compared
with == / bit for bit: thresholds, levels reached, every counter at every level and stream, the IoU sums, AMOTA / sAMOTA / AMOTP."""
import ctypes

import numpy as np
import pytest
import torch

import _gt_util as U
import _track_score_util as S
import _track_sweep_util as W
from _util import reference_state_dict
from ratrack_amd import _lib, gt_device as G
from ratrack_amd import synth, tracker as T, track_score as TS, vod_gt
from ratrack_amd.track4d import Args, Track4D

pytestmark = pytest.mark.gpu
DEV = "cuda"
MATCH = ("pred_gt_slot", "pred_gt_id", "gt_pred", "iou", "aff_target", "aff_defined")
STATE = ("counters", "iou_sum", "table_key", "table_last", "table_seen", "table_matched", "table_used", "prev_gt_id", "prev_count", "prev_gt",
         "flags")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _scorer(seq, **kw):
    return TS.TrackScorer(streams=seq["B"], max_objects=seq["K"], max_boxes=seq["K"], max_gt_tracks=64, **kw)


def _feed(seq, confs, scorer, plain=None, frames=None, each=None):
    """The frames through `update_raw` with logging; with `plain`, an unlogged scorer is fed the same and every output compared."""
    K = seq["K"]
    for f, (fr, conf) in enumerate(zip(seq["frames"], confs)):
        if frames is not None and f not in frames:
            continue
        pc1, nv = _dev(fr["pc1"]), _dev(fr["n_valid"])
        gobj = TS.gt_objects(pc1, G.pack_boxes(fr["per_stream"], K, DEV), TS.pack_box_types(fr["per_stream"], K, DEV), n_valid=nv,
                             min_obj_points=S.MIN_PTS)
        args = (pc1, _dev(fr["obj"]), _dev(fr["num"]), _dev(fr["ids"]), gobj, nv, _dev(fr["reset"]), _dev(fr["active"]))
        before = scorer.log_cursor.clone()
        m = scorer.update_raw(*args, object_conf=_dev(conf))
        if plain is not None:
            m0 = plain.update_raw(*args)
            for k in MATCH:
                assert torch.equal(getattr(m, k), getattr(m0, k)), (f, k)
        if each is not None:
            each(f, fr, before, scorer.log_cursor)


def _device_scores(scorer):
    """rtk_score_track_means on the scorer's log -> (B,R) float64 host array and the cursors."""
    score = torch.zeros(scorer.B, scorer.R, dtype=torch.float64, device=DEV)
    flags = torch.zeros(scorer.B, dtype=torch.int32, device=DEV)
    lg = scorer._log_block()
    _lib.call("rtk_score_track_means", scorer.B, ctypes.addressof(lg), score.data_ptr(), flags.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert int(flags.sum()) == 0
    return score.cpu().numpy(), scorer.log_cursor.cpu().numpy()


def _check_scores(scorer, logs, host):
    """Every logged record's track score, bit for bit, in log order."""
    score, cursor = _device_scores(scorer)
    for b, lb in enumerate(logs):
        flat = [s for per in host["scores"][b] for s in per]
        assert cursor[b, 0] == len(lb) and cursor[b, 1] == len(flat) and cursor[b, 2] == sum(len(e["labels"]) for e in lb), (b, cursor[b])
        assert np.array_equal(_bits(score[b, :len(flat)]), _bits(flat)), b


def _check_log(scorer, logs):
    """The log itself: frame slots, kept labels and the four per-detection fields."""
    get = lambda n: getattr(scorer, "log_" + n).cpu().numpy()
    frame, label, track, best, conf, iou = (get(n) for n in ("frame", "label", "track", "best", "conf", "iou"))
    for b, lb in enumerate(logs):
        r = l = 0
        for f, e in enumerate(lb):
            P, Gk = len(e["dets"]), len(e["labels"])
            assert frame[b, f].tolist() == [r, l, P + 65536 * int(e["reset"]), Gk], (b, f)
            assert label[b, l:l + Gk].tolist() == e["labels"], (b, f)
            assert track[b, r:r + P].tolist() == [d[0] for d in e["dets"]] and best[b, r:r + P].tolist() == [d[2] for d in e["dets"]], (b, f)
            assert np.array_equal(conf[b, r:r + P], np.array([d[1] for d in e["dets"]], dtype=np.float32)), (b, f)
            assert np.array_equal(_bits(iou[b, r:r + P]), _bits([d[3] for d in e["dets"]])), (b, f)
            r, l = r + P, l + Gk


def _check_sweep(sw, host, L=40):
    assert sw.levels == L and sw.reached == host["reached"], (sw.reached, host["reached"])
    assert np.array_equal(_bits(sw.thresholds), _bits(host["thresholds"])), (sw.thresholds, host["thresholds"])
    assert np.array_equal(sw.counters, host["counters"]), np.argwhere(sw.counters != host["counters"])[:8]
    assert np.array_equal(_bits(sw.iou_sums), _bits(host["iou_sums"]))
    assert sw.amota == host["amota"] and sw.samota == host["samota"] and sw.amotp == host["amotp"], (sw.amota, sw.samota, sw.amotp)
    for k in range(1, host["reached"] + 1):
        assert sw.mota[k] == host["mota"][k] and sw.smota[k] == host["smota"][k], k
        assert sw.motp[k] == host["motp"][k] or (np.isnan(sw.motp[k]) and np.isnan(host["motp"][k])), k
    assert (None if sw.best is None else sw.best["level"]) == host["best"]


def _same_sweep(a, b):
    assert np.array_equal(_bits(a.thresholds), _bits(b.thresholds)) and a.reached == b.reached and np.array_equal(a.counters, b.counters)
    assert np.array_equal(_bits(a.iou_sums), _bits(b.iou_sums)) and a.amota == b.amota and a.samota == b.samota and a.amotp == b.amotp


# ---- 1: the planned sequence -------------------------------------------------------------------------------------------------------
def test_logged_scorer_equals_the_unlogged_one_and_the_sweep_equals_the_host_statement():
    seq, confs, logs, host = W.planned()
    assert (seq["B"], seq["N"], seq["K"], len(seq["frames"])) == (16, 256, 32, 12)
    scorer, plain = _scorer(seq, sweep_frames=16, sweep_records=128), _scorer(seq)
    _feed(seq, confs, scorer, plain, frames=range(0, 6))
    mid = scorer.sweep()                                   # reads only: scoring goes on
    _feed(seq, confs, scorer, plain, frames=range(6, 12))
    for k in STATE:
        assert torch.equal(getattr(scorer, k), getattr(plain, k)), k
    scorer.check()
    _check_log(scorer, logs)
    _check_scores(scorer, logs, host)
    sw = scorer.sweep(40)
    print("reached %d levels; AMOTA %.6f sAMOTA %.6f AMOTP %.6f; best %s" % (sw.reached, sw.amota, sw.samota, sw.amotp, sw.best))
    _check_sweep(sw, host)
    assert sw.reached == 31 and sw.unfiltered["tp"] == 273 and sw.unfiltered["gt"] == 363 and mid.unfiltered["frames"] < sw.unfiltered["frames"]
    # index 0 is the scorer's own count: its counters where they do not wait for a clip to close, result() everywhere, the IoU sum's bits
    dev_c, res = scorer.counters.cpu().numpy(), scorer.result()
    assert np.array_equal(sw.counters[0][:, :7], dev_c[:, :7])
    for i, k in enumerate(TS.COUNTERS):
        assert np.array_equal(sw.counters[0][:, i], res["per_stream"][k]), k
    assert np.array_equal(_bits(sw.iou_sums[0]), _bits(scorer.iou_sum.cpu().numpy()))
    # the same bits on a second sweep, and the state it read is untouched
    _same_sweep(sw, scorer.sweep(40))
    for k in STATE:
        assert torch.equal(getattr(scorer, k), getattr(plain, k)), k
    # another number of levels
    host10 = W.host_sweep(logs, L=10)
    _check_sweep(scorer.sweep(10), host10, L=10)


# ---- 2: the order of the sums -------------------------------------------------------------------------------------------------------
def test_unquantised_confidences_give_the_hosts_log_order_sums():
    seq, confs, logs, host = W.planned(raw=True)
    runs = []
    for _ in range(2):
        scorer = _scorer(seq, sweep_frames=12, sweep_records=96)
        _feed(seq, confs, scorer)
        _check_scores(scorer, logs, host)
        runs.append(scorer.sweep())
    _check_sweep(runs[0], host)
    _same_sweep(runs[0], runs[1])


# ---- 3: a log that runs out ------------------------------------------------------------------------------------------------------------
def _fitted(logs, F, R):
    """The log's own rule on the host: a frame that does not fit is not logged at all; later frames that fit are."""
    kept, dropped = [], {}
    for b, lb in enumerate(logs):
        out, r, l = [], 0, 0
        for f, e in enumerate(lb):
            if len(out) < F and r + len(e["dets"]) <= R and l + len(e["labels"]) <= R:
                out.append(e)
                r, l = r + len(e["dets"]), l + len(e["labels"])
            else:
                dropped.setdefault(b, []).append(f)
        kept.append(out)
    return kept, dropped


def _overflow_case(F, R, expect):
    seq, confs, logs, _ = W.planned()
    kept, dropped = _fitted(logs, F, R)
    assert sorted(dropped) == expect, dropped
    scorer, plain = _scorer(seq, sweep_frames=F, sweep_records=R), _scorer(seq)
    _feed(seq, confs, scorer, plain)
    flags = scorer.flags.cpu().tolist()
    assert flags == [TS.FLAG_LOG if b in dropped else 0 for b in range(seq["B"])], flags
    for k in STATE[:-1]:                                    # the score itself does not depend on the log
        assert torch.equal(getattr(scorer, k), getattr(plain, k)), k
    for call in (scorer.check, scorer.sweep, scorer.result):
        with pytest.raises(RuntimeError, match="stream %d has a frame that did not fit its log of sweep_frames=%d" % (expect[0], F)):
            call()
    _check_log(scorer, kept)                                # nothing of a dropped frame is there, and nothing is truncated
    sw = scorer.sweep(check=False)
    host = W.host_sweep(kept)
    _check_sweep(sw, host)
    assert sw.flags.tolist() == flags
    return sw, dropped


def test_a_stream_that_runs_out_of_records_is_flagged_and_the_others_are_intact():
    _, _, logs, full = W.planned()
    need = [max(sum(len(e["dets"]) for e in lb), sum(len(e["labels"]) for e in lb)) for lb in logs]
    top = int(np.argmax(need))
    R = sorted(need)[-2]
    assert need[top] > R and sum(1 for v in need if v > R) == 1, need
    sw, dropped = _overflow_case(16, R, [top])
    print("stream %d needs %d entries, sweep_records=%d: frames %s of it are not logged" % (top, need[top], R, dropped[top]))
    # the unfiltered replay of every other stream is what the full log gives
    others = [b for b in range(len(logs)) if b != top]
    assert np.array_equal(sw.counters[0][others], full["counters"][0][others])
    assert sw.counters[0][top, 0] == full["counters"][0][top, 0] - len(dropped[top])


def test_streams_that_run_out_of_frames_are_flagged():
    _, _, logs, full = W.planned()
    F = max(len(lb) for lb in logs) - 1
    long = [b for b, lb in enumerate(logs) if len(lb) > F]
    assert 0 < len(long) < len(logs)
    sw, dropped = _overflow_case(F, 128, long)
    assert all(v == [F] for v in dropped.values())
    others = [b for b in range(len(logs)) if b not in long]
    assert np.array_equal(sw.counters[0][others], full["counters"][0][others])


# ---- 4: masks ------------------------------------------------------------------------------------------------------------------------
def test_inactive_streams_append_nothing_and_a_reset_opens_a_new_clip():
    seq, confs, logs, host = W.planned()
    scorer = _scorer(seq, sweep_frames=12, sweep_records=96)
    seen = dict(inactive=0)

    def each(f, fr, before, after):                        # on the device: no download inside the loop
        act = _dev(fr["active"]).bool()
        assert torch.equal(after[~act], before[~act]), f
        assert torch.equal(after[act][:, 0], before[act][:, 0] + 1), f
        assert torch.equal(after[act][:, 1], before[act][:, 1] + _dev(fr["num"])[act]), f
        seen["inactive"] += int((~act).sum())

    _feed(seq, confs, scorer, each=each)
    assert seen["inactive"] > 0
    # two calls with identical host arguments append two frames
    twice = _scorer(seq, sweep_frames=4, sweep_records=64)
    _feed(seq, confs, twice, frames=[0])
    _feed(seq, confs, twice, frames=[0])
    cur = twice.log_cursor.cpu().numpy()
    act = seq["frames"][0]["active"].astype(bool)
    assert (cur[act, 0] == 2).all() and (cur[act, 1] == 2 * seq["frames"][0]["num"][act]).all()
    # a reset at frame 6: the stream's tracks have one score per clip
    _check_scores(scorer, logs, host)
    split = 0
    for b, tab in enumerate(host["tables"]):
        if not seq["frames"][6]["reset"][b]:
            assert {c for c, _ in tab} <= {1}, b
            continue
        for tid in {t for _, t in tab}:
            split += int((1, tid) in tab and (2, tid) in tab and tab[(1, tid)] != tab[(2, tid)])
    assert split > 0
    _check_sweep(scorer.sweep(), host)


# ---- 5: behind the tracker ---------------------------------------------------------------------------------------------------------
def test_tracker_confidences_reach_the_sweep_through_update():
    sd = reference_state_dict(DEV)
    sd["fd_layer.cp.linear.bias"] = sd["fd_layer.cp.linear.bias"] + 0.09      # moving points in every frame (tests/test_tracker_gpu.py)
    net = Track4D(Args()).to(DEV)
    net.load_state_dict(sd, strict=True)
    net = net.eval()
    B, K, steps = 4, 8, 6
    trk = T.BatchedTracker(net, streams=B)
    t = {k: torch.from_numpy(v) for k, v in synth.make_frame_pairs(B, 128, case_id=50).items()}
    pairs = [(t["pc1"][i:i + 1], t["pc2"][i:i + 1], t["feature1"][i:i + 1], t["feature2"][i:i + 1]) for i in range(B)]
    per_stream = []
    for b in range(B):
        p = t["pc1"][b].numpy()
        mk = lambda k: vod_gt.Label("rider" if k == 2 else "Car", k, 0, 0, 0, 0, 0, 0, 3.0, 4.0, 6.0, float(p[0, 10 * k]), float(p[1, 10 * k]),
                                    float(p[2, 10 * k]), 0.3 * k)
        labels = {k: mk(k) for k in range(6)}
        per_stream.append((labels, U.IDENTITY_TF, labels, U.IDENTITY_TF))
    bb, types = G.pack_boxes(per_stream, K, DEV), TS.pack_box_types(per_stream, K, DEV)
    scorer = TS.TrackScorer(streams=B, max_objects=trk.K, max_boxes=K, max_gt_tracks=32, sweep_frames=8, sweep_records=8 * trk.K)
    kept = []
    for step in range(steps):
        pc1, pc2, f1, f2, nv = vod_gt.pad_frame_pairs(pairs, device=DEV)
        reset = torch.tensor([step == 0, step in (0, 3), step == 0, step == 0], dtype=torch.uint8, device=DEV)
        active = torch.ones(B, dtype=torch.uint8, device=DEV)
        with torch.no_grad():
            flow, h, cls, _, _, _, prop = net._fused_engine().backbone(pc1, pc2, f1, f2, trk.h, n_valid=nv)
        out = trk.associate(pc1, f1, flow, cls, prop, nv, reset, active)
        gobj = TS.gt_objects(pc1, bb, types, n_valid=nv, min_obj_points=net.min_obj_points)
        scorer.update(out, gobj, reset=reset, active=active)
        trk.h = h
        kept.append((pc1, nv, out, reset))
    scorer.check()
    logs, nonzero = [[] for _ in range(B)], 0
    for pc1, nv, out, reset in kept:
        out.check()
        p1, obj, ids, conf, num = (x.cpu().numpy() for x in (pc1, out.obj, out.object_ids, out.object_conf, out.num_objects))
        for b in range(B):
            n = int(nv[0, b])
            r = S.host_gt_objects(per_stream[b], p1[b], n, min_pts=net.min_obj_points)
            objects = S.objects_dict(p1[b], obj[b, :n], ids[b], int(num[b]))
            logs[b].append(W.frame_entry(r, objects, conf[b, :len(objects)], bool(reset[b])))
            nonzero += int((conf[b, :len(objects)] != 0).sum())
    host = W.host_sweep(logs)
    assert nonzero > 0 and host["counters"][0].sum(axis=0)[3] > 0            # confidences and true positives to sweep over
    _check_log(scorer, logs)
    _check_scores(scorer, logs, host)
    sw = scorer.sweep()
    print("behind the tracker: %d non-zero confidences, reached %d levels, AMOTA %.6f sAMOTA %.6f AMOTP %.6f"
          % (nonzero, sw.reached, sw.amota, sw.samota, sw.amotp))
    _check_sweep(sw, host)
    res = scorer.result()
    for i, k in enumerate(TS.COUNTERS):
        assert np.array_equal(sw.counters[0][:, i], res["per_stream"][k]), k
