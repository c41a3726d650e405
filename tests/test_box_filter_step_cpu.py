"""CPU: the host statement of the filter inside the tracked step (tests/_box_filter_step_util.py) against the offline rule it must
reproduce (tests/_box_filter_util.py, `filter_log` with smooth = 0 and size_rule = 0), and the argument checks of the option.  Every
comparison is of bits."""
import numpy as np
import pytest

import _box_filter_step_util as S
import _box_filter_util as K
from ratrack_amd import boxes as BX, tracker as T


def offline_of(steps, par):
    streams, where = S.as_log(steps)
    host = K.ids_log(streams)
    box, valid = S.record_boxes(steps, where, host.R)
    return K.filter_log(host.tables(), box, valid, par=par), where


@pytest.mark.parametrize("symmetry", [2, 4])
def test_the_statement_equals_the_offline_rule(symmetry):
    """The statement walked over the scripted sequence (every case of the rule) and over random full tables gives every measured row
    the bits `filter_log` gives its record, for box, vel, state, aligned and gap."""
    rng = np.random.default_rng(41)
    for name, g, steps in (("scripted", 2, S.scripted(rng, max_gap=2)[0]), ("scripted", 3, S.scripted(rng, max_gap=3)[0]),
                           ("random", 2, S.tables_of(rng, 3, 12, S.random_frames(rng, 3, 12, 14, 2)))):
        par = K.Par(symmetry=symmetry, max_gap=g, q_vel=0.25, r_yaw=0.5)
        res = S.walk(steps, par)
        offline, where = offline_of(steps, par)
        assert offline["flags"].tolist() == [0, 0, 0]
        members, continuing = S.compare_with_offline(steps, res, offline, where)
        gaps = {int(v) for r in res for v in r["out"]["gap"].reshape(-1)}
        assert members > 60 and continuing > 40 and gaps >= {-1, 1, g}, (name, members, continuing, gaps)
        # a row that is not measured has no record with a box, and the state of a carried row is its previous row's, bit for bit
        for t in range(1, len(steps)):
            s = steps[t]
            for b in range(3):
                for r in range(int(s["count_new"][b]) if s["active"][b] else 0):
                    if res[t]["since"][b, r] > 0:
                        prev = s["ids_prev"][b, :int(s["count_prev"][b])].tolist().index(int(s["ids_new"][b, r]))
                        assert S.same_bits(res[t]["state"][b, r], res[t - 1]["state"][b, prev]) and res[t]["out"]["valid"][b, r] == 0
                        assert res[t]["since"][b, r] == res[t - 1]["since"][b, prev] + 1


def test_the_scripted_sequence_holds_every_case():
    """What the GPU tests rely on, checked where it is cheap."""
    steps, marks = S.scripted(np.random.default_rng(42), max_gap=2)
    S.assert_cases(steps, marks, 2)


def test_the_option_is_checked_before_a_device_is_touched():
    class Net:
        training = False
        min_obj_points = 2

    with pytest.raises(ValueError, match="boxes=True"):
        T.BatchedTracker(Net(), streams=2, box_filter=BX.BoxFilter())
    for kw in (dict(smooth=1), dict(size_rule=1)):
        with pytest.raises(ValueError, match="causal.*ResultLog.filter_boxes"):
            BX.check_step_filter(BX.BoxFilter(**kw))
        with pytest.raises(ValueError, match="causal.*ResultLog.filter_boxes"):
            T.BatchedTracker(Net(), streams=2, boxes=True, box_filter=BX.BoxFilter(**kw))
    with pytest.raises(ValueError, match="BoxFilter"):
        BX.check_step_filter(dict(max_gap=2))
    flt = BX.BoxFilter(max_gap=3)
    assert BX.check_step_filter(flt) is flt
