"""CPU: coasted tracks that move (BatchedTracker(motion="flow"), rtk_track_memory_motion in csrc/track_motion.hip) -- declared, built
without scratch, arguments refused before any launch, and the host statement of its rules (tests/_track_motion_util.py) on
hand-written tables."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _track_memory_util as U
import _track_motion_util as MU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_header_and_abi_declare_the_entry_point_and_the_keywords_exist():
    import ctypes
    from ratrack_amd import abi, tracker as T, track_train as TT
    text = open(os.path.join(ROOT, "include", "rtk_fused.h")).read()
    assert re.search(r"RTK_EXPORT int rtk_track_memory_motion\(int B, int K, int max_age, float beta,", text)
    assert "rtk_track_memory_motion below" in text              # the pointer from rtk_track_memory's comment, whose wording stays
    assert "no motion model: a coasted" in text
    sig = abi.SIGNATURES["rtk_track_memory_motion"]
    assert sig[:4] == [ctypes.c_int] * 3 + [ctypes.c_float] and sig[4:] == [ctypes.c_void_p] * 25
    for cls in (T.BatchedTracker, TT.SequenceTrainer, TT._TrainTracker):
        p = inspect.signature(cls.__init__).parameters
        assert p["motion"].default is None and p["motion_beta"].default == 1.0, cls
    assert os.path.exists(os.path.join(ROOT, "ratrack_amd", "csrc", "track_motion.hip"))


def test_bad_motion_keywords_are_refused():
    from ratrack_amd import tracker as T, track_train as TT
    from ratrack_amd.track4d import Args, Track4D
    net = Track4D(Args()).eval()
    with pytest.raises(ValueError, match="max_age"):
        T.BatchedTracker(net, streams=2, motion="flow")
    for bad in ("kalman", "Flow", 1, True):
        with pytest.raises(ValueError, match="motion="):
            T.BatchedTracker(net, streams=2, max_age=2, motion=bad)
    for bad in (0.0, -0.5, 1.5, float("nan"), "0.5", None, True):
        with pytest.raises(ValueError, match="motion_beta"):
            T.BatchedTracker(net, streams=2, max_age=2, motion="flow", motion_beta=bad)
    with pytest.raises(ValueError, match="motion_beta"):
        T.BatchedTracker(net, streams=2, max_age=2, motion_beta=0.5)
    with pytest.raises(ValueError, match="motion_beta"):
        T.BatchedTracker(net, streams=2, motion_beta=0.5)
    with pytest.raises(ValueError, match="reacquire"):
        TT.SequenceTrainer(net, streams=2, motion="flow")
    with pytest.raises(ValueError, match="motion="):
        TT.SequenceTrainer(net, streams=2, reacquire=2, motion="kalman")
    with pytest.raises(ValueError, match="motion_beta"):
        TT.SequenceTrainer(net, streams=2, reacquire=2, motion="flow", motion_beta=0.0)


def test_track_motion_kernel_builds_for_gfx950_without_scratch(tmp_path):
    from ratrack_amd import build as B
    hipcc = B._hipcc()
    src = os.path.join(B.CSRC, "track_motion.hip")
    out = str(tmp_path / "track_motion.s")
    cmd = [hipcc] + [f for f in B.flags_for(src) if f != "-fPIC"] + ["-I", os.path.join(ROOT, "include"), "-I", B.CSRC, "-S",
                                                                    "--cuda-device-only", "-o", out, src]
    subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
    asm = open(out).read()
    notes = asm[asm.index("amdhsa.kernels"):]
    found = {}
    for e in re.split(r"\n\s+- \.", notes):
        m = re.search(r"\.name:\s+(\S+)", e)
        p = re.search(r"\.private_segment_fixed_size:\s+(\d+)", e)
        if m and p:
            found[m.group(1)] = int(p.group(1))
    assert [v for k, v in found.items() if "track_motion_kernel" in k] == [0], found
    assert not [k for k in found if "track_memory_kernel" in k], found        # that name belongs to track_batched.hip's one kernel


def _call_fails(name, *args):
    from ratrack_amd import _lib, fused  # noqa: F401
    with pytest.raises(_lib.RtkError) as e:
        _lib.call(name, *args)
    return str(e.value)


NAMES = ["active", "reset", "num_objects", "indices1", "object_conf", "prev_ids", "prev_age", "prev_hits", "prev_n_det", "prev_count",
         "desc_prev", "prev_vel", "ids", "age", "hits", "n_det", "count", "desc", "vel", "flags", "object_hits", "object_gap", "num_coasted",
         "object_velocity"]


def test_track_memory_motion_arguments_are_validated_before_any_launch():
    from ratrack_amd import tracker as T
    kmax = T.max_objects_limit()
    fake, other = 4096, 8192          # never dereferenced: the checks fail first

    def args(B=2, K=8, max_age=2, beta=0.5, **over):
        vals = {n: (other if n in ("ids", "age", "hits", "n_det", "count", "desc", "vel") else fake) for n in NAMES}
        vals.update(active=None, reset=None)
        vals.update(over)
        return [B, K, max_age, beta] + [vals[n] for n in NAMES] + [None]
    call = lambda **kw: _call_fails("rtk_track_memory_motion", *args(**kw))
    for beta in (0.0, 1.5, -0.25, float("nan")):
        assert "beta=" in call(beta=beta), beta
    for name in ("prev_vel", "vel", "object_velocity"):
        assert "bad arguments" in call(**{name: None}), name
    assert "alias" in call(vel=fake)
    # the remaining checks are rtk_track_memory's
    assert "K=%d" % (kmax + 1) in call(K=kmax + 1)
    assert "K=0" in call(K=0)
    assert "max_age=-1" in call(max_age=-1)
    assert "bad arguments" in call(B=0)
    for name in NAMES[2:]:
        assert "bad arguments" in call(**{name: None}), name
    for name in ("ids", "age", "hits", "desc"):
        assert "alias" in call(**{name: fake}), name


# ---- the host statement on hand-written tables --------------------------------------------------------------------------------------
def table(K, ids, age, hits, n_det):
    t = U.empty_table(K)
    c = len(ids)
    t["ids"][:c], t["age"][:c], t["hits"][:c] = ids, age, hits
    t.update(n_det=n_det, count=c)
    return t


def pad(x, K, fill):
    return list(x) + [fill] * (K - len(x))


def descs(K, centres, flows, seed=0):
    """A (K,141) float32 descriptor table: random words with the given centres (channels 0..2) and mean flows (134..136)."""
    d = np.random.default_rng(seed).standard_normal((K, MU.DESC)).astype(f32)
    d[len(centres):] = 0
    for r, (c, f) in enumerate(zip(centres, flows)):
        d[r, :3], d[r, MU.FLOW] = f32(c), f32(f)
    return d


def same(a, b):
    return np.array_equal(MU.ibits(a), MU.ibits(b))


def test_host_statement_fresh_and_inherited_velocities():
    K = 4
    prev = table(K, ids=[5, 6], age=[0, 0], hits=[2, 1], n_det=2)
    prev_vel = np.zeros((K, 3), f32)
    prev_vel[0], prev_vel[1] = f32([0.1, 0.2, 0.3]), f32([1.0, 0.0, 0.0])
    prev_desc = descs(K, [[0, 0, 0], [10, 0, 0]], [[0.1, 0.2, 0.3], [1, 0, 0]], seed=1)
    cur = descs(K, [[0.1, 0.2, 0.3], [50, 0, 0]], [[0.3, 0.1, -0.7], [0.9, 0.8, 0.7]], seed=2)
    # object 0 inherits row 0; object 1 is fresh (conf 0)
    call = lambda beta: MU.host_step_motion(prev, prev_vel, prev_desc, cur, pad([0, 1], K, -1), pad([0.9, 0.0], K, 0.0), 2, pad([5, 40], K, -1),
                                            False, True, 2, beta)
    new, vel, tab, out = call(1.0)
    assert same(vel[0], cur[0, MU.FLOW]) and same(vel[1], cur[1, MU.FLOW])             # beta = 1: the measured flow, bit for bit
    assert same(out["object_velocity"][:2], vel[:2]) and same(out["object_velocity"][2:], np.zeros((2, 3)))
    assert same(tab[:2], cur[:2])                                                       # a current row's descriptor is not touched
    new, vel, tab, out = call(0.25)
    v, f = prev_vel[0], cur[0, MU.FLOW]
    want = v + f32(0.25) * (f - v)
    assert want.dtype == f32 and same(vel[0], want) and not same(vel[0], f)
    assert np.allclose(vel[0], [0.15, 0.175, 0.05], atol=1e-6)
    assert same(vel[1], cur[1, MU.FLOW])                                                # fresh: no smoothing
    # row 1 of the previous table (id 6) was not matched: it coasts into row 2, moved by ITS velocity
    assert new["ids"] == [5, 40, 6, -1] and new["age"] == [0, 0, 1, 0] and out["src"] == [None, None, 1, None]
    assert same(tab[2, 3:], prev_desc[1, 3:]) and same(tab[2, :3], f32([11, 0, 0])) and same(vel[2], prev_vel[1])
    assert same(vel[3], np.zeros(3)) and same(tab[3], np.zeros(MU.DESC))


def test_host_statement_a_track_coasting_two_frames_moves_twice():
    K = 3
    step = f32([0.3, -0.1, 0.7])
    prev = table(K, ids=[9], age=[0], hits=[4], n_det=1)
    prev_vel = np.zeros((K, 3), f32)
    prev_vel[0] = step
    prev_desc = descs(K, [[1.1, 2.2, 3.3]], [[0.3, -0.1, 0.7]], seed=3)
    nothing = np.zeros((K, MU.DESC), f32)
    t1, v1, d1, o1 = MU.host_step_motion(prev, prev_vel, prev_desc, nothing, pad([], K, -1), pad([], K, 0.0), 0, pad([], K, -1), False, True, 2, 1.0)
    t2, v2, d2, o2 = MU.host_step_motion(t1, v1, d1, nothing, pad([], K, -1), pad([], K, 0.0), 0, pad([], K, -1), False, True, 2, 1.0)
    assert t1["age"][:1] == [1] and t2["age"][:1] == [2] and t2["ids"] == [9, -1, -1] and o2["num_coasted"] == 1
    once = prev_desc[0, :3] + step
    assert same(d1[0, :3], once) and same(d2[0, :3], once + step)                       # two separately rounded additions
    assert same(d2[0, 3:], prev_desc[0, 3:]) and same(v2[0], step)                      # the last measured flow stays in 134..136
    assert same(d2[0, MU.FLOW], prev_desc[0, MU.FLOW])
    # a third frame: the row dies (max_age = 2)
    t3, v3, d3, _ = MU.host_step_motion(t2, v2, d2, nothing, pad([], K, -1), pad([], K, 0.0), 0, pad([], K, -1), False, True, 2, 1.0)
    assert t3["count"] == 0 and same(v3, np.zeros((K, 3))) and same(d3, nothing)


def test_host_statement_reset_inactive_and_truncation():
    K = 4
    prev = table(K, ids=[1, 2, 3], age=[0, 1, 0], hits=[2, 3, 1], n_det=2)
    prev_vel = np.arange(12, dtype=f32).reshape(K, 3) * f32(0.1)
    prev_desc = descs(K, [[0, 0, 0], [10, 0, 0], [20, 0, 0]], [[0.1, 0, 0]] * 3, seed=4)
    cur = descs(K, [[0.1, 0, 0], [30, 0, 0]], [[0.4, 0.5, 0.6], [0.7, 0.8, 0.9]], seed=5)
    # reset: indices1 names a row, but the previous table is ignored -- no survivors, every current row takes its measured flow
    new, vel, tab, out = MU.host_step_motion(prev, prev_vel, prev_desc, cur, pad([0], K, -1), pad([0.9], K, 0.0), 1, pad([30], K, -1), True, True, 3, 0.25)
    assert new["count"] == 1 and same(vel[0], cur[0, MU.FLOW]) and same(vel[1:], np.zeros((3, 3))) and same(tab[1:], np.zeros((3, MU.DESC)))
    # inactive: every row's velocity stays (past the count too), no centre moves, nothing is reported
    new, vel, tab, out = MU.host_step_motion(prev, prev_vel, prev_desc, cur, pad([], K, -1), pad([], K, 0.0), 0, pad([], K, -1), False, False, 3, 0.25)
    assert new == prev and same(vel, prev_vel) and same(tab[:3], prev_desc[:3]) and same(out["object_velocity"], np.zeros((K, 3)))
    # truncation at K: two detections, three survivors, room for two -- in table order, each moved by its own velocity
    new, vel, tab, out = MU.host_step_motion(prev, prev_vel, prev_desc, cur, pad([-1, -1], K, -1), pad([0.0, 0.0], K, 0.0), 2, pad([20, 21], K, -1),
                                             False, True, 5, 1.0)
    assert out["truncated"] and new["ids"] == [20, 21, 1, 2] and out["src"] == [None, None, 0, 1]
    for r, i in ((2, 0), (3, 1)):
        assert same(tab[r, :3], prev_desc[i, :3] + prev_vel[i]) and same(tab[r, 3:], prev_desc[i, 3:]) and same(vel[r], prev_vel[i])


def test_frames_carry_the_flows_they_were_given():
    flows = MU.object_flows(4, b=1)
    s = MU.flow_stream(U.lattice(4), [True, False, True, True], 32, flows, points=3, seed=1)
    assert s["n_valid"] == 12
    for k in range(4):
        assert bool((s["flow"][:, 3 * k:3 * k + 3] == flows[k].view(3, 1)).all())
    assert bool((s["flow"][:, 12:] == s["flow"][:, :1]).all())
    assert len({tuple(f.tolist()) for f in flows}) == 4
    seq, vis = MU.motion_sequence(B=2, frames=3, N=64, objects=(6, 7), points=5)
    assert not bool((seq[1][0]["flow"] == seq[2][0]["flow"]).all())
