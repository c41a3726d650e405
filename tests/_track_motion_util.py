"""Shared by the track-motion tests: the host statement of rtk_track_memory_motion (include/rtk_fused.h) -- `host_step` of
tests/_track_memory_util.py for the lifecycle, numpy float32 for the velocities and the moved centres -- and frames whose objects
carry the flow the test gave them.  No GPU is needed to import this module."""
import numpy as np
import torch

import _track_memory_util as U
from _track_memory_util import host_step

DESC = U.DESC
FLOW = slice(134, 137)          # descriptor channels of the object's mean predicted scene flow


# ---- the host statement -------------------------------------------------------------------------------------------------------------
def empty_motion(K):
    """One stream's velocities and descriptor table before its first frame: (vel (K,3), desc (K,141)) float32 zeros."""
    return np.zeros((K, 3), np.float32), np.zeros((K, DESC), np.float32)


def ibits(x):
    """A float32 array as its int32 words: comparisons are on bits."""
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


def host_step_motion(prev, prev_vel, prev_desc, desc, indices1, object_conf, num_objects, object_ids, reset, active, max_age, beta):
    """One frame of one stream.  prev / indices1 / object_conf / num_objects / object_ids / reset / active / max_age: `host_step`'s.
    prev_vel (K,3), prev_desc (K,141) float32: the previous table's velocities and descriptors; desc (K,141) float32: this frame's
    descriptor table as rtk_object_descriptors left it (rows j < num_objects are read, for their mean flow and to be passed on).
    -> (new table, new_vel (K,3), new_desc (K,141) -- rows past the new count are zero --, `host_step`'s dict with object_velocity
    (K,3) added).  All arithmetic is numpy float32, one rounding per operation."""
    K = len(prev["ids"])
    prev_vel, prev_desc, desc = (np.ascontiguousarray(x, dtype=np.float32) for x in (prev_vel, prev_desc, desc))
    beta = np.float32(beta)
    new, out = host_step(prev, indices1, object_conf, num_objects, object_ids, reset, active, max_age)
    vel, table, ovel = np.zeros((K, 3), np.float32), np.zeros((K, DESC), np.float32), np.zeros((K, 3), np.float32)
    if not active:                      # no frame passed: every row's velocity stays, no centre moves
        vel[:] = prev_vel
        table[:new["count"]] = prev_desc[:new["count"]]
        return new, vel, table, dict(out, object_velocity=ovel)
    m = 0 if reset else prev["count"]
    for j in range(num_objects):
        f = desc[j, FLOW]
        i = indices1[j]
        inherited = 0 <= i < m and object_conf[j] != 0
        if inherited and beta != np.float32(1.0):
            v = prev_vel[i]
            d = (f - v).astype(np.float32)
            s = (beta * d).astype(np.float32)
            vel[j] = (v + s).astype(np.float32)
        else:
            vel[j] = f
        ovel[j] = vel[j]
        table[j] = desc[j]
    for r, i in enumerate(out["src"]):
        if i is not None:
            table[r] = prev_desc[i]
            table[r, :3] = (prev_desc[i, :3] + prev_vel[i]).astype(np.float32)
            vel[r] = prev_vel[i]
    return new, vel, table, dict(out, object_velocity=ovel)


# ---- frames ---------------------------------------------------------------------------------------------------------------------------
def set_flows(stream, flows, points):
    """Overwrites the flow of a `blob_stream` frame (which hard-codes 0.25): every point of object k gets flows[k] (3 values); the
    padding columns copy column 0 again.  -> the same dict."""
    f = torch.as_tensor(flows, dtype=torch.float32)
    n = stream["n_valid"]
    assert f.shape == (n // points, 3)
    stream["flow"][:, :n] = f.repeat_interleave(points, dim=0).t()
    stream["flow"][:, n:] = stream["flow"][:, :1]
    return stream


def flow_stream(centres, visible, N, flows, points=3, seed=0, sigma=0.05):
    """`blob_stream` with object k's points flowing by flows[k]."""
    return set_flows(U.blob_stream(centres, visible, N, points=points, seed=seed, sigma=sigma), flows, points)


def object_flows(count, b=0, step=0.2):
    """Distinct flows for `count` objects of stream b, none a short binary fraction: roughly `step` along x (the objects' true motion
    in `random_sequence`) plus a few centimetres that differ per object and axis."""
    k = torch.arange(count, dtype=torch.float32)
    return torch.stack((step + 0.0137 * (k + 1) + 0.0031 * b, 0.0071 * (k + 1) - 0.0113 * b - 0.019, -0.0053 * (k + 1) + 0.0171), dim=1)


def motion_sequence(B=3, frames=8, N=64, objects=(6, 7, 8), points=5, seed=7, step=0.2, min_visible=5):
    """`random_sequence` with the flows of `object_flows`, which change a little from frame to frame (so that a smoothed velocity
    differs from the last measurement).  -> (frames, visibility), as `random_sequence`."""
    seq, vis = U.random_sequence(B=B, frames=frames, N=N, objects=objects, points=points, seed=seed, step=step, min_visible=min_visible)
    for t, row in enumerate(seq):
        for b, s in enumerate(row):
            set_flows(s, object_flows(objects[b], b, step) * (1.0 + 0.043 * t), points)
    return seq, vis
