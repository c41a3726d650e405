"""Shared by the track-memory tests: the host statement of rtk_track_memory (include/rtk_fused.h), an Affinity whose output is known
in closed form, and a builder of frames whose objects are where the test put them.  No GPU is needed to import this module."""
import torch

DESC = 141


# ---- the host statement -------------------------------------------------------------------------------------------------------------
def empty_table(K):
    """One stream's table before its first frame."""
    return dict(ids=[-1] * K, age=[0] * K, hits=[0] * K, n_det=0, count=0)


def host_step(prev, indices1, object_conf, num_objects, object_ids, reset, active, max_age):
    """One frame of one stream.  prev: its table (`empty_table`'s keys; lists of K); indices1 / object_conf / object_ids: the K-long
    rows the association wrote for this stream, num_objects its n_b.
    -> (new table, dict(object_hits, object_gap (K-long), num_coasted, truncated, src)); src[r]: the previous row that new row r is a
    copy of (survivors), None for every other row."""
    K = len(prev["ids"])
    if not active:
        new = dict(ids=list(prev["ids"]), age=list(prev["age"]), hits=list(prev["hits"]), n_det=prev["n_det"], count=prev["count"])
        return new, dict(object_hits=[0] * K, object_gap=[-1] * K, num_coasted=prev["count"] - prev["n_det"], truncated=False,
                         src=[None] * K)
    m = 0 if reset else prev["count"]
    n = num_objects
    matched = [False] * m
    new = dict(ids=[-1] * K, age=[0] * K, hits=[0] * K, n_det=n, count=0)
    object_hits, object_gap, src = [0] * K, [-1] * K, [None] * K
    for j in range(n):
        i = indices1[j]
        inherited = 0 <= i < m and object_conf[j] != 0
        if inherited:
            assert not matched[i], "two current objects inherited previous row %d" % i
            matched[i] = True
        new["ids"][j] = object_ids[j]
        new["hits"][j] = prev["hits"][i] + 1 if inherited else 1
        object_hits[j] = new["hits"][j]
        object_gap[j] = prev["age"][i] if inherited else -1
    survivors = [i for i in range(m) if not matched[i] and prev["age"][i] + 1 <= max_age]
    for s, i in enumerate(survivors):
        r = n + s
        if r >= K:
            break
        new["ids"][r], new["age"][r], new["hits"][r], src[r] = prev["ids"][i], prev["age"][i] + 1, prev["hits"][i], i
    new["count"] = min(K, n + len(survivors))
    return new, dict(object_hits=object_hits, object_gap=object_gap, num_coasted=new["count"] - n, truncated=n + len(survivors) > K,
                     src=src)


# ---- an Affinity known in closed form -----------------------------------------------------------------------------------------------
def distance_affinity(c, s):
    """An `Affinity(141)` whose output is sigmoid(c - s * |centre_curr - centre_prev|_1) (the centre: descriptor channels 0..2)."""
    from ratrack_amd.track4d import Affinity
    aff = Affinity(DESC)
    lins = [m for m in aff.affinity if isinstance(m, torch.nn.Linear)]
    with torch.no_grad():
        for l in lins:
            l.weight.zero_()
            l.bias.zero_()
        for d in range(3):                        # layer 1: relu(+delta_d), relu(-delta_d)
            lins[0].weight[2 * d, d] = 1.0
            lins[0].weight[2 * d + 1, d] = -1.0
        lins[1].weight[0, :6] = 1.0               # layer 2: their sum = |delta|_1
        lins[2].weight[0, 0] = 1.0                # layers 3, 4: unit 0 passes through
        lins[3].weight[0, 0] = 1.0
        lins[4].weight[0, 0] = -float(s)
        lins[4].bias[0] = float(c)
    return aff


# ---- frames ---------------------------------------------------------------------------------------------------------------------------
def lattice(count, spacing=10.0, side=8):
    """`count` centres (count,3) on a lattice of the given spacing: at least `spacing` apart in xyz."""
    k = torch.arange(count)
    return torch.stack((k % side, (k // side) % side, k // (side * side)), dim=1).float() * spacing


def blob_stream(centres, visible, N, points=3, seed=0, sigma=0.05):
    """One stream's frame: object k is `points` points drawn around centres[k] (sigma 0.05), columns points*k .. points*k+points-1, so
    the objects' reference order is their index; the other clustering channels (flow, v_r, prop[0]) are constant.  visible[k] sets
    the cls of its points to 0.99 or 0.01.  The padding columns copy column 0 and are called movers: n_valid keeps them out.
    -> dict(pc1 (3,N), flow (3,N), feature1 (2,N), prop (128,N), cls (N), n_valid)."""
    g = torch.Generator().manual_seed(seed)
    n = len(visible) * points
    assert n <= N and len(centres) == len(visible)
    pc1 = torch.zeros(3, N)
    c = torch.as_tensor(centres, dtype=torch.float32)
    pc1[:, :n] = (c.repeat_interleave(points, dim=0) + sigma * torch.randn(n, 3, generator=g)).t()
    flow = torch.full((3, N), 0.25)
    f1 = torch.zeros(2, N)
    f1[0, :n] = torch.rand(n, generator=g)
    f1[1] = 0.5
    prop = torch.rand(128, N, generator=g)
    prop[0] = 0.125
    cls = torch.zeros(N)
    cls[:n] = torch.tensor([0.99 if v else 0.01 for v in visible]).repeat_interleave(points)
    for t in (pc1, flow, f1, prop):
        t[:, n:] = t[:, :1]
    cls[n:] = 0.99
    return dict(pc1=pc1, flow=flow, feature1=f1, prop=prop, cls=cls, n_valid=n)


def batch(streams, device):
    """Per-stream `blob_stream` dicts -> (pc1, feature1, flow, cls, prop, n_valid (2,B) int32) on `device`, the arguments of
    `BatchedTracker.associate` in its order."""
    st = lambda k: torch.stack([s[k] for s in streams]).to(device)
    nv = torch.tensor([[s["n_valid"] for s in streams]] * 2, dtype=torch.int32, device=device)
    return st("pc1"), st("feature1"), st("flow"), st("cls"), st("prop"), nv


def random_sequence(B=3, frames=8, N=64, objects=(6, 7, 8), points=3, seed=7, step=0.2, min_visible=4):
    """`frames` frames of B streams: stream b has objects[b] objects on a lattice, all moving `step` m per frame along x; their
    visibility bits are drawn from a seeded generator (p = 0.65), at least `min_visible` of them set in every frame.
    -> [[blob_stream dict per stream] per frame], [[visibility list per stream] per frame]."""
    g = torch.Generator().manual_seed(seed)
    seq, vis = [], []
    for t in range(frames):
        row, vrow = [], []
        for b in range(B):
            v = (torch.rand(objects[b], generator=g) < 0.65).tolist()
            k = 0
            while sum(v) < min_visible:
                v[k] = True
                k += 1
            c = lattice(objects[b]) + torch.tensor([step * t, 0.0, 0.0])
            row.append(blob_stream(c, v, N, points=points, seed=1000 * seed + 10 * t + b))
            vrow.append(v)
        seq.append(row)
        vis.append(vrow)
    return seq, vis


def written_slot(trk):
    """The slot of the tracker's double-buffered state that the last step wrote."""
    return 0 if trk.static_state else 1 - trk.cur
