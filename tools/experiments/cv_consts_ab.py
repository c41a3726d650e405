#!/usr/bin/env python3
"""The forward cost volume alone at the bench shape: its constants in LDS (the product's kernel) against the same kernel reading them
from global memory on every tile (rtk_cost_volume_split_gconst), in ONE process, alternating.

Both variants go through the entry point without the per-sample term, on the operands of a backbone() call with the term folded into p1
(the only difference between the two launches is the kernel).  Prints, per round and variant, the median of --iters launches, then per
variant the median over the rounds and the spread (max - min) of the rounds' medians.

    python tools/experiments/cv_consts_ab.py [--batch 64] [--rounds 5] [--iters 30] [--workgroups 0]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ENTRY = {"lds": "rtk_cost_volume_split_shared", "gconst": "rtk_cost_volume_split_gconst"}


def variant_launcher(eng, variant, workgroups=0):
    """-> go(): one launch of the forward cost volume `variant` on the operands of the engine's last backbone() call."""
    from ratrack_amd import _lib
    from ratrack_amd import fused as F
    assert eng._last_cv is not None, "run backbone() first"
    B, N, x1, x2, knn, p1, p2, cor, st = eng._last_cv
    if st is not None:
        p1 = p1 + st.repeat_interleave(N, 0)
    keep = (p1,)

    def go():
        _lib.call(ENTRY[variant], B, N, N, x1.data_ptr(), x2.data_ptr(), knn.data_ptr(), keep[0].data_ptr(), p2.data_ptr(), eng.cv_wd.data_ptr(),
                  eng.cv_images.data_ptr(), eng.cv_scales.data_ptr(), eng.cv_bias23[0].data_ptr(), eng.cv_bias23[1].data_ptr(), eng.wn1.arr,
                  cor.data_ptr(), 256, workgroups, F._stream())
    return go


def time_launches(go, iters):
    """-> milliseconds of `iters` launches, each between two events on the current stream."""
    import torch
    ev = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        go()
        e1.record()
        ev.append((e0, e1))
    torch.cuda.synchronize()
    return [s.elapsed_time(e) for s, e in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--workgroups", type=int, default=0)
    ap.add_argument("--so", default=None, help="another build of the library (tools/experiments/ab_lib.py --build)")
    a = ap.parse_args()
    if a.so:
        import ratrack_amd._lib as L
        L.SO_PATH = os.path.abspath(a.so)
        print("library:", a.so)
    import torch
    from ratrack_amd import synth
    from ratrack_amd.track4d import Args, Track4D
    net = Track4D(Args()).to("cuda").eval()
    synth.fill_state_dict(net.state_dict())
    net.invalidate_fused()
    d = synth.make_frame_pairs(a.batch, 256, 1)
    t = [torch.from_numpy(d[k]).to("cuda") for k in ("pc1", "pc2", "feature1", "feature2")]
    med = {v: [] for v in ENTRY}
    with torch.no_grad():
        net.backbone(*t, None)
        eng = net._fused_engine()
        go = {v: variant_launcher(eng, v, a.workgroups) for v in ENTRY}
        for v in ENTRY:
            time_launches(go[v], 10)
        for r in range(a.rounds):
            for v in (("lds", "gconst") if r % 2 == 0 else ("gconst", "lds")):
                ms = sorted(time_launches(go[v], a.iters))
                med[v].append(ms[len(ms) // 2] * 1e3)
                print("round %d  %-6s  median %.1f us  (min %.1f max %.1f of %d)" % (r, v, med[v][-1], ms[0] * 1e3, ms[-1] * 1e3, a.iters))
    for v in ENTRY:
        m = sorted(med[v])
        print("B=%d workgroups=%d  %-6s  median of rounds %.1f us, spread of rounds %.1f us" % (a.batch, a.workgroups, v, m[len(m) // 2], m[-1] - m[0]))
    m = {v: sorted(med[v])[len(med[v]) // 2] for v in ENTRY}
    print("lds / gconst = %.4f" % (m["lds"] / m["gconst"]))


if __name__ == "__main__":
    main()
