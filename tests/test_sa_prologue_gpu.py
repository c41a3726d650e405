"""GPU: the two-round-trip prologue of the set-abstraction scale kernels (rtk_sa_scale, rtk_sa_scale_split) and each copy of their tile
loop's body against the serial entries (rtk_sa_scale_serial, rtk_sa_scale_split_serial), bit for bit, for the six instances the PNHead
launches.  The prologue requests the un-redirected centroid and ball index of a wave's first unit before dst_nuniq[b] has arrived and
keeps them only for a unit wholly below live_c, so the duplicate-centroid counts here run through EVERY value 1 .. npoint (sample b
gets 1 + b mod npoint), which gives -- computed from the launchers' grid rule and asserted -- live_c = 1, live_c = npoint, a partial
first unit of a wave (chain instances: live_c mod CPT != 0), idle waves inside a live workgroup, workgroups that exit whole, and waves
with exactly 1, 2, 3 and 4 units (the prologue alone, the last-unit copy of the body, the copy with one unit left, the steady state).
A launch without the counters covers live_c = npoint with a null dst_nuniq.

Shapes.  A wave gets more than one unit only where the launcher halves the workgroups of a sample, which it does when samples x
workgroups exceed 1024: with 3 samples and npoint <= 520 every wave has at most one unit, so the 3-sample shape of
test_sa_pipeline_gpu.SHAPES serves the idle waves and the workgroups that exit whole, and its 300- and 520-sample shapes (n = 64,
npoint <= 74; a plain 2-D grid and the XCD-aware one) the unit counts.

What the kernels may read and discard but never USE is poisoned in the operands the default entries get (the serial entries compute the
reference on the clean ones): ball rows >= live_c past the zero tail hold an in-range index, of a source row that lies in no ball and
is NaN in q and xyz; new_xyz rows >= live_c are NaN; output rows >= live_c and the columns outside the scale's slice hold a sentinel."""
import pytest
import torch

from test_sa_pipeline_gpu import BALL_TAIL_ROWS, DEV, INSTANCES, PARTNER, RADIUS, SENT, centroids_per_tile, units_per_wave

pytestmark = pytest.mark.gpu

from ratrack_amd import fused as F  # noqa: E402

SHAPES = [(3, 48, 40), (300, 64, 72), (520, 64, 74)]


class Case:
    """One instance at one shape: clouds whose last source row lies far outside every ball, both ball tables of the level from
    rtk_ball_query_pair, weights, and the poisoned copies of the operands."""

    def __init__(self, entry, ns, c1, widths, samples, n, npoint, seed):
        from ratrack_amd import _lib
        g = torch.Generator().manual_seed(seed)
        self.entry, self.ns, self.c1, self.samples, self.n, self.npoint = entry, ns, c1, samples, n, npoint
        self.cout, self.far = widths[-1], n - 1
        xyz = torch.rand(samples, n, 3, generator=g) * (2.5 * RADIUS[ns])
        xyz[:, self.far] = 1.0e4                                                      # in no ball: the row the poison index names
        new_xyz = xyz[:, torch.randperm(n - 1, generator=g)[:npoint]] if npoint <= n - 1 else \
            torch.cat([xyz[:, :n - 1], xyz[:, :npoint - (n - 1)] + 0.25], 1)
        self.xyz, self.new_xyz = xyz.to(DEV), new_xyz.contiguous().to(DEV)
        self.dst_nu = (torch.arange(samples, dtype=torch.int32) % npoint + 1).to(DEV)      # every live_c in 1 .. npoint
        self.src_nu = torch.randint(n // 2, n - 1, (samples,), generator=g, dtype=torch.int32).to(DEV)
        ns2 = PARTNER[ns]
        (ra, na), (rb, nb) = sorted([(RADIUS[ns], ns), (RADIUS[ns2], ns2)])
        ta = torch.zeros(samples, npoint, na, dtype=torch.int32, device=DEV)
        tb = torch.zeros(samples, npoint, nb, dtype=torch.int32, device=DEV)
        _lib.call("rtk_ball_query_pair", samples, n, npoint, ra, na, rb, nb, self.new_xyz.data_ptr(), self.xyz.data_ptr(), ta.data_ptr(),
                  tb.data_ptr(), self.dst_nu.data_ptr(), F._stream())
        self.idx = ta if na == ns else tb
        self.dead = torch.arange(npoint, device=DEV)[None, :] >= self.dst_nu[:, None]           # (samples, npoint): rows >= live_c
        assert not bool((self.idx == self.far).any()), "the far row is in a ball"
        self.q = torch.randn(samples, n, c1, generator=g).to(DEV)
        rn = lambda *s: torch.randn(*s, generator=g).double()
        w1 = torch.cat([rn(c1, 3) * 0.25, rn(c1, 1) * 0.125], 1)
        self.w1img = F.offset_image(w1.to(DEV), DEV)
        layers, cin = [], c1
        for w in widths:
            layers.append(((rn(w, cin) / 8.0).to(DEV), (rn(w) * 0.125).to(DEV)))
            cin = w
        if entry == "split":
            (w2, b2), = layers
            self.img, self.inv = F.pack_split_device(w2.float().contiguous())
            self.b2 = b2.float().contiguous()
        else:
            self.chain = F.Chain([(w, b, F.ACT_RELU) for w, b in layers], DEV)
        self.out_pitch, self.out_offset = self.cout + 32, 16
        # the poisoned operands
        tail = ((self.dst_nu + BALL_TAIL_ROWS - 1) // BALL_TAIL_ROWS * BALL_TAIL_ROWS).clamp(max=npoint)
        self.p_idx = self.idx.clone()
        self.p_idx[torch.arange(npoint, device=DEV)[None, :] >= tail[:, None]] = self.far
        self.p_new_xyz = self.new_xyz.clone()
        self.p_new_xyz[self.dead] = float("nan")
        self.p_xyz, self.p_q = self.xyz.clone(), self.q.clone()
        self.p_xyz[:, self.far] = float("nan")
        self.p_q[:, self.far] = float("nan")
        self.p_q[torch.arange(n, device=DEV)[None, :] >= self.src_nu[:, None]] = float("nan")      # (as test_sa_pipeline_gpu: they alias row 0)

    def launch(self, serial, poisoned=False, counters=True):
        from ratrack_amd import _lib
        xyz, new_xyz, idx, q = (self.p_xyz, self.p_new_xyz, self.p_idx, self.p_q) if poisoned else (self.xyz, self.new_xyz, self.idx, self.q)
        q = q.reshape(self.samples * self.n, self.c1).contiguous()
        out = torch.full((self.samples * self.npoint, self.out_pitch), SENT, device=DEV)
        common = (self.samples, self.n, self.npoint, self.ns, xyz.data_ptr(), new_xyz.data_ptr(), idx.data_ptr(), q.data_ptr(), self.c1)
        tail = (out.data_ptr(), self.out_pitch, self.out_offset, self.src_nu.data_ptr() if counters else None,
                self.dst_nu.data_ptr() if counters else None, F._stream())
        if self.entry == "split":
            _lib.call("rtk_sa_scale_split" + ("_serial" if serial else ""), *common, self.c1, self.w1img.data_ptr(), self.img.data_ptr(),
                      self.inv.data_ptr(), self.b2.data_ptr(), *tail)
        else:
            _lib.call("rtk_sa_scale" + ("_serial" if serial else ""), *common, self.c1 // 16, self.w1img.data_ptr(), self.chain.n,
                      self.chain.arr, *tail)
        torch.cuda.synchronize()
        return out


def grid_cases(entry, ns, samples, npoint, dst_nu):
    """Which of the cases the docstring lists occur at this shape, by the launchers' grid rule."""
    cpt, seen = centroids_per_tile(entry, ns), set()
    for b, wgs in enumerate(units_per_wave(entry, ns, samples, npoint, dst_nu)):
        live_c = min(int(dst_nu[b]), npoint)
        live_units = -(-live_c // cpt)
        seen.update({"live_c=1"} if live_c == 1 else {"live_c=npoint"} if live_c == npoint else ())
        for x, waves in enumerate(wgs):
            if not any(waves):
                seen.add("workgroup exits whole")
                continue
            for w, units in enumerate(waves):
                if units == 0:
                    seen.add("idle wave in a live workgroup")
                else:
                    seen.add("%d units" % units if units <= 4 else ">4 units")
                    if live_c % cpt and 4 * x + w == live_units - 1:
                        seen.add("partial first unit")
    return seen


@pytest.mark.parametrize("entry,ns,c1,widths", INSTANCES, ids=["%s-%d-%d" % t[:3] for t in INSTANCES])
def test_prologue_and_every_loop_copy_match_the_serial_entries_bit_for_bit(entry, ns, c1, widths):
    seen = set()
    for k, (samples, n, npoint) in enumerate(SHAPES):
        case = Case(entry, ns, c1, widths, samples, n, npoint, seed=1000 * ns + c1 + k)
        seen |= grid_cases(entry, ns, samples, npoint, case.dst_nu.cpu())
        ref = case.launch(True)                                                          # serial, clean operands
        new = case.launch(False, poisoned=True)
        assert torch.equal(new, ref), (samples, n, npoint)
        assert torch.equal(case.launch(False), ref), (samples, n, npoint)
        rows = new.view(samples, npoint, -1)
        assert bool(case.dead.any()) and bool((rows[case.dead] == SENT).all())                   # duplicate centroids: not written
        assert bool((new[:, :case.out_offset] == SENT).all() and (new[:, case.out_offset + case.cout:] == SENT).all())
        live = rows[~case.dead][:, case.out_offset:case.out_offset + case.cout]
        assert bool(torch.isfinite(live).all()) and bool((live != SENT).all())
        # live_c = npoint with null counters (every table row is used: the clean operands, whose rows past the zero tail are zeros)
        assert torch.equal(case.launch(False, counters=False), case.launch(True, counters=False)), (samples, n, npoint)
    print("\n%s ns=%d c1=%d: %s" % (entry, ns, c1, sorted(seen)))
    want = {"live_c=1", "live_c=npoint", "idle wave in a live workgroup", "workgroup exits whole", "1 units", "2 units", "3 units", "4 units"}
    if centroids_per_tile(entry, ns) > 1:
        want.add("partial first unit")
    assert want <= seen, sorted(want - seen)


def test_backbone_is_bit_identical_with_the_serial_entries_at_64_points(monkeypatch):
    from ratrack_amd import synth
    from ratrack_amd.track4d import Args, Track4D
    net = Track4D(Args()).to(DEV).eval()
    synth.fill_state_dict(net.state_dict())
    net.invalidate_fused()
    d = synth.make_frame_pairs(2, 64, case_id=11)
    t = [torch.from_numpy(d[k]).to(DEV) for k in ("pc1", "pc2", "feature1", "feature2")]
    calls = []
    real = F._lib.call
    monkeypatch.setattr(F._lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    with torch.no_grad():
        new = [o.clone() for o in net.backbone(*t, None)]
        assert sum(c in F.SA_ENTRIES for c in calls) == 12 and not any(c in F.SA_ENTRIES_SERIAL for c in calls)
        monkeypatch.setattr(F, "SA_ENTRIES", F.SA_ENTRIES_SERIAL)
        del calls[:]
        old = [o.clone() for o in net.backbone(*t, None)]
        assert sum(c in F.SA_ENTRIES_SERIAL for c in calls) == 12 and not any(c in ("rtk_sa_scale", "rtk_sa_scale_split") for c in calls)
    assert len(new) == 7
    for a, b in zip(new, old):
        assert torch.equal(a, b)
