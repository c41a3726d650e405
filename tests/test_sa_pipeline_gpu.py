"""GPU: the software-pipelined tile loops of the set-abstraction scales (rtk_sa_scale, rtk_sa_scale_split) against the serial loops they
replaced (rtk_sa_scale_serial, rtk_sa_scale_split_serial), bit for bit, on ball tables built by rtk_ball_query_pair -- for the six
instances the PNHead launches, at shapes where the launchers' grid rule gives the waves 0, 1, 2 and >= 4 units and some waves of a
workgroup one unit more than others (computed here from that rule and asserted), with duplicate-centroid counters that leave one live
unit or a last tile that straddles the count, duplicate-source counters below the ball indices, and with everything the serial loop
does not read poisoned: a read the parent does not make shows as a mismatch."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

from ratrack_amd import fused as F  # noqa: E402

SA_WGS = 1024                # SA_MAX_WGS (fused_group.hip) and SA_WGS_TARGET (fused_split.hip)
BALL_TAIL_ROWS = 32          # RTK_BALL_TAIL_ROWS (rtk_common.h)
SENT = -7.5
RADIUS = {4: 2.0, 8: 4.0, 16: 8.0, 32: 16.0}
PARTNER = {4: 8, 8: 4, 16: 32, 32: 16}          # rtk_ball_query_pair fills two tables: the other scale of the level
# (entry, nsample, c1, widths after the offset layer): sa1 both scales and sa2 scale 0 on the chain kernel, the 64-channel scales split
INSTANCES = [("chain", 4, 16, (16, 32)), ("chain", 8, 16, (16, 32)), ("chain", 8, 32, (32,)),
             ("split", 32, 64, (64,)), ("split", 16, 64, (64,)), ("split", 16, 32, (64,))]
# (samples, n, npoint): a plain 2-D grid with idle waves, one unit per wave or a few, an odd sample count whose workgroups are halved
# until they fit, and the XCD-aware grid (samples % 8 == 0) with one workgroup per sample (every wave four units and more)
SHAPES = [(3, 48, 40), (130, 64, 64), (300, 64, 72), (520, 64, 74)]


def centroids_per_tile(entry, ns):
    return (16 // ns if ns < 16 else 1) if entry == "chain" else 32 // ns


def units_per_wave(entry, ns, samples, npoint, dst_nu):
    """[per sample: [per workgroup: [units of wave 0..3]]] by the launchers' rule: ceil(units / 4) workgroups per sample, halved while
    workgroups * samples exceed SA_WGS; wave w of workgroup x takes units 4 x + w, + 4 workgroups, ...; a workgroup whose first unit is
    past the live ones exits."""
    cpt = centroids_per_tile(entry, ns)
    bx = (-(-npoint // cpt) + 3) // 4
    while bx * samples > SA_WGS and bx > 1:
        bx = (bx + 1) // 2
    out = []
    for b in range(samples):
        live = -(-min(int(dst_nu[b]), npoint) // cpt)
        out.append([[len(range(4 * x + w, live, 4 * bx)) for w in range(4)] for x in range(bx)])
    return out


def dst_counts(samples, npoint, seed):
    g = torch.Generator().manual_seed(seed)
    choice = torch.tensor([npoint, 1, 7, npoint - 1], dtype=torch.int32)
    nu = choice[torch.randint(0, 4, (samples,), generator=g)]
    nu[:4] = choice[:min(4, samples)] if samples >= 4 else choice[:samples]          # every count at least once
    return nu


class Case:
    """One instance at one shape: clouds, both ball tables of the level from rtk_ball_query_pair, weights, and the poison."""

    def __init__(self, entry, ns, c1, widths, samples, n, npoint, seed):
        from ratrack_amd import _lib
        g = torch.Generator().manual_seed(seed)
        self.entry, self.ns, self.c1, self.samples, self.n, self.npoint = entry, ns, c1, samples, n, npoint
        self.cout = widths[-1]
        xyz = torch.rand(samples, n, 3, generator=g) * (2.5 * RADIUS[ns])
        self.xyz = xyz.to(DEV)
        self.new_xyz = xyz[:, torch.randperm(n, generator=g)[:npoint] % n].contiguous().to(DEV) if npoint <= n else \
            torch.cat([xyz, xyz[:, :npoint - n] + 0.25], 1).contiguous().to(DEV)
        self.dst_nu = dst_counts(samples, npoint, seed + 1).to(DEV)
        # duplicate source rows: the balls are searched over all n points, so indices >= src_nuniq occur and alias row 0
        self.src_nu = torch.randint(n // 2, n - 1, (samples,), generator=g, dtype=torch.int32).to(DEV)
        ns2 = PARTNER[ns]
        (ra, na), (rb, nb) = sorted([(RADIUS[ns], ns), (RADIUS[ns2], ns2)])
        ta = torch.zeros(samples, npoint, na, dtype=torch.int32, device=DEV)
        tb = torch.zeros(samples, npoint, nb, dtype=torch.int32, device=DEV)
        _lib.call("rtk_ball_query_pair", samples, n, npoint, ra, na, rb, nb, self.new_xyz.data_ptr(), self.xyz.data_ptr(), ta.data_ptr(),
                  tb.data_ptr(), self.dst_nu.data_ptr(), F._stream())
        self.idx = ta if na == ns else tb
        live = torch.arange(npoint, device=DEV)[None, :] < self.dst_nu[:, None]
        assert bool((self.idx[live] >= self.src_nu[:, None, None].expand_as(self.idx)[live]).any()), "no index beyond src_nuniq"
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

    def poisoned(self):
        """(idx, q) with what neither loop may read made harmful: the index rows past the zero tail of each sample's table hold in-range
        but wrong indices, the q rows >= src_nuniq NaN."""
        idx, q = self.idx.clone(), self.q.clone()
        g = torch.Generator().manual_seed(5)
        wrong = torch.randint(0, self.n, idx.shape, generator=g, dtype=torch.int32).to(DEV)
        tail = ((self.dst_nu + BALL_TAIL_ROWS - 1) // BALL_TAIL_ROWS * BALL_TAIL_ROWS).clamp(max=self.npoint)
        past = torch.arange(self.npoint, device=DEV)[None, :] >= tail[:, None]
        idx[past] = wrong[past]
        q[torch.arange(self.n, device=DEV)[None, :] >= self.src_nu[:, None]] = float("nan")
        return idx, q

    def launch(self, serial, idx=None, q=None, counters=True):
        from ratrack_amd import _lib
        idx = self.idx if idx is None else idx
        q = (self.q if q is None else q).reshape(self.samples * self.n, self.c1).contiguous()
        out = torch.full((self.samples * self.npoint, self.out_pitch), SENT, device=DEV)
        common = (self.samples, self.n, self.npoint, self.ns, self.xyz.data_ptr(), self.new_xyz.data_ptr(), idx.data_ptr(), q.data_ptr(), self.c1)
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


@pytest.mark.parametrize("entry,ns,c1,widths", INSTANCES, ids=["%s-%d-%d" % t[:3] for t in INSTANCES])
def test_pipelined_loop_matches_the_serial_loop_bit_for_bit(entry, ns, c1, widths):
    seen, uneven = set(), False
    for k, (samples, n, npoint) in enumerate(SHAPES):
        case = Case(entry, ns, c1, widths, samples, n, npoint, seed=100 * ns + c1 + k)
        for wgs in units_per_wave(entry, ns, samples, npoint, case.dst_nu.cpu()):
            for waves in wgs:
                seen.update(waves)
                uneven |= waves[0] > 0 and len(set(w for w in waves if w > 0)) > 1
        new, old = case.launch(False), case.launch(True)
        assert torch.equal(new, old), (samples, n, npoint)
        rows = torch.arange(npoint, device=DEV)[None, :] >= case.dst_nu[:, None]
        assert bool((new.view(samples, npoint, -1)[rows] == SENT).all())                       # duplicate centroids: not written
        assert bool((new[:, :case.out_offset] == SENT).all() and (new[:, case.out_offset + case.cout:] == SENT).all())
        assert bool((new.view(samples, npoint, -1)[~rows][:, case.out_offset:case.out_offset + case.cout] != SENT).all())
        if k == 1:                                                                            # without the counters: every row live
            assert torch.equal(case.launch(False, counters=False), case.launch(True, counters=False))
    print("\n%s ns=%d c1=%d: units per wave seen %s, uneven workgroups %s" % (entry, ns, c1, sorted(seen), uneven))
    assert {0, 1, 2} <= seen and max(seen) >= 4 and uneven, (sorted(seen), uneven)


@pytest.mark.parametrize("entry,ns,c1,widths", INSTANCES, ids=["%s-%d-%d" % t[:3] for t in INSTANCES])
def test_prefetching_reads_nothing_the_serial_loop_does_not_read(entry, ns, c1, widths):
    """Wrong indices in the table rows past each sample's zero tail, NaN in the q rows >= src_nuniq: the outputs are still the serial
    loop's on the clean operands, finite, and the sentinel stays in every row >= dst_nuniq."""
    samples, n, npoint = 300, 64, 72
    case = Case(entry, ns, c1, widths, samples, n, npoint, seed=7 * ns + c1)
    idx, q = case.poisoned()
    assert not torch.equal(idx, case.idx) and bool(torch.isnan(q).any())
    ref = case.launch(True)
    new = case.launch(False, idx, q)
    assert torch.equal(new, ref)
    assert bool(torch.isfinite(new).all())
    rows = torch.arange(npoint, device=DEV)[None, :] >= case.dst_nu[:, None]
    assert bool(rows.any()) and bool((new.view(samples, npoint, -1)[rows] == SENT).all())
    assert torch.equal(case.launch(True, idx, q), ref)                                        # (nor does the serial loop read them)


def test_backbone_is_bit_identical_with_the_serial_entries(monkeypatch):
    from ratrack_amd import synth
    from ratrack_amd.track4d import Args, Track4D
    net = Track4D(Args()).to(DEV).eval()
    synth.fill_state_dict(net.state_dict())
    net.invalidate_fused()
    d = synth.make_frame_pairs(2, 256, case_id=7)
    t = [torch.from_numpy(d[k]).to(DEV) for k in ("pc1", "pc2", "feature1", "feature2")]
    calls = []
    real = F._lib.call
    monkeypatch.setattr(F._lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    with torch.no_grad():
        new = [o.clone() for o in net.backbone(*t, None)]
        n_new = sum(c in F.SA_ENTRIES for c in calls)
        assert n_new == 12 and not any(c in F.SA_ENTRIES_SERIAL for c in calls)
        monkeypatch.setattr(F, "SA_ENTRIES", F.SA_ENTRIES_SERIAL)
        del calls[:]
        old = [o.clone() for o in net.backbone(*t, None)]
        assert sum(c in F.SA_ENTRIES_SERIAL for c in calls) == 12 and not any(c in ("rtk_sa_scale", "rtk_sa_scale_split") for c in calls)
    for a, b in zip(new, old):
        assert torch.equal(a, b)
