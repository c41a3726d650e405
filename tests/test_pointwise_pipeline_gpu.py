"""GPU: the software-pipelined tile loops of the per-point chains (rtk_pointwise_mlp_pipelined, rtk_pointwise_mlp_tap_pipelined: the
comparison implementation) against the serial loops the default entries run (rtk_pointwise_mlp, rtk_pointwise_mlp_tap), bit for bit --
for every instance of the chain kernel the backbone can launch with split images (the PW_CASE list of csrc/fused_pointwise.hip) and
for the tap entry, at shapes where the launchers' grid rule (pw_grid: PW_WGS_TARGET = 256 workgroups, groups of 64 rows) gives a
workgroup 1, 2, 3 and 4 trips of its loop (the last-group copy alone, the steady state once and twice, a ragged last group of 16 rows)
and two workgroups of a sample a different number of trips, with live-row counters that leave a dead next group, a partial last live
group or no live group at all, and with what the serial loop does not use poisoned: a prefetched value that reaches a live output
shows as a NaN or a changed bit (see test_prefetching_reads_nothing_the_serial_loop_does_not_read for what that does not cover)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

from ratrack_amd import fused as F  # noqa: E402

SENT = -7.5
WGS, GROUP = 256, 64            # PW_WGS_TARGET, PW_NW * 16 (fused_pointwise.hip)
# (samples, rows_per_sample): one workgroup per sample that walks 1, 2, 3, 4 groups (the last of 208 rows has 16), and gx = 2 with
# three groups: one workgroup makes two trips, its neighbour one
SHAPES = [(256, 64), (256, 128), (256, 144), (256, 208), (128, 192)]
# name -> (interp channels or 0, [(source channels, per_sample)], layer widths, out_channels, channel_major, sample_bias, colmax)
INSTANCES = {
    "1-2": (0, [(2, False)], [32], 32, False, False, False),
    "4-6": (0, [(64, False)], [96], 96, False, False, False),
    "6-12": (0, [(96, False)], [192], 192, False, False, False),
    "8-4": (0, [(128, False)], [64], 64, False, False, False),
    "8-8-interp": (128, [], [128], 128, False, False, True),
    "8-8-interp64-skip64": (64, [(64, False)], [128], 128, False, False, False),          # (a 64-channel segment: the serial loop under both entries)
    "10-8": (128, [(32, False)], [128], 128, False, False, False),
    "12-8": (128, [(64, False)], [128], 128, False, False, False),
    "8-16": (0, [(128, False)], [256], 256, False, True, False),
    "16-8-4-2-1": (0, [(256, False)], [128, 64, 32, 1], 1, True, False, False),
    "8-8-4-2-1": (0, [(128, False)], [128, 64, 32, 3], 3, True, True, False),
    "25-2": (0, [(2, False), (128, False), (256, False)], [32], 30, False, True, False),
    "8-2": (0, [(128, False)], [32], 32, False, False, False),
}


def trips(samples, rps, nu):
    """[per sample: [trips of each of its workgroups]] by pw_grid's rule and the kernels' liveness rule."""
    groups = -(-rps // GROUP)
    gx = max(1, min(WGS // samples, groups))
    return [[len(range(x, -(-min(int(n), rps) // GROUP), gx)) for x in range(gx)] for n in nu]


def live_counts(samples, rps, seed):
    g = torch.Generator().manual_seed(seed)
    choice = torch.tensor([1, 63, 64, 65, rps], dtype=torch.int32).clamp(max=rps)
    nu = choice[torch.randint(0, 5, (samples,), generator=g)]
    nu[:5] = choice
    return nu


class Case:
    def __init__(self, name, samples, rps, seed, m=None):
        ich, srcs, widths, self.oc, self.cm, sb, cmax = INSTANCES[name]
        g = torch.Generator(DEV).manual_seed(seed)
        rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
        self.samples, self.rps, self.rows = samples, rps, samples * rps
        self.nu_cpu = live_counts(samples, rps, seed + 1)
        self.nu = self.nu_cpu.to(DEV)
        self.ich, self.colmax = ich, cmax
        self.m = m if m is not None else 5
        cin = (ich + 15) // 16 * 16
        self.src_bufs = []
        for k, (ch, per) in enumerate(srcs):
            pitch = (ch + 3) // 4 * 4 + (8 if k % 2 else 0)                 # odd sources are column-sliced views of a wider buffer
            buf = rn(samples if per else self.rows, pitch)
            if ch % 4:
                buf[:, ch:] = 0.0                                           # (rtk_src_t: columns channels .. ceil4 hold zero)
            self.src_bufs.append((buf, ch, per))
            cin += (ch + 15) // 16 * 16
        if ich:
            self.known = rn(samples * self.m, ich + 4)                      # pitch > channels
            self.idx = torch.randint(0, self.m, (self.rows, 3), device=DEV, generator=g, dtype=torch.int32)
            self.d2 = torch.rand(self.rows, 3, device=DEV, generator=g) + 0.01
            self.inu = torch.randint(1, self.m + 1, (samples,), device=DEV, generator=g, dtype=torch.int32)       # interp.nuniq <= m
        layers, ci = [], cin            # every segment takes whole 16-channel slots: the columns over a segment's padding meet zeros
        for co in widths:
            layers.append((rn(co, ci).double() * 0.1, rn(co).double() * 0.1, F.ACT_RELU))
            ci = co
        self.chain = F.Chain(layers, DEV)
        self.sb = rn(samples, (widths[0] + 15) // 16 * 16) * 0.1 if sb else None

    def srcs(self, bufs=None):
        return [(b[:, :((ch + 3) // 4 * 4)], ch, per) for b, ch, per in (bufs or self.src_bufs)]

    def interp(self, known=None, idx=None, with_nuniq=True):
        if not self.ich:
            return None
        t = (self.known if known is None else known, self.ich, self.m, self.idx if idx is None else idx, self.d2)
        return t + (self.inu,) if with_nuniq else t

    def launch(self, serial, monkeypatch, counters=True, **poison):
        """-> [out (as the kernel wrote it into a sentinel-filled, wider buffer), colmax or None]"""
        monkeypatch.setattr(F, "PW_ENTRIES", ("rtk_pointwise_mlp", "rtk_pointwise_mlp_tap") if serial else F.PW_ENTRIES_PIPELINED)
        if self.cm:
            buf = torch.full((self.samples, self.oc, self.rps), SENT, device=DEV)
            out = buf
        else:
            buf = torch.full((self.rows, (self.oc + 3) // 4 * 4 + 8), SENT, device=DEV)
            out = buf[:, 4:4 + (self.oc + 3) // 4 * 4]                       # a column-sliced output
        cmax = torch.zeros(self.samples, self.chain.cout16 * 16, device=DEV) if self.colmax else None
        F.pointwise(self.rows, self.rps, self.srcs(poison.get("srcs")), self.chain, out, out_channels=self.oc, sample_bias=self.sb,
                    interp=self.interp(poison.get("known"), poison.get("idx"), poison.get("with_nuniq", True)), channel_major=self.cm,
                    row_nuniq=self.nu if counters else None, colmax=cmax)
        torch.cuda.synchronize()
        return [buf, cmax]

    def live_mask(self, counters=True):
        """(samples, rps) bool: the rows the kernel writes"""
        r = torch.arange(self.rps, device=DEV)[None, :]
        return (r < (self.nu[:, None] if counters else self.rps)).expand(self.samples, self.rps)

    def check_sentinel(self, buf, counters=True):
        live = self.live_mask(counters)
        if self.cm:
            assert bool((buf.permute(0, 2, 1)[~live] == SENT).all())
            assert bool((buf.permute(0, 2, 1)[live] != SENT).all())
        else:
            v = buf.view(self.samples, self.rps, -1)
            assert bool((v[~live] == SENT).all())
            assert bool((v[..., :4] == SENT).all() and (v[..., 4 + self.oc:] == SENT).all())      # only out_channels columns are written
            assert bool((v[live][:, 4:4 + self.oc] != SENT).all())


def same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", sorted(INSTANCES))
def test_pipelined_loop_matches_the_serial_loop_bit_for_bit(name, monkeypatch):
    seen, uneven, dead_next, partial, none_live = set(), False, False, False, False
    for k, (samples, rps) in enumerate(SHAPES):
        case = Case(name, samples, rps, seed=1000 + 10 * k, m=(1, 2, 3, 5, 5)[k])
        for n, t in zip(case.nu_cpu.tolist(), trips(samples, rps, case.nu_cpu)):
            seen.update(t)
            uneven |= len(set(t)) > 1 and min(t) > 0
            none_live |= 0 in t
            dead_next |= -(-n // GROUP) < -(-rps // GROUP)
            partial |= n % GROUP != 0
        new, old = case.launch(False, monkeypatch), case.launch(True, monkeypatch)
        assert same(new, old), (name, samples, rps)
        assert bool(torch.isfinite(new[0]).all())
        case.check_sentinel(new[0])
        case.check_sentinel(old[0])
        if k in (3, 4):                                           # without the counters: every group live, the ragged last group too
            new, old = case.launch(False, monkeypatch, counters=False), case.launch(True, monkeypatch, counters=False)
            assert same(new, old), (name, samples, rps)
            case.check_sentinel(new[0], counters=False)
            seen.update(t for ts in trips(samples, rps, [rps] * samples) for t in ts)
        if k == 1 and case.ich:                                   # without interp.nuniq
            assert same(case.launch(False, monkeypatch, with_nuniq=False), case.launch(True, monkeypatch, with_nuniq=False))
    print("\n%s: trips per workgroup seen %s" % (name, sorted(seen)))
    assert {0, 1, 2, 3, 4} <= seen and uneven and dead_next and partial and none_live


class TapCase:
    def __init__(self, samples, rps, seed, m):
        g = torch.Generator(DEV).manual_seed(seed)
        rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
        self.samples, self.rps, self.rows, self.m = samples, rps, samples * rps, m
        self.known = rn(samples * m, 128)
        self.idx = torch.randint(0, m, (self.rows, 3), device=DEV, generator=g, dtype=torch.int32)
        self.d2 = torch.rand(self.rows, 3, device=DEV, generator=g) + 0.01
        self.inu = torch.randint(1, m + 1, (samples,), device=DEV, generator=g, dtype=torch.int32)
        self.chain = F.Chain([(rn(128, 128).double() * 0.1, rn(128).double() * 0.1, F.ACT_RELU)], DEV)
        self.proj = [F.Chain([(rn(256, 128).double() * 0.1, rn(256).double() * 0.1, F.ACT_NONE)], DEV) for _ in range(2)]

    def launch(self, serial, monkeypatch, known=None):
        monkeypatch.setattr(F, "PW_ENTRIES", ("rtk_pointwise_mlp", "rtk_pointwise_mlp_tap") if serial else F.PW_ENTRIES_PIPELINED)
        buf = torch.full((self.rows, 128 + 8), SENT, device=DEV)
        pbuf = torch.full((self.rows, 256 + 8), SENT, device=DEV)
        cmax = torch.zeros(self.samples, 128, device=DEV)
        interp = (self.known if known is None else known, 128, self.m, self.idx, self.d2, self.inu)
        F.pointwise_tap(self.rows, self.rps, self.chain, buf[:, 4:132], cmax, interp, self.proj, self.samples // 2, pbuf[:, 4:260])
        torch.cuda.synchronize()
        return [buf, pbuf, cmax]


def test_pipelined_tap_loop_matches_the_serial_loop_bit_for_bit(monkeypatch):
    for k, (samples, rps) in enumerate(SHAPES):
        case = TapCase(samples, rps, seed=77 + k, m=(1, 2, 3, 5, 5)[k])
        new, old = case.launch(False, monkeypatch), case.launch(True, monkeypatch)
        assert same(new, old), (samples, rps)
        for t, w in zip(new[:2], (128, 256)):
            assert bool((t[:, :4] == SENT).all() and (t[:, 4 + w:] == SENT).all() and (t[:, 4:4 + w] != SENT).all())
            assert bool(torch.isfinite(t).all())


@pytest.mark.parametrize("name", ["4-6", "6-12", "8-8-interp", "10-8", "12-8", "25-2", "8-8-4-2-1"])
def test_prefetching_reads_nothing_the_serial_loop_does_not_read(name, monkeypatch):
    """The three-NN rows of dead groups point at a known row full of NaN (in range: nothing here can fault), the source rows and the
    known rows past the live counts are NaN: the live outputs are still the serial loop's on the clean operands, and finite.
    This guards USE, not reads: a value prefetched for a group that no tile consumes lands in registers nobody looks at, so the test
    would not fail if the pipelined loop requested the rows of a dead next group.  That it does not -- no address is formed from an
    index row of a dead group -- rests on the loop's structure alone (`while (G + nbx < live_groups)` around the steady-state body,
    the last-group body requesting nothing; pw_pipelined in csrc/fused_pointwise.hip).  What the test does catch: a prefetched row
    of the wrong group or sample, or of a dead row, reaching a live output."""
    for samples, rps in ((256, 208), (128, 192)):
        case = Case(name, samples, rps, seed=4242, m=6)
        ref = case.launch(True, monkeypatch)
        r = torch.arange(rps, device=DEV)[None, :]
        past_live = (r >= case.nu[:, None]).reshape(-1)                                       # rows at or past row_nuniq
        dead_group = (r >= (case.nu[:, None] + GROUP - 1) // GROUP * GROUP).reshape(-1)       # rows of groups with no live row
        assert bool(dead_group.any())
        poison = {}
        poison["srcs"] = []
        for buf, ch, per in case.src_bufs:
            b = buf.clone()
            if not per:
                b[past_live] = float("nan")
            poison["srcs"].append((b, ch, per))
        if case.ich:
            # the live groups' rows use known rows 0 .. m-2 and the sample's interp.nuniq is m-1: row m-1 is read by nobody
            case.idx = case.idx % (case.m - 1)
            case.inu = torch.full_like(case.inu, case.m - 1)
            ref = case.launch(True, monkeypatch)
            known = case.known.clone()
            known.view(samples, case.m, -1)[:, case.m - 1] = float("nan")
            idx = case.idx.clone()
            idx[dead_group] = case.m - 1
            poison["known"], poison["idx"] = known, idx
            case.inu = torch.full_like(case.inu, case.m)             # (the clamp does not hide a read of row m-1)
        new = case.launch(False, monkeypatch, **poison)
        assert same(new, ref), (name, samples, rps)
        assert bool(torch.isfinite(new[0]).all())
        case.check_sentinel(new[0])
        assert same(case.launch(True, monkeypatch, **poison), ref)                            # (nor does the serial loop read them)


def test_backbone_is_bit_identical_with_the_serial_entries(monkeypatch):
    from ratrack_amd import synth, vod_gt
    from ratrack_amd.track4d import Args, Track4D
    net = Track4D(Args()).to(DEV).eval()
    synth.fill_state_dict(net.state_dict())
    net.invalidate_fused()
    d = synth.make_frame_pairs(8, 256, case_id=7)
    fixed = [torch.from_numpy(d[k]).to(DEV) for k in ("pc1", "pc2", "feature1", "feature2")] + [None, None]
    pairs = []
    for i, (n1, n2) in enumerate([(256, 200), (131, 256), (64, 77)]):                          # one padded batch of clouds of different sizes
        e = synth.make_frame_pairs(1, 256, case_id=20 + i)
        pairs.append((torch.from_numpy(e["pc1"][:, :, :n1]), torch.from_numpy(e["pc2"][:, :, :n2]),
                      torch.from_numpy(e["feature1"][:, :, :n1]), torch.from_numpy(e["feature2"][:, :, :n2])))
    pc1, pc2, f1, f2, nv = vod_gt.pad_frame_pairs(pairs, device=DEV)
    padded = [pc1, pc2, f1, f2, None, nv]
    calls = []
    real = F._lib.call
    monkeypatch.setattr(F._lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    serial = ("rtk_pointwise_mlp", "rtk_pointwise_mlp_tap")
    for t in (fixed, padded):
        with torch.no_grad():
            monkeypatch.setattr(F, "PW_ENTRIES", F.PW_ENTRIES_PIPELINED)
            del calls[:]
            new = [o.clone() for o in net.backbone(*t)]
            n_new = sum(c in F.PW_ENTRIES_PIPELINED for c in calls)
            assert n_new >= 8 and not any(c in serial for c in calls)
            monkeypatch.setattr(F, "PW_ENTRIES", serial)
            del calls[:]
            old = [o.clone() for o in net.backbone(*t)]
            assert sum(c in serial for c in calls) == n_new and not any(c in F.PW_ENTRIES_PIPELINED for c in calls)
        assert len(new) == 7
        for a, b in zip(new, old):
            assert torch.equal(a, b)
