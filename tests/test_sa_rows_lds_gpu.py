"""GPU: the q rows of the pipelined split set-abstraction loops through LDS (rtk_sa_scale_split; csrc/fused_split.hip, SaRows) against the
serial entry's direct gather (rtk_sa_scale_split_serial), bit for bit, for the three instances -- what the shapes of test_sa_pipeline_gpu
and test_sa_prologue_gpu leave out:

* q is a column slice of a wider tensor at a non-zero column (C1 = 64: columns 64.. and 128.. of pitch 192; C1 = 32: columns 64.. of
  pitch 96), every column outside the slice NaN in the operand the default entry gets: a request past the C1 columns of a row, or a
  chunk taken from the wrong 16 bytes of the slab, shows.  The serial reference runs on the clean, contiguous rows.
* Source rows: sample b has src_nuniq = 5, n, 1, n - 1 (b mod 4), so most indices of every fourth sample alias row 0; the rows >=
  src_nuniq are NaN in the default entry's operand.  The ball tables are written by hand: random in-range indices, and in the first
  three tiles of every sample 32 times the same row, 32 distinct rows, and rows n - 1 and 0 alternating.
* Shapes: (3, 48, 40), a plain grid with one unit per wave and (two centroids per tile) a partial last unit; (520, 64, 74), the
  XCD-aware grid with one workgroup per sample, where dst_nuniq = 1 + b mod npoint gives waves of 1, 2, 3 and 4 units and more --
  computed from the launcher's grid rule and asserted.  (The three samples of the first shape get dst_nuniq = npoint, npoint - 1, 7.)
* The 32-bit offset rule: with n * q_pitch * 4 >= 2^32 the default entry takes the serial route and returns the serial bits.  Done with
  a real allocation (torch.empty of 4.4 GB, only the C1 columns used are written), not through a call trace: the route is taken inside
  the library, below what the trace of _lib sees, so the data is the witness.  The pitch puts the byte offset of row n - 1 itself past
  2^32 and src_nuniq is n (no row aliases row 0), and the hand-written table gathers row n - 1: without the route the staged path's
  32-bit offset of that row wraps to 240 bytes into row 0 -- inside the allocation, columns that are NaN here -- and the result differs."""
import pytest
import torch

from test_sa_pipeline_gpu import DEV, SENT, units_per_wave

pytestmark = pytest.mark.gpu

from ratrack_amd import fused as F  # noqa: E402

# (nsample, c1, [(first column, pitch)])
INSTANCES = [(32, 64, [(64, 192), (128, 192)]), (16, 64, [(64, 192), (128, 192)]), (16, 32, [(64, 96)])]
SHAPES = [(3, 48, 40), (520, 64, 74)]


class Case:
    def __init__(self, ns, c1, samples, n, npoint, seed, src_nu=None):
        g = torch.Generator().manual_seed(seed)
        self.ns, self.c1, self.samples, self.n, self.npoint = ns, c1, samples, n, npoint
        self.xyz = (torch.rand(samples, n, 3, generator=g) * 8.0).to(DEV)
        self.new_xyz = (torch.rand(samples, npoint, 3, generator=g) * 8.0).to(DEV)
        b = torch.arange(samples)
        # few samples: every unit live, an odd count (a partial last unit where a tile holds two centroids), a short one; else every count
        self.dst_nu = torch.tensor([npoint, npoint - 1, 7], dtype=torch.int32)[b % 3] if samples < 8 else (b % npoint + 1).to(torch.int32)
        self.src_nu = torch.tensor([5, n, 1, n - 1] if src_nu is None else [src_nu], dtype=torch.int32)[b % (4 if src_nu is None else 1)]
        idx = torch.randint(0, n, (samples, npoint * ns), generator=g, dtype=torch.int32)
        assert n >= 32 and npoint * ns >= 96
        idx[:, 0:32] = 3                                                                  # one tile, one row
        idx[:, 32:64] = (torch.arange(32) * 5 + 1) % n                                    # 32 distinct rows (5 is coprime to n = 48, 64)
        idx[:, 64:96] = torch.tensor([n - 1, 0], dtype=torch.int32).repeat(16)            # the last row next to the first
        assert len(set(idx[0, 32:64].tolist())) == 32
        self.idx = idx.view(samples, npoint, ns).contiguous().to(DEV)
        self.q = torch.randn(samples * n, c1, generator=g).to(DEV)
        rn = lambda *s: torch.randn(*s, generator=g).double()
        self.w1img = F.offset_image(torch.cat([rn(c1, 3) * 0.25, rn(c1, 1) * 0.125], 1).to(DEV), DEV)
        self.img, self.inv = F.pack_split_device((rn(64, c1) / 8.0).float().contiguous().to(DEV))
        self.b2 = (rn(64) * 0.125).float().contiguous().to(DEV)
        self.dst_nu, self.src_nu = self.dst_nu.to(DEV), self.src_nu.to(DEV)
        self.out_pitch, self.out_offset = 96, 16

    def sliced(self, col, pitch):
        """The rows as columns col .. col + c1 - 1 of a (samples * n, pitch) tensor that is NaN everywhere else and in the rows >= src_nuniq."""
        wide = torch.full((self.samples * self.n, pitch), float("nan"), device=DEV)
        wide[:, col:col + self.c1] = self.q
        dup = (torch.arange(self.n, device=DEV)[None, :] >= self.src_nu[:, None]).reshape(-1)
        wide[dup] = float("nan")
        return wide

    def launch(self, serial, q, q_pitch, q_col=0):
        from ratrack_amd import _lib
        out = torch.full((self.samples * self.npoint, self.out_pitch), SENT, device=DEV)
        _lib.call("rtk_sa_scale_split" + ("_serial" if serial else ""), self.samples, self.n, self.npoint, self.ns, self.xyz.data_ptr(),
                  self.new_xyz.data_ptr(), self.idx.data_ptr(), q.data_ptr() + 4 * q_col, q_pitch, self.c1, self.w1img.data_ptr(), self.img.data_ptr(),
                  self.inv.data_ptr(), self.b2.data_ptr(), out.data_ptr(), self.out_pitch, self.out_offset, self.src_nu.data_ptr(),
                  self.dst_nu.data_ptr(), F._stream())
        torch.cuda.synchronize()
        return out


@pytest.mark.parametrize("ns,c1,slices", INSTANCES, ids=["%d-%d" % t[:2] for t in INSTANCES])
def test_rows_through_lds_match_the_direct_gather_on_column_slices(ns, c1, slices):
    seen = set()
    for k, (samples, n, npoint) in enumerate(SHAPES):
        case = Case(ns, c1, samples, n, npoint, seed=31 * ns + c1 + k)
        for wgs in units_per_wave("split", ns, samples, npoint, case.dst_nu.cpu()):
            for waves in wgs:
                seen.update(waves)
        ref = case.launch(True, case.q, c1)                                           # serial, clean contiguous rows
        live = torch.arange(npoint, device=DEV)[None, :] < case.dst_nu[:, None]
        rows = ref.view(samples, npoint, -1)
        assert bool(torch.isfinite(rows[live]).all()) and bool((rows[~live] == SENT).all())
        for col, pitch in slices:
            wide = case.sliced(col, pitch)
            assert bool(torch.isnan(wide[:, :col]).all()) and bool(torch.isnan(wide[:, col + c1:]).all())
            assert torch.equal(case.launch(False, wide, pitch, col), ref), (samples, n, npoint, col, pitch)
        assert torch.equal(case.launch(False, case.q, c1), ref), (samples, n, npoint)
    print("\nns=%d c1=%d: units per wave seen %s" % (ns, c1, sorted(seen)))
    assert {1, 2, 3, 4} <= seen, sorted(seen)


def test_a_pitch_beyond_32_bit_offsets_takes_the_serial_route():
    ns, c1, n, npoint = 16, 32, 48, 40
    case = Case(ns, c1, 1, n, npoint, seed=9, src_nu=n)
    pitch = -(-(1 << 32) // (4 * (n - 1) * 4)) * 4
    wrapped = (n - 1) * pitch * 4 - (1 << 32)                                       # where a 32-bit offset of row n - 1 would land
    assert 4 * c1 <= wrapped < 4 * c1 + 1024 and wrapped % 16 == 0
    assert int(case.src_nu[0]) == n and int(case.dst_nu[0]) == npoint and bool((case.idx[0, :npoint] == n - 1).any())
    ref = case.launch(True, case.q, c1)
    wide = torch.empty((n, pitch), device=DEV)                                      # 4.4 GB, uninitialised: only the columns named here are written
    wide[:, :c1] = case.q
    wide[0, c1:c1 + 512] = float("nan")
    assert torch.equal(case.launch(False, wide, pitch), ref)
    assert torch.equal(case.launch(True, wide, pitch), ref)
    del wide
    torch.cuda.empty_cache()
