#!/usr/bin/env python3
"""What bounds sa_scale_split_kernel?  (round 5)  Patched COPIES of csrc/fused_split.hip (the product source carries no ablation
macros), each linked into ratrack_amd/lib/variants/librtk_sa_<tag>.so, all timed in one GPU call on the largest scale of the bench
batch (128 clouds x 256 live centroids x 32 neighbours, 64 -> 64 channels).  Results of the ablations are WRONG by construction;
only their times mean anything.

    python tools/experiments/sa_ablate.py --build     (CPU: hipcc)
    python tools/experiments/sa_ablate.py             (GPU: runs every variant in a subprocess)

The patterns of nogather, nolayer2 and noidx were written for the serial loop and match both loops or neither today; the others
address the default (pipelined) entry, which is what rtk_sa_scale_split launches.  Its q rows come through LDS today (SaRows), so
--variants base,row0 times the staged path with and without the spread of the rows, and --variants direct,direct_row0 the direct gather
it replaced -- the pair profiles/sa_rows_lds_bound.txt was taken with, on the source as it was before the rows were staged.  --passes N
alternates the variants N times, one process per variant and pass, and --out writes the table (minimum and maximum of the passes'
medians per shape, and the ratio of the minima) to a file.
"""
import argparse
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
VAR = os.path.join(ROOT, "ratrack_amd", "lib", "variants")

ROW0 = [("\n            const float *qrow = P.q + ((long)b * P.n + (id < src_e ? id : 0)) * P.q_pitch + 4 * hh;",
         "\n            const float *qrow = P.q + ((long)b * P.n + (id < 0 ? id : 0)) * P.q_pitch + 4 * hh;"),
        ("auto row_offset = [&](int id) { return (unsigned)(id < src_e ? id : 0) * ((unsigned)P.q_pitch * 4u); };",
         "auto row_offset = [&](int id) { return (unsigned)(id < 0 ? id : 0) * ((unsigned)P.q_pitch * 4u); }; (void)src_e;")]
DIRECT = [("constexpr bool sa_split_rows_lds(int ns, int c1) { return true; }", "constexpr bool sa_split_rows_lds(int ns, int c1) { return false; }")]
VARIANTS = {
    "base": [],
    # every position gathers ROW 0 of its sample: is the kernel bound by the spread of the gather?
    # Both forms of the pipelined loop's gather: the direct one (the leading indentation selects its lambda: the serial comparison loop
    # holds the same statement) and the row offsets of the requests through LDS.
    "row0": ROW0,
    # the direct gather in every instance (the pipelined loop as it was before its rows were staged in LDS), and its row-0 bound
    "direct": DIRECT,
    "direct_row0": DIRECT + ROW0,
    # schedules of the rows through LDS (C1 = 64): round 0 requested behind k-step 0 instead of 1; and read behind k-step 2 instead of 3
    "gs0": [("#define SA_GATHER_STEP 1", "#define SA_GATHER_STEP 0")],
    "gs0rs2": [("#define SA_GATHER_STEP 1", "#define SA_GATHER_STEP 0"), ("#define SA_ROWS_READ_STEP 3", "#define SA_ROWS_READ_STEP 2")],
    "rs2": [("#define SA_ROWS_READ_STEP 3", "#define SA_ROWS_READ_STEP 2")],
    # <16, 64> keeps the direct gather, the other two shapes go through LDS
    "direct1664": [("constexpr bool sa_split_rows_lds(int ns, int c1) { return true; }",
                    "constexpr bool sa_split_rows_lds(int ns, int c1) { return !(ns == 16 && c1 == 64); }")],
    # no gather at all: the lane's coordinates stand in for the row
    "nogather": [("                const f4 t = *reinterpret_cast<const f4 *>(qrow + 32 * v + 8 * q);\n                a[4 * q] = t.x;",
                  "                const f4 t = (f4){dx, dy, dz, (float)(v + q)}; (void)qrow;\n                a[4 * q] = t.x;")],
    # no split layer: the accumulators take the activations
    "nolayer2": [("            RTK_SA_MM(1, 0) RTK_SA_MM(0, 1) RTK_SA_MM(0, 0)\n", "            acc[0][s] += __uint_as_float(bp[0][0] ^ fr[0][0][0]); acc[1][s] += __uint_as_float(bp[1][1] ^ fr[1][1][1]);\n")],
    # ball indices and coordinates of a fixed pattern instead of loaded (removes the idx -> xyz / row dependent chain)
    "noidx": [("        const int id = P.idx[(long)c * NS + slot];", "        const int id = (c * 7 + slot * 13) & 255;")],
}


def build(tags):
    from ratrack_amd import build as B
    B.build(verbose=False)
    src0 = open(os.path.join(B.CSRC, "fused_split.hip")).read()
    os.makedirs(VAR, exist_ok=True)
    for tag in tags:
        patches = VARIANTS[tag]
        src = src0
        for a, r in patches:
            assert src.count(a) == 1, (tag, a)
            src = src.replace(a, r)
        patched = os.path.join(VAR, "fused_split_sa_%s.hip" % tag)
        open(patched, "w").write(src)
        obj = patched[:-4] + ".o"
        subprocess.check_call([B._hipcc()] + B.flags_for("fused_split.hip") + ["-I", os.path.join(ROOT, "include"), "-I", B.CSRC, "-c", patched, "-o", obj])
        objs = [o for o in glob.glob(os.path.join(B.LIBDIR, "obj", "*.o")) if os.path.basename(o) != "fused_split.o"]
        out = os.path.join(VAR, "librtk_sa_%s.so" % tag)
        subprocess.check_call([B._hipcc(), "-shared", "-fPIC", "--offload-arch=" + B.ARCH, "-o", out] + objs + [obj])
        os.remove(obj)
        os.remove(patched)
        print(out)


def run_one(so):
    import ratrack_amd._lib as L
    L.SO_PATH = so
    import torch
    from ratrack_amd import fused as F
    dev = "cuda"
    torch.manual_seed(0)
    # the bench batch (B = 64): one encoder launch over 2 B clouds and one decoder launch over B clouds of each shape
    for (ns, c1, n, npoint, live, samples) in ((32, 64, 512, 512, 256, 128), (16, 64, 512, 512, 256, 128), (16, 32, 512, 512, 256, 128),
                                               (32, 64, 512, 512, 256, 64), (16, 64, 512, 512, 256, 64), (16, 32, 512, 512, 256, 64)):
        xyz, new_xyz = torch.randn(samples, n, 3, device=dev), torch.randn(samples, npoint, 3, device=dev)
        idx = torch.randint(0, live, (samples, npoint, ns), device=dev, dtype=torch.int32)
        q = torch.randn(samples * n, c1, device=dev)
        w1img = F.offset_image((torch.randn(c1, 4, device=dev) * 0.3).double(), dev)
        w2, b2 = torch.randn(64, c1, device=dev) / 8, torch.randn(64, device=dev) * 0.1
        img, inv = F.pack_split_device(w2)
        nu = torch.full((samples,), live, device=dev, dtype=torch.int32)
        out = torch.zeros(samples * npoint, 128, device=dev)
        st = torch.cuda.current_stream().cuda_stream

        def launch():
            L.call("rtk_sa_scale_split", samples, n, npoint, ns, xyz.data_ptr(), new_xyz.data_ptr(), idx.data_ptr(), q.data_ptr(), c1, c1,
                   w1img.data_ptr(), img.data_ptr(), inv.data_ptr(), b2.data_ptr(), out.data_ptr(), 128, 0, nu.data_ptr(), nu.data_ptr(), st)
        for _ in range(20):
            launch()
        torch.cuda.synchronize()
        rounds = []
        for _ in range(7):                  # the median of seven rounds of 50 launches back to back
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(50):
                launch()
            e1.record()
            torch.cuda.synchronize()
            rounds.append(e0.elapsed_time(e1) * 1e3 / 50)
        us = sorted(rounds)[len(rounds) // 2]
        pos = samples * live * ns
        print("   ns=%2d c1=%2d clouds=%3d: %7.1f us   (%.2f TB/s of gathered rows, %.1f TFLOP/s of the %d -> 64 layer)"
              % (ns, c1, samples, us, pos * c1 * 4 / us / 1e6, 2.0 * pos * c1 * 64 / us / 1e6, c1), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--one", default=None)
    ap.add_argument("--variants", default=",".join(VARIANTS))
    ap.add_argument("--passes", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    tags = a.variants.split(",")
    if a.build:
        return build(tags)
    if a.one:
        return run_one(a.one)
    times = {}                              # (tag, shape) -> one time per pass
    lines = []
    for p in range(a.passes):
        for tag in tags:
            so = os.path.join(VAR, "librtk_sa_%s.so" % tag)
            print("%s (pass %d):" % (tag, p), flush=True)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", so], stdout=subprocess.PIPE, text=True, timeout=120)
            sys.stdout.write(r.stdout)
            if r.returncode != 0:           # nothing more on the GPU behind a process that failed
                sys.exit("variant %s ended with status %d" % (tag, r.returncode))
            lines.append("%s (pass %d):\n%s" % (tag, p, r.stdout))
            for ln in r.stdout.splitlines():
                if " us " in ln:
                    shape, rest = ln.strip().split(":", 1)
                    times.setdefault((tag, shape), []).append(float(rest.split()[0]))
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/experiments/sa_ablate.py --variants %s --passes %d: rtk_sa_scale_split (the pipelined loop) alone, the median of seven\n"
                    "# rounds of 50 launches per process, %d processes per variant, the variants alternating.  us: minimum .. maximum over the processes.\n"
                    % (a.variants, a.passes, a.passes))
            shapes = [k[1] for k in times if k[0] == tags[0]]
            for shape in shapes:
                b = times[(tags[0], shape)]
                row = "%-26s %-8s %6.1f .. %6.1f" % (shape, tags[0], min(b), max(b))
                for tag in tags[1:]:
                    t = times[(tag, shape)]
                    row += "   %-8s %6.1f .. %6.1f  (%+.1f %% of the minima; spread of %s %.1f %%)" % (
                        tag, min(t), max(t), 100.0 * (min(t) / min(b) - 1.0), tags[0], 100.0 * (max(b) / min(b) - 1.0))
                f.write(row + "\n")
            f.write("#\n# every process:\n" + "".join(lines))


if __name__ == "__main__":
    main()
