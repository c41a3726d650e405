// track_score_body.h -- the LDS layout, the body and the argument checks of the scoring kernels: rtk_track_score,
// rtk_track_score_logged, rtk_track_score_memory, rtk_track_score_pairs, rtk_track_score_pairs_centre and rtk_track_score_pairs_box
// launch instantiations of the one body through the one kernel template and the one launcher of track_score.hip.
#pragma once
#include <math.h>

#include "batch_common.h"
#include "rtk_common.h"
#include "rtk_score.h"

#define TS_THREADS 256
#define TS_WAVES (TS_THREADS / RTK_WAVE)

// LDS: pts[N] float4 | best_iou[Kobj] f64 | gmask[N] u64 | plist[N] | qlist[N] | common[Kobj][K] | psize, best, cur_id, prev_id [Kobj] |
//      gsize, glabel, gslot, gpred, entry [K] | 8 scalars (all i32)
static inline size_t ts_score_lds(int Kobj, int K, int N) {
    return (size_t)N * sizeof(float4) + (size_t)Kobj * sizeof(double) + (size_t)N * sizeof(unsigned long long) +
           ((size_t)2 * N + (size_t)Kobj * K + (size_t)4 * Kobj + (size_t)5 * K + 8) * sizeof(int);
}

// the memory variant also keeps the old record's track ids: old_track[Kobj] i32 after the scalars
static inline size_t ts_score_memory_lds(int Kobj, int K, int N) { return ts_score_lds(Kobj, K, N) + (size_t)Kobj * sizeof(int); }

// the centre variant keeps, 8-byte aligned behind either layout: gpos[K][3] f64, the kept objects' positions | zero_distance f64 | the
// address of the stream's part of pair_sim (64 bits) -- read from the arguments once, at the start, so that they are not carried in
// scalar registers through the whole body
static inline size_t ts_score_centre_lds(int Kobj, int K, int N, bool memory) {
    const size_t base = memory ? ts_score_memory_lds(Kobj, K, N) : ts_score_lds(Kobj, K, N);
    return ((base + 7) & ~(size_t)7) + ((size_t)3 * K + 2) * sizeof(double);
}

// the box variant keeps, 8-byte aligned behind either layout: gbox[K][8] f64, the kept objects' upright boxes (centre x, y | heading x, y |
// half length, half width (half length 0: no box) | bottom, top) | the mode (64 bits) | the address of the stream's part of pair_sim
static inline size_t ts_score_box_lds(int Kobj, int K, int N, bool memory) {
    const size_t base = memory ? ts_score_memory_lds(Kobj, K, N) : ts_score_lds(Kobj, K, N);
    return ((base + 7) & ~(size_t)7) + ((size_t)8 * K + 2) * sizeof(double);
}

// The body of the scoring kernels.  LOG: the frame is also appended to the stream's log (rtk_score_log_t) -- thread i writes
// detection i's record where it finds its pre-greedy best object, thread j the j-th kept label id, thread 0 the frame's slot and the
// cursors; a frame that does not fit writes nothing and raises RTK_SCORE_FLAG_LOG.  Without LOG `lg` is not read.
// MEM: the record (prev_gt_id, prev_count, and mm.row_track beside them) covers every row of the tracker's new table, not only this
// frame's detections -- thread r gives row r >= P the label id of the old record's first row with the same track id (a scan of at
// most Kobj words of LDS), thread 0 counts the labelled ones.  Without MEM `mm` is not read.
// PAIRS (only with LOG): the frame's (detection, kept object) pairs with common > 0 are appended to the pair log (rtk_score_pairs_t)
// in (i, then j) order -- thread i counts row i's pairs, an ordered prefix over the rows (a wave scan, the four wave totals through
// scal[4..7], one barrier more) gives every row its place and the frame its pair count, which joins the fit test; thread i then writes
// its row's pairs and its size, thread j the j-th kept object's size, thread 0 the frame's slot and the cursor.  Without PAIRS `pr` is
// not read and the body is what it was.
// CENTRE (only with PAIRS): the pair log's similarity is TrackEval's centre-distance similarity (include/rtk_score.h, its section)
// -- every live column keeps its detection index in pts[p].w, thread i forms detection i's centre in ascending column order in
// registers (N broadcast reads of LDS), decides row i's pairs once (s > 0, a 64-bit mask over the kept objects) where PAIRS counts
// common > 0, and writes key, common and s behind the same ordered prefix; the kept objects' positions are G broadcast reads of LDS,
// where they, zero_distance and the stream's pair_sim address are put at the start (ts_score_centre_lds: 24 K + 16 bytes more).
// Without CENTRE the three arguments are not read and the body is what it was.
// BOX (only with PAIRS, never with CENTRE): the pair log's similarity is the oriented-box IoU (include/rtk_score.h, the last section) in
// CENTRE's arrangement -- thread j stages kept object j's upright box in LDS at the start (ts_score_box_lds: 64 K + 16 bytes more, the
// mode and the stream's pair_sim address among them); the P G decisions (s > 0) are spread over the 256 threads, each reading its
// detection's box from global memory and raising a bit of its row's 64-bit mask in LDS (where best_iou lies later; one barrier more);
// thread i then takes row i's mask and writes key, common and s, formed again by the same operations, behind the ordered prefix.
// Without BOX the four arguments are not read and the body is what it was.
static_assert(RTK_SCORE_MAX_OBJECTS <= TS_THREADS, "PAIRS: one thread per detection row");
// s = 1 - |c - g| / zero_distance in float64, every operation rounded on its own (the build has contraction off)
__device__ __forceinline__ double ts_centre_similarity(double cx, double cy, double cz, const double *g, double zero_distance) {
    const double dx = cx - g[0], dy = cy - g[1], dz = cz - g[2];
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    return 1.0 - sqrt(d2) / zero_distance;
}

// ---- the oriented-box IoU (include/rtk_score.h, the last section): every operation float64 and rounded on its own ----
// The area of the detection's footprint -- centre D, half axes (lx, ly) = L E and (-wx, wy) = W E' in the kept object's own frame -- cut
// by the object's rectangle |x| <= a, |y| <= b: Sutherland-Hodgman by the four half-planes, kept as a set of directed edges in eight
// fixed slots (the footprint's four, then the one edge a cut adds along its bound, from where the outline leaves to where it comes
// back), so that no index into them is computed at run time, and Green's theorem over the slots in order.  A crossing point is formed
// once, with its cut coordinate set to the bound itself, and serves the edge it shortens and the edge the cut adds.
__device__ __forceinline__ double ts_box_cut_area(double Dx, double Dy, double lx, double ly, double wx, double wy, double a, double b) {
    double x0[8], y0[8], x1[8], y1[8];
    unsigned valid = 0xfu;
    // the corners, counter-clockwise: D + LE + WE', D - LE + WE', D - LE - WE', D + LE - WE'
    x0[0] = (Dx + lx) - wx; y0[0] = (Dy + ly) + wy;
    x0[1] = (Dx - lx) - wx; y0[1] = (Dy - ly) + wy;
    x0[2] = (Dx - lx) + wx; y0[2] = (Dy - ly) - wy;
    x0[3] = (Dx + lx) + wx; y0[3] = (Dy + ly) - wy;
#pragma unroll
    for (int e = 0; e < 4; ++e) { x1[e] = x0[(e + 1) & 3]; y1[e] = y0[(e + 1) & 3]; }
#pragma unroll
    for (int e = 4; e < 8; ++e) { x0[e] = 0.0; y0[e] = 0.0; x1[e] = 0.0; y1[e] = 0.0; }
#pragma unroll
    for (int k = 0; k < 4; ++k) {      // x <= a, x >= -a, y <= b, y >= -b
        const double lim = k < 2 ? a : b, bound = (k & 1) ? -lim : lim;
        bool left = false, came = false;
        double ox = 0.0, oy = 0.0, ix = 0.0, iy = 0.0;      // where the outline leaves, where it comes back
#pragma unroll
        for (int e = 0; e < 4 + k; ++e) {
            if (!((valid >> e) & 1u)) continue;
            const double v0 = k < 2 ? x0[e] : y0[e], v1 = k < 2 ? x1[e] : y1[e];
            const double s0 = (k & 1) ? v0 + lim : lim - v0, s1 = (k & 1) ? v1 + lim : lim - v1;
            const bool in0 = s0 >= 0.0, in1 = s1 >= 0.0;
            if (in0 && in1) continue;
            if (!in0 && !in1) { valid &= ~(1u << e); continue; }
            const double t = s0 / (s0 - s1);
            const double cx = k < 2 ? bound : x0[e] + t * (x1[e] - x0[e]), cy = k < 2 ? y0[e] + t * (y1[e] - y0[e]) : bound;
            if (in0) { x1[e] = cx; y1[e] = cy; ox = cx; oy = cy; left = true; }
            else { x0[e] = cx; y0[e] = cy; ix = cx; iy = cy; came = true; }
        }
        if (left && came) { x0[4 + k] = ox; y0[4 + k] = oy; x1[4 + k] = ix; y1[4 + k] = iy; valid |= 1u << (4 + k); }
    }
    double acc = 0.0;
#pragma unroll
    for (int e = 0; e < 8; ++e)
        if ((valid >> e) & 1u) acc += x0[e] * y1[e] - x1[e] * y0[e];
    return 0.5 * acc;
}

// Row d (8 words, rtk_object_boxes') and its valid word -> whether the detection has a box, and the box's terms: centre, half length and
// width, heading (c, s), z range and height.
__device__ __forceinline__ bool ts_box_detection(const double *d, int valid, bool bev, double &cx, double &cy, double &L, double &W, double &c,
                                                 double &s, double &bot, double &top, double &h) {
    const double x = d[0], y = d[1], z = d[2], l = d[3], w = d[4], hh = d[5], yaw = d[6];
    if (!(valid > 0 && isfinite(x) && isfinite(y) && isfinite(z) && isfinite(l) && isfinite(w) && isfinite(hh) && isfinite(yaw) && l > 0.0 &&
          w > 0.0 && (bev || hh > 0.0)))
        return false;
    cx = x; cy = y; h = hh;
    L = 0.5 * l; W = 0.5 * w; bot = z - 0.5 * hh; top = z + 0.5 * hh;
    sincos(yaw, &s, &c);
    return true;
}

// s of a detection (centre dcx, dcy, half length L and width W, heading (c, s), z range [dbot, dtop], height h) and the staged upright
// box g (ts_score_box_lds) of a kept object; bev: the bird's-eye-view IoU.  A box without extent (g[4] == 0) gives 0.0.
__device__ __forceinline__ double ts_box_similarity(double dcx, double dcy, double L, double W, double hc, double hs, double dbot, double dtop,
                                                    double h, const double *g, bool bev) {
    const double a = g[4], b = g[5];
    if (!(a > 0.0)) return 0.0;
    const double dx = dcx - g[0], dy = dcy - g[1];
    const double ri = sqrt(L * L + W * W), rj = sqrt(a * a + b * b), rr = ri + rj;
    if ((dx * dx + dy * dy) > rr * rr) return 0.0;      // the prefilter: part of the definition
    double zo = 1.0;
    if (!bev) {
        const double top = dtop < g[7] ? dtop : g[7], bottom = dbot > g[6] ? dbot : g[6];
        zo = top - bottom;
        if (!(zo > 0.0)) return 0.0;
    }
    // the ground-truth box's own frame: the detection's centre D and axis E there
    const double hx = g[2], hy = g[3];
    const double Dx = dx * hx + dy * hy, Dy = dy * hx - dx * hy;
    const double ex = hc * hx + hs * hy, ey = hs * hx - hc * hy;
    const double I2 = ts_box_cut_area(Dx, Dy, L * ex, L * ey, W * ey, W * ex, a, b);
    const double l = 2.0 * L, w = 2.0 * W, a2 = 2.0 * a, b2 = 2.0 * b;
    const double Ai = l * w, Aj = a2 * b2;
    double s;
    if (bev) {
        s = I2 / ((Ai + Aj) - I2);
    } else {
        const double I3 = I2 * zo;
        s = I3 / ((Ai * h + Aj * (g[7] - g[6])) - I3);
    }
    return s < 1.0 ? s : (s >= 1.0 ? 1.0 : s);      // min(s, 1.0); a NaN stays one
}

template <bool LOG, bool MEM, bool PAIRS, bool CENTRE, bool BOX>
__device__ __forceinline__ void track_score_body(const rtk_track_score_in_t &in, const rtk_track_score_state_t &st,
                                                 const rtk_track_score_out_t &out, const rtk_score_log_t &lg,
                                                 const rtk_score_memory_t &mm, const rtk_score_pairs_t &pr, double *pair_sim,
                                                 const double *gt_centre, double zero_distance, const double *det_box, const int *det_valid,
                                                 const double *gt_boxes, int mode) {
    static_assert(LOG || !PAIRS, "the pair log goes with the main log");
    static_assert(PAIRS || !CENTRE, "the centre similarity is the pair log's");
    static_assert((PAIRS && !CENTRE) || !BOX, "the box similarity is the pair log's, and a log has one similarity");
    constexpr int SIMW = BOX ? 8 : 3;      // the float64 words staged per kept object
    extern __shared__ __attribute__((aligned(16))) unsigned char ts_smem[];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & (RTK_WAVE - 1), wave = t / RTK_WAVE;
    const int N = in.N, Kobj = in.Kobj, K = in.K, T = in.T, W = (N + 31) / 32;
    float4 *pts = reinterpret_cast<float4 *>(ts_smem);
    double *best_iou = reinterpret_cast<double *>(pts + N);
    unsigned long long *gmask = reinterpret_cast<unsigned long long *>(best_iou + Kobj);
    int *plist = reinterpret_cast<int *>(gmask + N), *qlist = plist + N, *common = qlist + N;
    int *psize = common + (size_t)Kobj * K, *best = psize + Kobj, *cur_id = best + Kobj, *prev_id = cur_id + Kobj;
    int *gsize = prev_id + Kobj, *glabel = gsize + K, *gslot = glabel + K, *gpred = gslot + K, *entry = gpred + K;
    int *scal = entry + K;      // 0: predicted points | 1: ground-truth columns | 2..4: mt, pt, ml of a closing clip
    int *old_track = scal + 8;  // MEM only
    double *gpos = nullptr;     // CENTRE: the kept objects' positions; BOX: their upright boxes
    if (CENTRE || BOX) gpos = reinterpret_cast<double *>(ts_smem + ((reinterpret_cast<unsigned char *>(MEM ? old_track + Kobj : old_track) - ts_smem + 7) & ~(size_t)7));

    const size_t ob = (size_t)b * Kobj, kb = (size_t)b * K, tb = (size_t)b * T;
    float *target = out.aff_target + ob * Kobj;
    if (in.active && !in.active[b]) {
        for (int i = t; i < Kobj; i += TS_THREADS) { out.pred_gt_slot[ob + i] = -1; out.pred_gt_id[ob + i] = -1; out.iou[ob + i] = 0.0; }
        for (int j = t; j < K; j += TS_THREADS) out.gt_pred[kb + j] = -1;
        for (int e = t; e < Kobj * Kobj; e += TS_THREADS) target[e] = 0.f;
        if (t == 0) out.aff_defined[b] = 0;
        return;
    }
    const int nv = in.n_valid ? in.n_valid[b] : N, n = count_clamp(nv, N);
    const int rawp = in.num_objects[b], P = count_clamp(rawp, Kobj);
    const int G = count_clamp(in.gt_count[b], K);
    const bool reset = in.reset && in.reset[b];
    int used = count_clamp(st.table_used[b], T);
    int prevP = st.prev_count[b], prevG = st.prev_gt[b];
    long long *cnt = st.counters + (size_t)b * RTK_SCORE_COUNTERS;
    // MEM: the rows of the new record (the table's count clamped to [P, Kobj]) and the old record's labelled coasted rows
    int rawr = 0, R = 0, prevL = 0;
    if (MEM) {
        rawr = mm.table_count[b];
        R = max(count_clamp(rawr, Kobj), P);
        prevL = reset ? 0 : mm.labelled_coasted[b];
    }
    // the stream's cursors, read by every thread before thread 0 moves them (after two barriers at least)
    int log_f = 0, log_r = 0, log_l = 0;
    bool log_fits = false;
    if (LOG) {
        log_f = lg.cursor[b * 4 + 0];
        log_r = lg.cursor[b * 4 + 1];
        log_l = lg.cursor[b * 4 + 2];
        log_fits = log_f >= 0 && log_f < lg.F && log_r >= 0 && log_r <= lg.R - P && log_l >= 0 && log_l <= lg.R - G;
    }
    int log_q = 0, pair_at = 0, pair_total = 0;      // PAIRS: the pair cursor, the first pair of this thread's row, the frame's pairs
    if (PAIRS) log_q = pr.cursor[b];

    if (CENTRE) {      // the three arguments end here
        for (int e = t; e < 3 * G; e += TS_THREADS) gpos[e] = gt_centre[kb * 3 + e];
        if (t == 0) {
            gpos[3 * K] = zero_distance;
            reinterpret_cast<unsigned long long *>(gpos)[3 * K + 1] = (unsigned long long)(pair_sim + (size_t)b * pr.Q);
        }
    }
    if (BOX) {      // the four arguments end here
        for (int j = t; j < G; j += TS_THREADS) {
            const int slot = in.gt_slot[kb + j];
            double gx = 0.0, gy = 0.0, gz = 0.0, ux = 0.0, uy = 0.0, h0 = 0.0, h1 = 0.0, h2 = 0.0;
            bool ok = slot >= 0 && slot < K;
            if (ok) {      // centre | R row-major | half-extent: the heading is R's first column
                const double *bx = gt_boxes + (kb + slot) * RTK_GT_BOX_WORDS;
                gx = bx[0]; gy = bx[1]; gz = bx[2]; ux = bx[3]; uy = bx[6]; h0 = bx[12]; h1 = bx[13]; h2 = bx[14];
            }
            const double nn = sqrt(ux * ux + uy * uy);
            ok = ok && isfinite(gx) && isfinite(gy) && isfinite(gz) && isfinite(ux) && isfinite(uy) && isfinite(h0) && isfinite(h1) &&
                 isfinite(h2) && isfinite(nn) && nn != 0.0 && h0 > 0.0 && h1 > 0.0 && h2 > 0.0;
            double *g = gpos + 8 * j;
            g[0] = gx; g[1] = gy; g[2] = ux / nn; g[3] = uy / nn;
            g[4] = ok ? h0 : 0.0; g[5] = h1; g[6] = gz - h2; g[7] = gz + h2;
        }
        for (int i = t; i < Kobj; i += TS_THREADS) reinterpret_cast<unsigned long long *>(best_iou)[i] = 0ull;      // the rows' pair masks
        if (t == 0) {
            reinterpret_cast<unsigned long long *>(gpos)[8 * K] = (unsigned long long)mode;
            reinterpret_cast<unsigned long long *>(gpos)[8 * K + 1] = (unsigned long long)(pair_sim + (size_t)b * pr.Q);
        }
    }
    if (t < 8) scal[t] = 0;
    for (int i = t; i < Kobj; i += TS_THREADS) {
        psize[i] = 0;
        prev_id[i] = (!reset && i < prevP) ? st.prev_gt_id[ob + i] : -1;
        cur_id[i] = -1;
        if (MEM) old_track[i] = (!reset && i < prevP) ? mm.row_track[ob + i] : -1;
    }
    for (int e = t; e < Kobj * K; e += TS_THREADS) common[e] = 0;
    for (int j = t; j < K; j += TS_THREADS) {
        gsize[j] = j < G ? in.gt_size[kb + j] : 0;
        glabel[j] = j < G ? in.gt_label_id[kb + j] : -1;
        gslot[j] = j < G ? in.gt_slot[kb + j] : -1;
        gpred[j] = -1;
        entry[j] = -1;
    }
    __syncthreads();

    // ---- a reset closes the clip: classify the table's entries, clear it, drop the previous frame ----
    if (reset) {
        int mt = 0, pt = 0, ml = 0;
        for (int e = t; e < used; e += TS_THREADS) {
            const double r = (double)st.table_matched[tb + e] / (double)st.table_seen[tb + e];
            if (r > 0.8) ++mt; else if (r < 0.2) ++ml; else ++pt;
        }
        if (mt) atomicAdd(&scal[2], mt);
        if (pt) atomicAdd(&scal[3], pt);
        if (ml) atomicAdd(&scal[4], ml);
        __syncthreads();
        if (t == 0) { cnt[7] += used; cnt[8] += scal[2]; cnt[9] += scal[3]; cnt[10] += scal[4]; }
        used = 0;
        prevP = -1;
        prevG = 0;
    }

    // ---- this frame's tables: coordinates, the kept objects of every column, the two compacted lists ----
    for (int p = t; p < N; p += TS_THREADS) {
        const bool live = p < n;
        pts[p] = make_float4(live ? bcn_at(in.pc1, b, 0, p) : 0.f, live ? bcn_at(in.pc1, b, 1, p) : 0.f, live ? bcn_at(in.pc1, b, 2, p) : 0.f, 0.f);
        unsigned long long m = 0ull;
        if (live) {
            for (int j = 0; j < G; ++j)
                m |= (unsigned long long)((in.gt_members[(kb + j) * W + (p >> 5)] >> (p & 31)) & 1u) << j;
        }
        gmask[p] = m;
        if (m) qlist[atomicAdd(&scal[1], 1)] = p;
        const int o = live ? in.obj[(size_t)b * N + p] : -1;
        if (CENTRE) pts[p].w = __int_as_float((o >= 0 && o < P) ? o : -1);
        if (o >= 0 && o < P) {
            atomicAdd(&psize[o], 1);
            plist[atomicAdd(&scal[0], 1)] = p | (o << 16);
        }
    }
    __syncthreads();

    // ---- the pair count ----
    const int np = scal[0], nq = scal[1];
    for (int pi = wave; pi < np; pi += TS_WAVES) {
        const int p = plist[pi] & 0xffff, i = plist[pi] >> 16;
        const float4 a = pts[p];
        for (int qi = lane; qi < nq; qi += RTK_WAVE) {
            const int q = qlist[qi];
            const float4 o = pts[q];
            const float dx = a.x - o.x, dy = a.y - o.y, dz = a.z - o.z;        // float32 differences, as the host takes them
            const double d2 = ((double)dx * (double)dx + (double)dy * (double)dy) + (double)dz * (double)dz;
            if (d2 < 1e-5 * 1e-5) {
                unsigned long long m = gmask[q];
                while (m) {
                    const int j = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    atomicAdd(&common[i * K + j], 1);
                }
            }
        }
    }
    __syncthreads();

    // ---- PAIRS: the rows' pair counts, their ordered prefix, and whether the frame's pairs fit ----
    if (PAIRS) {
        int mine = 0;
        double cx = 0.0, cy = 0.0, cz = 0.0;      // CENTRE: the centre of this thread's detection
        unsigned long long logged = 0ull;          // CENTRE, BOX: the kept objects (K <= 64) this thread's row is logged with
        double bl = 0.0, bw = 0.0, bc = 0.0, bs = 0.0, bbot = 0.0, btop = 0.0, bh = 0.0;      // BOX: this thread's detection (cx, cy: its centre)
        bool bev = false;
        if (BOX) {
            // the (i, j) decisions spread over the workgroup: pair e = i G + j to thread e mod 256, which forms detection i's terms for
            // itself and raises bit j of row i's mask in LDS (an integer OR: any order, the same word).  The masks lie where best_iou
            // will: zeroed at the start, read back by the row's own thread, which is also the one that writes best_iou[i] below.
            unsigned long long *rowmask = reinterpret_cast<unsigned long long *>(best_iou);
            bev = reinterpret_cast<unsigned long long *>(gpos)[8 * K] == (unsigned long long)RTK_SCORE_BOX_BEV;
            for (int e = t; e < P * G; e += TS_THREADS) {
                const int i = e / G, j = e - i * G;
                if (ts_box_detection(det_box + (ob + i) * 8, det_valid[ob + i], bev, cx, cy, bl, bw, bc, bs, bbot, btop, bh) &&
                    ts_box_similarity(cx, cy, bl, bw, bc, bs, bbot, btop, bh, gpos + 8 * j, bev) > 0.0)      // the one place a pair is decided: s > 0.0, a NaN is not
                    atomicOr(&rowmask[i], 1ull << j);
            }
            __syncthreads();
            if (t < P) {
                logged = rowmask[t];
                if (logged) ts_box_detection(det_box + (ob + t) * 8, det_valid[ob + t], bev, cx, cy, bl, bw, bc, bs, bbot, btop, bh);
            }
            mine = __popcll(logged);
        } else if (CENTRE) {
            if (t < P) {
                double sx = 0.0, sy = 0.0, sz = 0.0;
                int m = 0;
                // ascending column order: rtk_gt_objects' rule for its own centres.  Without a branch, so that the reads of LDS run ahead
                // of the adds (behind a test of .w every column costs a round trip of its own): another detection's column adds +0.0,
                // which changes no bit -- a sum that starts from +0.0 is never -0.0 (x + -x is +0.0 under round-to-nearest)
#pragma unroll 8
                for (int p = 0; p < n; ++p) {
                    const float4 a = pts[p];
                    const bool own = __float_as_int(a.w) == t;
                    sx += own ? (double)a.x : 0.0;
                    sy += own ? (double)a.y : 0.0;
                    sz += own ? (double)a.z : 0.0;
                    m += own ? 1 : 0;
                }
                if (m > 0) {
                    cx = sx / (double)m; cy = sy / (double)m; cz = sz / (double)m;
#pragma unroll 4
                    for (int j = 0; j < G; ++j)      // the one place a pair is decided: s > 0.0, a NaN is not
                        if (ts_centre_similarity(cx, cy, cz, gpos + 3 * j, gpos[3 * K]) > 0.0) logged |= 1ull << j;
                }
            }
            mine = __popcll(logged);
        } else if (t < P) {
            for (int j = 0; j < G; ++j) mine += common[t * K + j] > 0 ? 1 : 0;
        }
        const int upto = wave_inclusive_scan(mine, lane);
        if (lane == RTK_WAVE - 1) scal[4 + wave] = upto;      // 4..7: free since the reset's barrier
        __syncthreads();
        for (int w = 0; w < TS_WAVES; ++w) {
            const int total = scal[4 + w];
            if (w < wave) pair_at += total;
            pair_total += total;
        }
        pair_at += upto - mine;
        log_fits = log_fits && log_q >= 0 && log_q <= pr.Q - pair_total;
        if ((CENTRE || BOX) && log_fits) {      // row t's pairs in ascending j: key, common, and s formed again by the same operations
            double *sim = reinterpret_cast<double *>(reinterpret_cast<unsigned long long *>(gpos)[SIMW * K + 1]) + log_q + pair_at;
            size_t q = (size_t)b * pr.Q + log_q + pair_at;
            while (logged) {
                const int j = __ffsll((long long)logged) - 1;
                logged &= logged - 1;
                pr.pair_key[q] = (t << 8) | j;
                pr.pair_common[q] = common[t * K + j];
                if (BOX) *sim++ = ts_box_similarity(cx, cy, bl, bw, bc, bs, bbot, btop, bh, gpos + 8 * j, bev);
                else *sim++ = ts_centre_similarity(cx, cy, cz, gpos + 3 * j, gpos[3 * K]);
                ++q;
            }
        }
    }

    // ---- every prediction's best object: strict > from 0, the first of equals ----
    for (int i = t; i < P; i += TS_THREADS) {
        int bj = -1;
        double bi = 0.0;
        for (int j = 0; j < G; ++j) {
            const int c = common[i * K + j], den = psize[i] + gsize[j] - c;
            const double iou = den == 0 ? 0.0 : (double)c / (double)den;
            if (iou > bi) { bi = iou; bj = j; }
        }
        best[i] = bj;
        best_iou[i] = bi;
        if (LOG && log_fits) {
            const size_t r = (size_t)b * lg.R + log_r + i;
            lg.rec_track[r] = in.object_ids[ob + i];
            lg.rec_conf[r] = lg.object_conf[ob + i];
            lg.rec_best[r] = bj >= 0 ? glabel[bj] : -1;
            lg.rec_iou[r] = bi;
            if (PAIRS) {
                pr.rec_size[r] = psize[i];
                if (!CENTRE && !BOX) {      // (CENTRE, BOX: written with the prefix above)
                    size_t q = (size_t)b * pr.Q + log_q + pair_at;
                    for (int j = 0; j < G; ++j) {
                        const int c = common[i * K + j];
                        if (c > 0) { pr.pair_key[q] = (i << 8) | j; pr.pair_common[q] = c; ++q; }
                    }
                }
            }
        }
    }
    if (LOG && log_fits) {
        for (int j = t; j < G; j += TS_THREADS) {
            lg.label[(size_t)b * lg.R + log_l + j] = glabel[j];
            if (PAIRS) pr.label_size[(size_t)b * lg.R + log_l + j] = gsize[j];
        }
    }
    // ---- which table entry holds each kept object's label id ----
    for (int e = t; e < used; e += TS_THREADS) {
        const int key = st.table_key[tb + e];
        for (int j = 0; j < G; ++j)
            if (glabel[j] == key) entry[j] = e;      // label ids are distinct within a frame and within the table
    }
    // ---- MEM: a coasted row keeps the label id its track had in the old record (the first row of that track id) ----
    if (MEM) {
        const int rows = (!reset && prevP > 0) ? min(prevP, Kobj) : 0;
        for (int r = P + t; r < R; r += TS_THREADS) {
            const int track = mm.table_ids[ob + r];
            int label = -1;
            for (int i = rows - 1; i >= 0; --i)
                if (old_track[i] == track) label = prev_id[i];
            cur_id[r] = label;      // the greedy pass below writes the rows < P only
        }
    }
    __syncthreads();

    // ---- greedy assignment, table and counters: one thread, in order ----
    if (t == 0) {
        int M = 0, idsw = 0, flags = (nv != n ? RTK_SCORE_FLAG_NVALID : 0) | (rawp != P ? RTK_SCORE_FLAG_OBJECTS : 0);
        if (MEM && rawr != R) flags |= RTK_SCORE_FLAG_TABLE;
        double iou_sum = st.iou_sum[b];
        for (int i = 0; i < P; ++i) {
            const int j = best[i];
            if (j < 0 || gpred[j] >= 0) { best[i] = -1; best_iou[i] = 0.0; continue; }      // taken: no second choice
            gpred[j] = i;
            cur_id[i] = glabel[j];
            iou_sum += best_iou[i];
            ++M;
        }
        for (int j = 0; j < G; ++j) {
            int e = entry[j];
            if (e < 0) {
                if (used >= T) { flags |= RTK_SCORE_FLAG_TRACKS; continue; }
                e = used++;
                st.table_key[tb + e] = glabel[j];
                st.table_last[tb + e] = -1;
                st.table_seen[tb + e] = 0;
                st.table_matched[tb + e] = 0;
            }
            st.table_seen[tb + e] += 1;
            if (gpred[j] >= 0) {
                const int track = in.object_ids[ob + gpred[j]], last = st.table_last[tb + e];
                if (last != -1 && last != track) ++idsw;
                st.table_last[tb + e] = track;
                st.table_matched[tb + e] += 1;
            }
        }
        st.table_used[b] = used;
        st.iou_sum[b] = iou_sum;
        cnt[0] += 1; cnt[1] += G; cnt[2] += P; cnt[3] += M; cnt[4] += P - M; cnt[5] += G - M; cnt[6] += idsw;
        if (LOG) {
            if (log_fits) {
                int *fr = lg.frame + ((size_t)b * lg.F + log_f) * 4;
                fr[0] = log_r; fr[1] = log_l; fr[2] = P | (reset ? 65536 : 0); fr[3] = G;
                lg.cursor[b * 4 + 0] = log_f + 1; lg.cursor[b * 4 + 1] = log_r + P; lg.cursor[b * 4 + 2] = log_l + G;
                if (PAIRS) {
                    pr.frame_pair[((size_t)b * lg.F + log_f) * 2 + 0] = log_q;
                    pr.frame_pair[((size_t)b * lg.F + log_f) * 2 + 1] = pair_total;
                    pr.cursor[b] = log_q + pair_total;
                }
            } else {
                flags |= RTK_SCORE_FLAG_LOG;
            }
        }
        if (flags) st.flags[b] |= flags;
        if (MEM) {
            int labelled = 0;
            for (int r = P; r < R; ++r) labelled += cur_id[r] >= 0 ? 1 : 0;
            mm.labelled_coasted[b] = labelled;
            st.prev_count[b] = R;
            st.prev_gt[b] = G;
            out.aff_defined[b] = (prevP > 0 && (prevG > 0 || prevL > 0) && P > 0 && G > 0) ? 1 : 0;
        } else {
            st.prev_count[b] = P;
            st.prev_gt[b] = G;
            out.aff_defined[b] = (prevP > 0 && prevG > 0 && P > 0 && G > 0) ? 1 : 0;
        }
    }
    __syncthreads();

    // ---- outputs, and this frame as the next one's previous frame ----
    for (int i = t; i < Kobj; i += TS_THREADS) {
        const int j = i < P ? best[i] : -1;
        out.pred_gt_slot[ob + i] = j >= 0 ? gslot[j] : -1;
        out.pred_gt_id[ob + i] = j >= 0 ? glabel[j] : -1;
        out.iou[ob + i] = j >= 0 ? best_iou[i] : 0.0;
        st.prev_gt_id[ob + i] = cur_id[i];
        if (MEM) mm.row_track[ob + i] = i < P ? in.object_ids[ob + i] : (i < R ? mm.table_ids[ob + i] : -1);
    }
    for (int j = t; j < K; j += TS_THREADS) out.gt_pred[kb + j] = gpred[j];
    const int rows = prevP > 0 ? prevP : 0;
    for (int e = t; e < Kobj * Kobj; e += TS_THREADS) {
        const int i = e / Kobj, j = e - i * Kobj;
        target[e] = (i < rows && j < P && prev_id[i] >= 0 && prev_id[i] == cur_id[j]) ? 1.f : 0.f;
    }
}

// The checks every scoring entry point makes before its launch (lg NULL: no log); lds: the bytes of its variant.
static inline int ts_score_validate(const rtk_track_score_in_t *in, const rtk_track_score_state_t *st, const rtk_track_score_out_t *out,
                                    const rtk_score_log_t *lg, size_t lds) {
    RTK_REQUIRE(in->B >= 1 && in->B <= 65535 && in->N >= 1 && in->N <= RTK_SCORE_MAX_POINTS && in->T >= 1,
                "track_score: bad sizes B=%d N=%d T=%d", in->B, in->N, in->T);
    RTK_REQUIRE(in->Kobj >= 1 && in->Kobj <= RTK_SCORE_MAX_OBJECTS, "track_score: Kobj=%d object slots outside [1, %d]", in->Kobj,
                RTK_SCORE_MAX_OBJECTS);
    RTK_REQUIRE(in->K >= 1 && in->K <= RTK_SCORE_MAX_BOXES, "track_score: K=%d ground-truth slots outside [1, %d]", in->K, RTK_SCORE_MAX_BOXES);
    RTK_REQUIRE(lds <= RTK_SCORE_LDS_LIMIT, "track_score: Kobj=%d, K=%d, N=%d need %zu bytes of LDS per stream, the limit is %d", in->Kobj,
                in->K, in->N, lds, RTK_SCORE_LDS_LIMIT);
    RTK_REQUIRE(in->pc1.ptr && in->obj && in->num_objects && in->object_ids && in->gt_slot && in->gt_label_id && in->gt_count &&
                in->gt_size && in->gt_members, "track_score: null input");
    RTK_REQUIRE(st->counters && st->iou_sum && st->table_key && st->table_last && st->table_seen && st->table_matched && st->table_used &&
                st->prev_gt_id && st->prev_count && st->prev_gt && st->flags, "track_score: null state");
    RTK_REQUIRE(out->pred_gt_slot && out->pred_gt_id && out->gt_pred && out->iou && out->aff_target && out->aff_defined,
                "track_score: null output");
    if (lg) {
        RTK_REQUIRE(lg->F >= 1 && lg->R >= 1, "track_score_logged: a log of F=%d frames and R=%d records per stream", lg->F, lg->R);
        RTK_REQUIRE(lg->object_conf && lg->cursor && lg->frame && lg->label && lg->rec_track && lg->rec_best && lg->rec_conf && lg->rec_iou,
                    "track_score_logged: null log");
    }
    return RTK_OK;
}
