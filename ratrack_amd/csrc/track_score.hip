// track_score.hip -- ground-truth objects and the tracking score of a batch on the device (include/rtk_score.h,
// ratrack_amd/track_score.py).
//
//   rtk_gt_objects    one workgroup per stream: the point set of every frame-1 box as an N-bit mask, the float64 centres, the serial
//                     rider merge and the minimum object size (vod_gt.filter_object_points' objs_combined; track4d_utils.py:105-176)
//   rtk_track_score   one workgroup per stream: vod_gt.map_gt_objects (track4d_utils.py:50-102), the 0/1 target of
//                     loss.affinity_loss against the stream's previous frame, and the running CLEAR-MOT counts with the per-stream
//                     table of ground-truth tracks; rtk_track_score_logged is the same launch that also appends the frame to the
//                     stream's log for the confidence sweep (track_sweep.hip); rtk_track_score_memory
//                     (track_score_memory.hip) is the same body with a record as tall as the table of a tracker that keeps lost tracks
//
// Layout of both: 256 threads = 4 waves of 64, one stream's tables in LDS (the byte counts are ts_gto_lds / ts_score_lds below).
//
// gt_objects: thread p tests column p against every box (the box words are broadcast reads) and a wave's ballot is two mask words
// of that box at once.  `canon` marks the first column of every distinct coordinate triple (each thread scans the columns before
// its own).  A box's membership depends on the coordinates alone, so equal triples sit in the same masks and the de-duplicated set
// of a merged object is simply mask & canon.  The centre sums are one thread per box walking its mask in column order; a rider's
// target depends on the ORIGINAL centres only, so all targets are found in parallel (thread k) and what stays serial is the
// OR-ing in label order, one barrier per box.
//
// track_score: the predicted points (column | object << 16) and the columns that lie in a kept ground-truth object are compacted
// into two lists; wave w takes the predicted points w, w + 4, ..., its lanes the ground-truth columns.  A pair closer than 1e-5 adds
// one to common[i][j] for every kept object j whose mask holds the column (the bits of a 64-bit word per column).  Thread i then
// finds prediction i's best object; the greedy pass over the predictions, the table update and the counters are thread 0 alone:
// a few hundred steps over small LDS tables, kept serial and exact.  Every sum but iou_sum is an integer; iou_sum is added in
// prediction order by that one thread.
#include <math.h>

#include "batch_common.h"
#include "rtk_common.h"
#include "rtk_score.h"
#include "track_score_body.h"


// masks are written two words (one wave) at a time: an even number of words per row
static inline int ts_row_words(int N) { return 2 * ((N + 63) / 64); }

// gt_objects LDS: pts[N] float4 (x, y, z, -: one 16-byte read per point) | box[K][16] f64 | centre[K][3] f64 | cur[K][WR] u32 |
//                 canon[WR] u32 | cnt, near, state, size [K] i32
static size_t ts_gto_lds(int K, int N) {
    const size_t WR = (size_t)ts_row_words(N);
    return (size_t)N * sizeof(float4) + (size_t)K * (RTK_GT_BOX_WORDS + 3) * sizeof(double) + ((size_t)K + 1) * WR * sizeof(unsigned) +
           (size_t)4 * K * sizeof(int);
}

#define TS_OBJECT 1      // the box holds a point
#define TS_RIDER 2
#define TS_MERGED 4      // received a rider's points
#define TS_DROPPED 8     // a rider merged away
#define TS_KEPT 16

__global__ __launch_bounds__(TS_THREADS) void gt_objects_kernel(const rtk_gt_objects_in_t in, const rtk_gt_objects_out_t out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ts_smem[];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & (RTK_WAVE - 1);
    const int N = in.N, K = in.K, W = (N + 31) / 32, WR = 2 * ((N + 63) / 64);
    float4 *pts = reinterpret_cast<float4 *>(ts_smem);
    double *box = reinterpret_cast<double *>(pts + N), *centre = box + (size_t)K * RTK_GT_BOX_WORDS;
    unsigned *cur = reinterpret_cast<unsigned *>(centre + (size_t)K * 3), *canon = cur + (size_t)K * WR;
    int *cnt = reinterpret_cast<int *>(canon + WR), *near = cnt + K, *state = near + K, *size = state + K;

    const int raw = in.frame1.count[b], nb = count_clamp(raw, K);
    const int nv = in.n_valid ? in.n_valid[b] : N, n = count_clamp(nv, N);
    if (t == 0) out.flags[b] = (raw != nb ? RTK_SCORE_FLAG_BOXES : 0) | (nv != n ? RTK_SCORE_FLAG_NVALID : 0);
    const size_t kb = (size_t)b * K;
    for (int e = t; e < nb * RTK_GT_BOX_WORDS; e += TS_THREADS) box[e] = in.frame1.boxes[kb * RTK_GT_BOX_WORDS + e];
    for (int p = t; p < N; p += TS_THREADS) {
        const bool live = p < n;
        pts[p] = make_float4(live ? bcn_at(in.pc1, b, 0, p) : 0.f, live ? bcn_at(in.pc1, b, 1, p) : 0.f, live ? bcn_at(in.pc1, b, 2, p) : 0.f, 0.f);
    }
    __syncthreads();

    // ---- membership masks, and the first column of every distinct triple ----
    for (int base = 0; base < WR * 32; base += TS_THREADS) {
        const int p = base + t;
        const bool live = p < n;
        const float4 mine = live ? pts[p] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float xf = mine.x, yf = mine.y, zf = mine.z;
        const double x = (double)xf, y = (double)yf, z = (double)zf;
        const int w = (p >> 6) * 2;               // the wave's two words (p < WR * 32 for the whole wave, or for none of it)
        for (int k = 0; k < nb; ++k) {
            const unsigned long long m = __ballot(live && box_inside(box + (size_t)k * RTK_GT_BOX_WORDS, x, y, z));
            if (lane == 0 && p < WR * 32) {
                cur[(size_t)k * WR + w] = (unsigned)m;
                cur[(size_t)k * WR + w + 1] = (unsigned)(m >> 32);
            }
        }
        bool first = live;
        const unsigned xb = __float_as_uint(xf), yb = __float_as_uint(yf), zb = __float_as_uint(zf);
        const int top = min(base + TS_THREADS, n);
#pragma unroll 8
        for (int q = 0; q < top; ++q) {           // every lane reads the same 16 bytes: a broadcast; eight reads in flight
            const float4 o = pts[q];
            const bool same = __float_as_uint(o.x) == xb && __float_as_uint(o.y) == yb && __float_as_uint(o.z) == zb;
            first = first && !(q < p && same);
        }
        const unsigned long long m = __ballot(first);
        if (lane == 0 && p < WR * 32) {
            canon[w] = (unsigned)m;
            canon[w + 1] = (unsigned)(m >> 32);
        }
    }
    __syncthreads();

    // ---- centres: one thread per box, float64 sums in column order ----
    for (int k = t; k < K; k += TS_THREADS) {
        int c = 0;
        double sx = 0.0, sy = 0.0, sz = 0.0;
        if (k < nb) {
            for (int w = 0; w < W; ++w) {
                unsigned m = cur[(size_t)k * WR + w];
                while (m) {               // four columns per turn: their reads travel together, the additions stay in column order
                    int p[4];
                    bool v[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        v[u] = m != 0u;
                        p[u] = v[u] ? w * 32 + __ffs(m) - 1 : p[0];
                        m &= m - 1u;
                    }
                    float4 a[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) a[u] = pts[p[u]];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        if (v[u]) { sx += (double)a[u].x; sy += (double)a[u].y; sz += (double)a[u].z; ++c; }
                    }
                }
            }
        }
        cnt[k] = c;
        centre[k * 3 + 0] = c ? sx / (double)c : 0.0;
        centre[k * 3 + 1] = c ? sy / (double)c : 0.0;
        centre[k * 3 + 2] = c ? sz / (double)c : 0.0;
        state[k] = (c ? TS_OBJECT : 0) | ((k < nb && in.types[kb + k]) ? TS_RIDER : 0);
    }
    __syncthreads();
    // ---- every rider's target: the nearest other object by its original centre, strict <
    for (int k = t; k < K; k += TS_THREADS) {
        int best = -1;
        if ((state[k] & (TS_OBJECT | TS_RIDER)) == (TS_OBJECT | TS_RIDER)) {
            double bd = INFINITY;
            for (int o = 0; o < nb; ++o) {
                if (o == k || !(state[o] & TS_OBJECT)) continue;
                const double dx = centre[k * 3] - centre[o * 3], dy = centre[k * 3 + 1] - centre[o * 3 + 1],
                             dz = centre[k * 3 + 2] - centre[o * 3 + 2];
                const double d = sqrt((dx * dx + dy * dy) + dz * dz);
                if (d < bd) { bd = d; best = o; }
            }
        }
        near[k] = best;
    }
    __syncthreads();
    // ---- the merge, serial in label order (near[] and the rider bits do not change: the branch is uniform) ----
    for (int k = 0; k < nb; ++k) {
        const int target = near[k];
        if (target < 0) continue;
        for (int w = t; w < WR; w += TS_THREADS) cur[(size_t)target * WR + w] |= cur[(size_t)k * WR + w];
        if (t == 0) { state[target] |= TS_MERGED; state[k] |= TS_DROPPED; }
        __syncthreads();
    }
    // ---- sizes: a merged object counts each distinct triple once ----
    for (int k = t; k < K; k += TS_THREADS) {
        int s = 0;
        const bool merged = (state[k] & TS_MERGED) != 0;
        if (state[k] & TS_OBJECT) {
            for (int w = 0; w < W; ++w) s += __popc(cur[(size_t)k * WR + w] & (merged ? canon[w] : 0xffffffffu));
        }
        size[k] = s;
        if ((state[k] & TS_OBJECT) && !(state[k] & TS_DROPPED) && s >= in.min_obj_points) state[k] |= TS_KEPT;
    }
    __syncthreads();
    // ---- the kept objects in label order ----
    int kept = 0;
    for (int k = 0; k < K; ++k) kept += (state[k] & TS_KEPT) ? 1 : 0;
    if (t == 0) out.count[b] = kept;
    for (int j = kept + t; j < K; j += TS_THREADS) {
        out.slot[kb + j] = -1;
        out.label_id[kb + j] = -1;
        out.size[kb + j] = 0;
        for (int c = 0; c < 3; ++c) out.centre[(kb + j) * 3 + c] = 0.0;
    }
    for (int e = kept * W + t; e < K * W; e += TS_THREADS) out.members[kb * W + e] = 0u;
    int j = 0;
    for (int k = 0; k < K; ++k) {
        if (!(state[k] & TS_KEPT)) continue;
        const bool merged = (state[k] & TS_MERGED) != 0;
        for (int w = t; w < W; w += TS_THREADS)
            out.members[(kb + j) * W + w] = cur[(size_t)k * WR + w] & (merged ? canon[w] : 0xffffffffu);
        if (t == 0) {
            out.slot[kb + j] = k;
            out.label_id[kb + j] = in.frame1.box_id[kb + k];
            out.size[kb + j] = size[k];
            for (int c = 0; c < 3; ++c) out.centre[(kb + j) * 3 + c] = centre[k * 3 + c];
        }
        ++j;
    }
}

extern "C" int rtk_gt_objects_lds_bytes(int K, int N) {
    if (K < 1 || N < 1 || K > RTK_SCORE_MAX_BOXES || N > RTK_SCORE_MAX_POINTS) return -1;
    return (int)ts_gto_lds(K, N);
}

extern "C" int rtk_gt_objects(const rtk_gt_objects_in_t *in, const rtk_gt_objects_out_t *out, rtk_stream_t stream) {
    RTK_REQUIRE(in && out, "gt_objects: null argument block");
    RTK_REQUIRE(in->B >= 1 && in->B <= 65535 && in->N >= 1 && in->N <= RTK_SCORE_MAX_POINTS, "gt_objects: bad sizes B=%d N=%d", in->B, in->N);
    RTK_REQUIRE(in->K >= 1 && in->K <= RTK_SCORE_MAX_BOXES, "gt_objects: K=%d box slots outside [1, %d]", in->K, RTK_SCORE_MAX_BOXES);
    const size_t lds = ts_gto_lds(in->K, in->N);
    RTK_REQUIRE(lds <= RTK_SCORE_LDS_LIMIT, "gt_objects: K=%d, N=%d need %zu bytes of LDS per stream, the limit is %d", in->K, in->N, lds,
                RTK_SCORE_LDS_LIMIT);
    RTK_REQUIRE(in->pc1.ptr && in->frame1.boxes && in->frame1.box_id && in->frame1.count && in->types, "gt_objects: null input");
    RTK_REQUIRE(out->slot && out->label_id && out->count && out->size && out->members && out->centre && out->flags,
                "gt_objects: null output");
    (void)hipFuncSetAttribute((const void *)gt_objects_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RTK_SCORE_LDS_LIMIT);
    gt_objects_kernel<<<in->B, TS_THREADS, lds, (hipStream_t)stream>>>(*in, *out);
    RTK_CHECK_LAUNCH("gt_objects");
    return RTK_OK;
}

// ------------------------------------------------------------------------------------------------
// rtk_track_score
// ------------------------------------------------------------------------------------------------
// The LDS layout and the body of the scoring kernels: track_score_body.h (shared with track_score_memory.hip).
__global__ __launch_bounds__(TS_THREADS) void track_score_kernel(const rtk_track_score_in_t in, const rtk_track_score_state_t st,
                                                                 const rtk_track_score_out_t out) {
    track_score_body<false, false>(in, st, out, rtk_score_log_t{}, rtk_score_memory_t{});
}

// the logged variant: the same body (and the same LDS: the log goes straight to memory)
__global__ __launch_bounds__(TS_THREADS) void ts_logged_kernel(const rtk_track_score_in_t in, const rtk_track_score_state_t st,
                                                               const rtk_track_score_out_t out, const rtk_score_log_t lg) {
    track_score_body<true, false>(in, st, out, lg, rtk_score_memory_t{});
}

extern "C" int rtk_track_score_lds_bytes(int Kobj, int K, int N) {
    if (Kobj < 1 || K < 1 || N < 1 || Kobj > RTK_SCORE_MAX_OBJECTS || K > RTK_SCORE_MAX_BOXES || N > RTK_SCORE_MAX_POINTS) return -1;
    return (int)ts_score_lds(Kobj, K, N);
}

static int ts_score_launch(const rtk_track_score_in_t *in, const rtk_track_score_state_t *st, const rtk_track_score_out_t *out,
                           const rtk_score_log_t *lg, rtk_stream_t stream) {
    RTK_REQUIRE(in && st && out, "track_score: null argument block");
    const size_t lds = ts_score_lds(in->Kobj, in->K, in->N);
    const int status = ts_score_validate(in, st, out, lg, lds);
    if (status != RTK_OK) return status;
    if (lg) {
        (void)hipFuncSetAttribute((const void *)ts_logged_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RTK_SCORE_LDS_LIMIT);
        ts_logged_kernel<<<in->B, TS_THREADS, lds, (hipStream_t)stream>>>(*in, *st, *out, *lg);
        RTK_CHECK_LAUNCH("track_score_logged");
        return RTK_OK;
    }
    (void)hipFuncSetAttribute((const void *)track_score_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RTK_SCORE_LDS_LIMIT);
    track_score_kernel<<<in->B, TS_THREADS, lds, (hipStream_t)stream>>>(*in, *st, *out);
    RTK_CHECK_LAUNCH("track_score");
    return RTK_OK;
}

extern "C" int rtk_track_score(const rtk_track_score_in_t *in, const rtk_track_score_state_t *st, const rtk_track_score_out_t *out,
                               rtk_stream_t stream) {
    return ts_score_launch(in, st, out, nullptr, stream);
}

extern "C" int rtk_track_score_logged(const rtk_track_score_in_t *in, const rtk_track_score_state_t *st, const rtk_track_score_out_t *out,
                                      const rtk_score_log_t *lg, rtk_stream_t stream) {
    RTK_REQUIRE(lg, "track_score_logged: null log block");
    return ts_score_launch(in, st, out, lg, stream);
}
