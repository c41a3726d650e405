// track_score.hip -- ground-truth objects and the tracking score of a batch on the device (include/rtk_score.h,
// ratrack_amd/track_score.py).
//
//   rtk_gt_objects    one workgroup per stream: the point set of every frame-1 box as an N-bit mask, the float64 centres, the serial
//                     rider merge and the minimum object size (vod_gt.filter_object_points' objs_combined; track4d_utils.py:105-176)
//   rtk_track_score   one workgroup per stream: vod_gt.map_gt_objects (track4d_utils.py:50-102), the 0/1 target of
//                     loss.affinity_loss against the stream's previous frame, and the running CLEAR-MOT counts with the per-stream
//                     table of ground-truth tracks; rtk_track_score_logged is the same launch that also appends the frame to the
//                     stream's log for the confidence sweep (track_sweep.hip); rtk_track_score_memory, rtk_track_score_pairs,
//                     rtk_track_score_pairs_centre and rtk_track_score_pairs_box are further variants of that launch (listed below)
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
// The LDS layouts and the one body of the scoring kernels are track_score_body.h's; this is everything around the body: the one kernel
// template, the LDS figure, the launcher and the six entry points.  The ten instantiations, each one workgroup of 256 threads per
// stream with the stream's tables in dynamic LDS:
//   plain, logged             rtk_track_score, rtk_track_score_logged: the same LDS, the log goes straight to memory
//   memory (with any other)   rtk_track_score_memory, or a memory block given to the pair-logging entry points: a record as tall as the
//                             table of a tracker that keeps lost tracks (BatchedTracker(max_age=...), rtk_track_memory), so that the 0/1
//                             target of the tracking loss has a row for every coasted track; Kobj words of LDS more
//   pairs                     rtk_track_score_pairs: every (detection, kept object) pair with common > 0 also goes to the pair log, the
//                             input of the per-frame optimal matching (track_optimal.hip); the same LDS
//   centre                    rtk_track_score_pairs_centre: the pair log under s = max(0, 1 - |c_i - g_j| / zero_distance) in place of the
//                             point IoU; 24 K + 16 bytes of LDS more
//   box                       rtk_track_score_pairs_box: the pair log under the IoU of each detection's fitted box (rtk_object_boxes) and
//                             each kept object's label box read upright, in three dimensions or in the bird's-eye view; 64 K + 16 bytes more
// Under centre and box a pair is logged iff s > 0, whatever its common count, and the similarity's arguments are staged in LDS once, so
// that none rides in scalar registers through the body.  Everything but the pair log is bit for bit what the plain launch writes, and
// the main log is the same in every logging variant.  One writer per word or row, plain stores, no floating-point atomics: the same
// bits on every run.  A block an instantiation has no switch for is not read by it.
struct ts_sim_args_t {      // the similarity of the pair log: pair_sim with CENTRE or BOX, the next two with CENTRE, the last four with BOX
    double *pair_sim;
    const double *gt_centre;
    double zero_distance;
    const double *det_box;
    const int *det_valid;
    const double *gt_boxes;
    int mode;
};

template <bool LOG, bool MEM, bool PAIRS, bool CENTRE, bool BOX>
__global__ __launch_bounds__(TS_THREADS) void ts_kernel(const rtk_track_score_in_t in, const rtk_track_score_state_t st,
                                                        const rtk_track_score_out_t out, const rtk_score_log_t lg, const rtk_score_memory_t mm,
                                                        const rtk_score_pairs_t pr, const ts_sim_args_t sa) {
    track_score_body<LOG, MEM, PAIRS, CENTRE, BOX>(in, st, out, lg, mm, pr, sa.pair_sim, sa.gt_centre, sa.zero_distance, sa.det_box, sa.det_valid,
                                                   sa.gt_boxes, sa.mode);
}

typedef void (*ts_kernel_t)(const rtk_track_score_in_t, const rtk_track_score_state_t, const rtk_track_score_out_t, const rtk_score_log_t,
                            const rtk_score_memory_t, const rtk_score_pairs_t, const ts_sim_args_t);
enum ts_variant_t { TS_PLAIN, TS_LOGGED, TS_PAIRS, TS_CENTRE, TS_BOX };
static const ts_kernel_t ts_kernels[5][2] = {      // [variant][without | with the memory block]: the ten instantiations there are
    {ts_kernel<false, false, false, false, false>, ts_kernel<false, true, false, false, false>},
    {ts_kernel<true, false, false, false, false>, ts_kernel<true, true, false, false, false>},
    {ts_kernel<true, false, true, false, false>, ts_kernel<true, true, true, false, false>},
    {ts_kernel<true, false, true, true, false>, ts_kernel<true, true, true, true, false>},
    {ts_kernel<true, false, true, false, true>, ts_kernel<true, true, true, false, true>},
};

// the dynamic LDS of a variant: the log and the pair log take none
static size_t ts_lds(int Kobj, int K, int N, bool memory, ts_variant_t variant) {
    if (variant == TS_CENTRE) return ts_score_centre_lds(Kobj, K, N, memory);
    if (variant == TS_BOX) return ts_score_box_lds(Kobj, K, N, memory);
    return memory ? ts_score_memory_lds(Kobj, K, N) : ts_score_lds(Kobj, K, N);
}

// what the exported functions answer: -1 outside the sizes any variant takes
static int ts_lds_bytes(int Kobj, int K, int N, bool memory, ts_variant_t variant) {
    if (Kobj < 1 || K < 1 || N < 1 || Kobj > RTK_SCORE_MAX_OBJECTS || K > RTK_SCORE_MAX_BOXES || N > RTK_SCORE_MAX_POINTS) return -1;
    return (int)ts_lds(Kobj, K, N, memory, variant);
}

extern "C" int rtk_track_score_lds_bytes(int Kobj, int K, int N) { return ts_lds_bytes(Kobj, K, N, false, TS_PLAIN); }
extern "C" int rtk_track_score_memory_lds_bytes(int Kobj, int K, int N) { return ts_lds_bytes(Kobj, K, N, true, TS_PLAIN); }
extern "C" int rtk_track_score_centre_lds_bytes(int Kobj, int K, int N, int memory) { return ts_lds_bytes(Kobj, K, N, memory != 0, TS_CENTRE); }
extern "C" int rtk_track_score_box_lds_bytes(int Kobj, int K, int N, int memory) { return ts_lds_bytes(Kobj, K, N, memory != 0, TS_BOX); }

#define TS_NEED_LOG 1
#define TS_NEED_MEMORY 2
#define TS_NEED_PAIRS 4

// The one scoring launch.  name: the entry point's name in the refusals; launched: its name in the report of a failed launch; need: the
// blocks it cannot do without (lg, mm and pr may each be NULL otherwise); sim: TS_CENTRE or TS_BOX with the arguments in sa, which the
// caller has checked, or TS_PLAIN for the point IoU, where the blocks given choose the variant.
static int ts_launch(const char *name, const char *launched, unsigned need, const rtk_track_score_in_t *in,
                     const rtk_track_score_state_t *st, const rtk_track_score_out_t *out, const rtk_score_log_t *lg,
                     const rtk_score_memory_t *mm, const rtk_score_pairs_t *pr, ts_variant_t sim, const ts_sim_args_t &sa, rtk_stream_t stream) {
    RTK_REQUIRE(in && st && out, "%s: null argument block", name);
    RTK_REQUIRE(mm || !(need & TS_NEED_MEMORY), "%s: null memory block", name);
    RTK_REQUIRE(lg || !(need & TS_NEED_LOG), "%s: null log block", name);
    RTK_REQUIRE(pr || !(need & TS_NEED_PAIRS), "%s: null pair-log block", name);
    const ts_variant_t variant = sim != TS_PLAIN ? sim : pr ? TS_PAIRS : lg ? TS_LOGGED : TS_PLAIN;
    const size_t lds = ts_lds(in->Kobj, in->K, in->N, mm != nullptr, variant);
    const int status = ts_score_validate(in, st, out, lg, lds);
    if (status != RTK_OK) return status;
    if (pr) {
        RTK_REQUIRE(pr->Q >= 1, "%s: a pair log of Q=%d pairs per stream", name, pr->Q);
        RTK_REQUIRE(pr->cursor && pr->frame_pair && pr->pair_key && pr->pair_common && pr->rec_size && pr->label_size, "%s: null pair log", name);
    }
    if (mm) RTK_REQUIRE(mm->table_ids && mm->table_count && mm->row_track && mm->labelled_coasted, "%s: null table or state", name);
    const ts_kernel_t kernel = ts_kernels[variant][mm ? 1 : 0];
    (void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RTK_SCORE_LDS_LIMIT);
    kernel<<<in->B, TS_THREADS, lds, (hipStream_t)stream>>>(*in, *st, *out, lg ? *lg : rtk_score_log_t{}, mm ? *mm : rtk_score_memory_t{},
                                                           pr ? *pr : rtk_score_pairs_t{}, sa);
    RTK_CHECK_LAUNCH(launched);
    return RTK_OK;
}

extern "C" int rtk_track_score(const rtk_track_score_in_t *in, const rtk_track_score_state_t *st, const rtk_track_score_out_t *out,
                               rtk_stream_t stream) {
    return ts_launch("track_score", "track_score", 0, in, st, out, nullptr, nullptr, nullptr, TS_PLAIN, ts_sim_args_t{}, stream);
}

extern "C" int rtk_track_score_logged(const rtk_track_score_in_t *in, const rtk_track_score_state_t *st, const rtk_track_score_out_t *out,
                                      const rtk_score_log_t *lg, rtk_stream_t stream) {
    RTK_REQUIRE(lg, "track_score_logged: null log block");
    return ts_launch("track_score", "track_score_logged", 0, in, st, out, lg, nullptr, nullptr, TS_PLAIN, ts_sim_args_t{}, stream);
}

extern "C" int rtk_track_score_memory(const rtk_track_score_in_t *in, const rtk_track_score_state_t *st, const rtk_track_score_out_t *out,
                                      const rtk_score_log_t *lg, const rtk_score_memory_t *mm, rtk_stream_t stream) {
    return ts_launch("track_score_memory", "track_score_memory", TS_NEED_MEMORY, in, st, out, lg, mm, nullptr, TS_PLAIN, ts_sim_args_t{},
                     stream);
}

extern "C" int rtk_track_score_pairs(const rtk_track_score_in_t *in, const rtk_track_score_state_t *st, const rtk_track_score_out_t *out,
                                     const rtk_score_log_t *lg, const rtk_score_memory_t *mm, const rtk_score_pairs_t *pr,
                                     rtk_stream_t stream) {
    return ts_launch("track_score_pairs", "track_score_pairs", TS_NEED_LOG | TS_NEED_PAIRS, in, st, out, lg, mm, pr, TS_PLAIN, ts_sim_args_t{},
                     stream);
}

extern "C" int rtk_track_score_pairs_centre(const rtk_track_score_in_t *in, const rtk_track_score_state_t *st, const rtk_track_score_out_t *out,
                                            const rtk_score_log_t *lg, const rtk_score_memory_t *mm, const rtk_score_pairs_t *pr,
                                            double *pair_sim, const double *gt_centre, double zero_distance, rtk_stream_t stream) {
    RTK_REQUIRE(pair_sim, "track_score_pairs_centre: null pair_sim (the similarity of every logged pair)");
    RTK_REQUIRE(gt_centre, "track_score_pairs_centre: null gt_centre (the kept objects' positions)");
    RTK_REQUIRE(zero_distance > 0.0 && zero_distance < INFINITY, "track_score_pairs_centre: zero_distance=%g must be finite and above 0", zero_distance);
    return ts_launch("track_score_pairs_centre", "track_score_pairs_centre", TS_NEED_LOG | TS_NEED_PAIRS, in, st, out, lg, mm, pr, TS_CENTRE,
                     ts_sim_args_t{pair_sim, gt_centre, zero_distance, nullptr, nullptr, nullptr, 0}, stream);
}

extern "C" int rtk_track_score_pairs_box(const rtk_track_score_in_t *in, const rtk_track_score_state_t *st, const rtk_track_score_out_t *out,
                                         const rtk_score_log_t *lg, const rtk_score_memory_t *mm, const rtk_score_pairs_t *pr, double *pair_sim,
                                         const double *det_box, const int *det_valid, const double *gt_boxes, int mode, rtk_stream_t stream) {
    RTK_REQUIRE(pair_sim, "track_score_pairs_box: null pair_sim (the similarity of every logged pair)");
    RTK_REQUIRE(det_box && det_valid, "track_score_pairs_box: null det_box or det_valid (the detections' boxes, rtk_object_boxes' output)");
    RTK_REQUIRE(gt_boxes, "track_score_pairs_box: null gt_boxes (the frame-1 box table)");
    RTK_REQUIRE(mode == RTK_SCORE_BOX_3D || mode == RTK_SCORE_BOX_BEV, "track_score_pairs_box: mode=%d is neither RTK_SCORE_BOX_3D nor RTK_SCORE_BOX_BEV",
                mode);
    return ts_launch("track_score_pairs_box", "track_score_pairs_box", TS_NEED_LOG | TS_NEED_PAIRS, in, st, out, lg, mm, pr, TS_BOX,
                     ts_sim_args_t{pair_sim, nullptr, 0.0, det_box, det_valid, gt_boxes, mode}, stream);
}
