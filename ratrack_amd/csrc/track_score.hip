// track_score.hip -- ground-truth objects and the tracking score of a batch on the device (include/rtk_score.h,
// ratrack_amd/track_score.py).
//
//   rtk_gt_objects    one workgroup per stream: the point set of every frame-1 box as an N-bit mask, the float64 centres, the serial
//                     rider merge and the minimum object size (vod_gt.filter_object_points' objs_combined; track4d_utils.py:105-176)
//   rtk_track_score   one workgroup per stream: vod_gt.map_gt_objects (track4d_utils.py:50-102), the 0/1 target of
//                     loss.affinity_loss against the stream's previous frame, and the running CLEAR-MOT counts with the per-stream
//                     table of ground-truth tracks; rtk_track_score_logged is the same launch that also appends the frame to the
//                     stream's log for the confidence sweep (track_sweep.hip)
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

#define TS_THREADS 256
#define TS_WAVES (TS_THREADS / RTK_WAVE)

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
// LDS: pts[N] float4 | best_iou[Kobj] f64 | gmask[N] u64 | plist[N] | qlist[N] | common[Kobj][K] | psize, best, cur_id, prev_id [Kobj] |
//      gsize, glabel, gslot, gpred, entry [K] | 8 scalars (all i32)
static size_t ts_score_lds(int Kobj, int K, int N) {
    return (size_t)N * sizeof(float4) + (size_t)Kobj * sizeof(double) + (size_t)N * sizeof(unsigned long long) +
           ((size_t)2 * N + (size_t)Kobj * K + (size_t)4 * Kobj + (size_t)5 * K + 8) * sizeof(int);
}

// The body of both scoring kernels.  LOG: the frame is also appended to the stream's log (rtk_score_log_t) -- thread i writes
// detection i's record where it finds its pre-greedy best object, thread j the j-th kept label id, thread 0 the frame's slot and the
// cursors; a frame that does not fit writes nothing and raises RTK_SCORE_FLAG_LOG.  Without LOG `lg` is not read.
template <bool LOG>
__device__ __forceinline__ void track_score_body(const rtk_track_score_in_t &in, const rtk_track_score_state_t &st,
                                                 const rtk_track_score_out_t &out, const rtk_score_log_t &lg) {
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
    // the stream's cursors, read by every thread before thread 0 moves them (after two barriers at least)
    int log_f = 0, log_r = 0, log_l = 0;
    bool log_fits = false;
    if (LOG) {
        log_f = lg.cursor[b * 4 + 0];
        log_r = lg.cursor[b * 4 + 1];
        log_l = lg.cursor[b * 4 + 2];
        log_fits = log_f >= 0 && log_f < lg.F && log_r >= 0 && log_r <= lg.R - P && log_l >= 0 && log_l <= lg.R - G;
    }

    if (t < 8) scal[t] = 0;
    for (int i = t; i < Kobj; i += TS_THREADS) {
        psize[i] = 0;
        prev_id[i] = (!reset && i < prevP) ? st.prev_gt_id[ob + i] : -1;
        cur_id[i] = -1;
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
        }
    }
    if (LOG && log_fits) {
        for (int j = t; j < G; j += TS_THREADS) lg.label[(size_t)b * lg.R + log_l + j] = glabel[j];
    }
    // ---- which table entry holds each kept object's label id ----
    for (int e = t; e < used; e += TS_THREADS) {
        const int key = st.table_key[tb + e];
        for (int j = 0; j < G; ++j)
            if (glabel[j] == key) entry[j] = e;      // label ids are distinct within a frame and within the table
    }
    __syncthreads();

    // ---- greedy assignment, table and counters: one thread, in order ----
    if (t == 0) {
        int M = 0, idsw = 0, flags = (nv != n ? RTK_SCORE_FLAG_NVALID : 0) | (rawp != P ? RTK_SCORE_FLAG_OBJECTS : 0);
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
            } else {
                flags |= RTK_SCORE_FLAG_LOG;
            }
        }
        if (flags) st.flags[b] |= flags;
        st.prev_count[b] = P;
        st.prev_gt[b] = G;
        out.aff_defined[b] = (prevP > 0 && prevG > 0 && P > 0 && G > 0) ? 1 : 0;
    }
    __syncthreads();

    // ---- outputs, and this frame as the next one's previous frame ----
    for (int i = t; i < Kobj; i += TS_THREADS) {
        const int j = i < P ? best[i] : -1;
        out.pred_gt_slot[ob + i] = j >= 0 ? gslot[j] : -1;
        out.pred_gt_id[ob + i] = j >= 0 ? glabel[j] : -1;
        out.iou[ob + i] = j >= 0 ? best_iou[i] : 0.0;
        st.prev_gt_id[ob + i] = cur_id[i];
    }
    for (int j = t; j < K; j += TS_THREADS) out.gt_pred[kb + j] = gpred[j];
    const int rows = prevP > 0 ? prevP : 0;
    for (int e = t; e < Kobj * Kobj; e += TS_THREADS) {
        const int i = e / Kobj, j = e - i * Kobj;
        target[e] = (i < rows && j < P && prev_id[i] >= 0 && prev_id[i] == cur_id[j]) ? 1.f : 0.f;
    }
}

__global__ __launch_bounds__(TS_THREADS) void track_score_kernel(const rtk_track_score_in_t in, const rtk_track_score_state_t st,
                                                                 const rtk_track_score_out_t out) {
    track_score_body<false>(in, st, out, rtk_score_log_t{});
}

// the logged variant: the same body (and the same LDS: the log goes straight to memory)
__global__ __launch_bounds__(TS_THREADS) void ts_logged_kernel(const rtk_track_score_in_t in, const rtk_track_score_state_t st,
                                                               const rtk_track_score_out_t out, const rtk_score_log_t lg) {
    track_score_body<true>(in, st, out, lg);
}

extern "C" int rtk_track_score_lds_bytes(int Kobj, int K, int N) {
    if (Kobj < 1 || K < 1 || N < 1 || Kobj > RTK_SCORE_MAX_OBJECTS || K > RTK_SCORE_MAX_BOXES || N > RTK_SCORE_MAX_POINTS) return -1;
    return (int)ts_score_lds(Kobj, K, N);
}

static int ts_score_launch(const rtk_track_score_in_t *in, const rtk_track_score_state_t *st, const rtk_track_score_out_t *out,
                           const rtk_score_log_t *lg, rtk_stream_t stream) {
    RTK_REQUIRE(in && st && out, "track_score: null argument block");
    RTK_REQUIRE(in->B >= 1 && in->B <= 65535 && in->N >= 1 && in->N <= RTK_SCORE_MAX_POINTS && in->T >= 1,
                "track_score: bad sizes B=%d N=%d T=%d", in->B, in->N, in->T);
    RTK_REQUIRE(in->Kobj >= 1 && in->Kobj <= RTK_SCORE_MAX_OBJECTS, "track_score: Kobj=%d object slots outside [1, %d]", in->Kobj,
                RTK_SCORE_MAX_OBJECTS);
    RTK_REQUIRE(in->K >= 1 && in->K <= RTK_SCORE_MAX_BOXES, "track_score: K=%d ground-truth slots outside [1, %d]", in->K, RTK_SCORE_MAX_BOXES);
    const size_t lds = ts_score_lds(in->Kobj, in->K, in->N);
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
