// track_results.hip -- the result log of the batched tracker (include/rtk_fused.h, "The result log"; ratrack_amd/result_log.py).
//
//   rtk_result_log_append   one workgroup per stream: the frame's records (track id, confidence, hits, size) and the xyz of its points
//                           grouped by object -- object after object, inside an object in increasing column -- appended behind the
//                           stream's device-side cursors
//   rtk_result_log_select   one workgroup per stream: the score and the length of every (clip, track id) and, from them, which
//                           records a result file keeps; the walk and the track table are score_log_walk.h's, the sums
//                           rtk_score_track_means' (track_sweep.hip), in the same order: the same bits
//
// The grouping is a counting sort that is stable at any N.  The N columns are cut into one contiguous segment per wave; every wave
// counts its segment's columns per object in LDS (integer atomics: the counts do not depend on their order); thread j turns object j's
// four counts into four starting offsets behind an exclusive scan over the objects; then every wave walks its segment in 64-column
// chunks, in order, and inside a chunk ranks the lanes of one object after the other: the first pending lane's object is broadcast,
// the lanes that hold it come from a 64-bit ballot, a lane's rank is the popcount of the mask below it, and the object's running
// offset moves on by the popcount of the whole mask.  A chunk costs as many rounds as it has distinct objects, never N.
// Every word of the log has one writer and plain stores.
#include <math.h>

#include "score_log_walk.h"

#define RL_THREADS 256
#define RL_WAVES (RL_THREADS / RTK_WAVE)
static_assert(RTK_RESULT_MAX_OBJECTS == RTK_SCORE_MAX_OBJECTS, "the frame word is the scorer's: lw_frame clamps P to RTK_SCORE_MAX_OBJECTS");
static_assert(RTK_RESULT_MAX_OBJECTS <= RL_THREADS, "thread j scans object j");

// ------------------------------------------------------------------------------------------------
// rtk_result_log_append
// ------------------------------------------------------------------------------------------------
struct rl_step_t {
    int N, K;
    rtk_bcn_view_t pc1;
    const int *obj, *num_objects, *object_ids;
    const float *object_conf;
    const int *object_hits, *step_flags, *seq, *index;
    const unsigned char *reset, *active;
};

__global__ __launch_bounds__(RL_THREADS) void result_append_kernel(const rl_step_t in, const rtk_result_log_t lg) {
    __shared__ int wcnt[RL_WAVES * RTK_RESULT_MAX_OBJECTS];      // [wave][object]: the segment's count, then its running offset
    __shared__ int wsum[RL_WAVES];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & (RTK_WAVE - 1), wave = t / RTK_WAVE;
    if (in.active && !in.active[b]) return;
    const int Pf = in.num_objects[b], sf = in.step_flags ? in.step_flags[b] : 0;
    int bad = 0;
    if (Pf < 0 || Pf > in.K) bad |= RTK_RESULT_FLAG_OBJECTS;
    if (sf & 3) bad |= RTK_RESULT_FLAG_STEP;
    if (bad) {
        if (t == 0) lg.flags[b] |= bad;
        return;
    }
    const int cf = lg.cursor[b * 4 + 0], cr = lg.cursor[b * 4 + 1], cp = lg.cursor[b * 4 + 2];

    // ---- the counts of every wave's segment ----
    for (int i = t; i < RL_WAVES * RTK_RESULT_MAX_OBJECTS; i += RL_THREADS) wcnt[i] = 0;
    __syncthreads();
    const int N = in.N, S = ((N + RL_THREADS - 1) / RL_THREADS) * RTK_WAVE;      // columns per wave, whole chunks
    const int p0 = wave * S < N ? wave * S : N, p1 = N - p0 < S ? N : p0 + S;
    const int *ob = in.obj + (size_t)b * N;
    for (int p = p0 + lane; p < p1; p += RTK_WAVE) {
        const int o = ob[p];
        if (o >= 0 && o < Pf) atomicAdd(&wcnt[wave * RTK_RESULT_MAX_OBJECTS + o], 1);
    }
    __syncthreads();

    // ---- thread j: object j's size, its first point (an exclusive scan over the objects) and its four segments' offsets ----
    int c[RL_WAVES], size = 0;
#pragma unroll
    for (int w = 0; w < RL_WAVES; ++w) { c[w] = wcnt[w * RTK_RESULT_MAX_OBJECTS + t]; size += c[w]; }
    const int incl = wave_inclusive_scan(size, lane);
    if (lane == RTK_WAVE - 1) wsum[wave] = incl;
    __syncthreads();
    int first = incl - size, total = 0;
#pragma unroll
    for (int w = 0; w < RL_WAVES; ++w) {
        if (w < wave) first += wsum[w];
        total += wsum[w];
    }
    const bool fits = cf >= 0 && cr >= 0 && cp >= 0 && cf < lg.F && cr <= lg.R - Pf && cp <= lg.P - total;
    if (!fits) {
        if (t == 0) lg.flags[b] |= RTK_RESULT_FLAG_FULL;
        return;
    }
#pragma unroll
    for (int w = 0, o = first; w < RL_WAVES; ++w) { wcnt[w * RTK_RESULT_MAX_OBJECTS + t] = o; o += c[w]; }
    if (t < Pf) {
        const size_t r = (size_t)b * lg.R + cr + t, k = (size_t)b * in.K + t;
        lg.rec_track[r] = in.object_ids[k];
        lg.rec_conf[r] = in.object_conf[k];
        lg.rec_hits[r] = in.object_hits ? in.object_hits[k] : 0;
        lg.rec_size[r] = size;
    }
    __syncthreads();

    // ---- the points: every wave its segment, chunk after chunk ----
    volatile int *woff = wcnt + wave * RTK_RESULT_MAX_OBJECTS;
    float *pts = lg.points + ((size_t)b * lg.P + cp) * 3;
    for (int q0 = p0; q0 < p1; q0 += RTK_WAVE) {
        const int p = q0 + lane;
        int o = -1;
        if (p < p1) {
            o = ob[p];
            if (o < 0 || o >= Pf) o = -1;
        }
        bool pending = o >= 0;
        int dest = -1;
        for (;;) {
            const unsigned long long rem = __ballot(pending);
            if (rem == 0ull) break;
            const int leader = __ffsll(rem) - 1;
            const int lead = __shfl(o, leader);
            const bool mine = pending && o == lead;
            const unsigned long long mask = __ballot(mine);
            const int at = woff[lead];
            if (mine) {
                dest = at + __popcll(mask & ((1ull << lane) - 1ull));
                pending = false;
            }
            __builtin_amdgcn_wave_barrier();
            if (lane == leader) woff[lead] = at + __popcll(mask);
            __builtin_amdgcn_wave_barrier();
        }
        if (dest >= 0) {
            float *d = pts + (size_t)dest * 3;
            d[0] = bcn_at(in.pc1, b, 0, p);
            d[1] = bcn_at(in.pc1, b, 1, p);
            d[2] = bcn_at(in.pc1, b, 2, p);
        }
    }

    // ---- the frame's two words and the cursors (every thread read the cursors before the barriers above) ----
    if (t == 0) {
        int *fw = lg.frame + ((size_t)b * lg.F + cf) * 4, *tw = lg.tag + ((size_t)b * lg.F + cf) * 4;
        fw[0] = cr; fw[1] = cp; fw[2] = Pf + ((in.reset && in.reset[b]) ? 65536 : 0); fw[3] = 0;
        tw[0] = in.seq[b]; tw[1] = in.index[b]; tw[2] = total; tw[3] = sf;
        lg.cursor[b * 4 + 0] = cf + 1; lg.cursor[b * 4 + 1] = cr + Pf; lg.cursor[b * 4 + 2] = cp + total;
    }
}

// ------------------------------------------------------------------------------------------------
// rtk_result_log_select
// ------------------------------------------------------------------------------------------------
// LDS: sum[H] f64 | key[H], cnt[H] i32 | slot[MAX_OBJECTS] i32 | 2 scalars.  H = LW_SLOTS (48 KB): sweep_means_kernel's tables.
__global__ __launch_bounds__(RL_THREADS) void result_select_kernel(const rtk_result_log_t rl, const double *threshold, double threshold_value,
                                                                   int min_hits, int min_track_frames, unsigned char *keep,
                                                                   double *track_score, int *track_frames, int *flags) {
    __shared__ double sum[LW_SLOTS];
    __shared__ int key[LW_SLOTS], cnt[LW_SLOTS], slot[RTK_SCORE_MAX_OBJECTS], scal[2];      // scal: 0 ids in the table | 1 overflow
    const int b = blockIdx.x, t = threadIdx.x;
    rtk_score_log_t lg = {};      // the part of the scorer's log block the walk reads: the frame words are the scorer's
    lg.F = rl.F; lg.R = rl.R; lg.cursor = rl.cursor; lg.frame = rl.frame; lg.rec_track = rl.rec_track; lg.rec_conf = rl.rec_conf;
    const double tau = threshold ? *threshold : threshold_value;
    const int frames = lw_frames(lg, b);
    const size_t rb = (size_t)b * lg.R;
    for (int h = t; h < LW_SLOTS; h += RL_THREADS) { key[h] = LW_EMPTY; cnt[h] = 0; sum[h] = 0.0; }
    if (t < 2) scal[t] = 0;
    __syncthreads();
    int clip_rec = 0, end_rec = 0;      // the open clip's first record, and one past the last record walked
    for (int f = 0; f <= frames; ++f) {
        lw_frame_t fr = {};
        if (f < frames) fr = lw_frame(lg, b, f);
        if (f == frames || (fr.reset && f > 0)) {
            // ---- the clip closes (second pass): every record of it receives its track's score, length and decision ----
            if (!scal[1]) {
                for (int r = clip_rec + t; r < end_rec; r += RL_THREADS) {
                    const int s = lw_track_slot<false>(key, scal, lg.rec_track[rb + r]);
                    if (s < 0) continue;
                    const int n = cnt[s];
                    const double score = sum[s] / (double)n;
                    track_score[rb + r] = score;
                    track_frames[rb + r] = n;
                    // (min_hits 1 asks nothing: a frame logged without hit counts holds 0, and write_results filters from 2 on)
                    keep[rb + r] = (lw_stays(score, tau) && (min_hits <= 1 || rl.rec_hits[rb + r] >= min_hits) && n >= min_track_frames) ? 1 : 0;
                }
            }
            __syncthreads();
            for (int h = t; h < LW_SLOTS; h += RL_THREADS) { key[h] = LW_EMPTY; cnt[h] = 0; sum[h] = 0.0; }
            if (t == 0) scal[0] = 0;
            __syncthreads();
            clip_rec = end_rec;
            if (f == frames) break;
        }
        // ---- the frame's records (first pass): the lanes find the slots, thread 0 adds in record order ----
        for (int i = t; i < fr.P; i += RL_THREADS) {
            const int s = lw_track_slot<true>(key, scal, lg.rec_track[rb + fr.rec + i]);
            slot[i] = s;
            if (s < 0) scal[1] = 1;
        }
        __syncthreads();
        if (t == 0) {
            for (int i = 0; i < fr.P; ++i) {
                const int s = slot[i];
                if (s < 0) continue;
                sum[s] += (double)lg.rec_conf[rb + fr.rec + i];
                cnt[s] += 1;
            }
        }
        __syncthreads();
        end_rec = fr.rec + fr.P;
    }
    if (t == 0) flags[b] = scal[1] ? RTK_RESULT_FLAG_TRACKS : 0;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static bool rl_log_ok(const rtk_result_log_t *lg) {
    return lg && lg->F >= 1 && lg->R >= 1 && lg->P >= 1 && lg->cursor && lg->frame && lg->tag && lg->rec_track && lg->rec_conf && lg->rec_hits &&
           lg->rec_size && lg->points && lg->flags;
}

static bool rl_log_small(int B, const rtk_result_log_t *lg) {
    const long long lim = 1ll << 31, b = B;
    return b * 4 * lg->F < lim && b * lg->R < lim && b * 3 * lg->P < lim;
}

extern "C" int rtk_result_log_append(int B, int N, int K, const rtk_bcn_view_t *pc1, const int *obj, const int *num_objects,
                                     const int *object_ids, const float *object_conf, const int *object_hits, const int *step_flags,
                                     const int *seq, const int *index, const unsigned char *reset, const unsigned char *active,
                                     const rtk_result_log_t *lg, rtk_stream_t stream) {
    RTK_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && K >= 1 && K <= RTK_RESULT_MAX_OBJECTS, "result_log_append: bad sizes B=%d N=%d K=%d (K <= %d)", B,
                N, K, RTK_RESULT_MAX_OBJECTS);
    RTK_REQUIRE((long long)B * N < (1ll << 31) - RL_THREADS, "result_log_append: B=%d streams of N=%d columns: 2^31 or more", B, N);
    RTK_REQUIRE(pc1 && pc1->ptr && obj && num_objects && object_ids && object_conf && seq && index, "result_log_append: null argument");
    RTK_REQUIRE(rl_log_ok(lg), "result_log_append: null or empty log");
    RTK_REQUIRE(rl_log_small(B, lg), "result_log_append: a log of B=%d x (F=%d, R=%d, P=%d): a table of 2^31 words or more", B, lg->F, lg->R, lg->P);
    rl_step_t in;
    in.N = N; in.K = K; in.pc1 = *pc1; in.obj = obj; in.num_objects = num_objects; in.object_ids = object_ids; in.object_conf = object_conf;
    in.object_hits = object_hits; in.step_flags = step_flags; in.seq = seq; in.index = index; in.reset = reset; in.active = active;
    result_append_kernel<<<B, RL_THREADS, 0, (hipStream_t)stream>>>(in, *lg);
    RTK_CHECK_LAUNCH("result_log_append");
    return RTK_OK;
}

extern "C" int rtk_result_log_select(int B, const rtk_result_log_t *lg, const double *threshold, double threshold_value, int min_hits,
                                     int min_track_frames, unsigned char *keep, double *track_score, int *track_frames, int *flags,
                                     rtk_stream_t stream) {
    RTK_REQUIRE(B >= 1 && B <= 65535, "result_log_select: B=%d streams", B);
    RTK_REQUIRE(rl_log_ok(lg), "result_log_select: null or empty log");
    RTK_REQUIRE(rl_log_small(B, lg), "result_log_select: a log of B=%d x (F=%d, R=%d, P=%d): a table of 2^31 words or more", B, lg->F, lg->R, lg->P);
    RTK_REQUIRE(threshold || !isnan(threshold_value), "result_log_select: the threshold is not a number");
    RTK_REQUIRE(keep && track_score && track_frames && flags, "result_log_select: null output");
    result_select_kernel<<<B, RL_THREADS, 0, (hipStream_t)stream>>>(*lg, threshold, threshold_value, min_hits, min_track_frames, keep, track_score,
                                                                    track_frames, flags);
    RTK_CHECK_LAUNCH("result_log_select");
    return RTK_OK;
}
