// track_sweep.hip -- the confidence sweep over the scorer's per-frame log: sAMOTA / AMOTA / AMOTP (include/rtk_score.h, the
// definitions are stated there; ratrack_amd/track_score.py, TrackScorer.sweep).
//
//   rtk_score_track_means   one workgroup per stream: the score of every (clip, track id) -- the float64 sum of the fp32 confidences
//                           of its logged detections in log order over their number -- written to each of its records
//   rtk_score_thresholds    one thread: the KITTI walk over the descending-sorted true-positive scores (a bisection per level)
//   rtk_score_replay        one wave per (stream, threshold): the stream's log walked frame by frame with the detections below the
//                           threshold removed, rtk_track_score's greedy rule, counters and track table
//
// The log holds a few detections per frame, so all three are latency bound and kept simple: whatever has an order (the sums, the
// greedy pass, the table) is one thread in that order; the lanes only fetch, probe and look up.  Integer sums and fixed-order float64
// sums only: the same bits on every run, and the bits of a host loop written from the definitions.  The frame decode and the track
// table are score_log_walk.h's.
#include <math.h>

#include "score_log_walk.h"

#define SW_THREADS 256

// ------------------------------------------------------------------------------------------------
// rtk_score_track_means
// ------------------------------------------------------------------------------------------------
// LDS: sum[H] f64 | key[H], cnt[H] i32 | slot[MAX_OBJECTS] i32 | 2 scalars.  H = LW_SLOTS (48 KB), the track table of score_log_walk.h.
#define SW_SLOTS LW_SLOTS

__global__ __launch_bounds__(SW_THREADS) void sweep_means_kernel(const rtk_score_log_t lg, double *rec_score, int *flags) {
    __shared__ double sum[SW_SLOTS];
    __shared__ int key[SW_SLOTS], cnt[SW_SLOTS], slot[RTK_SCORE_MAX_OBJECTS], scal[2];      // scal: 0 ids in the table | 1 overflow
    const int b = blockIdx.x, t = threadIdx.x;
    const int frames = lw_frames(lg, b);
    const size_t rb = (size_t)b * lg.R;
    for (int h = t; h < SW_SLOTS; h += SW_THREADS) { key[h] = LW_EMPTY; cnt[h] = 0; sum[h] = 0.0; }
    if (t < 2) scal[t] = 0;
    __syncthreads();
    int clip_rec = 0, end_rec = 0;      // the open clip's first record, and one past the last record walked
    for (int f = 0; f <= frames; ++f) {
        lw_frame_t fr = {};
        if (f < frames) fr = lw_frame(lg, b, f);
        if (f == frames || fr.reset) {
            // ---- the clip closes: every record of it receives its track's score, the table empties ----
            for (int r = clip_rec + t; r < end_rec; r += SW_THREADS) {
                const int s = lw_track_slot<false>(key, scal, lg.rec_track[rb + r]);
                if (s >= 0) rec_score[rb + r] = sum[s] / (double)cnt[s];
            }
            __syncthreads();
            for (int h = t; h < SW_SLOTS; h += SW_THREADS) { key[h] = LW_EMPTY; cnt[h] = 0; sum[h] = 0.0; }
            if (t == 0) scal[0] = 0;
            __syncthreads();
            clip_rec = end_rec;
            if (f == frames) break;
        }
        // ---- the frame's detections: the lanes find the slots, thread 0 adds in detection order ----
        for (int i = t; i < fr.P; i += SW_THREADS) {
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
    if (t == 0 && scal[1]) flags[b] |= RTK_SCORE_FLAG_SWEEP;
}

// ------------------------------------------------------------------------------------------------
// rtk_score_thresholds
// ------------------------------------------------------------------------------------------------
__global__ void sweep_thresholds_kernel(const double *sorted, const long long *n_ptr, const long long *gt_ptr, int levels,
                                        double *thresholds, int *reached) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const long long n = *n_ptr;
    const double G = (double)*gt_ptr, step = 1.0 / (double)levels;
    double cur = 0.0;
    int found = 0;      // thresholds so far, the dropped first one included
    thresholds[0] = -INFINITY;
    // The walk visits every i, but `cur` only moves at an append, and between two appends "i is skipped" is monotone in i: l and r
    // are correctly rounded quotients of growing numerators, so (r - cur) never falls and (cur - l) never grows -- once an i is not
    // skipped none after it is.  The next append is therefore found by bisection, with the serial walk's own comparisons.
    for (long long i = 0; i < n && found <= levels; ++i) {
        long long lo = i, hi = n - 1;      // the last i is never skipped
        while (lo < hi) {
            const long long mid = lo + (hi - lo) / 2;      // mid < n - 1
            const double l = (double)(mid + 1) / G, r = (double)(mid + 2) / G;
            if ((r - cur) < (cur - l)) lo = mid + 1; else hi = mid;
        }
        i = lo;
        if (found > 0) thresholds[found] = sorted[i];
        ++found;
        cur += step;
    }
    const int k = found > 0 ? found - 1 : 0;
    for (int e = k + 1; e <= levels; ++e) thresholds[e] = INFINITY;
    *reached = k;
}

// ------------------------------------------------------------------------------------------------
// rtk_score_replay
// ------------------------------------------------------------------------------------------------
// One wave.  LDS: riou[MAX_OBJECTS] f64 | table key, last, seen, matched [T] | rj, rtrack [MAX_OBJECTS] | glabel, gpred, entry
// [MAX_BOXES] | 3 scalars (mt, pt, ml of a closing clip)
static size_t sw_replay_lds(int T) {
    return (size_t)RTK_SCORE_MAX_OBJECTS * sizeof(double) + ((size_t)4 * T + 2 * RTK_SCORE_MAX_OBJECTS + 3 * RTK_SCORE_MAX_BOXES + 4) * sizeof(int);
}

__global__ __launch_bounds__(RTK_WAVE) void sweep_replay_kernel(int T, const rtk_score_log_t lg, const double *rec_score,
                                                                const double *thresholds, const int *reached, long long *counters,
                                                                double *iou_sums, unsigned char *tp_mask) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sw_smem[];
    const int b = blockIdx.x, x = blockIdx.y, B = gridDim.x, t = threadIdx.x;
    double *riou = reinterpret_cast<double *>(sw_smem);
    int *tkey = reinterpret_cast<int *>(riou + RTK_SCORE_MAX_OBJECTS), *tlast = tkey + T, *tseen = tlast + T, *tmatched = tseen + T;
    int *rj = tmatched + T, *rtrack = rj + RTK_SCORE_MAX_OBJECTS;
    int *glabel = rtrack + RTK_SCORE_MAX_OBJECTS, *gpred = glabel + RTK_SCORE_MAX_BOXES, *entry = gpred + RTK_SCORE_MAX_BOXES;
    int *scal = entry + RTK_SCORE_MAX_BOXES;
    long long *cnt = counters + ((size_t)x * B + b) * RTK_SCORE_COUNTERS;
    const bool mask = tp_mask != nullptr && x == 0;
    const size_t rb = (size_t)b * lg.R;

    if (reached && x > *reached) {      // a level the walk never reached
        if (t < RTK_SCORE_COUNTERS) cnt[t] = 0;
        if (t == 0) iou_sums[(size_t)x * B + b] = 0.0;
        return;
    }
    const double tau = thresholds[x];
    const int frames = lw_frames(lg, b);
    // thread 0's running values
    long long c_frames = 0, c_gt = 0, c_pred = 0, c_tp = 0, c_idsw = 0, c_tracks = 0, c_mt = 0, c_pt = 0, c_ml = 0;
    double iou_sum = 0.0;
    int used = 0;      // uniform: thread 0 publishes it through scal[3]
    if (t < 4) scal[t] = 0;
    __syncthreads();

    for (int f = 0; f <= frames; ++f) {
        lw_frame_t fr = {};
        if (f < frames) fr = lw_frame(lg, b, f);
        if (f == frames || fr.reset) {
            // ---- the clip closes ----
            int mt = 0, pt = 0, ml = 0;
            for (int e = t; e < used; e += RTK_WAVE) {
                const double r = (double)tmatched[e] / (double)tseen[e];
                if (r > 0.8) ++mt; else if (r < 0.2) ++ml; else ++pt;
            }
            if (mt) atomicAdd(&scal[0], mt);
            if (pt) atomicAdd(&scal[1], pt);
            if (ml) atomicAdd(&scal[2], ml);
            __syncthreads();
            if (t == 0) {
                c_tracks += used; c_mt += scal[0]; c_pt += scal[1]; c_ml += scal[2];
                scal[0] = scal[1] = scal[2] = scal[3] = 0;
            }
            used = 0;
            __syncthreads();
            if (f == frames) break;
        }
        // ---- the frame's tables: kept labels with their table entries, the remaining detections with their best object ----
        for (int j = t; j < fr.G; j += RTK_WAVE) {
            const int lab = lg.label[rb + fr.lab + j];
            glabel[j] = lab;
            gpred[j] = -1;
            int e = -1;
            for (int k = 0; k < used; ++k)
                if (tkey[k] == lab) e = k;      // label ids are distinct within the table
            entry[j] = e;
        }
        __syncthreads();
        for (int i = t; i < fr.P; i += RTK_WAVE) {
            const size_t r = rb + fr.rec + i;
            const int lab = lg.rec_best[r];
            const bool stays = lw_stays(rec_score[r], tau);
            int j = -1;
            if (stays && lab != -1) {
                for (int k = fr.G - 1; k >= 0; --k)
                    if (glabel[k] == lab) j = k;
            }
            rj[i] = stays ? j : -2;      // -2: removed, -1: remains without a best object
            rtrack[i] = lg.rec_track[r];
            riou[i] = lg.rec_iou[r];
        }
        __syncthreads();
        // ---- greedy assignment, table and counters: one thread, in order (rtk_track_score's serial part) ----
        if (t == 0) {
            int M = 0, pred = 0, idsw = 0;
            for (int i = 0; i < fr.P; ++i) {
                const int j = rj[i];
                if (j == -2) continue;
                ++pred;
                if (j < 0 || gpred[j] >= 0) continue;      // taken by a remaining detection: no second choice
                gpred[j] = i;
                iou_sum += riou[i];
                ++M;
            }
            for (int j = 0; j < fr.G; ++j) {
                int e = entry[j];
                if (e < 0) {
                    if (used >= T) continue;      // the scorer raised RTK_SCORE_FLAG_TRACKS on this frame
                    e = used++;
                    tkey[e] = glabel[j]; tlast[e] = -1; tseen[e] = 0; tmatched[e] = 0;
                }
                tseen[e] += 1;
                if (gpred[j] >= 0) {
                    const int track = rtrack[gpred[j]], last = tlast[e];
                    if (last != -1 && last != track) ++idsw;
                    tlast[e] = track;
                    tmatched[e] += 1;
                }
            }
            scal[3] = used;
            c_frames += 1; c_gt += fr.G; c_pred += pred; c_tp += M; c_idsw += idsw;
        }
        __syncthreads();
        used = scal[3];
        if (mask) {
            for (int i = t; i < fr.P; i += RTK_WAVE) {
                const int j = rj[i];
                tp_mask[rb + fr.rec + i] = (j >= 0 && gpred[j] == i) ? 1 : 0;
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        cnt[0] = c_frames; cnt[1] = c_gt; cnt[2] = c_pred; cnt[3] = c_tp; cnt[4] = c_pred - c_tp; cnt[5] = c_gt - c_tp; cnt[6] = c_idsw;
        cnt[7] = c_tracks; cnt[8] = c_mt; cnt[9] = c_pt; cnt[10] = c_ml;
        iou_sums[(size_t)x * B + b] = iou_sum;
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
extern "C" int rtk_score_track_means(int B, const rtk_score_log_t *lg, double *rec_score, int *flags, rtk_stream_t stream) {
    RTK_REQUIRE(B >= 1 && B <= 65535, "score_track_means: B=%d streams", B);
    RTK_REQUIRE(lw_log_ok(lg), "score_track_means: null or empty log");
    RTK_REQUIRE(rec_score && flags, "score_track_means: null output");
    sweep_means_kernel<<<B, SW_THREADS, 0, (hipStream_t)stream>>>(*lg, rec_score, flags);
    RTK_CHECK_LAUNCH("score_track_means");
    return RTK_OK;
}

extern "C" int rtk_score_thresholds(const double *sorted, const long long *n, const long long *gt, int levels, double *thresholds,
                                    int *reached, rtk_stream_t stream) {
    RTK_REQUIRE(levels >= 1 && levels <= 65534, "score_thresholds: levels=%d recall levels", levels);
    RTK_REQUIRE(sorted && n && gt && thresholds && reached, "score_thresholds: null argument");
    sweep_thresholds_kernel<<<1, RTK_WAVE, 0, (hipStream_t)stream>>>(sorted, n, gt, levels, thresholds, reached);
    RTK_CHECK_LAUNCH("score_thresholds");
    return RTK_OK;
}

extern "C" int rtk_score_replay(int B, int T, const rtk_score_log_t *lg, const double *rec_score, const double *thresholds,
                                const int *reached, int count, long long *counters, double *iou_sum, unsigned char *tp_mask,
                                rtk_stream_t stream) {
    RTK_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && count >= 1 && count <= 65535, "score_replay: bad sizes B=%d T=%d count=%d", B, T, count);
    const size_t lds = sw_replay_lds(T);
    RTK_REQUIRE(lds <= RTK_SCORE_LDS_LIMIT, "score_replay: T=%d track-table entries need %zu bytes of LDS per stream, the limit is %d", T, lds,
                RTK_SCORE_LDS_LIMIT);
    RTK_REQUIRE(lw_log_ok(lg), "score_replay: null or empty log");
    RTK_REQUIRE(rec_score && thresholds && counters && iou_sum, "score_replay: null argument");
    (void)hipFuncSetAttribute((const void *)sweep_replay_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RTK_SCORE_LDS_LIMIT);
    sweep_replay_kernel<<<dim3(B, count), RTK_WAVE, lds, (hipStream_t)stream>>>(T, *lg, rec_score, thresholds, reached, counters, iou_sum,
                                                                                tp_mask);
    RTK_CHECK_LAUNCH("score_replay");
    return RTK_OK;
}
