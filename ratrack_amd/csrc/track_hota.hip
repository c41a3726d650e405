// track_hota.hip -- HOTA (DetA, AssA, LocA) over the scorer's per-frame log (include/rtk_score.h, the definitions are stated there;
// ratrack_amd/track_score.py, TrackScorer.hota).
//
//   rtk_score_hota   one wave per (stream, alpha): the stream's log walked frame by frame as rtk_score_replay walks it, with the
//                    detections below the threshold removed and the pairs below alpha zeroed BEFORE the greedy rule; per clip a
//                    label table (frames seen), a track table (remaining detections) and the list of matched (label, track) pairs
//                    in order of first appearance, folded into the association sums when the clip closes
//
// As in track_sweep.hip the log holds a few detections per frame and the kernel is latency bound and kept simple: whatever has an
// order (the greedy pass, the pair insertions, the four sums) is one thread in that order; the lanes fetch, probe, look up and compute
// the quotients.  Integers and fixed-order float64 sums only: the same bits on every run, and the bits of a host loop written from
// the definitions.  The frame decode, the track table and the pair list are score_log_walk.h's.
#include <math.h>

#include "score_log_walk.h"

#define HT_SLOTS LW_SLOTS                                                   // the track table
#define HT_PSLOTS (2 * RTK_SCORE_HOTA_PAIRS)                                // the pair lookup: half stays empty
#define HT_SLOT_BITS 12                                                     // a pair's key: label entry << 12 | track slot
static_assert(HT_SLOTS <= (1 << HT_SLOT_BITS), "a track slot must fit the pair key");

// LDS: riou[MAX_OBJECTS], quot[3][WAVE] f64 | label table key, cg [T] | track table key, ct [HT_SLOTS] | pair list key, n [PAIRS] |
// pair lookup [2 PAIRS] | rj, rslot [MAX_OBJECTS] | glabel, gpred, entry, gpair [MAX_BOXES] | 8 scalars
static size_t ht_lds(int T) {
    return ((size_t)RTK_SCORE_MAX_OBJECTS + 3 * RTK_WAVE) * sizeof(double) +
           ((size_t)2 * T + 2 * HT_SLOTS + 2 * RTK_SCORE_HOTA_PAIRS + HT_PSLOTS + 2 * RTK_SCORE_MAX_OBJECTS + 4 * RTK_SCORE_MAX_BOXES + 8) * sizeof(int);
}

enum { HT_S_LABELS = 0, HT_S_TRACKS = 1, HT_S_PAIRS = 2, HT_S_OVERFLOW = 3 };

__global__ __launch_bounds__(RTK_WAVE) void hota_kernel(int T, const rtk_score_log_t lg, const double *rec_score, const double *threshold,
                                                        long long *counters, double *sums, int *flags) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ht_smem[];
    const int b = blockIdx.x, a = blockIdx.y, B = gridDim.x, A = gridDim.y, t = threadIdx.x;
    double *riou = reinterpret_cast<double *>(ht_smem), *quot = riou + RTK_SCORE_MAX_OBJECTS;
    int *lkey = reinterpret_cast<int *>(quot + 3 * RTK_WAVE), *lcg = lkey + T;
    int *tkey = lcg + T, *tct = tkey + HT_SLOTS;
    int *pkey = tct + HT_SLOTS, *pn = pkey + RTK_SCORE_HOTA_PAIRS, *ptab = pn + RTK_SCORE_HOTA_PAIRS;
    int *rj = ptab + HT_PSLOTS, *rslot = rj + RTK_SCORE_MAX_OBJECTS;
    int *glabel = rslot + RTK_SCORE_MAX_OBJECTS, *gpred = glabel + RTK_SCORE_MAX_BOXES, *entry = gpred + RTK_SCORE_MAX_BOXES;
    int *gpair = entry + RTK_SCORE_MAX_BOXES, *scal = gpair + RTK_SCORE_MAX_BOXES;

    const double alpha = (double)(a + 1) / (double)(A + 1);
    const bool filter = rec_score != nullptr && threshold != nullptr;
    const double tau = filter ? *threshold : 0.0;
    const int frames = lw_frames(lg, b);
    const size_t rb = (size_t)b * lg.R;
    // thread 0's running values
    long long c_frames = 0, c_clips = 0, c_gt = 0, c_pred = 0, c_tp = 0, c_pairs = 0;
    double s_ass = 0.0, s_re = 0.0, s_pr = 0.0, s_loc = 0.0;
    int used = 0, npairs = 0;      // uniform: thread 0 publishes them through scal

    for (int h = t; h < HT_SLOTS; h += RTK_WAVE) { tkey[h] = LW_EMPTY; tct[h] = 0; }
    for (int h = t; h < HT_PSLOTS; h += RTK_WAVE) ptab[h] = -1;
    if (t < 8) scal[t] = 0;
    __syncthreads();

    for (int f = 0; f <= frames; ++f) {
        lw_frame_t fr = {};
        if (f < frames) fr = lw_frame(lg, b, f);
        if ((f == frames || fr.reset) && f > 0) {
            // ---- the clip closes: the lanes compute a wave's width of quotients, thread 0 adds them in the pairs' order ----
            for (int base = 0; base < npairs; base += RTK_WAVE) {
                const int p = base + t;
                if (p < npairs) {
                    const int key = pkey[p], n = pn[p];
                    const int cg = lcg[key >> HT_SLOT_BITS], ct = tct[key & ((1 << HT_SLOT_BITS) - 1)];
                    const double N = (double)((long long)n * (long long)n);
                    quot[t] = N / (double)(cg + ct - n);
                    quot[RTK_WAVE + t] = N / (double)cg;
                    quot[2 * RTK_WAVE + t] = N / (double)ct;
                }
                __syncthreads();
                if (t == 0) {
                    const int m = min(npairs - base, RTK_WAVE);
                    for (int k = 0; k < m; ++k) {
                        s_ass += quot[k];
                        s_re += quot[RTK_WAVE + k];
                        s_pr += quot[2 * RTK_WAVE + k];
                    }
                }
                __syncthreads();
            }
            for (int h = t; h < HT_SLOTS; h += RTK_WAVE) { tkey[h] = LW_EMPTY; tct[h] = 0; }
            for (int h = t; h < HT_PSLOTS; h += RTK_WAVE) ptab[h] = -1;
            if (t == 0) {
                c_clips += 1; c_pairs += npairs;
                scal[HT_S_LABELS] = scal[HT_S_TRACKS] = scal[HT_S_PAIRS] = 0;
            }
            used = 0; npairs = 0;
            __syncthreads();
        }
        if (f == frames) break;
        // ---- the frame's tables: kept labels with their table entries; the remaining detections with their track slot (and its
        //      count) and, if they are candidates at this alpha, their best object ----
        for (int j = t; j < fr.G; j += RTK_WAVE) {
            const int lab = lg.label[rb + fr.lab + j];
            glabel[j] = lab;
            gpred[j] = -1;
            gpair[j] = -1;
            int e = -1;
            for (int k = 0; k < used; ++k)
                if (lkey[k] == lab) e = k;      // label ids are distinct within the table
            entry[j] = e;
        }
        __syncthreads();
        for (int i = t; i < fr.P; i += RTK_WAVE) {
            const size_t r = rb + fr.rec + i;
            const bool stays = !filter || lw_stays(rec_score[r], tau);
            const int lab = lg.rec_best[r];
            const double iou = lg.rec_iou[r];
            int j = -1, s = -1;
            if (stays) {
                s = lw_track_slot<true>(tkey, &scal[HT_S_TRACKS], lg.rec_track[r]);
                if (s >= 0) atomicAdd(&tct[s], 1); else scal[HT_S_OVERFLOW] = 1;
                if (lab != -1 && iou >= alpha) {
                    for (int k = fr.G - 1; k >= 0; --k)
                        if (glabel[k] == lab) j = k;
                }
            }
            rj[i] = stays ? j : -2;      // -2: removed, -1: remains and is no candidate
            rslot[i] = s;
            riou[i] = iou;
        }
        __syncthreads();
        // ---- the greedy rule and the label table: one thread, in order ----
        if (t == 0) {
            int M = 0, pred = 0;
            for (int i = 0; i < fr.P; ++i) {
                const int j = rj[i];
                if (j == -2) continue;
                ++pred;
                if (j < 0 || gpred[j] >= 0) continue;      // taken by an earlier candidate: no second choice
                gpred[j] = i;
                s_loc += riou[i];
                ++M;
            }
            for (int j = 0; j < fr.G; ++j) {
                int e = entry[j];
                if (e < 0) {
                    if (used >= T) { scal[HT_S_OVERFLOW] = 1; continue; }
                    e = used++;
                    lkey[e] = glabel[j]; lcg[e] = 0;
                    entry[j] = e;
                }
                lcg[e] += 1;
            }
            scal[HT_S_LABELS] = used;
            c_frames += 1; c_gt += fr.G; c_pred += pred; c_tp += M;
        }
        __syncthreads();
        used = scal[HT_S_LABELS];
        // ---- the lanes look the frame's true positives up in the pair list (labels are distinct: no two of them share a pair) ----
        for (int j = t; j < fr.G; j += RTK_WAVE) {
            const int i = gpred[j];
            if (i < 0 || entry[j] < 0 || rslot[i] < 0) continue;
            gpair[j] = lw_pair_find<HT_PSLOTS>(ptab, pkey, (entry[j] << HT_SLOT_BITS) | rslot[i]);
        }
        __syncthreads();
        // ---- and thread 0 counts them, new pairs appended in detection order ----
        if (t == 0) {
            for (int i = 0; i < fr.P; ++i) {
                const int j = rj[i];
                if (j < 0 || gpred[j] != i || entry[j] < 0 || rslot[i] < 0) continue;
                int p = gpair[j];
                if (p < 0) {
                    if (npairs >= RTK_SCORE_HOTA_PAIRS) { scal[HT_S_OVERFLOW] = 1; continue; }
                    p = npairs++;
                    lw_pair_append<HT_PSLOTS>(ptab, pkey, pn, p, (entry[j] << HT_SLOT_BITS) | rslot[i]);      // at most PAIRS of 2 PAIRS slots are taken
                }
                pn[p] += 1;
            }
            scal[HT_S_PAIRS] = npairs;
        }
        __syncthreads();
        npairs = scal[HT_S_PAIRS];
    }
    if (t == 0) {
        long long *cnt = counters + ((size_t)a * B + b) * RTK_SCORE_HOTA_COUNTERS;
        double *sm = sums + ((size_t)a * B + b) * RTK_SCORE_HOTA_SUMS;
        cnt[0] = c_frames; cnt[1] = c_clips; cnt[2] = c_gt; cnt[3] = c_pred; cnt[4] = c_tp; cnt[5] = c_pairs;
        sm[0] = s_ass; sm[1] = s_re; sm[2] = s_pr; sm[3] = s_loc;
        if (scal[HT_S_OVERFLOW]) atomicOr(&flags[b], RTK_SCORE_FLAG_HOTA);
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
extern "C" int rtk_score_hota(int B, int T, const rtk_score_log_t *lg, const double *rec_score, const double *threshold, int alphas,
                              long long *counters, double *sums, int *flags, rtk_stream_t stream) {
    RTK_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && alphas >= 1 && alphas <= 63, "score_hota: bad sizes B=%d T=%d alphas=%d", B, T, alphas);
    const size_t lds = ht_lds(T);
    RTK_REQUIRE(lds <= RTK_SCORE_LDS_LIMIT, "score_hota: T=%d label-table entries need %zu bytes of LDS per stream, the limit is %d", T, lds,
                RTK_SCORE_LDS_LIMIT);
    RTK_REQUIRE(lw_log_ok(lg), "score_hota: null or empty log");
    RTK_REQUIRE(counters && sums && flags, "score_hota: null output");
    (void)hipFuncSetAttribute((const void *)hota_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RTK_SCORE_LDS_LIMIT);
    hota_kernel<<<dim3(B, alphas), RTK_WAVE, lds, (hipStream_t)stream>>>(T, *lg, rec_score, threshold, counters, sums, flags);
    RTK_CHECK_LAUNCH("score_hota");
    return RTK_OK;
}
