// track_optimal_body.h -- the LDS layout, the body and the argument checks of the replay under a per-frame OPTIMAL matching at a
// similarity threshold (include/rtk_score.h): track_optimal.hip's kernel template instantiates the body on the point IoU of the logged
// integers for rtk_score_replay_optimal and on the similarity the pair log carries for rtk_score_replay_optimal_sim.  The walk is
// described in track_optimal.hip.
#pragma once
#include <math.h>

#include "lds_assignment.h"
#include "score_log_walk.h"

#define OP_WEIGHT_ONE (1 << 23)      // a match; the quantised IoUs of a frame sum to at most MAX_BOXES * 65536 = 2^22 below it
static_assert(RTK_SCORE_MAX_BOXES * 65536 < OP_WEIGHT_ONE && OP_WEIGHT_ONE + 65536 < (1 << 29), "the weights of one frame: la_solve's range");
static_assert(RTK_SCORE_MAX_BOXES <= (1 << 8) && RTK_SCORE_MAX_BOXES <= (1 << LA_COL_BITS), "a kept-object index must fit the pair key");

// LDS, in ints: miou[MAX_BOXES] f64 | edge key, weight [PAIR_EDGES] | the solver's tables (MAX_OBJECTS rows, MAX_BOXES columns,
// PAIR_EDGES edges) | track table key, last, seen, matched, gap [TCAP] | rstay, rtrack [MAX_OBJECTS] | glabel, entry, gpred
// [MAX_BOXES] | 8 scalars
constexpr int op_fixed_words() {
    return 2 * RTK_SCORE_MAX_BOXES + 2 * RTK_SCORE_PAIR_EDGES + la_words(RTK_SCORE_MAX_OBJECTS, RTK_SCORE_MAX_BOXES, RTK_SCORE_PAIR_EDGES) +
           2 * RTK_SCORE_MAX_OBJECTS + 3 * RTK_SCORE_MAX_BOXES + 8;
}
constexpr int op_words(int TCAP) { return op_fixed_words() + 5 * TCAP; }
// The track-table capacities the kernel is built for: a T takes the smallest that holds it.  Static LDS, so the code object states each figure.
#define OP_TCAP_SMALL 1024
#define OP_TCAP_LARGE 1303      // the most that fits the limit
static_assert(op_words(OP_TCAP_LARGE) * sizeof(int) <= RTK_SCORE_LDS_LIMIT && op_words(OP_TCAP_LARGE + 1) * sizeof(int) > RTK_SCORE_LDS_LIMIT,
              "the large instance is the largest that fits one workgroup's LDS");

static size_t op_lds(int T) {
    if (T <= OP_TCAP_SMALL) return op_words(OP_TCAP_SMALL) * sizeof(int);
    if (T <= OP_TCAP_LARGE) return op_words(OP_TCAP_LARGE) * sizeof(int);
    return ((size_t)op_fixed_words() + (size_t)5 * T) * sizeof(int);      // past the limit
}

enum { OP_S_MT = 0, OP_S_PT = 1, OP_S_ML = 2, OP_S_USED = 3, OP_S_EDGES = 4, OP_S_OVERFLOW = 5 };

// the IoU of a logged pair of frame `fr` and its place in the assignment, or false: the pair does not describe its frame, its
// detection was removed, or its IoU is below min_iou.  SIM: the IoU is read as the log's own similarity pair_sim[q], which must be > 0
// (pair_common and the sizes are not read); without SIM pair_sim is not read and the function is what it was.
template <bool SIM>
__device__ __forceinline__ bool op_candidate(const rtk_score_pairs_t &pr, const lw_pair_frame_t &fr, size_t rb, size_t qb, int p, const int *rstay,
                                             double min_iou, int *row, int *col, double *iou, const double *pair_sim) {
    if (SIM) {
        const int key = pr.pair_key[qb + fr.pair + p];
        const int i = key >> 8, j = key & 255;
        if (key < 0 || i >= fr.P || j >= fr.G || !rstay[i]) return false;
        const double v = pair_sim[qb + fr.pair + p];
        if (!(v > 0.0) || !(v >= min_iou)) return false;
        *row = i; *col = j; *iou = v;
        return true;
    }
    const int key = pr.pair_key[qb + fr.pair + p], c = pr.pair_common[qb + fr.pair + p];
    const int i = key >> 8, j = key & 255;
    if (key < 0 || i >= fr.P || j >= fr.G || c <= 0 || !rstay[i]) return false;
    const int si = pr.rec_size[rb + fr.rec + i], sj = pr.label_size[rb + fr.lab + j];
    const long long den = (long long)si + (long long)sj - (long long)c;
    if (den <= 0) return false;      // the scorer's IoU is 0 (or negative) there: coincident points count once per PAIR, so c may exceed a size
    const double v = (double)c / (double)den;
    if (!(v >= min_iou)) return false;
    *row = i; *col = j; *iou = v;
    return true;
}

// op_smem: the kernel's static LDS, op_words(TCAP) ints aligned to 16 bytes
template <int TCAP, bool SIM>
__device__ __forceinline__ void optimal_replay_body(int *op_smem, int T, const rtk_score_log_t &lg, const rtk_score_pairs_t &pr,
                                                    const double *rec_score, const double *thresholds, const int *reached, double min_iou,
                                                    long long *counters, long long *iou_qs, double *iou_sums, unsigned char *tp_mask, int *flags,
                                                    const double *pair_sim) {
    const int b = blockIdx.x, x = blockIdx.y, B = gridDim.x, t = threadIdx.x;
    double *miou = reinterpret_cast<double *>(op_smem);
    int *ekey = op_smem + 2 * RTK_SCORE_MAX_BOXES, *ew = ekey + RTK_SCORE_PAIR_EDGES, *work = ew + RTK_SCORE_PAIR_EDGES;
    int *tkey = work + la_words(RTK_SCORE_MAX_OBJECTS, RTK_SCORE_MAX_BOXES, RTK_SCORE_PAIR_EDGES);
    int *tlast = tkey + TCAP, *tseen = tlast + TCAP, *tmatched = tseen + TCAP, *tgap = tmatched + TCAP;
    int *rstay = tgap + TCAP, *rtrack = rstay + RTK_SCORE_MAX_OBJECTS;
    int *glabel = rtrack + RTK_SCORE_MAX_OBJECTS, *entry = glabel + RTK_SCORE_MAX_BOXES, *gpred = entry + RTK_SCORE_MAX_BOXES;
    int *scal = gpred + RTK_SCORE_MAX_BOXES;
    long long *cnt = counters + ((size_t)x * B + b) * RTK_SCORE_OPTIMAL_COUNTERS;
    const bool mask = tp_mask != nullptr && x == 0;
    const size_t rb = (size_t)b * lg.R, qb = (size_t)b * pr.Q;
    const int cap = min(T, TCAP);

    if (reached && x > *reached) {      // a level the walk never reached
        if (t < RTK_SCORE_OPTIMAL_COUNTERS) cnt[t] = 0;
        if (t == 0) { iou_qs[(size_t)x * B + b] = 0; iou_sums[(size_t)x * B + b] = 0.0; }
        return;
    }
    const double tau = thresholds[x];
    const int frames = lw_frames(lg, b);
    // uniform running values: every lane counts them alike
    long long c_frames = 0, c_gt = 0, c_pred = 0, c_tp = 0, c_iouq = 0;
    // thread 0's running values
    long long c_idsw = 0, c_frag = 0, c_tracks = 0, c_mt = 0, c_pt = 0, c_ml = 0;
    double iou_sum = 0.0;
    int used = 0;      // uniform: thread 0 publishes it through scal
    if (t < 8) scal[t] = 0;
    __syncthreads();

    for (int f = 0; f <= frames; ++f) {
        lw_pair_frame_t fr = {};
        if (f < frames) fr = lw_pair_frame(lg, pr, b, f);
        if (f == frames || fr.reset) {
            // ---- the clip closes ----
            int mt = 0, pt = 0, ml = 0;
            for (int e = t; e < used; e += RTK_WAVE) {
                const double r = (double)tmatched[e] / (double)tseen[e];
                if (r > 0.8) ++mt; else if (r < 0.2) ++ml; else ++pt;
            }
            if (mt) atomicAdd(&scal[OP_S_MT], mt);
            if (pt) atomicAdd(&scal[OP_S_PT], pt);
            if (ml) atomicAdd(&scal[OP_S_ML], ml);
            __syncthreads();
            if (t == 0) {
                c_tracks += used; c_mt += scal[OP_S_MT]; c_pt += scal[OP_S_PT]; c_ml += scal[OP_S_ML];
                scal[OP_S_MT] = scal[OP_S_PT] = scal[OP_S_ML] = scal[OP_S_USED] = 0;
            }
            used = 0;
            __syncthreads();
            if (f == frames) break;
        }
        // ---- the frame's tables: kept labels with their table entries, which detections remain ----
        for (int j = t; j < fr.G; j += RTK_WAVE) {
            const int lab = lg.label[rb + fr.lab + j];
            glabel[j] = lab;
            miou[j] = 0.0;
            int e = -1;
            for (int k = 0; k < used; ++k)
                if (tkey[k] == lab) e = k;      // label ids are distinct within the table
            entry[j] = e;
        }
        for (int base = 0; base < fr.P; base += RTK_WAVE) {
            const int i = base + t;
            bool stays = false;
            if (i < fr.P) {
                const size_t r = rb + fr.rec + i;
                stays = lw_stays(rec_score[r], tau);
                rstay[i] = stays ? 1 : 0;
                rtrack[i] = lg.rec_track[r];
            }
            c_pred += __popcll(__ballot(stays));
        }
        if (t == 0) scal[OP_S_EDGES] = 0;
        __syncthreads();
        // ---- the candidate pairs are the edges (in any order: the solver's result depends on the edge set alone) ----
        for (int p = t; p < fr.pairs; p += RTK_WAVE) {
            int i, j;
            double v;
            if (!op_candidate<SIM>(pr, fr, rb, qb, p, rstay, min_iou, &i, &j, &v, pair_sim)) continue;
            const int at = atomicAdd(&scal[OP_S_EDGES], 1);
            if (at < RTK_SCORE_PAIR_EDGES) {
                ekey[at] = (i << LA_COL_BITS) | j;
                ew[at] = OP_WEIGHT_ONE + (int)fmin(floor(v * 65536.0), 65536.0);      // an IoU above 1 (coincident points) weighs as 1
            }
        }
        __syncthreads();
        int E = scal[OP_S_EDGES];
        if (E > RTK_SCORE_PAIR_EDGES) {      // the frame does not fit: the stream is flagged, the edges that fit are solved
            E = RTK_SCORE_PAIR_EDGES;
            if (t == 0) scal[OP_S_OVERFLOW] = 1;
        }
        c_frames += 1; c_gt += fr.G;
        if (E > 0) {      // uniform; a frame without a candidate (many are, at a high threshold) matches nothing
            const long long weight = la_solve(fr.P, fr.G, E, ekey, ew, work);
            const int *cp = work + la_cp_offset(fr.P, fr.G, E);
            c_tp += weight >> 23;
            c_iouq += weight & (OP_WEIGHT_ONE - 1);
            __syncthreads();
            // ---- the matching: the detection of every kept object, its IoU, and the matched rows ----
            for (int j = t; j < fr.G; j += RTK_WAVE) gpred[j] = cp[j];
            for (int p = t; p < fr.pairs; p += RTK_WAVE) {
                int i, j;
                double v;
                if (!op_candidate<SIM>(pr, fr, rb, qb, p, rstay, min_iou, &i, &j, &v, pair_sim)) continue;
                if (cp[j] == i) { miou[j] = v; rstay[i] = 2; }      // one pair per (i, j), one row per column: no two lanes meet
            }
        } else {
            for (int j = t; j < fr.G; j += RTK_WAVE) gpred[j] = -1;
        }
        __syncthreads();
        // ---- the IoU sum, the table and its counters: one thread, in kept-object order ----
        if (t == 0) {
            int idsw = 0, frag = 0;
            for (int j = 0; j < fr.G; ++j) {
                const bool matched = gpred[j] >= 0;
                if (matched) iou_sum += miou[j];
                int e = entry[j];
                if (e < 0) {
                    if (used >= cap) continue;      // the scorer raised RTK_SCORE_FLAG_TRACKS on this frame
                    e = used++;
                    tkey[e] = glabel[j]; tlast[e] = -1; tseen[e] = 0; tmatched[e] = 0; tgap[e] = 0;
                }
                tseen[e] += 1;
                if (matched) {
                    const int track = rtrack[gpred[j]], last = tlast[e];
                    if (last != -1 && last != track) ++idsw;
                    if (tmatched[e] > 0 && tgap[e]) ++frag;
                    tlast[e] = track;
                    tmatched[e] += 1;
                    tgap[e] = 0;
                } else {
                    tgap[e] = 1;
                }
            }
            scal[OP_S_USED] = used;
            c_idsw += idsw; c_frag += frag;
        }
        if (mask) {
            for (int i = t; i < fr.P; i += RTK_WAVE) tp_mask[rb + fr.rec + i] = rstay[i] == 2 ? 1 : 0;
        }
        __syncthreads();
        used = scal[OP_S_USED];
    }
    if (t == 0) {
        cnt[0] = c_frames; cnt[1] = c_gt; cnt[2] = c_pred; cnt[3] = c_tp; cnt[4] = c_pred - c_tp; cnt[5] = c_gt - c_tp; cnt[6] = c_idsw;
        cnt[7] = c_frag; cnt[8] = c_tracks; cnt[9] = c_mt; cnt[10] = c_pt; cnt[11] = c_ml;
        iou_qs[(size_t)x * B + b] = c_iouq;
        iou_sums[(size_t)x * B + b] = iou_sum;
        if (scal[OP_S_OVERFLOW]) atomicOr(&flags[b], RTK_SCORE_FLAG_OPTIMAL);
    }
}

// ------------------------------------------------------------------------------------------------
// host side: the checks both entry points make before their launch (`who` names the entry point in the message)
// ------------------------------------------------------------------------------------------------
static inline int op_validate(const char *who, int B, int T, const rtk_score_log_t *lg, const rtk_score_pairs_t *pr, const double *rec_score,
                              const double *thresholds, int count, double min_iou, const long long *counters, const long long *iou_q,
                              const double *iou_sum, const int *flags) {
    RTK_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && T <= (1 << 24) && count >= 1 && count <= 65535, "%s: bad sizes B=%d T=%d count=%d", who, B, T, count);
    const size_t lds = op_lds(T);
    RTK_REQUIRE(lds <= RTK_SCORE_LDS_LIMIT, "%s: T=%d track-table entries need %zu bytes of LDS per stream, the limit is %d (at most T=%d)", who, T, lds,
                RTK_SCORE_LDS_LIMIT, OP_TCAP_LARGE);
    RTK_REQUIRE(min_iou > 0.0 && min_iou < INFINITY, "%s: min_iou=%g must be finite and above 0", who, min_iou);
    RTK_REQUIRE(lw_log_ok(lg), "%s: null or empty log", who);
    RTK_REQUIRE(lw_pairs_ok(pr), "%s: null or empty pair log", who);
    RTK_REQUIRE(rec_score && thresholds && counters && iou_q && iou_sum && flags, "%s: null argument", who);
    return RTK_OK;
}
