// track_hota_optimal_body.h -- the LDS layouts, the bodies and the argument checks of HOTA under TrackEval's matching (include/rtk_score.h,
// "HOTA under the optimal matching"): track_hota_optimal.hip's kernel templates instantiate the bodies on the point IoU of the logged
// integers for rtk_score_alignment and rtk_score_hota_optimal, and on the similarity the pair log carries for rtk_score_alignment_sim and
// rtk_score_hota_optimal_sim.  The two walks are described in track_hota_optimal.hip.
#pragma once
#include <math.h>

#include "lds_assignment.h"
#include "score_log_walk.h"

#define HO_PAIRS RTK_SCORE_ALIGN_PAIRS                                      // the potential pairs of one clip
#define HO_PSLOTS (2 * HO_PAIRS)                                            // the pair lookup: half stays empty
#define HO_SLOT_BITS 12                                                     // a pair's key: label entry << 12 | track slot
#define HO_SLOT_MASK ((1 << HO_SLOT_BITS) - 1)
#define HO_WEIGHT_ONE 268435456.0                                           // 2^28: a score of 1
static_assert(LW_SLOTS <= (1 << HO_SLOT_BITS), "a track slot must fit the pair key");
static_assert(RTK_SCORE_MAX_BOXES <= RTK_WAVE && RTK_SCORE_MAX_BOXES <= (1 << 8) && RTK_SCORE_MAX_BOXES <= (1 << LA_COL_BITS),
              "a kept object has a lane of its own and its index fits both pair keys");

// ------------------------------------------------------------------------------------------------
// the alignment pass
// ------------------------------------------------------------------------------------------------
// LDS, in ints: rsum[MAX_OBJECTS], ksum[MAX_BOXES], cq[WAVE], pmc[PAIRS] f64 | ckey, cidx [WAVE] | pair list key, n [PAIRS] | pair lookup
// [2 PAIRS] | track table key, ct [LW_SLOTS] | label table key, cg [TCAP] | rslot [MAX_OBJECTS] | glabel, entry [MAX_BOXES] | 8 scalars
// (n is lw_pair_append's count word: here the valid logged pairs of the clip-pair, which nothing reads)
constexpr int al_fixed_words() {
    return 2 * (RTK_SCORE_MAX_OBJECTS + RTK_SCORE_MAX_BOXES + RTK_WAVE + HO_PAIRS) + 2 * RTK_WAVE + 2 * HO_PAIRS + HO_PSLOTS + 2 * LW_SLOTS +
           RTK_SCORE_MAX_OBJECTS + 2 * RTK_SCORE_MAX_BOXES + 8;
}
constexpr int al_words(int TCAP) { return al_fixed_words() + 2 * TCAP; }
// The label capacities the kernel is built for: a T takes the smallest that holds it.  Static LDS, so the code object states each figure.
#define AL_TCAP_SMALL 1024
#define AL_TCAP_LARGE 1404      // the most that fits the limit
static_assert(al_words(AL_TCAP_LARGE) * sizeof(int) <= RTK_SCORE_LDS_LIMIT && al_words(AL_TCAP_LARGE + 1) * sizeof(int) > RTK_SCORE_LDS_LIMIT,
              "the large instance is the largest that fits one workgroup's LDS");

static size_t al_lds(int T) {
    if (T <= AL_TCAP_SMALL) return al_words(AL_TCAP_SMALL) * sizeof(int);
    if (T <= AL_TCAP_LARGE) return al_words(AL_TCAP_LARGE) * sizeof(int);
    return ((size_t)al_fixed_words() + (size_t)2 * T) * sizeof(int);      // past the limit
}

enum { AL_S_LABELS = 0, AL_S_TRACKS = 1, AL_S_PAIRS = 2, AL_S_OVERFLOW = 3 };

// al_smem: the kernel's static LDS, al_words(TCAP) ints aligned to 16 bytes.  SIM: lw_valid_pair's switch (pair_sim is read only with it)
template <int TCAP, bool SIM>
__device__ __forceinline__ void alignment_body(int *al_smem, int T, const rtk_score_log_t &lg, const rtk_score_pairs_t &pr, const double *rec_score,
                                               const double *threshold, double *pair_a, int *pair_index, int *clip_cg, int *clip_ct, int *flags,
                                               const double *pair_sim) {
    const int b = blockIdx.x, t = threadIdx.x;
    double *rsum = reinterpret_cast<double *>(al_smem), *ksum = rsum + RTK_SCORE_MAX_OBJECTS, *cq = ksum + RTK_SCORE_MAX_BOXES, *pmc = cq + RTK_WAVE;
    int *ckey = reinterpret_cast<int *>(pmc + HO_PAIRS), *cidx = ckey + RTK_WAVE;
    int *pkey = cidx + RTK_WAVE, *pn = pkey + HO_PAIRS, *ptab = pn + HO_PAIRS;
    int *tkey = ptab + HO_PSLOTS, *tct = tkey + LW_SLOTS;
    int *lkey = tct + LW_SLOTS, *lcg = lkey + TCAP;
    int *rslot = lcg + TCAP, *glabel = rslot + RTK_SCORE_MAX_OBJECTS, *entry = glabel + RTK_SCORE_MAX_BOXES, *scal = entry + RTK_SCORE_MAX_BOXES;

    const bool filter = rec_score != nullptr && threshold != nullptr;
    const double tau = filter ? *threshold : 0.0;
    const int frames = lw_frames(lg, b), cap = min(T, TCAP);
    const size_t rb = (size_t)b * lg.R, qb = (size_t)b * pr.Q;
    int used = 0, npairs = 0;      // uniform: thread 0 publishes them through scal
    int first = 0, cbase = 0;      // uniform: the open clip's first frame, and the clip-pairs of the clips before it

    for (int h = t; h < LW_SLOTS; h += RTK_WAVE) { tkey[h] = LW_EMPTY; tct[h] = 0; }
    for (int h = t; h < HO_PSLOTS; h += RTK_WAVE) ptab[h] = -1;
    if (t < 8) scal[t] = 0;
    __syncthreads();

    for (int f = 0; f <= frames; ++f) {
        lw_pair_frame_t fr = {};
        if (f < frames) fr = lw_pair_frame(lg, pr, b, f);
        if ((f == frames || fr.reset) && f > 0) {
            // ---- the clip closes: its clip-pairs' cg and ct, then its frames a second time -- every logged pair reads its index back
            //      (the lane that wrote it: pair p is lane p % 64 in both walks) and receives A = pmc / ((cg + ct) - pmc) ----
            for (int p = t; p < npairs; p += RTK_WAVE) {
                if (cbase + p >= pr.Q) continue;
                clip_cg[qb + cbase + p] = lcg[pkey[p] >> HO_SLOT_BITS];
                clip_ct[qb + cbase + p] = tct[pkey[p] & HO_SLOT_MASK];
            }
            for (int g = first; g < f; ++g) {
                const lw_pair_frame_t fg = lw_pair_frame(lg, pr, b, g);
                for (int p = t; p < fg.pairs; p += RTK_WAVE) {
                    const int at = pair_index[qb + fg.pair + p] - cbase;
                    double a = 0.0;
                    if (at >= 0 && at < npairs) {
                        const int key = pkey[at];
                        const double m = pmc[at];
                        a = m / ((double)(lcg[key >> HO_SLOT_BITS] + tct[key & HO_SLOT_MASK]) - m);
                    }
                    pair_a[qb + fg.pair + p] = a;
                }
            }
            __syncthreads();
            for (int h = t; h < LW_SLOTS; h += RTK_WAVE) { tkey[h] = LW_EMPTY; tct[h] = 0; }
            for (int h = t; h < HO_PSLOTS; h += RTK_WAVE) ptab[h] = -1;
            if (t == 0) scal[AL_S_LABELS] = scal[AL_S_TRACKS] = scal[AL_S_PAIRS] = 0;
            cbase = min(cbase + npairs, pr.Q);
            first = f; used = 0; npairs = 0;
            __syncthreads();
        }
        if (f == frames) break;
        // ---- the frame's tables: kept labels with their table entries; the remaining detections with their track slot and its count ----
        for (int j = t; j < fr.G; j += RTK_WAVE) {
            const int lab = lg.label[rb + fr.lab + j];
            glabel[j] = lab;
            ksum[j] = 0.0;
            int e = -1;
            for (int k = 0; k < used; ++k)
                if (lkey[k] == lab) e = k;      // label ids are distinct within the table
            entry[j] = e;
        }
        for (int i = t; i < fr.P; i += RTK_WAVE) {
            const size_t r = rb + fr.rec + i;
            int s = LW_REMOVED;
            if (!filter || lw_stays(rec_score[r], tau)) {
                s = lw_track_slot<true>(tkey, &scal[AL_S_TRACKS], lg.rec_track[r]);
                if (s >= 0) atomicAdd(&tct[s], 1); else scal[AL_S_OVERFLOW] = 1;
            }
            rslot[i] = s;      // LW_REMOVED | -1: remains, the track table is full | its track slot
            rsum[i] = 0.0;
        }
        __syncthreads();
        if (t == 0) {      // the label table: one thread, in order
            for (int j = 0; j < fr.G; ++j) {
                int e = entry[j];
                if (e < 0) {
                    if (used >= cap) { scal[AL_S_OVERFLOW] = 1; continue; }
                    e = used++;
                    lkey[e] = glabel[j]; lcg[e] = 0;
                    entry[j] = e;
                }
                lcg[e] += 1;
            }
            scal[AL_S_LABELS] = used;
        }
        __syncthreads();
        used = scal[AL_S_LABELS];
        // ---- r and k: a wave's width of pairs at a time; lane t owns the rows i = t mod 64 and column t and adds in pair-log order ----
        for (int base = 0; base < fr.pairs; base += RTK_WAVE) {
            int key = -1;
            double sb = 0.0;
            if (base + t < fr.pairs) {
                int i, j;
                double s;
                if (lw_valid_pair<SIM>(pr, fr, rb, qb, base + t, rslot, &i, &j, &s, pair_sim)) { key = (i << 8) | j; sb = fmin(s, 1.0); }
            }
            ckey[t] = key; cq[t] = sb;
            __syncthreads();
            const int m = min(fr.pairs - base, RTK_WAVE);
            for (int e = 0; e < m; ++e) {
                const int k = ckey[e];
                if (k < 0) continue;
                const double v = cq[e];
                if (((k >> 8) & (RTK_WAVE - 1)) == t) rsum[k >> 8] += v;
                if ((k & 255) == t) ksum[k & 255] += v;
            }
            __syncthreads();
        }
        // ---- q = s / ((r + k) - s) of every valid pair, its (label, track) looked up by the lanes; thread 0 appends the new ones and
        //      adds in pair-log order ----
        for (int base = 0; base < fr.pairs; base += RTK_WAVE) {
            int key = -1, at = -1;
            bool valid = false;
            double q = 0.0;
            if (base + t < fr.pairs) {
                int i, j;
                double s;
                if (lw_valid_pair<SIM>(pr, fr, rb, qb, base + t, rslot, &i, &j, &s, pair_sim)) {
                    const double sb = fmin(s, 1.0);
                    valid = true;
                    q = sb / ((rsum[i] + ksum[j]) - sb);
                    if (entry[j] >= 0 && rslot[i] >= 0) {
                        key = (entry[j] << HO_SLOT_BITS) | rslot[i];
                        at = lw_pair_find<HO_PSLOTS>(ptab, pkey, key);
                    }
                }
            }
            ckey[t] = key; cidx[t] = at; cq[t] = q;
            __syncthreads();
            if (t == 0) {
                const int m = min(fr.pairs - base, RTK_WAVE);
                for (int e = 0; e < m; ++e) {
                    const int k = ckey[e];
                    if (k < 0) continue;
                    int p = cidx[e];
                    if (p < 0) p = lw_pair_find<HO_PSLOTS>(ptab, pkey, k);      // appended by an earlier pair of this chunk
                    if (p < 0) {
                        if (npairs >= HO_PAIRS) { scal[AL_S_OVERFLOW] = 1; cidx[e] = -1; continue; }
                        p = npairs++;
                        lw_pair_append<HO_PSLOTS>(ptab, pkey, pn, p, k);      // at most PAIRS of 2 PAIRS slots are taken
                        pmc[p] = 0.0;
                    }
                    cidx[e] = p;
                    pmc[p] += cq[e];
                    pn[p] += 1;
                }
                scal[AL_S_PAIRS] = npairs;
            }
            __syncthreads();
            npairs = scal[AL_S_PAIRS];
            if (base + t < fr.pairs) {
                const int p = key >= 0 ? cidx[t] : -1;
                pair_index[qb + fr.pair + base + t] = p >= 0 && cbase + p < pr.Q ? cbase + p : -1;
                if (valid && p < 0) scal[AL_S_OVERFLOW] = 1;      // a valid pair without a clip-pair: a table was full
            }
            __syncthreads();
        }
    }
    if (t == 0 && scal[AL_S_OVERFLOW]) atomicOr(&flags[b], RTK_SCORE_FLAG_HOTA);
}

// ------------------------------------------------------------------------------------------------
// the matching and the sums
// ------------------------------------------------------------------------------------------------
// LDS, in ints: miou[MAX_BOXES], quot[3][WAVE] f64 | edge key, weight [PAIR_EDGES] | the solver's tables (MAX_OBJECTS rows, MAX_BOXES
// columns, PAIR_EDGES edges) | n [PAIRS] | rstay [MAX_OBJECTS] | gpred, gidx [MAX_BOXES] | qn [WAVE] | 8 scalars
constexpr int ho_words() {
    return 2 * (RTK_SCORE_MAX_BOXES + 3 * RTK_WAVE) + 2 * RTK_SCORE_PAIR_EDGES + la_words(RTK_SCORE_MAX_OBJECTS, RTK_SCORE_MAX_BOXES, RTK_SCORE_PAIR_EDGES) +
           HO_PAIRS + RTK_SCORE_MAX_OBJECTS + 2 * RTK_SCORE_MAX_BOXES + RTK_WAVE + 8;
}
static_assert(ho_words() * sizeof(int) <= RTK_SCORE_LDS_LIMIT, "the matching kernel's tables fit one workgroup's LDS");

enum { HO_S_EDGES = 0, HO_S_TOP = 1, HO_S_OVERFLOW = 2 };

// a valid pair of frame `fr` that has a clip-pair of the open clip (the clips before it hold cbase): its place in the assignment, its
// similarity and its clip-pair's index within the clip -- or false
template <bool SIM>
__device__ __forceinline__ bool ho_edge(const rtk_score_pairs_t &pr, const lw_pair_frame_t &fr, size_t rb, size_t qb, int p, const int *rstay,
                                        const int *pair_index, int cbase, int *row, int *col, double *s, int *at, const double *pair_sim) {
    if (!lw_valid_pair<SIM>(pr, fr, rb, qb, p, rstay, row, col, s, pair_sim)) return false;
    const int gi = pair_index[qb + fr.pair + p];
    if (gi < cbase || gi >= pr.Q || gi - cbase >= HO_PAIRS) return false;
    *at = gi - cbase;
    return true;
}

// ho_smem: the kernel's static LDS, ho_words() ints aligned to 16 bytes
template <bool SIM>
__device__ __forceinline__ void hota_optimal_body(int *ho_smem, const rtk_score_log_t &lg, const rtk_score_pairs_t &pr, const double *rec_score,
                                                  const double *threshold, const double *pair_a, const int *pair_index, const int *clip_cg,
                                                  const int *clip_ct, long long *counters, double *sums, int *flags, const double *pair_sim) {
    const int b = blockIdx.x, a = blockIdx.y, B = gridDim.x, A = gridDim.y, t = threadIdx.x;
    double *miou = reinterpret_cast<double *>(ho_smem), *quot = miou + RTK_SCORE_MAX_BOXES;
    int *ekey = reinterpret_cast<int *>(quot + 3 * RTK_WAVE), *ew = ekey + RTK_SCORE_PAIR_EDGES, *work = ew + RTK_SCORE_PAIR_EDGES;
    int *pn = work + la_words(RTK_SCORE_MAX_OBJECTS, RTK_SCORE_MAX_BOXES, RTK_SCORE_PAIR_EDGES);
    int *rstay = pn + HO_PAIRS, *gpred = rstay + RTK_SCORE_MAX_OBJECTS, *gidx = gpred + RTK_SCORE_MAX_BOXES;
    int *qn = gidx + RTK_SCORE_MAX_BOXES, *scal = qn + RTK_WAVE;

    const double alpha = (double)(a + 1) / (double)(A + 1);
    const bool filter = rec_score != nullptr && threshold != nullptr;
    const double tau = filter ? *threshold : 0.0;
    const int frames = lw_frames(lg, b);
    const size_t rb = (size_t)b * lg.R, qb = (size_t)b * pr.Q;
    long long c_frames = 0, c_clips = 0, c_gt = 0, c_pred = 0;      // uniform: every lane counts them alike
    long long c_tp = 0, c_pairs = 0;                                // thread 0's running values
    double s_ass = 0.0, s_re = 0.0, s_pr = 0.0, s_loc = 0.0;
    int cbase = 0;      // uniform: the clip-pairs of the clips before the open one

    for (int p = t; p < HO_PAIRS; p += RTK_WAVE) pn[p] = 0;
    if (t < 8) scal[t] = 0;
    __syncthreads();

    for (int f = 0; f <= frames; ++f) {
        lw_pair_frame_t fr = {};
        if (f < frames) fr = lw_pair_frame(lg, pr, b, f);
        if ((f == frames || fr.reset) && f > 0) {
            // ---- the clip closes: the lanes compute a wave's width of quotients, thread 0 adds them in the clip-pairs' order ----
            const int top = scal[HO_S_TOP];
            __syncthreads();
            for (int base = 0; base < top; base += RTK_WAVE) {
                const int p = base + t;
                int n = 0;
                if (p < top) { n = pn[p]; pn[p] = 0; }
                if (n > 0) {
                    const int cg = clip_cg[qb + cbase + p], ct = clip_ct[qb + cbase + p];
                    const double N = (double)((long long)n * (long long)n);
                    quot[t] = N / (double)(cg + ct - n);
                    quot[RTK_WAVE + t] = N / (double)cg;
                    quot[2 * RTK_WAVE + t] = N / (double)ct;
                }
                qn[t] = n;
                __syncthreads();
                if (t == 0) {
                    const int m = min(top - base, RTK_WAVE);
                    for (int k = 0; k < m; ++k) {
                        if (qn[k] <= 0) continue;
                        s_ass += quot[k];
                        s_re += quot[RTK_WAVE + k];
                        s_pr += quot[2 * RTK_WAVE + k];
                        c_pairs += 1;
                    }
                }
                __syncthreads();
            }
            if (t == 0) scal[HO_S_TOP] = 0;
            cbase = min(cbase + top, pr.Q);
            c_clips += 1;
            __syncthreads();
        }
        if (f == frames) break;
        // ---- which detections remain ----
        for (int base = 0; base < fr.P; base += RTK_WAVE) {
            const int i = base + t;
            bool stays = false;
            if (i < fr.P) {
                stays = !filter || lw_stays(rec_score[rb + fr.rec + i], tau);
                rstay[i] = stays ? 0 : LW_REMOVED;
            }
            c_pred += __popcll(__ballot(stays));
        }
        for (int j = t; j < fr.G; j += RTK_WAVE) { gpred[j] = -1; gidx[j] = -1; }
        if (t == 0) scal[HO_S_EDGES] = 0;
        __syncthreads();
        // ---- the valid pairs are the edges (in any order: the solver's result depends on the edge set alone) ----
        for (int p = t; p < fr.pairs; p += RTK_WAVE) {
            int i, j, at;
            double s;
            if (!ho_edge<SIM>(pr, fr, rb, qb, p, rstay, pair_index, cbase, &i, &j, &s, &at, pair_sim)) continue;
            atomicMax(&scal[HO_S_TOP], at + 1);
            const double w = pair_a[qb + fr.pair + p] * fmin(s, 1.0);
            const int e = atomicAdd(&scal[HO_S_EDGES], 1);
            if (e < RTK_SCORE_PAIR_EDGES) {
                ekey[e] = (i << LA_COL_BITS) | j;
                ew[e] = w > 0.0 ? max(1, (int)floor(fmin(w, 1.0) * HO_WEIGHT_ONE)) : 1;      // a positive overlap never vanishes
            }
        }
        __syncthreads();
        int E = scal[HO_S_EDGES];
        if (E > RTK_SCORE_PAIR_EDGES) {      // the frame does not fit: the stream is flagged, the edges that fit are solved
            E = RTK_SCORE_PAIR_EDGES;
            if (t == 0) scal[HO_S_OVERFLOW] = 1;
        }
        c_frames += 1; c_gt += fr.G;
        if (E > 0) {      // uniform
            la_solve(fr.P, fr.G, E, ekey, ew, work);
            const int *cp = work + la_cp_offset(fr.P, fr.G, E);
            __syncthreads();
            // ---- the matching: the detection of every kept object, the pair's similarity and its clip-pair ----
            for (int j = t; j < fr.G; j += RTK_WAVE) gpred[j] = cp[j];
            for (int p = t; p < fr.pairs; p += RTK_WAVE) {
                int i, j, at;
                double s;
                if (!ho_edge<SIM>(pr, fr, rb, qb, p, rstay, pair_index, cbase, &i, &j, &s, &at, pair_sim)) continue;
                if (cp[j] == i) { miou[j] = s; gidx[j] = at; }      // one pair per (i, j), one row per column: no two lanes meet
            }
            __syncthreads();
            // ---- this level's true positives: one thread, in kept-object order ----
            if (t == 0) {
                for (int j = 0; j < fr.G; ++j) {
                    if (gpred[j] < 0 || gidx[j] < 0 || !(miou[j] >= alpha)) continue;      // (gidx < 0: only in a frame that overflowed)
                    c_tp += 1;
                    s_loc += miou[j];
                    pn[gidx[j]] += 1;
                }
            }
            __syncthreads();
        }
    }
    if (t == 0) {
        long long *cnt = counters + ((size_t)a * B + b) * RTK_SCORE_HOTA_COUNTERS;
        double *sm = sums + ((size_t)a * B + b) * RTK_SCORE_HOTA_SUMS;
        cnt[0] = c_frames; cnt[1] = c_clips; cnt[2] = c_gt; cnt[3] = c_pred; cnt[4] = c_tp; cnt[5] = c_pairs;
        sm[0] = s_ass; sm[1] = s_re; sm[2] = s_pr; sm[3] = s_loc;
        if (scal[HO_S_OVERFLOW]) atomicOr(&flags[b], RTK_SCORE_FLAG_OPTIMAL);
    }
}

// ------------------------------------------------------------------------------------------------
// host side: the checks the entry points make before their launch (`who` names the entry point in the message)
// ------------------------------------------------------------------------------------------------
static inline int al_validate(const char *who, int B, int T, const rtk_score_log_t *lg, const rtk_score_pairs_t *pr, const double *pair_a,
                              const int *pair_index, const int *clip_cg, const int *clip_ct, const int *flags) {
    RTK_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && T <= (1 << 24), "%s: bad sizes B=%d T=%d", who, B, T);
    const size_t lds = al_lds(T);
    RTK_REQUIRE(lds <= RTK_SCORE_LDS_LIMIT, "%s: T=%d label-table entries need %zu bytes of LDS per stream, the limit is %d (at most T=%d)", who, T, lds,
                RTK_SCORE_LDS_LIMIT, AL_TCAP_LARGE);
    RTK_REQUIRE(lw_log_ok(lg), "%s: null or empty log", who);
    RTK_REQUIRE(lw_pairs_ok(pr), "%s: null or empty pair log", who);
    RTK_REQUIRE(pair_a && pair_index && clip_cg && clip_ct && flags, "%s: null output", who);
    return RTK_OK;
}

static inline int ho_validate(const char *who, int B, const rtk_score_log_t *lg, const rtk_score_pairs_t *pr, int alphas, const double *pair_a,
                              const int *pair_index, const int *clip_cg, const int *clip_ct, const long long *counters, const double *sums,
                              const int *flags) {
    RTK_REQUIRE(B >= 1 && B <= 65535 && alphas >= 1 && alphas <= 63, "%s: bad sizes B=%d alphas=%d", who, B, alphas);
    RTK_REQUIRE(lw_log_ok(lg), "%s: null or empty log", who);
    RTK_REQUIRE(lw_pairs_ok(pr), "%s: null or empty pair log", who);
    RTK_REQUIRE(pair_a && pair_index && clip_cg && clip_ct, "%s: null alignment tables", who);
    RTK_REQUIRE(counters && sums && flags, "%s: null output", who);
    return RTK_OK;
}
