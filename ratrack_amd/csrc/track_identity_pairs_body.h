// track_identity_pairs_body.h -- the LDS layout, the body and the argument checks of the identity metrics over every pair
// (include/rtk_score.h, "Identity over every pair"): track_identity_pairs.hip's kernel template instantiates the body on the point IoU of the
// logged integers for rtk_score_identity_pairs and on the similarity the pair log carries for rtk_score_identity_pairs_sim.  The walk is
// described in track_identity_pairs.hip.
#pragma once
#include "lds_assignment.h"
#include "score_log_walk.h"

#define IP_SLOTS LW_SLOTS                                                   // the track table
#define IP_PSLOTS (2 * RTK_SCORE_ID_PAIRS)                                  // the pair lookup: half stays empty
#define IP_SLOT_BITS LA_COL_BITS                                            // a pair's key: label entry << 12 | track slot
#define IP_SLOT_MASK ((1 << IP_SLOT_BITS) - 1)
#define IP_MAX_FRAMES (1 << 28)                                             // a pair's weight is at most the frames of its clip
static_assert(IP_SLOTS <= (1 << IP_SLOT_BITS), "a track slot must fit the pair key");
static_assert(RTK_SCORE_ID_PAIRS <= (1 << IP_SLOT_BITS), "a compacted track index must fit the pair key");

// LDS, in ints.  The pair list (key, n) comes first and lives through the clip's close; behind it EITHER the walk's tables -- label
// table [TCAP] | track table [IP_SLOTS] | pair lookup [IP_PSLOTS] | last frame of every pair [PAIRS] | rslot [MAX_OBJECTS] | ckey, cpair
// [WAVE] | glabel, entry [MAX_BOXES] | 8 scalars -- OR the solver's (TCAP rows, at most PAIRS columns and edges).
constexpr int ip_walk_words(int TCAP) {
    return TCAP + IP_SLOTS + IP_PSLOTS + RTK_SCORE_ID_PAIRS + RTK_SCORE_MAX_OBJECTS + 2 * RTK_WAVE + 2 * RTK_SCORE_MAX_BOXES + 8;
}
constexpr int ip_words(int TCAP) {
    return 2 * RTK_SCORE_ID_PAIRS + (ip_walk_words(TCAP) > la_words(TCAP, RTK_SCORE_ID_PAIRS, RTK_SCORE_ID_PAIRS)
                                         ? ip_walk_words(TCAP)
                                         : la_words(TCAP, RTK_SCORE_ID_PAIRS, RTK_SCORE_ID_PAIRS));
}
// The label capacities the kernel is built for: a T takes the smallest that holds it.  Static LDS, so the code object states each figure.
#define IP_TCAP_SMALL 1024
#define IP_TCAP_LARGE 3583      // the most that fits the limit
static_assert(ip_words(IP_TCAP_LARGE) * sizeof(int) <= RTK_SCORE_LDS_LIMIT && ip_words(IP_TCAP_LARGE + 1) * sizeof(int) > RTK_SCORE_LDS_LIMIT,
              "the large instance is the largest that fits one workgroup's LDS");

static size_t ip_lds(int T) {
    if (T <= IP_TCAP_SMALL) return ip_words(IP_TCAP_SMALL) * sizeof(int);
    if (T <= IP_TCAP_LARGE) return ip_words(IP_TCAP_LARGE) * sizeof(int);
    return ((size_t)2 * T + 1 + 9 * RTK_SCORE_ID_PAIRS) * sizeof(int);      // the pair list and la_words(T, PAIRS, PAIRS): past the limit
}

enum { IP_S_LABELS = 0, IP_S_TRACKS = 1, IP_S_PAIRS = 2, IP_S_OVERFLOW = 3 };

// ip_smem: the kernel's static LDS, ip_words(TCAP) ints aligned to 16 bytes.  SIM: lw_valid_pair's switch (pair_sim is read only with it)
template <int TCAP, bool SIM>
__device__ __forceinline__ void identity_pairs_body(int *ip_smem, int T, const rtk_score_log_t &lg, const rtk_score_pairs_t &pr, const double *rec_score,
                                                    const double *threshold, const double *alphas, long long *counters, int *flags,
                                                    const double *pair_sim) {
    const int b = blockIdx.x, a = blockIdx.y, B = gridDim.x, t = threadIdx.x;
    int *pkey = ip_smem, *pn = pkey + RTK_SCORE_ID_PAIRS, *work = pn + RTK_SCORE_ID_PAIRS;
    int *lkey = work, *tkey = lkey + TCAP, *ptab = tkey + IP_SLOTS, *plast = ptab + IP_PSLOTS;
    int *rslot = plast + RTK_SCORE_ID_PAIRS, *ckey = rslot + RTK_SCORE_MAX_OBJECTS, *cpair = ckey + RTK_WAVE;
    int *glabel = cpair + RTK_WAVE, *entry = glabel + RTK_SCORE_MAX_BOXES, *scal = entry + RTK_SCORE_MAX_BOXES;

    const double alpha = alphas[a];
    const bool filter = rec_score != nullptr && threshold != nullptr;
    const double tau = filter ? *threshold : 0.0;
    const int frames = lw_frames(lg, b);
    const size_t rb = (size_t)b * lg.R, qb = (size_t)b * pr.Q;
    long long c_frames = 0, c_clips = 0, c_gt = 0, c_pred = 0, c_idtp = 0, c_pairs = 0;      // uniform: every lane counts them alike
    int used = 0, npairs = 0, overflow = 0;      // uniform: thread 0 publishes them through scal

    for (int h = t; h < IP_SLOTS; h += RTK_WAVE) tkey[h] = LW_EMPTY;
    for (int h = t; h < IP_PSLOTS; h += RTK_WAVE) ptab[h] = -1;
    if (t < 8) scal[t] = 0;
    __syncthreads();

    for (int f = 0; f <= frames; ++f) {
        lw_pair_frame_t fr = {};
        if (f < frames) fr = lw_pair_frame(lg, pr, b, f);
        if ((f == frames || fr.reset) && f > 0) {
            // ---- the clip closes.  The tracks that appear in a pair are numbered 0, 1, ... in the order of their first pair: the
            //      track table gives way to "first pair of this slot", the pair lookup to that pair's number ----
            overflow |= scal[IP_S_OVERFLOW];
            __syncthreads();
            for (int h = t; h < IP_SLOTS; h += RTK_WAVE) tkey[h] = LA_INF;
            __syncthreads();
            for (int p = t; p < npairs; p += RTK_WAVE) atomicMin(&tkey[pkey[p] & IP_SLOT_MASK], p);
            __syncthreads();
            int ncols = 0;
            for (int base = 0; base < npairs; base += RTK_WAVE) {
                const int p = base + t;
                const bool first = p < npairs && tkey[pkey[p] & IP_SLOT_MASK] == p;
                const unsigned long long firsts = __ballot(first);
                if (first) ptab[p] = ncols + __popcll(firsts & ((1ull << t) - 1ull));
                ncols += __popcll(firsts);
            }
            __syncthreads();
            for (int p = t; p < npairs; p += RTK_WAVE) {
                const int key = pkey[p];
                pkey[p] = (key & ~IP_SLOT_MASK) | ptab[tkey[key & IP_SLOT_MASK]];
            }
            __syncthreads();
            c_idtp += la_solve(used, ncols, npairs, pkey, pn, work);
            c_clips += 1; c_pairs += npairs;
            __syncthreads();
            for (int h = t; h < IP_SLOTS; h += RTK_WAVE) tkey[h] = LW_EMPTY;
            for (int h = t; h < IP_PSLOTS; h += RTK_WAVE) ptab[h] = -1;
            if (t < 8) scal[t] = 0;
            used = 0; npairs = 0;
            __syncthreads();
        }
        if (f == frames) break;
        // ---- the frame's kept labels with their table entries ----
        for (int j = t; j < fr.G; j += RTK_WAVE) {
            const int lab = lg.label[rb + fr.lab + j];
            glabel[j] = lab;
            int e = -1;
            for (int k = 0; k < used; ++k)
                if (lkey[k] == lab) e = k;      // label ids are distinct within the table
            entry[j] = e;
        }
        __syncthreads();
        if (t == 0) {
            for (int j = 0; j < fr.G; ++j) {
                if (entry[j] >= 0) continue;
                if (used >= min(T, TCAP)) { scal[IP_S_OVERFLOW] = 1; continue; }      // the label stays without an entry: its pairs go uncounted
                lkey[used] = glabel[j];
                entry[j] = used++;
            }
            scal[IP_S_LABELS] = used;
        }
        __syncthreads();
        used = scal[IP_S_LABELS];
        c_frames += 1; c_gt += fr.G;
        // ---- the remaining detections and their track slots ----
        for (int base = 0; base < fr.P; base += RTK_WAVE) {
            const int i = base + t;
            bool stays = false;
            if (i < fr.P) {
                const size_t r = rb + fr.rec + i;
                stays = !filter || lw_stays(rec_score[r], tau);
                int s = LW_REMOVED;
                if (stays) {
                    s = lw_track_slot<true>(tkey, &scal[IP_S_TRACKS], lg.rec_track[r]);
                    if (s < 0) scal[IP_S_OVERFLOW] = 1;
                }
                rslot[i] = s;      // LW_REMOVED | -1: remains, the track table is full | its track slot
            }
            c_pred += __popcll(__ballot(stays));
        }
        __syncthreads();
        // ---- the frame's pairs, a wave's width at a time: the lanes test them and look the (label, track) up; thread 0 counts them in
        //      pair-log order, new ones appended, each at most once per frame ----
        for (int base = 0; base < fr.pairs; base += RTK_WAVE) {
            int key = -1;
            if (base + t < fr.pairs) {
                int i, j;
                double s;
                if (lw_valid_pair<SIM>(pr, fr, rb, qb, base + t, rslot, &i, &j, &s, pair_sim) && s >= alpha && entry[j] >= 0 && rslot[i] >= 0)
                    key = (entry[j] << IP_SLOT_BITS) | rslot[i];
            }
            ckey[t] = key;
            cpair[t] = key < 0 ? -1 : lw_pair_find<IP_PSLOTS>(ptab, pkey, key);
            __syncthreads();
            if (t == 0) {
                const int m = min(fr.pairs - base, RTK_WAVE);
                for (int e = 0; e < m; ++e) {
                    const int k = ckey[e];
                    if (k < 0) continue;
                    int p = cpair[e];
                    if (p < 0) p = lw_pair_find<IP_PSLOTS>(ptab, pkey, k);      // appended by an earlier pair of this chunk
                    if (p < 0) {
                        if (npairs >= RTK_SCORE_ID_PAIRS) { scal[IP_S_OVERFLOW] = 1; continue; }
                        p = npairs++;
                        lw_pair_append<IP_PSLOTS>(ptab, pkey, pn, p, k);      // at most PAIRS of 2 PAIRS slots are taken
                        plast[p] = -1;
                    }
                    if (plast[p] == f) continue;      // a pair counts a frame once
                    plast[p] = f;
                    pn[p] += 1;
                }
                scal[IP_S_PAIRS] = npairs;
            }
            __syncthreads();
            npairs = scal[IP_S_PAIRS];
        }
    }
    if (t == 0) {
        long long *cnt = counters + ((size_t)a * B + b) * RTK_SCORE_ID_COUNTERS;
        cnt[0] = c_frames; cnt[1] = c_clips; cnt[2] = c_gt; cnt[3] = c_pred; cnt[4] = c_idtp; cnt[5] = c_pairs;
        if (overflow | scal[IP_S_OVERFLOW]) atomicOr(&flags[b], RTK_SCORE_FLAG_IDENTITY);
    }
}

// ------------------------------------------------------------------------------------------------
// host side: the checks both entry points make before their launch (`who` names the entry point in the message)
// ------------------------------------------------------------------------------------------------
static inline int ip_validate(const char *who, int B, int T, const rtk_score_log_t *lg, const rtk_score_pairs_t *pr, const double *alphas, int count,
                              const long long *counters, const int *flags) {
    RTK_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && T <= (1 << 24) && count >= 1 && count <= 63, "%s: bad sizes B=%d T=%d count=%d", who, B, T, count);
    const size_t lds = ip_lds(T);
    RTK_REQUIRE(lds <= RTK_SCORE_LDS_LIMIT, "%s: T=%d label-table entries need %zu bytes of LDS per stream, the limit is %d", who, T, lds,
                RTK_SCORE_LDS_LIMIT);
    RTK_REQUIRE(lw_log_ok(lg), "%s: null or empty log", who);
    RTK_REQUIRE(lg->F <= IP_MAX_FRAMES, "%s: a log of F=%d frames per stream, the limit is %d", who, lg->F, IP_MAX_FRAMES);
    RTK_REQUIRE(lw_pairs_ok(pr), "%s: null or empty pair log", who);
    RTK_REQUIRE(alphas && counters && flags, "%s: null levels or null output", who);
    return RTK_OK;
}
