// score_log_walk.h -- what a kernel needs to walk the scorer's per-frame log (rtk_score_log_t, include/rtk_score.h), stated once:
// track_sweep.hip, track_hota.hip, track_identity.hip, track_optimal.hip, track_hota_optimal.hip and track_identity_pairs.hip replay
// the log with it, and a new replay kernel includes it and restates none of it.  Everything here is inlined into its caller, and the kernels' code is what it was when each
// file carried these lines itself.
//
//   lw_frame / lw_pair_frame   a frame slot of the log (and of the pair log), clamped to what the stream's log can hold
//   lw_frames                  the stream's frame count, clamped
//   lw_hash, LW_EMPTY, LW_SLOTS, lw_track_slot<INSERT>   the per-clip track table: open addressing, slots claimed by CAS
//   lw_pair_find / lw_pair_append <PSLOTS>               the (label entry, track slot) pair list with its lookup
//   lw_stays                   whether a detection remains at a threshold
//   lw_valid_pair<SIM>, LW_REMOVED  a logged pair as a valid pair of its frame, with its similarity (SIM: the one the log carries)
//   lw_log_ok / lw_pairs_ok    the host's check of a log / pair-log argument
//
// Three short loops stay in the kernels: a label id's entry in the label table, the first kept object with a label id, and the
// MT / PT / ML classification of a closing clip.  As functions they were inlined with the loop's exit behind its body where the
// kernels have it in front, which flipped branches in every kernel that took them ("The log walk").
#pragma once
#include "batch_common.h"
#include "rtk_common.h"
#include "rtk_score.h"

#define LW_EMPTY ((int)0x80000000)      // no track id (ids are >= -1 in every producer of the log)
// the track table: H = 1.5 * RTK_SCORE_SWEEP_TRACKS slots, linear probing; at most RTK_SCORE_SWEEP_TRACKS ids, so a third stays empty
#define LW_SLOTS (RTK_SCORE_SWEEP_TRACKS + RTK_SCORE_SWEEP_TRACKS / 2)

struct lw_frame_t { int rec, lab, P, G, reset; };
struct lw_pair_frame_t : lw_frame_t { int pair, pairs; };

// a frame slot of the log, its counts brought into what the stream's log can hold (a log is only ever written by ts_logged_kernel,
// which keeps these bounds; the clamps keep a foreign buffer from being read out of bounds)
__device__ __forceinline__ lw_frame_t lw_frame(const rtk_score_log_t &lg, int b, int f) {
    const int4 w = *reinterpret_cast<const int4 *>(lg.frame + ((size_t)b * lg.F + f) * 4);
    lw_frame_t fr;
    fr.reset = (w.z >> 16) & 1;
    fr.P = count_clamp(w.z & 0xffff, RTK_SCORE_MAX_OBJECTS);
    fr.G = count_clamp(w.w, RTK_SCORE_MAX_BOXES);
    fr.rec = count_clamp(w.x, lg.R - fr.P);
    fr.lab = count_clamp(w.y, lg.R - fr.G);
    if (fr.rec < 0) { fr.rec = 0; fr.P = 0; }
    if (fr.lab < 0) { fr.lab = 0; fr.G = 0; }
    return fr;
}

// the same slot with the frame's part of the pair log (rtk_score_pairs_t), clamped to what the stream's pair log can hold
__device__ __forceinline__ lw_pair_frame_t lw_pair_frame(const rtk_score_log_t &lg, const rtk_score_pairs_t &pr, int b, int f) {
    lw_pair_frame_t fr;
    static_cast<lw_frame_t &>(fr) = lw_frame(lg, b, f);
    const int *fp = pr.frame_pair + ((size_t)b * lg.F + f) * 2;
    fr.pairs = count_clamp(fp[1], pr.Q);
    fr.pair = count_clamp(fp[0], pr.Q - fr.pairs);
    return fr;
}

// the frames stream b has logged
__device__ __forceinline__ int lw_frames(const rtk_score_log_t &lg, int b) { return count_clamp(lg.cursor[b * 4 + 0], lg.F); }

__device__ __forceinline__ unsigned lw_hash(int id) { return ((unsigned)id * 2654435761u) >> 8; }

// the track table's slot of `id` (key[LW_SLOTS], LW_EMPTY where free; *used counts the ids); with INSERT an empty slot is claimed
// for it (at most RTK_SCORE_SWEEP_TRACKS ids: a third of the table stays empty, so a probe sequence ends).  -1: not there / no
// room -- lanes that lose a slot to one another count twice for a moment, so a clip within a wave's width of the limit may be
// refused as well; it is never accepted wrongly.
template <bool INSERT>
__device__ __forceinline__ int lw_track_slot(int *key, int *used, int id) {
    unsigned h = lw_hash(id) % LW_SLOTS;
    for (int probe = 0; probe < LW_SLOTS; ++probe, h = (h + 1) % LW_SLOTS) {
        int k = key[h];
        if (k == id) return (int)h;
        if (k != LW_EMPTY) continue;
        if (!INSERT) return -1;
        if (atomicAdd(used, 1) >= RTK_SCORE_SWEEP_TRACKS) return -1;
        k = atomicCAS(&key[h], LW_EMPTY, id);
        if (k == LW_EMPTY) return (int)h;
        atomicSub(used, 1);
        if (k == id) return (int)h;      // another lane claimed the slot for the same id: one slot per id
    }
    return -1;
}

// the pair lookup: ptab[PSLOTS] holds pair indices (-1 empty), the keys live in the insertion-ordered list.  -> the pair's index or -1
template <int PSLOTS>
__device__ __forceinline__ int lw_pair_find(const int *ptab, const int *pkey, int key) {
    unsigned h = lw_hash(key) % PSLOTS;
    for (int probe = 0; probe < PSLOTS; ++probe, h = (h + 1) % PSLOTS) {
        const int p = ptab[h];
        if (p < 0) return -1;
        if (pkey[p] == key) return p;
    }
    return -1;
}

// one thread appends `key` as pair p, the list's next index, with a count of 0 (the caller keeps p below PSLOTS / 2: half stays empty)
template <int PSLOTS>
__device__ __forceinline__ void lw_pair_append(int *ptab, int *pkey, int *pn, int p, int key) {
    pkey[p] = key; pn[p] = 0;
    unsigned h = lw_hash(key) % PSLOTS;
    while (ptab[h] >= 0) h = (h + 1) % PSLOTS;
    ptab[h] = p;
}

// whether a detection of this track score remains at threshold tau: a score equal to the threshold stays
__device__ __forceinline__ bool lw_stays(double score, double tau) { return !(score < tau); }

#define LW_REMOVED (-2)      // a detection's row word where its track score is below the threshold (any other value: it remains)

// a logged pair of frame `fr` as a VALID pair (include/rtk_score.h, "HOTA under the optimal matching"): its detection, its kept object
// and its similarity (double)c / (double)(|i| + |j| - c), unclamped -- or false: the pair does not describe its frame, its detection
// was removed (rrow[i] == LW_REMOVED), or there is no overlap (c <= 0, or a denominator that is not positive: coincident points count
// once per PAIR, so c may exceed a size).
// SIM: the log carries its pairs' similarity (pair_sim (B,Q), include/rtk_score.h, the last section) -- valid iff the key describes the
// frame, the detection remains and s = pair_sim[q] > 0.0 (a NaN is not); pair_common and the sizes are not read.  Without SIM pair_sim
// is not read and the function is what it was.
template <bool SIM = false>
__device__ __forceinline__ bool lw_valid_pair(const rtk_score_pairs_t &pr, const lw_pair_frame_t &fr, size_t rb, size_t qb, int p, const int *rrow,
                                              int *row, int *col, double *s, const double *pair_sim = nullptr) {
    if (SIM) {
        const int key = pr.pair_key[qb + fr.pair + p];
        const int i = key >> 8, j = key & 255;
        if (key < 0 || i >= fr.P || j >= fr.G || rrow[i] == LW_REMOVED) return false;
        const double v = pair_sim[qb + fr.pair + p];
        if (!(v > 0.0)) return false;
        *row = i; *col = j; *s = v;
        return true;
    }
    const int key = pr.pair_key[qb + fr.pair + p], c = pr.pair_common[qb + fr.pair + p];
    const int i = key >> 8, j = key & 255;
    if (key < 0 || i >= fr.P || j >= fr.G || c <= 0 || rrow[i] == LW_REMOVED) return false;
    const int si = pr.rec_size[rb + fr.rec + i], sj = pr.label_size[rb + fr.lab + j];
    const long long den = (long long)si + (long long)sj - (long long)c;
    if (den <= 0) return false;
    *row = i; *col = j; *s = (double)c / (double)den;
    return true;
}

// The pair log as a replay kernel's argument: the pair block and, with SIM, pair_sim right behind it.  One kernel template then has, for
// either value of SIM, exactly the argument segment of a kernel written for that value alone: a kernel without SIM carries no unused word.
template <bool SIM>
struct lw_pairs_arg_t {
    rtk_score_pairs_t pr;
    lw_pairs_arg_t(const rtk_score_pairs_t &p, const double *) : pr(p) {}
    __device__ const double *sim() const { return nullptr; }
};
template <>
struct lw_pairs_arg_t<true> {
    rtk_score_pairs_t pr;
    const double *pair_sim;
    lw_pairs_arg_t(const rtk_score_pairs_t &p, const double *s) : pr(p), pair_sim(s) {}
    __device__ const double *sim() const { return pair_sim; }
};

// host side: a log argument with every table present
static inline bool lw_log_ok(const rtk_score_log_t *lg) {
    return lg && lg->F >= 1 && lg->R >= 1 && lg->cursor && lg->frame && lg->label && lg->rec_track && lg->rec_best && lg->rec_conf && lg->rec_iou;
}

// host side: a pair-log argument with every table present
static inline bool lw_pairs_ok(const rtk_score_pairs_t *pr) {
    return pr && pr->Q >= 1 && pr->cursor && pr->frame_pair && pr->pair_key && pr->pair_common && pr->rec_size && pr->label_size;
}
