// track_identity.hip -- the identity metrics IDF1, IDP and IDR over the scorer's per-frame log (include/rtk_score.h, the definitions
// are stated there; ratrack_amd/track_score.py, TrackScorer.identity).
//
//   rtk_score_identity   one wave per (stream, level): the stream's log walked frame by frame as rtk_score_hota walks it, with the
//                        detections below the threshold removed; per clip a label table, a track table and the list of (label, track)
//                        pairs with the number of frames in which a candidate of that track had that label as its best object; when
//                        the clip closes, the weight of a maximum-weight one-to-one matching of its labels and tracks
//                        (lds_assignment.h) is added to idtp
//
// As in track_hota.hip the log holds a few detections per frame and the kernel is latency bound and kept simple: whatever has an order
// (the label table, the pair insertions) is one thread in that order; the lanes fetch, probe and look up, and solve the assignment
// together.  Integers only: the same numbers on every run.  gt and pred are running sums, so the tables carry neither per-id counts
// nor float64 scratch, and every table of the walk except the pair list is dead when a clip closes: the solver works in their place.
// The frame decode, the track table and the pair list are score_log_walk.h's.
#include "lds_assignment.h"
#include "score_log_walk.h"

#define ID_SLOTS LW_SLOTS                                                   // the track table
#define ID_PSLOTS (2 * RTK_SCORE_ID_PAIRS)                                  // the pair lookup: half stays empty
#define ID_SLOT_BITS LA_COL_BITS                                            // a pair's key: label entry << 12 | track slot
#define ID_SLOT_MASK ((1 << ID_SLOT_BITS) - 1)
#define ID_MAX_FRAMES (1 << 28)                                             // a pair's weight is at most the frames of its clip
static_assert(ID_SLOTS <= (1 << ID_SLOT_BITS), "a track slot must fit the pair key");
static_assert(RTK_SCORE_ID_PAIRS <= (1 << ID_SLOT_BITS), "a compacted track index must fit the pair key");

// LDS, in ints.  The pair list (key, n) comes first and lives through the clip's close; behind it EITHER the walk's tables -- label
// table [TCAP] | track table [ID_SLOTS] | pair lookup [ID_PSLOTS] | rkey, rpair [MAX_OBJECTS] | glabel, entry [MAX_BOXES] | 8 scalars --
// OR the solver's (TCAP rows, at most PAIRS columns and edges).
constexpr int id_walk_words(int TCAP) { return TCAP + ID_SLOTS + ID_PSLOTS + 2 * RTK_SCORE_MAX_OBJECTS + 2 * RTK_SCORE_MAX_BOXES + 8; }
constexpr int id_words(int TCAP) {
    return 2 * RTK_SCORE_ID_PAIRS + (id_walk_words(TCAP) > la_words(TCAP, RTK_SCORE_ID_PAIRS, RTK_SCORE_ID_PAIRS)
                                         ? id_walk_words(TCAP)
                                         : la_words(TCAP, RTK_SCORE_ID_PAIRS, RTK_SCORE_ID_PAIRS));
}
// The label capacities the kernel is built for: a T takes the smallest that holds it.  Static LDS, so the code object states each figure.
#define ID_TCAP_SMALL 1024
#define ID_TCAP_LARGE 3583      // the most that fits the limit
static_assert(id_words(ID_TCAP_LARGE) * sizeof(int) <= RTK_SCORE_LDS_LIMIT && id_words(ID_TCAP_LARGE + 1) * sizeof(int) > RTK_SCORE_LDS_LIMIT,
              "the large instance is the largest that fits one workgroup's LDS");

static size_t id_lds(int T) {
    if (T <= ID_TCAP_SMALL) return id_words(ID_TCAP_SMALL) * sizeof(int);
    if (T <= ID_TCAP_LARGE) return id_words(ID_TCAP_LARGE) * sizeof(int);
    return ((size_t)2 * T + 1 + 9 * RTK_SCORE_ID_PAIRS) * sizeof(int);      // the pair list and la_words(T, PAIRS, PAIRS): past the limit
}

enum { ID_S_LABELS = 0, ID_S_TRACKS = 1, ID_S_PAIRS = 2, ID_S_OVERFLOW = 3 };

template <int TCAP>
__global__ __launch_bounds__(RTK_WAVE) void identity_kernel(int T, const rtk_score_log_t lg, const double *rec_score, const double *threshold,
                                                            const double *alphas, long long *counters, int *flags) {
    __shared__ __attribute__((aligned(16))) int id_smem[id_words(TCAP)];
    const int b = blockIdx.x, a = blockIdx.y, B = gridDim.x, t = threadIdx.x;
    int *pkey = id_smem, *pn = pkey + RTK_SCORE_ID_PAIRS, *work = pn + RTK_SCORE_ID_PAIRS;
    int *lkey = work, *tkey = lkey + TCAP, *ptab = tkey + ID_SLOTS;
    int *rkey = ptab + ID_PSLOTS, *rpair = rkey + RTK_SCORE_MAX_OBJECTS;
    int *glabel = rpair + RTK_SCORE_MAX_OBJECTS, *entry = glabel + RTK_SCORE_MAX_BOXES, *scal = entry + RTK_SCORE_MAX_BOXES;

    const double alpha = alphas[a];
    const bool filter = rec_score != nullptr && threshold != nullptr;
    const double tau = filter ? *threshold : 0.0;
    const int frames = lw_frames(lg, b);
    const size_t rb = (size_t)b * lg.R;
    long long c_frames = 0, c_clips = 0, c_gt = 0, c_pred = 0, c_idtp = 0, c_pairs = 0;      // uniform: every lane counts them alike
    int used = 0, npairs = 0, overflow = 0;      // uniform: thread 0 publishes them through scal

    for (int h = t; h < ID_SLOTS; h += RTK_WAVE) tkey[h] = LW_EMPTY;
    for (int h = t; h < ID_PSLOTS; h += RTK_WAVE) ptab[h] = -1;
    if (t < 8) scal[t] = 0;
    __syncthreads();

    for (int f = 0; f <= frames; ++f) {
        lw_frame_t fr = {};
        if (f < frames) fr = lw_frame(lg, b, f);
        if ((f == frames || fr.reset) && f > 0) {
            // ---- the clip closes.  The tracks that appear in a pair are numbered 0, 1, ... in the order of their first pair: the
            //      track table gives way to "first pair of this slot", the pair lookup to that pair's number ----
            overflow |= scal[ID_S_OVERFLOW];
            __syncthreads();
            for (int h = t; h < ID_SLOTS; h += RTK_WAVE) tkey[h] = LA_INF;
            __syncthreads();
            for (int p = t; p < npairs; p += RTK_WAVE) atomicMin(&tkey[pkey[p] & ID_SLOT_MASK], p);
            __syncthreads();
            int ncols = 0;
            for (int base = 0; base < npairs; base += RTK_WAVE) {
                const int p = base + t;
                const bool first = p < npairs && tkey[pkey[p] & ID_SLOT_MASK] == p;
                const unsigned long long firsts = __ballot(first);
                if (first) ptab[p] = ncols + __popcll(firsts & ((1ull << t) - 1ull));
                ncols += __popcll(firsts);
            }
            __syncthreads();
            for (int p = t; p < npairs; p += RTK_WAVE) {
                const int key = pkey[p];
                pkey[p] = (key & ~ID_SLOT_MASK) | ptab[tkey[key & ID_SLOT_MASK]];
            }
            __syncthreads();
            c_idtp += la_solve(used, ncols, npairs, pkey, pn, work);
            c_clips += 1; c_pairs += npairs;
            __syncthreads();
            for (int h = t; h < ID_SLOTS; h += RTK_WAVE) tkey[h] = LW_EMPTY;
            for (int h = t; h < ID_PSLOTS; h += RTK_WAVE) ptab[h] = -1;
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
                if (used >= min(T, TCAP)) { scal[ID_S_OVERFLOW] = 1; continue; }      // the label stays without an entry: its pairs go uncounted
                lkey[used] = glabel[j];
                entry[j] = used++;
            }
            scal[ID_S_LABELS] = used;
        }
        __syncthreads();
        used = scal[ID_S_LABELS];
        c_frames += 1; c_gt += fr.G;
        // ---- the remaining detections: their track slot and, for a candidate at this level, the pair's key and its place in the list ----
        for (int base = 0; base < fr.P; base += RTK_WAVE) {
            const int i = base + t;
            bool stays = false;
            if (i < fr.P) {
                const size_t r = rb + fr.rec + i;
                stays = !filter || lw_stays(rec_score[r], tau);
                int key = -1;
                if (stays) {
                    const int s = lw_track_slot<true>(tkey, &scal[ID_S_TRACKS], lg.rec_track[r]);
                    if (s < 0) scal[ID_S_OVERFLOW] = 1;
                    const int lab = lg.rec_best[r];
                    if (s >= 0 && lab != -1 && lg.rec_iou[r] >= alpha) {
                        int j = -1;
                        for (int k = fr.G - 1; k >= 0; --k)
                            if (glabel[k] == lab) j = k;
                        if (j >= 0 && entry[j] >= 0) key = (entry[j] << ID_SLOT_BITS) | s;
                    }
                }
                rkey[i] = key;
                rpair[i] = key < 0 ? -1 : lw_pair_find<ID_PSLOTS>(ptab, pkey, key);
            }
            c_pred += __popcll(__ballot(stays));
        }
        __syncthreads();
        // a pair counts a frame once: a later detection of the frame with the same key (a log whose track ids repeat within a frame) is set aside
        for (int i = t; i < fr.P; i += RTK_WAVE) {
            const int key = rkey[i];
            if (key < 0) continue;
            for (int k = 0; k < i; ++k)
                if (rkey[k] == key) rpair[i] = -2;
        }
        __syncthreads();
        // ---- thread 0 counts the frame's pairs, new ones appended in detection order ----
        if (t == 0) {
            for (int i = 0; i < fr.P; ++i) {
                const int key = rkey[i];
                int p = rpair[i];
                if (key < 0 || p == -2) continue;
                if (p < 0) {
                    if (npairs >= RTK_SCORE_ID_PAIRS) { scal[ID_S_OVERFLOW] = 1; continue; }
                    p = npairs++;
                    lw_pair_append<ID_PSLOTS>(ptab, pkey, pn, p, key);      // at most PAIRS of 2 PAIRS slots are taken
                }
                pn[p] += 1;
            }
            scal[ID_S_PAIRS] = npairs;
        }
        __syncthreads();
        npairs = scal[ID_S_PAIRS];
    }
    if (t == 0) {
        long long *cnt = counters + ((size_t)a * B + b) * RTK_SCORE_ID_COUNTERS;
        cnt[0] = c_frames; cnt[1] = c_clips; cnt[2] = c_gt; cnt[3] = c_pred; cnt[4] = c_idtp; cnt[5] = c_pairs;
        if (overflow | scal[ID_S_OVERFLOW]) atomicOr(&flags[b], RTK_SCORE_FLAG_IDENTITY);
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
extern "C" int rtk_score_identity_lds_bytes(int T) {
    if (T < 1 || T > (1 << 24)) return -1;
    return (int)id_lds(T);
}

extern "C" int rtk_score_identity(int B, int T, const rtk_score_log_t *lg, const double *rec_score, const double *threshold, const double *alphas,
                                  int count, long long *counters, int *flags, rtk_stream_t stream) {
    RTK_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && T <= (1 << 24) && count >= 1 && count <= 63, "score_identity: bad sizes B=%d T=%d count=%d", B, T,
                count);
    const size_t lds = id_lds(T);
    RTK_REQUIRE(lds <= RTK_SCORE_LDS_LIMIT, "score_identity: T=%d label-table entries need %zu bytes of LDS per stream, the limit is %d", T, lds,
                RTK_SCORE_LDS_LIMIT);
    RTK_REQUIRE(lw_log_ok(lg), "score_identity: null or empty log");
    RTK_REQUIRE(lg->F <= ID_MAX_FRAMES, "score_identity: a log of F=%d frames per stream, the limit is %d", lg->F, ID_MAX_FRAMES);
    RTK_REQUIRE(alphas && counters && flags, "score_identity: null levels or null output");
    if (T <= ID_TCAP_SMALL)
        identity_kernel<ID_TCAP_SMALL><<<dim3(B, count), RTK_WAVE, 0, (hipStream_t)stream>>>(T, *lg, rec_score, threshold, alphas, counters, flags);
    else
        identity_kernel<ID_TCAP_LARGE><<<dim3(B, count), RTK_WAVE, 0, (hipStream_t)stream>>>(T, *lg, rec_score, threshold, alphas, counters, flags);
    RTK_CHECK_LAUNCH("score_identity");
    return RTK_OK;
}
