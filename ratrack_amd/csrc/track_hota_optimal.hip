// track_hota_optimal.hip -- HOTA under TrackEval's matching over the scorer's two logs (include/rtk_score.h, "HOTA under the optimal
// matching": the definitions are stated there; ratrack_amd/track_score.py, TrackScorer.hota(matching="optimal")).
//
//   rtk_score_alignment      one wave per stream: the log walked once, clip by clip, with a label table (frames seen), a track table
//                            (remaining detections) and the insertion-ordered list of the clip's potential (label, track) pairs with
//                            their float64 sums of normalised overlap; when a clip closes its frames are walked a second time and
//                            every logged pair receives the global alignment score A of its (label, track).  It also leaves, per
//                            logged pair, the index of its (label, track) in a per-stream table of clip-pairs, and per clip-pair its
//                            cg and ct: the second kernel needs neither a label table nor a track table
//   rtk_score_hota_optimal   one wave per (stream, alpha): per frame ONE maximum-weight assignment (lds_assignment.h) over the valid
//                            pairs, weight max(1, floor(min(A * min(s, 1), 1) * 2^28)); the matched pairs with s >= alpha are the true
//                            positives, counted per clip-pair index and folded into the association sums when the clip closes
//
// As in track_hota.hip and track_optimal.hip the log holds a few detections per frame and the kernels are latency bound and kept
// simple: whatever has an order (a float64 sum, an insertion) is one thread in that order; the lanes fetch, test the pairs, look up and
// solve the assignment together.  Integers and fixed-order float64 sums only: the same bits on every run, and the bits of a host loop
// written from the definitions.  Every level re-solves the same assignment: the grid fills the device with it (DESIGN.md section 4.9
// has the measured cost).  The frame decode, the track table, the pair list and the valid-pair test are score_log_walk.h's.
// The LDS layouts and the bodies are track_hota_optimal_body.h's, instantiated here on the point IoU of the logged integers.
#include "track_hota_optimal_body.h"

template <int TCAP>
__global__ __launch_bounds__(RTK_WAVE) void alignment_kernel(int T, const rtk_score_log_t lg, const rtk_score_pairs_t pr, const double *rec_score,
                                                             const double *threshold, double *pair_a, int *pair_index, int *clip_cg, int *clip_ct,
                                                             int *flags) {
    __shared__ __attribute__((aligned(16))) int al_smem[al_words(TCAP)];
    alignment_body<TCAP, false>(al_smem, T, lg, pr, rec_score, threshold, pair_a, pair_index, clip_cg, clip_ct, flags, nullptr);
}

__global__ __launch_bounds__(RTK_WAVE) void hota_optimal_kernel(const rtk_score_log_t lg, const rtk_score_pairs_t pr, const double *rec_score,
                                                                const double *threshold, const double *pair_a, const int *pair_index,
                                                                const int *clip_cg, const int *clip_ct, long long *counters, double *sums, int *flags) {
    __shared__ __attribute__((aligned(16))) int ho_smem[ho_words()];
    hota_optimal_body<false>(ho_smem, lg, pr, rec_score, threshold, pair_a, pair_index, clip_cg, clip_ct, counters, sums, flags, nullptr);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
extern "C" int rtk_score_alignment_lds_bytes(int T) {
    if (T < 1 || T > (1 << 24)) return -1;
    return (int)al_lds(T);
}

extern "C" int rtk_score_alignment(int B, int T, const rtk_score_log_t *lg, const rtk_score_pairs_t *pr, const double *rec_score,
                                   const double *threshold, double *pair_a, int *pair_index, int *clip_cg, int *clip_ct, int *flags,
                                   rtk_stream_t stream) {
    const int status = al_validate("score_alignment", B, T, lg, pr, pair_a, pair_index, clip_cg, clip_ct, flags);
    if (status != RTK_OK) return status;
    if (T <= AL_TCAP_SMALL)
        alignment_kernel<AL_TCAP_SMALL><<<B, RTK_WAVE, 0, (hipStream_t)stream>>>(T, *lg, *pr, rec_score, threshold, pair_a, pair_index, clip_cg, clip_ct,
                                                                                  flags);
    else
        alignment_kernel<AL_TCAP_LARGE><<<B, RTK_WAVE, 0, (hipStream_t)stream>>>(T, *lg, *pr, rec_score, threshold, pair_a, pair_index, clip_cg, clip_ct,
                                                                                  flags);
    RTK_CHECK_LAUNCH("score_alignment");
    return RTK_OK;
}

extern "C" int rtk_score_hota_optimal(int B, const rtk_score_log_t *lg, const rtk_score_pairs_t *pr, const double *rec_score, const double *threshold,
                                      int alphas, const double *pair_a, const int *pair_index, const int *clip_cg, const int *clip_ct,
                                      long long *counters, double *sums, int *flags, rtk_stream_t stream) {
    const int status = ho_validate("score_hota_optimal", B, lg, pr, alphas, pair_a, pair_index, clip_cg, clip_ct, counters, sums, flags);
    if (status != RTK_OK) return status;
    hota_optimal_kernel<<<dim3(B, alphas), RTK_WAVE, 0, (hipStream_t)stream>>>(*lg, *pr, rec_score, threshold, pair_a, pair_index, clip_cg, clip_ct,
                                                                                counters, sums, flags);
    RTK_CHECK_LAUNCH("score_hota_optimal");
    return RTK_OK;
}
