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
// The LDS layouts and the bodies are track_hota_optimal_body.h's, instantiated here twice: on the point IoU of the logged integers
// (rtk_score_alignment, rtk_score_hota_optimal) and, SIM, on the similarity the pair log itself carries (rtk_score_alignment_sim,
// rtk_score_hota_optimal_sim; track_optimal.hip's header has the rule).  The same LDS tables, grids and arithmetic either way.
#include "track_hota_optimal_body.h"

template <int TCAP, bool SIM>
__global__ __launch_bounds__(RTK_WAVE) void alignment_kernel(int T, const rtk_score_log_t lg, const lw_pairs_arg_t<SIM> pa,
                                                             const double *rec_score, const double *threshold, double *pair_a, int *pair_index,
                                                             int *clip_cg, int *clip_ct, int *flags) {
    __shared__ __attribute__((aligned(16))) int al_smem[al_words(TCAP)];
    alignment_body<TCAP, SIM>(al_smem, T, lg, pa.pr, rec_score, threshold, pair_a, pair_index, clip_cg, clip_ct, flags, pa.sim());
}

template <bool SIM>
__global__ __launch_bounds__(RTK_WAVE) void hota_optimal_kernel(const rtk_score_log_t lg, const lw_pairs_arg_t<SIM> pa,
                                                                const double *rec_score, const double *threshold, const double *pair_a,
                                                                const int *pair_index, const int *clip_cg, const int *clip_ct, long long *counters,
                                                                double *sums, int *flags) {
    __shared__ __attribute__((aligned(16))) int ho_smem[ho_words()];
    hota_optimal_body<SIM>(ho_smem, lg, pa.pr, rec_score, threshold, pair_a, pair_index, clip_cg, clip_ct, counters, sums, flags, pa.sim());
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
extern "C" int rtk_score_alignment_lds_bytes(int T) {
    if (T < 1 || T > (1 << 24)) return -1;
    return (int)al_lds(T);
}

// name: the entry point's, for its messages; SIM: the pass on pair_sim, refused when that is NULL
template <bool SIM>
static int al_launch(const char *name, int B, int T, const rtk_score_log_t *lg, const rtk_score_pairs_t *pr, const double *pair_sim,
                     const double *rec_score, const double *threshold, double *pair_a, int *pair_index, int *clip_cg, int *clip_ct, int *flags,
                     rtk_stream_t stream) {
    const int status = al_validate(name, B, T, lg, pr, pair_a, pair_index, clip_cg, clip_ct, flags);
    if (status != RTK_OK) return status;
    if (SIM) RTK_REQUIRE(pair_sim, "%s: null pair_sim", name);
    const auto kernel = T <= AL_TCAP_SMALL ? alignment_kernel<AL_TCAP_SMALL, SIM> : alignment_kernel<AL_TCAP_LARGE, SIM>;
    kernel<<<B, RTK_WAVE, 0, (hipStream_t)stream>>>(T, *lg, lw_pairs_arg_t<SIM>(*pr, pair_sim), rec_score, threshold, pair_a, pair_index, clip_cg, clip_ct,
                                                    flags);
    RTK_CHECK_LAUNCH(name);
    return RTK_OK;
}

template <bool SIM>
static int ho_launch(const char *name, int B, const rtk_score_log_t *lg, const rtk_score_pairs_t *pr, const double *pair_sim, const double *rec_score,
                     const double *threshold, int alphas, const double *pair_a, const int *pair_index, const int *clip_cg, const int *clip_ct,
                     long long *counters, double *sums, int *flags, rtk_stream_t stream) {
    const int status = ho_validate(name, B, lg, pr, alphas, pair_a, pair_index, clip_cg, clip_ct, counters, sums, flags);
    if (status != RTK_OK) return status;
    if (SIM) RTK_REQUIRE(pair_sim, "%s: null pair_sim", name);
    hota_optimal_kernel<SIM><<<dim3(B, alphas), RTK_WAVE, 0, (hipStream_t)stream>>>(*lg, lw_pairs_arg_t<SIM>(*pr, pair_sim), rec_score, threshold, pair_a,
                                                                                     pair_index, clip_cg, clip_ct, counters, sums, flags);
    RTK_CHECK_LAUNCH(name);
    return RTK_OK;
}

extern "C" int rtk_score_alignment(int B, int T, const rtk_score_log_t *lg, const rtk_score_pairs_t *pr, const double *rec_score,
                                   const double *threshold, double *pair_a, int *pair_index, int *clip_cg, int *clip_ct, int *flags,
                                   rtk_stream_t stream) {
    return al_launch<false>("score_alignment", B, T, lg, pr, nullptr, rec_score, threshold, pair_a, pair_index, clip_cg, clip_ct, flags, stream);
}

extern "C" int rtk_score_alignment_sim(int B, int T, const rtk_score_log_t *lg, const rtk_score_pairs_t *pr, const double *pair_sim,
                                       const double *rec_score, const double *threshold, double *pair_a, int *pair_index, int *clip_cg, int *clip_ct,
                                       int *flags, rtk_stream_t stream) {
    return al_launch<true>("score_alignment_sim", B, T, lg, pr, pair_sim, rec_score, threshold, pair_a, pair_index, clip_cg, clip_ct, flags, stream);
}

extern "C" int rtk_score_hota_optimal(int B, const rtk_score_log_t *lg, const rtk_score_pairs_t *pr, const double *rec_score, const double *threshold,
                                      int alphas, const double *pair_a, const int *pair_index, const int *clip_cg, const int *clip_ct,
                                      long long *counters, double *sums, int *flags, rtk_stream_t stream) {
    return ho_launch<false>("score_hota_optimal", B, lg, pr, nullptr, rec_score, threshold, alphas, pair_a, pair_index, clip_cg, clip_ct, counters, sums,
                            flags, stream);
}

extern "C" int rtk_score_hota_optimal_sim(int B, const rtk_score_log_t *lg, const rtk_score_pairs_t *pr, const double *pair_sim, const double *rec_score,
                                          const double *threshold, int alphas, const double *pair_a, const int *pair_index, const int *clip_cg,
                                          const int *clip_ct, long long *counters, double *sums, int *flags, rtk_stream_t stream) {
    return ho_launch<true>("score_hota_optimal_sim", B, lg, pr, pair_sim, rec_score, threshold, alphas, pair_a, pair_index, clip_cg, clip_ct, counters,
                           sums, flags, stream);
}
