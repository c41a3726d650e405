// track_replay_sim.hip -- the four replays of the pair log on the similarity the log itself carries (include/rtk_score.h, "TrackEval's
// centre-distance similarity": rtk_score_replay_optimal_sim, rtk_score_alignment_sim, rtk_score_hota_optimal_sim and
// rtk_score_identity_pairs_sim; ratrack_amd/track_score.py, TrackScorer(similarity="centre")).
//
// The bodies are those of track_optimal.hip, track_hota_optimal.hip and track_identity_pairs.hip (their *_body.h), instantiated with the
// similarity switch on: a logged pair is valid iff its key describes its frame, its detection remains and s = pair_sim[q] > 0, and
// wherever those kernels form the point IoU of the logged integers these read s; pair_common and the sizes are not read.  The same LDS
// tables, hence the same static LDS figures, one wave of 64 threads each, the same grids, integers and fixed-order float64 sums: the same
// bits on every run.  The kernels here have names of their own, so the code objects of the three files above stay what they are.
#include "track_hota_optimal_body.h"
#include "track_identity_pairs_body.h"
#include "track_optimal_body.h"

template <int TCAP>
__global__ __launch_bounds__(RTK_WAVE) void optimal_replay_sim_kernel(int T, const rtk_score_log_t lg, const rtk_score_pairs_t pr, const double *pair_sim,
                                                                      const double *rec_score, const double *thresholds, const int *reached,
                                                                      double min_iou, long long *counters, long long *iou_qs, double *iou_sums,
                                                                      unsigned char *tp_mask, int *flags) {
    __shared__ __attribute__((aligned(16))) int op_smem[op_words(TCAP)];
    optimal_replay_body<TCAP, true>(op_smem, T, lg, pr, rec_score, thresholds, reached, min_iou, counters, iou_qs, iou_sums, tp_mask, flags, pair_sim);
}

template <int TCAP>
__global__ __launch_bounds__(RTK_WAVE) void alignment_sim_kernel(int T, const rtk_score_log_t lg, const rtk_score_pairs_t pr, const double *pair_sim,
                                                                 const double *rec_score, const double *threshold, double *pair_a, int *pair_index,
                                                                 int *clip_cg, int *clip_ct, int *flags) {
    __shared__ __attribute__((aligned(16))) int al_smem[al_words(TCAP)];
    alignment_body<TCAP, true>(al_smem, T, lg, pr, rec_score, threshold, pair_a, pair_index, clip_cg, clip_ct, flags, pair_sim);
}

__global__ __launch_bounds__(RTK_WAVE) void hota_optimal_sim_kernel(const rtk_score_log_t lg, const rtk_score_pairs_t pr, const double *pair_sim,
                                                                    const double *rec_score, const double *threshold, const double *pair_a,
                                                                    const int *pair_index, const int *clip_cg, const int *clip_ct, long long *counters,
                                                                    double *sums, int *flags) {
    __shared__ __attribute__((aligned(16))) int ho_smem[ho_words()];
    hota_optimal_body<true>(ho_smem, lg, pr, rec_score, threshold, pair_a, pair_index, clip_cg, clip_ct, counters, sums, flags, pair_sim);
}

template <int TCAP>
__global__ __launch_bounds__(RTK_WAVE) void identity_pairs_sim_kernel(int T, const rtk_score_log_t lg, const rtk_score_pairs_t pr, const double *pair_sim,
                                                                      const double *rec_score, const double *threshold, const double *alphas,
                                                                      long long *counters, int *flags) {
    __shared__ __attribute__((aligned(16))) int ip_smem[ip_words(TCAP)];
    identity_pairs_body<TCAP, true>(ip_smem, T, lg, pr, rec_score, threshold, alphas, counters, flags, pair_sim);
}

// ------------------------------------------------------------------------------------------------
// host side: the checks of the plain entry points, and the similarity
// ------------------------------------------------------------------------------------------------
extern "C" int rtk_score_replay_optimal_sim(int B, int T, const rtk_score_log_t *lg, const rtk_score_pairs_t *pr, const double *pair_sim,
                                            const double *rec_score, const double *thresholds, const int *reached, int count, double min_iou,
                                            long long *counters, long long *iou_q, double *iou_sum, unsigned char *tp_mask, int *flags,
                                            rtk_stream_t stream) {
    const int status = op_validate("score_replay_optimal_sim", B, T, lg, pr, rec_score, thresholds, count, min_iou, counters, iou_q, iou_sum, flags);
    if (status != RTK_OK) return status;
    RTK_REQUIRE(pair_sim, "score_replay_optimal_sim: null pair_sim");
    if (T <= OP_TCAP_SMALL)
        optimal_replay_sim_kernel<OP_TCAP_SMALL><<<dim3(B, count), RTK_WAVE, 0, (hipStream_t)stream>>>(T, *lg, *pr, pair_sim, rec_score, thresholds, reached,
                                                                                                       min_iou, counters, iou_q, iou_sum, tp_mask, flags);
    else
        optimal_replay_sim_kernel<OP_TCAP_LARGE><<<dim3(B, count), RTK_WAVE, 0, (hipStream_t)stream>>>(T, *lg, *pr, pair_sim, rec_score, thresholds, reached,
                                                                                                       min_iou, counters, iou_q, iou_sum, tp_mask, flags);
    RTK_CHECK_LAUNCH("score_replay_optimal_sim");
    return RTK_OK;
}

extern "C" int rtk_score_alignment_sim(int B, int T, const rtk_score_log_t *lg, const rtk_score_pairs_t *pr, const double *pair_sim,
                                       const double *rec_score, const double *threshold, double *pair_a, int *pair_index, int *clip_cg, int *clip_ct,
                                       int *flags, rtk_stream_t stream) {
    const int status = al_validate("score_alignment_sim", B, T, lg, pr, pair_a, pair_index, clip_cg, clip_ct, flags);
    if (status != RTK_OK) return status;
    RTK_REQUIRE(pair_sim, "score_alignment_sim: null pair_sim");
    if (T <= AL_TCAP_SMALL)
        alignment_sim_kernel<AL_TCAP_SMALL><<<B, RTK_WAVE, 0, (hipStream_t)stream>>>(T, *lg, *pr, pair_sim, rec_score, threshold, pair_a, pair_index, clip_cg,
                                                                                      clip_ct, flags);
    else
        alignment_sim_kernel<AL_TCAP_LARGE><<<B, RTK_WAVE, 0, (hipStream_t)stream>>>(T, *lg, *pr, pair_sim, rec_score, threshold, pair_a, pair_index, clip_cg,
                                                                                      clip_ct, flags);
    RTK_CHECK_LAUNCH("score_alignment_sim");
    return RTK_OK;
}

extern "C" int rtk_score_hota_optimal_sim(int B, const rtk_score_log_t *lg, const rtk_score_pairs_t *pr, const double *pair_sim, const double *rec_score,
                                          const double *threshold, int alphas, const double *pair_a, const int *pair_index, const int *clip_cg,
                                          const int *clip_ct, long long *counters, double *sums, int *flags, rtk_stream_t stream) {
    const int status = ho_validate("score_hota_optimal_sim", B, lg, pr, alphas, pair_a, pair_index, clip_cg, clip_ct, counters, sums, flags);
    if (status != RTK_OK) return status;
    RTK_REQUIRE(pair_sim, "score_hota_optimal_sim: null pair_sim");
    hota_optimal_sim_kernel<<<dim3(B, alphas), RTK_WAVE, 0, (hipStream_t)stream>>>(*lg, *pr, pair_sim, rec_score, threshold, pair_a, pair_index, clip_cg,
                                                                                    clip_ct, counters, sums, flags);
    RTK_CHECK_LAUNCH("score_hota_optimal_sim");
    return RTK_OK;
}

extern "C" int rtk_score_identity_pairs_sim(int B, int T, const rtk_score_log_t *lg, const rtk_score_pairs_t *pr, const double *pair_sim,
                                            const double *rec_score, const double *threshold, const double *alphas, int count, long long *counters,
                                            int *flags, rtk_stream_t stream) {
    const int status = ip_validate("score_identity_pairs_sim", B, T, lg, pr, alphas, count, counters, flags);
    if (status != RTK_OK) return status;
    RTK_REQUIRE(pair_sim, "score_identity_pairs_sim: null pair_sim");
    if (T <= IP_TCAP_SMALL)
        identity_pairs_sim_kernel<IP_TCAP_SMALL><<<dim3(B, count), RTK_WAVE, 0, (hipStream_t)stream>>>(T, *lg, *pr, pair_sim, rec_score, threshold, alphas,
                                                                                                       counters, flags);
    else
        identity_pairs_sim_kernel<IP_TCAP_LARGE><<<dim3(B, count), RTK_WAVE, 0, (hipStream_t)stream>>>(T, *lg, *pr, pair_sim, rec_score, threshold, alphas,
                                                                                                       counters, flags);
    RTK_CHECK_LAUNCH("score_identity_pairs_sim");
    return RTK_OK;
}
