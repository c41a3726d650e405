// track_optimal.hip -- the replay of the scorer's log under a per-frame OPTIMAL matching at an IoU threshold: the KITTI / AB3DMOT
// matching scheme on the reference's point IoU (include/rtk_score.h, the definitions are stated there; ratrack_amd/track_score.py,
// TrackScorer.sweep(matching="optimal") and TrackScorer.clear_optimal).
//
//   rtk_score_replay_optimal   one wave per (stream, threshold): the stream's log walked frame by frame as rtk_score_replay walks it,
//                              with the detections below the threshold removed; the frame's logged pairs (rtk_score_pairs_t) at or
//                              above min_iou are the edges of one maximum-weight assignment (lds_assignment.h), weight
//                              2^23 + min(floor(iou * 65536), 65536): most matches first, then the largest quantised IoU sum
//
// As in track_sweep.hip the log holds a few detections per frame and the kernel is latency bound and kept simple: whatever has an
// order (the IoU sum, the track table) is one thread in that order; the lanes fetch, test the pairs and solve the assignment together.
// Integers and one fixed-order float64 sum: the same bits on every run.  The frame decode of the two logs is score_log_walk.h's.
// The LDS layout and the body are track_optimal_body.h's, instantiated here twice: on the point IoU of the logged integers
// (rtk_score_replay_optimal) and, SIM, on the similarity the pair log itself carries (rtk_score_replay_optimal_sim; include/rtk_score.h,
// "TrackEval's centre-distance similarity"): a logged pair is then valid iff its key describes its frame, its detection remains and
// s = pair_sim[q] > 0, and wherever the kernel forms the point IoU it reads s; pair_common and the sizes are not read.  The same LDS
// tables, grid and arithmetic either way.
#include "track_optimal_body.h"

template <int TCAP, bool SIM>
__global__ __launch_bounds__(RTK_WAVE) void optimal_replay_kernel(int T, const rtk_score_log_t lg, const lw_pairs_arg_t<SIM> pa,
                                                                  const double *rec_score, const double *thresholds, const int *reached,
                                                                  double min_iou, long long *counters, long long *iou_qs, double *iou_sums,
                                                                  unsigned char *tp_mask, int *flags) {
    __shared__ __attribute__((aligned(16))) int op_smem[op_words(TCAP)];
    optimal_replay_body<TCAP, SIM>(op_smem, T, lg, pa.pr, rec_score, thresholds, reached, min_iou, counters, iou_qs, iou_sums, tp_mask, flags, pa.sim());
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
extern "C" int rtk_score_optimal_lds_bytes(int T) {
    if (T < 1 || T > (1 << 24)) return -1;
    return (int)op_lds(T);
}

// name: the entry point's, for its messages; SIM: the replay on pair_sim, refused when that is NULL
template <bool SIM>
static int op_launch(const char *name, int B, int T, const rtk_score_log_t *lg, const rtk_score_pairs_t *pr, const double *pair_sim,
                     const double *rec_score, const double *thresholds, const int *reached, int count, double min_iou, long long *counters,
                     long long *iou_q, double *iou_sum, unsigned char *tp_mask, int *flags, rtk_stream_t stream) {
    const int status = op_validate(name, B, T, lg, pr, rec_score, thresholds, count, min_iou, counters, iou_q, iou_sum, flags);
    if (status != RTK_OK) return status;
    if (SIM) RTK_REQUIRE(pair_sim, "%s: null pair_sim", name);
    const auto kernel = T <= OP_TCAP_SMALL ? optimal_replay_kernel<OP_TCAP_SMALL, SIM> : optimal_replay_kernel<OP_TCAP_LARGE, SIM>;
    kernel<<<dim3(B, count), RTK_WAVE, 0, (hipStream_t)stream>>>(T, *lg, lw_pairs_arg_t<SIM>(*pr, pair_sim), rec_score, thresholds, reached, min_iou,
                                                                 counters, iou_q, iou_sum, tp_mask, flags);
    RTK_CHECK_LAUNCH(name);
    return RTK_OK;
}

extern "C" int rtk_score_replay_optimal(int B, int T, const rtk_score_log_t *lg, const rtk_score_pairs_t *pr, const double *rec_score,
                                        const double *thresholds, const int *reached, int count, double min_iou, long long *counters,
                                        long long *iou_q, double *iou_sum, unsigned char *tp_mask, int *flags, rtk_stream_t stream) {
    return op_launch<false>("score_replay_optimal", B, T, lg, pr, nullptr, rec_score, thresholds, reached, count, min_iou, counters, iou_q, iou_sum,
                            tp_mask, flags, stream);
}

extern "C" int rtk_score_replay_optimal_sim(int B, int T, const rtk_score_log_t *lg, const rtk_score_pairs_t *pr, const double *pair_sim,
                                            const double *rec_score, const double *thresholds, const int *reached, int count, double min_iou,
                                            long long *counters, long long *iou_q, double *iou_sum, unsigned char *tp_mask, int *flags,
                                            rtk_stream_t stream) {
    return op_launch<true>("score_replay_optimal_sim", B, T, lg, pr, pair_sim, rec_score, thresholds, reached, count, min_iou, counters, iou_q, iou_sum,
                           tp_mask, flags, stream);
}
