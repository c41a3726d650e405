// track_identity_pairs.hip -- the identity metrics IDF1, IDP and IDR with EVERY pair above the level counted, over the scorer's two logs
// (include/rtk_score.h, "Identity over every pair"; ratrack_amd/track_score.py, TrackScorer.identity(pairs="all")).
//
//   rtk_score_identity_pairs   one wave per (stream, level): rtk_score_identity's walk and clip close (track_identity.hip), with the
//                              per-frame part reading the pair log: a (label, track) pair gains the frame when some remaining detection
//                              of that track has a VALID pair with that label's object and similarity >= the level -- there is no
//                              best-object restriction, so a detection may count for several labels of a frame
//
// A sibling of identity_kernel in a file of its own, so that track_identity.hip's code object stays what it is; the clip close is that
// kernel's, statement for statement.  What differs in the tables: a detection keeps only its track slot, the frame's pairs go through
// a wave's width of staging words, and every pair of the list carries the last frame that counted it (a frame adds at most 1 to a
// pair, also in a log that repeats a track id within a frame).  Those words lie in the walk's part of the LDS, which the solver's
// tables exceed: the figure per label capacity is rtk_score_identity's.  Integers only: the same numbers on every run.
// The LDS layout and the body are track_identity_pairs_body.h's, instantiated here twice: on the point IoU of the logged integers
// (rtk_score_identity_pairs) and, SIM, on the similarity the pair log itself carries (rtk_score_identity_pairs_sim; track_optimal.hip's
// header has the rule).  The same LDS tables, grid and arithmetic either way.
#include "track_identity_pairs_body.h"

template <int TCAP, bool SIM>
__global__ __launch_bounds__(RTK_WAVE) void identity_pairs_kernel(int T, const rtk_score_log_t lg, const lw_pairs_arg_t<SIM> pa,
                                                                  const double *rec_score, const double *threshold, const double *alphas,
                                                                  long long *counters, int *flags) {
    __shared__ __attribute__((aligned(16))) int ip_smem[ip_words(TCAP)];
    identity_pairs_body<TCAP, SIM>(ip_smem, T, lg, pa.pr, rec_score, threshold, alphas, counters, flags, pa.sim());
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
extern "C" int rtk_score_identity_pairs_lds_bytes(int T) {
    if (T < 1 || T > (1 << 24)) return -1;
    return (int)ip_lds(T);
}

// name: the entry point's, for its messages; SIM: the walk on pair_sim, refused when that is NULL
template <bool SIM>
static int ip_launch(const char *name, int B, int T, const rtk_score_log_t *lg, const rtk_score_pairs_t *pr, const double *pair_sim,
                     const double *rec_score, const double *threshold, const double *alphas, int count, long long *counters, int *flags,
                     rtk_stream_t stream) {
    const int status = ip_validate(name, B, T, lg, pr, alphas, count, counters, flags);
    if (status != RTK_OK) return status;
    if (SIM) RTK_REQUIRE(pair_sim, "%s: null pair_sim", name);
    const auto kernel = T <= IP_TCAP_SMALL ? identity_pairs_kernel<IP_TCAP_SMALL, SIM> : identity_pairs_kernel<IP_TCAP_LARGE, SIM>;
    kernel<<<dim3(B, count), RTK_WAVE, 0, (hipStream_t)stream>>>(T, *lg, lw_pairs_arg_t<SIM>(*pr, pair_sim), rec_score, threshold, alphas, counters,
                                                                 flags);
    RTK_CHECK_LAUNCH(name);
    return RTK_OK;
}

extern "C" int rtk_score_identity_pairs(int B, int T, const rtk_score_log_t *lg, const rtk_score_pairs_t *pr, const double *rec_score,
                                        const double *threshold, const double *alphas, int count, long long *counters, int *flags,
                                        rtk_stream_t stream) {
    return ip_launch<false>("score_identity_pairs", B, T, lg, pr, nullptr, rec_score, threshold, alphas, count, counters, flags, stream);
}

extern "C" int rtk_score_identity_pairs_sim(int B, int T, const rtk_score_log_t *lg, const rtk_score_pairs_t *pr, const double *pair_sim,
                                            const double *rec_score, const double *threshold, const double *alphas, int count, long long *counters,
                                            int *flags, rtk_stream_t stream) {
    return ip_launch<true>("score_identity_pairs_sim", B, T, lg, pr, pair_sim, rec_score, threshold, alphas, count, counters, flags, stream);
}
