// track_score_centre.hip -- rtk_track_score_pairs_centre (include/rtk_score.h, "TrackEval's centre-distance similarity"): the pair-logging
// launch of track_score_pairs.hip with the pair log written under the centre-distance similarity s = max(0, 1 - |c_i - g_j| / zero_distance)
// in place of the point IoU -- a pair is logged iff s > 0, whatever its common count.  The body is track_score_body.h's with PAIRS and
// CENTRE on: the same workgroup per stream, the same 256 threads, and 24 K + 16 bytes of LDS more (the kept objects' positions,
// zero_distance and the stream's pair_sim address, staged once so that no argument rides in scalar registers through the body; the
// column's detection index rides in pts[p].w, the centres live in registers).  Everything but the pair log is rtk_track_score_pairs' bit for bit.  One writer per word, plain stores, no
// floating-point atomics: the same bits on every run.  The instantiations without CENTRE are not touched by this file.
#include "track_score_body.h"

__global__ __launch_bounds__(TS_THREADS) void ts_centre_kernel(const rtk_track_score_in_t in, const rtk_track_score_state_t st,
                                                               const rtk_track_score_out_t out, const rtk_score_log_t lg,
                                                               const rtk_score_pairs_t pr, double *pair_sim, const double *gt_centre,
                                                               double zero_distance) {
    track_score_body<true, false, true, true>(in, st, out, lg, rtk_score_memory_t{}, pr, pair_sim, gt_centre, zero_distance);
}

// behind a tracker that keeps lost tracks: the record as tall as its table
__global__ __launch_bounds__(TS_THREADS) void ts_centre_memory_kernel(const rtk_track_score_in_t in, const rtk_track_score_state_t st,
                                                                      const rtk_track_score_out_t out, const rtk_score_log_t lg,
                                                                      const rtk_score_memory_t mm, const rtk_score_pairs_t pr, double *pair_sim,
                                                                      const double *gt_centre, double zero_distance) {
    track_score_body<true, true, true, true>(in, st, out, lg, mm, pr, pair_sim, gt_centre, zero_distance);
}

extern "C" int rtk_track_score_centre_lds_bytes(int Kobj, int K, int N, int memory) {
    if (Kobj < 1 || K < 1 || N < 1 || Kobj > RTK_SCORE_MAX_OBJECTS || K > RTK_SCORE_MAX_BOXES || N > RTK_SCORE_MAX_POINTS) return -1;
    return (int)ts_score_centre_lds(Kobj, K, N, memory != 0);
}

extern "C" int rtk_track_score_pairs_centre(const rtk_track_score_in_t *in, const rtk_track_score_state_t *st, const rtk_track_score_out_t *out,
                                            const rtk_score_log_t *lg, const rtk_score_memory_t *mm, const rtk_score_pairs_t *pr,
                                            double *pair_sim, const double *gt_centre, double zero_distance, rtk_stream_t stream) {
    RTK_REQUIRE(in && st && out, "track_score_pairs_centre: null argument block");
    RTK_REQUIRE(lg, "track_score_pairs_centre: null log block");
    RTK_REQUIRE(pr, "track_score_pairs_centre: null pair-log block");
    RTK_REQUIRE(pair_sim, "track_score_pairs_centre: null pair_sim (the similarity of every logged pair)");
    RTK_REQUIRE(gt_centre, "track_score_pairs_centre: null gt_centre (the kept objects' positions)");
    RTK_REQUIRE(zero_distance > 0.0 && zero_distance < INFINITY, "track_score_pairs_centre: zero_distance=%g must be finite and above 0", zero_distance);
    const size_t lds = ts_score_centre_lds(in->Kobj, in->K, in->N, mm != nullptr);
    const int status = ts_score_validate(in, st, out, lg, lds);
    if (status != RTK_OK) return status;
    RTK_REQUIRE(pr->Q >= 1, "track_score_pairs_centre: a pair log of Q=%d pairs per stream", pr->Q);
    RTK_REQUIRE(pr->cursor && pr->frame_pair && pr->pair_key && pr->pair_common && pr->rec_size && pr->label_size,
                "track_score_pairs_centre: null pair log");
    if (mm) {
        RTK_REQUIRE(mm->table_ids && mm->table_count && mm->row_track && mm->labelled_coasted, "track_score_pairs_centre: null table or state");
        (void)hipFuncSetAttribute((const void *)ts_centre_memory_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RTK_SCORE_LDS_LIMIT);
        ts_centre_memory_kernel<<<in->B, TS_THREADS, lds, (hipStream_t)stream>>>(*in, *st, *out, *lg, *mm, *pr, pair_sim, gt_centre, zero_distance);
    } else {
        (void)hipFuncSetAttribute((const void *)ts_centre_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RTK_SCORE_LDS_LIMIT);
        ts_centre_kernel<<<in->B, TS_THREADS, lds, (hipStream_t)stream>>>(*in, *st, *out, *lg, *pr, pair_sim, gt_centre, zero_distance);
    }
    RTK_CHECK_LAUNCH("track_score_pairs_centre");
    return RTK_OK;
}
