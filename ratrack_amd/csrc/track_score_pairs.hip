// track_score_pairs.hip -- rtk_track_score_pairs (include/rtk_score.h): the logged scoring launch of track_score.hip /
// track_score_memory.hip that also appends every (detection, kept object) pair with common > 0 to the stream's pair log, the input of
// the per-frame optimal matching (track_optimal.hip).  The body is track_score_body.h's with PAIRS on: the same workgroup per stream,
// the same 256 threads and the same LDS; thread i counts and later writes row i's pairs, an ordered prefix over the rows (one wave
// scan and one more barrier) places them and tells whether the frame's pairs fit.  One writer per word, plain stores: the same bits
// on every run.  The instantiations without PAIRS are not touched by this file.
#include "track_score_body.h"

__global__ __launch_bounds__(TS_THREADS) void ts_pairs_kernel(const rtk_track_score_in_t in, const rtk_track_score_state_t st,
                                                              const rtk_track_score_out_t out, const rtk_score_log_t lg,
                                                              const rtk_score_pairs_t pr) {
    track_score_body<true, false, true>(in, st, out, lg, rtk_score_memory_t{}, pr);
}

// behind a tracker that keeps lost tracks: the record as tall as its table
__global__ __launch_bounds__(TS_THREADS) void ts_pairs_memory_kernel(const rtk_track_score_in_t in, const rtk_track_score_state_t st,
                                                                     const rtk_track_score_out_t out, const rtk_score_log_t lg,
                                                                     const rtk_score_memory_t mm, const rtk_score_pairs_t pr) {
    track_score_body<true, true, true>(in, st, out, lg, mm, pr);
}

extern "C" int rtk_track_score_pairs(const rtk_track_score_in_t *in, const rtk_track_score_state_t *st, const rtk_track_score_out_t *out,
                                     const rtk_score_log_t *lg, const rtk_score_memory_t *mm, const rtk_score_pairs_t *pr,
                                     rtk_stream_t stream) {
    RTK_REQUIRE(in && st && out, "track_score_pairs: null argument block");
    RTK_REQUIRE(lg, "track_score_pairs: null log block");
    RTK_REQUIRE(pr, "track_score_pairs: null pair-log block");
    const size_t lds = mm ? ts_score_memory_lds(in->Kobj, in->K, in->N) : ts_score_lds(in->Kobj, in->K, in->N);
    const int status = ts_score_validate(in, st, out, lg, lds);
    if (status != RTK_OK) return status;
    RTK_REQUIRE(pr->Q >= 1, "track_score_pairs: a pair log of Q=%d pairs per stream", pr->Q);
    RTK_REQUIRE(pr->cursor && pr->frame_pair && pr->pair_key && pr->pair_common && pr->rec_size && pr->label_size,
                "track_score_pairs: null pair log");
    if (mm) {
        RTK_REQUIRE(mm->table_ids && mm->table_count && mm->row_track && mm->labelled_coasted, "track_score_pairs: null table or state");
        (void)hipFuncSetAttribute((const void *)ts_pairs_memory_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RTK_SCORE_LDS_LIMIT);
        ts_pairs_memory_kernel<<<in->B, TS_THREADS, lds, (hipStream_t)stream>>>(*in, *st, *out, *lg, *mm, *pr);
    } else {
        (void)hipFuncSetAttribute((const void *)ts_pairs_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RTK_SCORE_LDS_LIMIT);
        ts_pairs_kernel<<<in->B, TS_THREADS, lds, (hipStream_t)stream>>>(*in, *st, *out, *lg, *pr);
    }
    RTK_CHECK_LAUNCH("track_score_pairs");
    return RTK_OK;
}
