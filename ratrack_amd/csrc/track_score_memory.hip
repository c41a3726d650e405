// track_score_memory.hip -- rtk_track_score_memory (include/rtk_score.h): the scoring launch of track_score.hip with a record as tall
// as the table of a tracker that keeps lost tracks (BatchedTracker(max_age=...), rtk_track_memory), so that the 0/1 target of the
// tracking loss has a row for every coasted track.  The body is track_score_body.h's with MEM on; nothing else differs: one workgroup
// per stream, 256 threads, the stream's tables in LDS plus the old record's Kobj track ids.  Thread r looks row r of the new table up
// in the old record (at most Kobj words of LDS, the first row of that track id), thread 0 counts the labelled coasted rows: plain
// stores, one writer per row, the same bits on every run.
#include "track_score_body.h"

__global__ __launch_bounds__(TS_THREADS) void ts_memory_kernel(const rtk_track_score_in_t in, const rtk_track_score_state_t st,
                                                               const rtk_track_score_out_t out, const rtk_score_memory_t mm) {
    track_score_body<false, true>(in, st, out, rtk_score_log_t{}, mm);
}

// with the log of the confidence sweep as well
__global__ __launch_bounds__(TS_THREADS) void ts_memory_logged_kernel(const rtk_track_score_in_t in, const rtk_track_score_state_t st,
                                                                      const rtk_track_score_out_t out, const rtk_score_log_t lg,
                                                                      const rtk_score_memory_t mm) {
    track_score_body<true, true>(in, st, out, lg, mm);
}

extern "C" int rtk_track_score_memory_lds_bytes(int Kobj, int K, int N) {
    if (Kobj < 1 || K < 1 || N < 1 || Kobj > RTK_SCORE_MAX_OBJECTS || K > RTK_SCORE_MAX_BOXES || N > RTK_SCORE_MAX_POINTS) return -1;
    return (int)ts_score_memory_lds(Kobj, K, N);
}

extern "C" int rtk_track_score_memory(const rtk_track_score_in_t *in, const rtk_track_score_state_t *st, const rtk_track_score_out_t *out,
                                      const rtk_score_log_t *lg, const rtk_score_memory_t *mm, rtk_stream_t stream) {
    RTK_REQUIRE(in && st && out, "track_score_memory: null argument block");
    RTK_REQUIRE(mm, "track_score_memory: null memory block");
    const size_t lds = ts_score_memory_lds(in->Kobj, in->K, in->N);
    const int status = ts_score_validate(in, st, out, lg, lds);
    if (status != RTK_OK) return status;
    RTK_REQUIRE(mm->table_ids && mm->table_count && mm->row_track && mm->labelled_coasted, "track_score_memory: null table or state");
    if (lg) {
        (void)hipFuncSetAttribute((const void *)ts_memory_logged_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RTK_SCORE_LDS_LIMIT);
        ts_memory_logged_kernel<<<in->B, TS_THREADS, lds, (hipStream_t)stream>>>(*in, *st, *out, *lg, *mm);
    } else {
        (void)hipFuncSetAttribute((const void *)ts_memory_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RTK_SCORE_LDS_LIMIT);
        ts_memory_kernel<<<in->B, TS_THREADS, lds, (hipStream_t)stream>>>(*in, *st, *out, *mm);
    }
    RTK_CHECK_LAUNCH("track_score_memory");
    return RTK_OK;
}
