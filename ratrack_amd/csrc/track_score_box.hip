// track_score_box.hip -- rtk_track_score_pairs_box (include/rtk_score.h, "The oriented-box IoU on the pair log"): the pair-logging launch
// of track_score_pairs.hip with the pair log written under the IoU of each detection's fitted box (rtk_object_boxes) and each kept
// object's label box read upright, in three dimensions or in the bird's-eye view -- a pair is logged iff s > 0, whatever its common
// count.  The body is track_score_body.h's with PAIRS and BOX on, in the centre variant's arrangement: the same workgroup per stream, the
// same 256 threads, 64 K + 16 bytes of LDS more (the kept objects' upright boxes, the mode and the stream's pair_sim address, staged
// once so that no argument rides in scalar registers through the body).  The P G decisions are spread over the workgroup: thread e mod 256
// takes pair e = i G + j, reads detection i's box from global memory, cuts its footprint by kept object j's rectangle (Sutherland-Hodgman
// on eight fixed edge slots, no array in private memory) and raises bit j of row i's mask in LDS (the words best_iou takes later); thread
// i then writes row i behind the ordered prefix, forming each logged s again by the same operations.  Everything but the pair log is rtk_track_score_pairs' bit for bit.  One writer
// per word, plain stores, no floating-point atomics: the same bits on every run.  The instantiations without BOX are not touched by this
// file.
#include "track_score_body.h"

__global__ __launch_bounds__(TS_THREADS) void ts_box_kernel(const rtk_track_score_in_t in, const rtk_track_score_state_t st,
                                                            const rtk_track_score_out_t out, const rtk_score_log_t lg,
                                                            const rtk_score_pairs_t pr, double *pair_sim, const double *det_box,
                                                            const int *det_valid, const double *gt_boxes, int mode) {
    track_score_body<true, false, true, false, true>(in, st, out, lg, rtk_score_memory_t{}, pr, pair_sim, nullptr, 0.0, det_box, det_valid,
                                                     gt_boxes, mode);
}

// behind a tracker that keeps lost tracks: the record as tall as its table
__global__ __launch_bounds__(TS_THREADS) void ts_box_memory_kernel(const rtk_track_score_in_t in, const rtk_track_score_state_t st,
                                                                   const rtk_track_score_out_t out, const rtk_score_log_t lg,
                                                                   const rtk_score_memory_t mm, const rtk_score_pairs_t pr, double *pair_sim,
                                                                   const double *det_box, const int *det_valid, const double *gt_boxes,
                                                                   int mode) {
    track_score_body<true, true, true, false, true>(in, st, out, lg, mm, pr, pair_sim, nullptr, 0.0, det_box, det_valid, gt_boxes, mode);
}

extern "C" int rtk_track_score_box_lds_bytes(int Kobj, int K, int N, int memory) {
    if (Kobj < 1 || K < 1 || N < 1 || Kobj > RTK_SCORE_MAX_OBJECTS || K > RTK_SCORE_MAX_BOXES || N > RTK_SCORE_MAX_POINTS) return -1;
    return (int)ts_score_box_lds(Kobj, K, N, memory != 0);
}

extern "C" int rtk_track_score_pairs_box(const rtk_track_score_in_t *in, const rtk_track_score_state_t *st, const rtk_track_score_out_t *out,
                                         const rtk_score_log_t *lg, const rtk_score_memory_t *mm, const rtk_score_pairs_t *pr, double *pair_sim,
                                         const double *det_box, const int *det_valid, const double *gt_boxes, int mode, rtk_stream_t stream) {
    RTK_REQUIRE(in && st && out, "track_score_pairs_box: null argument block");
    RTK_REQUIRE(lg, "track_score_pairs_box: null log block");
    RTK_REQUIRE(pr, "track_score_pairs_box: null pair-log block");
    RTK_REQUIRE(pair_sim, "track_score_pairs_box: null pair_sim (the similarity of every logged pair)");
    RTK_REQUIRE(det_box && det_valid, "track_score_pairs_box: null det_box or det_valid (the detections' boxes, rtk_object_boxes' output)");
    RTK_REQUIRE(gt_boxes, "track_score_pairs_box: null gt_boxes (the frame-1 box table)");
    RTK_REQUIRE(mode == RTK_SCORE_BOX_3D || mode == RTK_SCORE_BOX_BEV, "track_score_pairs_box: mode=%d is neither RTK_SCORE_BOX_3D nor RTK_SCORE_BOX_BEV",
                mode);
    const size_t lds = ts_score_box_lds(in->Kobj, in->K, in->N, mm != nullptr);
    const int status = ts_score_validate(in, st, out, lg, lds);
    if (status != RTK_OK) return status;
    RTK_REQUIRE(pr->Q >= 1, "track_score_pairs_box: a pair log of Q=%d pairs per stream", pr->Q);
    RTK_REQUIRE(pr->cursor && pr->frame_pair && pr->pair_key && pr->pair_common && pr->rec_size && pr->label_size,
                "track_score_pairs_box: null pair log");
    if (mm) {
        RTK_REQUIRE(mm->table_ids && mm->table_count && mm->row_track && mm->labelled_coasted, "track_score_pairs_box: null table or state");
        (void)hipFuncSetAttribute((const void *)ts_box_memory_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RTK_SCORE_LDS_LIMIT);
        ts_box_memory_kernel<<<in->B, TS_THREADS, lds, (hipStream_t)stream>>>(*in, *st, *out, *lg, *mm, *pr, pair_sim, det_box, det_valid, gt_boxes,
                                                                              mode);
    } else {
        (void)hipFuncSetAttribute((const void *)ts_box_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RTK_SCORE_LDS_LIMIT);
        ts_box_kernel<<<in->B, TS_THREADS, lds, (hipStream_t)stream>>>(*in, *st, *out, *lg, *pr, pair_sim, det_box, det_valid, gt_boxes, mode);
    }
    RTK_CHECK_LAUNCH("track_score_pairs_box");
    return RTK_OK;
}
