/*
 * rtk_gt.h -- C ABI of the device-side ground truth and scoring of librtk_hip.so (csrc/gt_eval.hip, ratrack_amd/gt_device.py).
 *
 * Two entry points, one launch each, one workgroup per stream of a batch of B frame pairs:
 *
 *   rtk_gt_labels    oriented-box membership of both frames + the GT warped positions: what the reference's epoch loop derives per
 *                    frame on the host (models/utils/track4d_utils.py:105-176 filter_object_points up to the rider merge,
 *                    :337-359 get_gt_flow_new; dataset_classes/track_vod_3d.py:107-108 ego-motion compensation)
 *   rtk_eval_frame   the scene-flow and motion-segmentation metrics of main_utils.py:342-389, per stream
 *
 * Same conventions as rtk_fused.h: caller-allocated device buffers, explicit stream, 0 / negative status, rtk_last_error; (B,C,N)
 * inputs are rtk_bcn_view_t and are read in place (the backbone's outputs are permuted views).
 */
#ifndef RTK_GT_H
#define RTK_GT_H

#include "rtk_fused.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The largest K (box slots per stream and frame): both frames' tables of a stream live in one workgroup's LDS. */
#define RTK_GT_MAX_BOXES 256
#define RTK_GT_BOX_WORDS 16

/* The boxes of one frame of every stream.  boxes (B,K,16) float64: centre (3) | R (9, row-major; COLUMN k of R is box axis k) |
 * half-extent (3) | pad.  box_id (B,K) int32: the label id of each box; count (B) int32: boxes of stream b (its first count[b]
 * slots, in label order). */
typedef struct {
    const double *boxes;
    const int *box_id;
    const int *count;
} rtk_gt_boxes_t;

typedef struct {
    int B, N, N2, K;
    rtk_bcn_view_t pc1, pc2;      /* (B,3,N), (B,3,N2) */
    const int *n_valid;           /* (2,B) int32: row 0 frame 1, row 1 frame 2; or NULL: N / N2 points */
    rtk_gt_boxes_t frame1, frame2;
    const int *pair;              /* (B,K): for frame-1 box k the frame-2 box with the same label id, or -1 */
    const float *motion;          /* (B,K,12): rows 0..2 of T_box2 . inv(T_box1), row-major 3 x 4 */
    const double *ego;            /* (B,12): rows 0..2 of inv(ego_motion^T)^T, row-major 3 x 4; or NULL: pc1_comp is an INPUT */
} rtk_gt_in_t;

typedef struct {
    unsigned char *gt_cls;        /* (B,N) 1 = inside a frame-1 box */
    int *box_index;               /* (B,N) slot of the LAST frame-1 box containing the point, -1: none */
    int *obj_id;                  /* (B,N) that box's label id, -1: none */
    float *gt_warp;               /* (B,3,N) */
    float *pc1_comp;              /* (B,3,N) ego-motion compensated frame 1: written when in->ego != NULL, else read */
    int *counts1, *counts2;       /* (B,K) valid points inside each box of frame 1 / frame 2 (0 past count) */
    int *flags;                   /* (B) bit 0: a count > K (clamped to K), bit 1: an n_valid outside [0, N] / [0, N2] (clamped) */
} rtk_gt_out_t;

/* Per stream b:
 *   membership   point p is inside box (c, R, h) iff |d . R[:,k]| <= h_k for k = 0, 1, 2 (closed), d = p - c, all in float64:
 *                (d0 R[0][k] + d1 R[1][k]) + d2 R[2][k], each product and sum rounded on its own (Open3D's OrientedBoundingBox test);
 *   ids          a point inside several boxes carries the LAST box (the reference overwrites in label order);
 *   pc1_comp     float32 of ((x E[j][0] + y E[j][1]) + z E[j][2]) + E[j][3] in float64 (E = ego), for all N columns;
 *   gt_warp      labelled point whose box k has pair[k] >= 0 and counts2[pair[k]] > 0: ((T[j][0] x + T[j][1] y) + T[j][2] z) + T[j][3]
 *                in fp32 (T = motion[b][k]), every other point: pc1_comp;
 *   padding      columns >= n_valid take part in nothing: gt_cls 0, box_index = obj_id = -1, gt_warp = pc1_comp. */
RTK_EXPORT int rtk_gt_labels(const rtk_gt_in_t *in, const rtk_gt_out_t *out, rtk_stream_t stream);

#define RTK_EVAL_SUMS 13
#define RTK_EVAL_VALUES 10

typedef struct {
    int B, N;
    rtk_bcn_view_t pc1, warp, gt_warp;   /* (B,3,N); warp = pc1 + flow */
    rtk_bcn_view_t cls;                  /* (B,1,N) or (B,N) (sc unused): motion-segmentation score, moving iff cls > threshold */
    const float *mask;                   /* (B,N): == 1 static, == 0 moving, anything else neither */
    const unsigned char *gt_cls;         /* (B,N) */
    float threshold;
    const int *n_valid;                  /* (B) or NULL: N points */
    const unsigned char *active;         /* (B) or NULL: every stream is scored */
} rtk_eval_in_t;

/* sums (B,13) float64, per stream over its n_valid points:
 *   0 points | 1 sum error | 2 sum rn_error | 3 sum rn_error over moving | 4 moving points | 5 sum rn_error over static |
 *   6 static points | 7 sas hits | 8 ras hits | 9 tp | 10 tn | 11 fp | 12 fn
 * values (B,10) float64 = the reference's metrics from those sums, in the order
 *   rne | 50-50 rne | mov_rne | stat_rne | sas | ras | epe | acc | sen | miou
 * (stat_rne of a stream without a static point is NaN, the mean of an empty slice).  Inactive streams: all zeros.
 * All arithmetic is float64 on the float32 inputs; sums are taken in a fixed order (the result does not vary from run to run). */
RTK_EXPORT int rtk_eval_frame(const rtk_eval_in_t *in, double *sums, double *values, rtk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RTK_GT_H */
