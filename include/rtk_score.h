/*
 * rtk_score.h -- C ABI of the device-side ground-truth objects and tracking score of librtk_hip.so (csrc/track_score.hip,
 * ratrack_amd/track_score.py).
 *
 * Two entry points, one launch each, one workgroup per stream of a batch of B frames:
 *
 *   rtk_gt_objects    the reference's objs_combined: per-box point sets, the rider merge and the minimum object size
 *                     (models/utils/track4d_utils.py:105-176 filter_object_points, elements 7 to 9 of its tuple)
 *   rtk_track_score   map_gt_objects (track4d_utils.py:50-102) for every active stream, the 0/1 target of the tracking loss
 *                     (losses/loss.py:48-72) against the stream's previous frame, and running CLEAR-MOT counts
 *
 * Same conventions as rtk_gt.h: caller-allocated device buffers, argument blocks passed by address, explicit stream, 0 / negative
 * status, rtk_last_error; (B,C,N) inputs are rtk_bcn_view_t and are read in place.
 */
#ifndef RTK_SCORE_H
#define RTK_SCORE_H

#include "rtk_gt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Each kernel keeps one stream's tables in one workgroup's LDS; a configuration whose tables need more than this is refused. */
#define RTK_SCORE_LDS_LIMIT 65536
/* Box slots per stream: the ground-truth objects that hold a point are one 64-bit mask per point. */
#define RTK_SCORE_MAX_BOXES 64
/* Predicted objects per stream and points per cloud (a (point, object) pair is packed into one 32-bit word). */
#define RTK_SCORE_MAX_OBJECTS 256
#define RTK_SCORE_MAX_POINTS 32768

#define RTK_SCORE_FLAG_BOXES 1       /* a box count outside [0, K] (clamped) */
#define RTK_SCORE_FLAG_NVALID 2      /* an n_valid outside [0, N] (clamped) */
#define RTK_SCORE_FLAG_TRACKS 4      /* rtk_track_score: more label ids in a clip than the track table holds */
#define RTK_SCORE_FLAG_OBJECTS 8     /* rtk_track_score: a num_objects outside [0, Kobj] (clamped) */

/* LDS bytes of one workgroup for these sizes (host functions: no device is touched). */
RTK_EXPORT int rtk_gt_objects_lds_bytes(int K, int N);
RTK_EXPORT int rtk_track_score_lds_bytes(int Kobj, int K, int N);

/* W = (N + 31) / 32 mask words per object; bit p & 31 of word p >> 5 is point p. */
typedef struct {
    int B, N, K;
    rtk_bcn_view_t pc1;           /* (B,3,N) */
    const int *n_valid;           /* (B) int32 or NULL: N points */
    rtk_gt_boxes_t frame1;        /* the tables rtk_gt_labels takes for frame 1 */
    const unsigned char *types;   /* (B,K): 1 = the box's label type is rider */
    int min_obj_points;
} rtk_gt_objects_in_t;

typedef struct {
    int *slot;                    /* (B,K) box slot of the j-th kept object (label order), -1 past count */
    int *label_id;                /* (B,K) its label id, -1 past count */
    int *count;                   /* (B) kept objects */
    int *size;                    /* (B,K) its size, 0 past count */
    unsigned int *members;        /* (B,K,W) its point set, 0 past count */
    double *centre;               /* (B,K,3) the mean of the points of its OWN box, 0 past count */
    int *flags;                   /* (B) RTK_SCORE_FLAG_BOXES | RTK_SCORE_FLAG_NVALID */
} rtk_gt_objects_out_t;

/* Per stream b, over its n_valid columns:
 *   membership   rtk_gt_labels' float64 box test, operation by operation; a point inside two boxes belongs to both objects; a box
 *                without a point is no object;
 *   centres      sum of the object's points in float64 in column order, divided by their number;
 *   rider merge  serial in label order: a rider's nearest OTHER object (sqrt of the float64 squared centre distance, original
 *                centres, strict <: the first of equals; objects already merged away still count, as in the host loop) receives
 *                the rider's current point set -- what was merged into the rider before included -- and the rider is dropped; a
 *                rider alone in its frame stays;
 *   size         an object that received a merge counts bit-identical coordinate triples once (the host's torch.unique): its
 *                `members` keep the FIRST column of each distinct triple, so size = popcount(members) for every object and the
 *                coordinates of `members` are the host's point set; other objects keep their duplicates;
 *   minimum      objects of size < min_obj_points are dropped. */
RTK_EXPORT int rtk_gt_objects(const rtk_gt_objects_in_t *in, const rtk_gt_objects_out_t *out, rtk_stream_t stream);

#define RTK_SCORE_COUNTERS 11        /* frames | gt | pred | tp | fp | fn | idsw | tracks | mt | pt | ml */

typedef struct {
    int B, N, Kobj, K, T;         /* Kobj: predicted-object slots, K: ground-truth slots, T: track-table entries per stream */
    rtk_bcn_view_t pc1;           /* (B,3,N) */
    const int *obj;               /* (B,N) predicted object index of each point, -1 none (association order) */
    const int *num_objects;       /* (B) */
    const int *object_ids;        /* (B,Kobj) track id of each predicted object */
    const int *n_valid;           /* (B) or NULL */
    const int *gt_slot, *gt_label_id, *gt_count, *gt_size;     /* rtk_gt_objects' outputs */
    const unsigned int *gt_members;
    const unsigned char *reset;   /* (B) or NULL */
    const unsigned char *active;  /* (B) or NULL: every stream is scored */
} rtk_track_score_in_t;

/* The scorer's state: zero-initialised by the caller except prev_count = -1; only rtk_track_score writes it afterwards. */
typedef struct {
    long long *counters;          /* (B,11) */
    double *iou_sum;              /* (B) */
    int *table_key, *table_last, *table_seen, *table_matched;      /* (B,T): label id | last matched track id (-1 none) | frames */
    int *table_used;              /* (B) */
    int *prev_gt_id;              /* (B,Kobj) label id each object of the stream's last active frame was matched to, -1 none */
    int *prev_count, *prev_gt;    /* (B) its predictions (-1: no such frame) and its kept ground-truth objects */
    int *flags;                   /* (B) sticky: RTK_SCORE_FLAG_* */
} rtk_track_score_state_t;

typedef struct {
    int *pred_gt_slot, *pred_gt_id;      /* (B,Kobj) the box slot / label id prediction i is matched to, -1 none */
    int *gt_pred;                        /* (B,K) the prediction kept ground-truth object j is matched to, -1 none */
    double *iou;                         /* (B,Kobj) the match's IoU, 0 when unmatched */
    float *aff_target;                   /* (B,Kobj,Kobj) [i][j] = 1: previous object i and current object j carry one label id */
    unsigned char *aff_defined;          /* (B) both frames had a kept ground-truth object and a prediction */
} rtk_track_score_out_t;

/* Per active stream b:
 *   reset        (first) every table entry is classified by matched / seen (float64): > 0.8 mostly tracked, < 0.2 mostly lost, else
 *                partly tracked, and added to tracks / mt / pt / ml; the table is cleared and the previous-frame record dropped;
 *   common       for prediction i and kept object j the number of (point of i, point of j) PAIRS whose float32 coordinate
 *                differences have a squared float64 norm < 1e-5 * 1e-5;
 *   iou          (double)common / (double)(|i| + |j| - common) on integers, 0 when the denominator is 0;
 *   match        predictions in order: the object of the largest iou > 0 (strict >: the first of equals); taken already: unmatched;
 *   score        frames += 1, gt += G, pred += P, tp += M, fp += P - M, fn += G - M, iou_sum += the matched ious in prediction
 *                order; every kept object's table entry (appended on first sight; a full table raises RTK_SCORE_FLAG_TRACKS and
 *                the object goes uncounted) gains a frame seen, a matched one a frame matched, and idsw += 1 when the entry's last
 *                matched track id is another one than object_ids[i];
 *   target       against the record of the stream's last active frame, which this frame then replaces.
 * An inactive stream changes no state; its outputs are -1 / 0.  Integer sums only, except iou_sum (fixed order): the same bits on
 * every run. */
RTK_EXPORT int rtk_track_score(const rtk_track_score_in_t *in, const rtk_track_score_state_t *state, const rtk_track_score_out_t *out,
                               rtk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RTK_SCORE_H */
