/*
 * rtk_score.h -- C ABI of the device-side ground-truth objects and tracking score of librtk_hip.so (csrc/track_score.hip,
 * ratrack_amd/track_score.py).
 *
 * Two per-frame entry points, one launch each, one workgroup per stream of a batch of B frames (and the confidence sweep over a
 * log of such frames, at the end of this file):
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
#define RTK_SCORE_FLAG_LOG 16        /* rtk_track_score_logged: a frame did not fit the stream's log and was not logged at all */
#define RTK_SCORE_FLAG_SWEEP 32      /* rtk_score_track_means: more track ids in one clip than RTK_SCORE_SWEEP_TRACKS (no score written) */
#define RTK_SCORE_FLAG_TABLE 64      /* rtk_track_score_memory: a table_count outside [num_objects, Kobj] (clamped) */
#define RTK_SCORE_FLAG_HOTA 128      /* rtk_score_hota, rtk_score_alignment: a clip with more labels, track ids or pairs than its tables hold (outputs unspecified) */
#define RTK_SCORE_FLAG_IDENTITY 256  /* rtk_score_identity, rtk_score_identity_pairs: the same, of its tables */
#define RTK_SCORE_FLAG_OPTIMAL 512   /* rtk_score_replay_optimal, rtk_score_hota_optimal: a frame with more candidate pairs than RTK_SCORE_PAIR_EDGES (outputs unspecified) */

/* LDS bytes of one workgroup for these sizes (host functions: no device is touched). */
RTK_EXPORT int rtk_gt_objects_lds_bytes(int K, int N);
RTK_EXPORT int rtk_track_score_lds_bytes(int Kobj, int K, int N);
RTK_EXPORT int rtk_track_score_memory_lds_bytes(int Kobj, int K, int N);      /* rtk_track_score_memory: Kobj more words */

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

/* ---- the confidence sweep: sAMOTA / AMOTA / AMOTP (csrc/track_sweep.hip, TrackScorer.sweep) -----------------------------------
 *
 * The sweep metrics of Weng et al., "3D Multi-Object Tracking: A Baseline and New Evaluation Metrics", under rtk_track_score's
 * matching rule.  L recall levels (40 in that paper).
 *   clip         a stream's frames from one reset to the next.
 *   track score  a track is a (stream, clip, track id); its score is the float64 sum of the fp32 object_conf of its logged
 *                detections, added in log order, divided by their number.
 *   replay at t  every stream is walked frame by frame.  Detections whose track score is < t are removed (a score equal to t
 *                stays).  The others go through rtk_track_score's rule in detection order: each takes its best object -- the
 *                largest IoU > 0, strict >, against ALL kept ground-truth objects, so it does not depend on the filter --; if a
 *                remaining detection took that object already it is unmatched, without a second choice; a removed detection takes
 *                nothing, so a later one can win an object it lost in the unfiltered pass.  gt, pred (the remaining detections),
 *                tp, fp, fn, idsw, iou_sum and the per-clip track table (tracks / mt / pt / ml, 0.8 / 0.2) are counted as above;
 *                clips still open are closed at the end.  t = -infinity reproduces rtk_track_score's counters and iou_sum bit for
 *                bit (with the open clips closed).
 *   thresholds   the KITTI walk: the track scores of the true positives of the unfiltered replay, pooled over the streams and
 *                sorted descending into s[0..n); G the pooled gt count; cur = 0; for i in order: l = (i+1)/G, r = (i+2)/G if
 *                i < n-1 else l; if (r - cur) < (cur - l) and i < n-1 the i is skipped, otherwise s[i] is the next threshold and
 *                cur += 1/L.  float64 throughout.  The first threshold (recall 0) is dropped; the k-th remaining one belongs to
 *                recall level r_k = k/L; levels the walk never reaches contribute 0 to every average.
 *   per level    MOTA_k = 1 - (FP+FN+IDSW)/G, sMOTA_k = max(0, 1 - (FP+FN+IDSW - (1-r_k) G)/(r_k G)), MOTP_k = iou_sum/TP.
 *   averages     AMOTA, sAMOTA, AMOTP: the sum over the reached levels divided by L.
 * The device produces integers and fixed-order IoU sums; every ratio above is host arithmetic in float64 (track_score.py). */

/* Most track ids of one clip of one stream rtk_score_track_means can tell apart (an open-addressed table in LDS). */
#define RTK_SCORE_SWEEP_TRACKS 2048

/* The per-stream log rtk_track_score_logged appends to: packed, with per-frame offsets.  F frames and R entries per stream bound the
 * memory; a frame needs one frame slot, P detection records and G kept-label entries (P, G: its clamped counts), and a frame that
 * does not fit is not logged at all (RTK_SCORE_FLAG_LOG).  Zero-initialised by the caller; only rtk_track_score_logged writes it. */
typedef struct {
    int F, R;
    const float *object_conf;     /* (B,Kobj) this frame's confidences: the only per-call input of the log */
    int *cursor;                  /* (B,4) frames | detection records | label entries logged so far | unused: the cursors live here */
    int *frame;                   /* (B,F,4) first record | first label entry | P + 65536 * (the frame began a clip) | G */
    int *label;                   /* (B,R) kept label ids, frame after frame */
    int *rec_track, *rec_best;    /* (B,R) per detection, in order: its track id | the label id of its pre-greedy best object, -1 none */
    float *rec_conf;              /* (B,R) its object_conf */
    double *rec_iou;              /* (B,R) the IoU with that best object, 0 when none */
} rtk_score_log_t;

/* rtk_track_score, bit for bit (counters, state, outputs), in the same single launch; every active stream also appends the frame to
 * its log.  The frame's position is read from log->cursor on the device, so two calls with identical host arguments append two
 * frames (a captured launch replays correctly).  An inactive stream appends nothing. */
RTK_EXPORT int rtk_track_score_logged(const rtk_track_score_in_t *in, const rtk_track_score_state_t *state, const rtk_track_score_out_t *out,
                                      const rtk_score_log_t *log, rtk_stream_t stream);

/* The record of a tracker that keeps lost tracks (BatchedTracker(max_age=...), rtk_track_memory in rtk_fused.h).  The previous table
 * of such a tracker is taller than the previous frame's detections: rows of coasted tracks follow them, and `aff` has a row for each.
 * rtk_track_score_memory keeps a record as tall as that table, so that row i of aff_target is row i of aff. */
typedef struct {
    const int *table_ids;         /* (B,Kobj) input: the track id of every row of the tracker's NEW table -- the one this frame's */
    const int *table_count;       /* (B) input:      rtk_associate_batched and rtk_track_memory wrote -- and its row count */
    int *row_track;               /* (B,Kobj) state: the track id of every row of the record, -1 past prev_count */
    int *labelled_coasted;        /* (B) state: the record's rows at or past its frame's detection count whose label id is >= 0 */
} rtk_score_memory_t;

/* rtk_track_score (with log == NULL) or rtk_track_score_logged, in the same single launch, with a record of the whole table.  In the
 * state block prev_gt_id is the label id of EVERY row of the record and prev_count the record's row count; prev_gt keeps its meaning.
 * mem->row_track is -1-initialised and mem->labelled_coasted zero-initialised by the caller; only this entry point writes them.
 * Counters, table, matching and log are rtk_track_score's, bit for bit.  What differs, per active stream b with P = its clamped
 * num_objects:
 *   target       the formula is unchanged: aff_target[i][j] = 1 iff i < prev_count, j < P, prev_gt_id[i] >= 0 and prev_gt_id[i] is
 *                detection j's label id.  The record is as tall as the previous table, so target row i is aff row i, a coasted row
 *                included.  Two rows of the record may carry one label id -- a lost track still coasts while its object was detected
 *                again under a fresh id -- and then BOTH rows get the 1.  That is intended: both rows are that object, and either
 *                is a correct row for the detection to be associated with.  A coasted row that never matched an object has label
 *                id -1 and an all-zero target row.
 *   new record   R = table_count[b] clamped to [P, Kobj] rows; outside that range RTK_SCORE_FLAG_TABLE is raised (sticky).  Row
 *                r < P holds (object_ids[r], detection r's label id or -1).  Row P <= r < R holds table_ids[r] and the label id
 *                of the OLD record's first row with the same row_track, -1 when there is none or the stream is reset.  Track ids
 *                are unique within a stream's table, so no permutation has to come out of rtk_track_memory; a row the tracker
 *                dropped is simply not found again.  Rows past R: -1 / -1.  labelled_coasted = the rows P <= r < R with a label
 *                id >= 0.
 *   aff_defined  prev_count > 0 && P > 0 && G > 0 && (prev_gt > 0 || labelled_coasted > 0), the state read before this frame
 *                replaces it.  Without coasted rows that is rtk_track_score's rule bit for bit; with them a frame stays defined
 *                when the previous frame had no kept ground-truth object but a coasted row remembers one (an object hidden for
 *                one frame: the re-acquisition to train).
 *   reset        drops the record first, as above; an inactive stream changes no state and writes -1 / 0 outputs.
 * With table_ids = object_ids and table_count = num_objects every output and every shared state tensor equals rtk_track_score's.
 * Every row is written by exactly one thread with plain stores: the same bits on every run. */
RTK_EXPORT int rtk_track_score_memory(const rtk_track_score_in_t *in, const rtk_track_score_state_t *state, const rtk_track_score_out_t *out,
                                      const rtk_score_log_t *log /* NULL: no log */, const rtk_score_memory_t *mem, rtk_stream_t stream);

/* rec_score (B,R) float64: for every logged detection the score of its track.  One workgroup per stream; flags (B) gains
 * RTK_SCORE_FLAG_SWEEP for a stream with more than RTK_SCORE_SWEEP_TRACKS track ids in a clip. */
RTK_EXPORT int rtk_score_track_means(int B, const rtk_score_log_t *log, double *rec_score, int *flags, rtk_stream_t stream);

/* The walk: sorted (*n or more) float64 descending, *n true positives, *gt ground-truth objects (device scalars).  thresholds
 * (levels + 1): [0] = -infinity, [k] the threshold of level k for k <= *reached, +infinity beyond; *reached <= levels. */
RTK_EXPORT int rtk_score_thresholds(const double *sorted, const long long *n, const long long *gt, int levels, double *thresholds,
                                    int *reached, rtk_stream_t stream);

/* Grid (stream, threshold index): counters (count,B,11) and iou_sum (count,B) of the replay at thresholds[index]; T as in
 * rtk_track_score.  reached NULL: every index is replayed; otherwise indices above *reached write zeros.  tp_mask NULL or (B,R)
 * uint8, written for index 0 only: 1 where the logged detection is a true positive.  One IoU-sum order per (stream, index):
 * frames in order, detections in order, from 0. */
RTK_EXPORT int rtk_score_replay(int B, int T, const rtk_score_log_t *log, const double *rec_score, const double *thresholds,
                                const int *reached, int count, long long *counters, double *iou_sum, unsigned char *tp_mask,
                                rtk_stream_t stream);

/* ---- HOTA: DetA, AssA, LocA (csrc/track_hota.hip, TrackScorer.hota) --------------------------------------------------------------
 *
 * The metric of Luiten et al., "HOTA: A Higher Order Metric for Evaluating Multi-Object Tracking", over the same log, under
 * rtk_track_score's matching rule and the reference's point IoU.  TrackEval's own numbers use a Hungarian assignment on box IoU:
 * these are NOT those, as the sweep's are not the reference README's table.
 *   levels       A of them (19 by default), alpha_a = (double)a / (double)(A + 1) for a = 1..A (0.05 ... 0.95).
 *   removal      clip, log, track score and the removal by a threshold t are the sweep's: a detection whose track score is < t is
 *                removed -- it is no prediction, belongs to no track and takes nothing.  No rec_score, no threshold or
 *                t = -infinity removes nothing.
 *   candidate    per (stream, alpha_a), frames in log order: a remaining detection with a best label (rec_best != -1) and
 *                rec_iou >= alpha_a (float64 >=; both are correctly rounded quotients, so an IoU of 3/5 is a candidate at
 *                alpha = 12/20).  A remaining detection that is no candidate takes nothing and is a false positive at this alpha,
 *                and THE OBJECT STAYS FREE for a later detection: threshold first, then match, as TrackEval zeroes the pairs below
 *                alpha before it matches -- not "replay, then drop the weak matches".
 *   match        candidates in detection order take their best object; taken by an earlier candidate: unmatched, no second
 *                choice.  A match is a true positive (label g, track t, IoU).
 *   per clip     cg[g] the frames of the clip whose kept labels contain g; ct[t] the remaining detections of the clip with track
 *                id t (neither depends on alpha); n[g,t] the true positives of the pair.  A clip closes at a reset frame or at the
 *                end of the log.
 *   counters     running over the stream: frames | clips | gt = sum cg | pred = sum ct | tp = sum n | pairs = the distinct (g,t)
 *                with n > 0.  Hence fn = gt - tp and fp = pred - tp.
 *   sums         each one running float64 from 0 over the whole stream: loc gains a true positive's IoU when it is matched, in
 *                log order; at a clip's close, for its pairs IN ORDER OF FIRST APPEARANCE (frame order, then detection order), with
 *                N = (double)(n*n) from the integer product: ass += N / (double)(cg + ct - n), ass_re += N / (double)cg,
 *                ass_pr += N / (double)ct -- one division and one addition each, no FMA contraction.
 *   host         float64, the streams pooled in stream order, per alpha: DetA = TP/(TP+FN+FP), DetRe = TP/(TP+FN),
 *                DetPr = TP/(TP+FP), AssA = ass/TP, AssRe = ass_re/TP, AssPr = ass_pr/TP, LocA = loc/TP,
 *                HOTA_alpha = sqrt(DetA * AssA); a ratio without a denominator is NaN.  HOTA, DetA, AssA, DetRe, DetPr, AssRe,
 *                AssPr, LocA are the sums over alpha, in alpha order, of the non-NaN terms, divided by A (AMOTP's rule).
 * The device produces the integers and the four sums; every ratio is host arithmetic (track_score.py, hota_values). */
#define RTK_SCORE_HOTA_COUNTERS 6    /* frames | clips | gt | pred | tp | pairs */
#define RTK_SCORE_HOTA_SUMS 4        /* ass | ass_re | ass_pr | loc */
/* Most distinct (label id, track id) pairs of one clip of one stream (an insertion-ordered list with a lookup table in LDS). */
#define RTK_SCORE_HOTA_PAIRS 1024

/* Grid (stream, alpha index): counters (alphas,B,6) and sums (alphas,B,4) of level a = index + 1 of `alphas` levels (1..63).  T bounds
 * the label ids of one clip (rtk_track_score's T; a T whose tables do not fit RTK_SCORE_LDS_LIMIT is refused), and
 * RTK_SCORE_SWEEP_TRACKS its track ids.  A clip of stream b with more labels than T, more track ids than RTK_SCORE_SWEEP_TRACKS or
 * more pairs than RTK_SCORE_HOTA_PAIRS raises RTK_SCORE_FLAG_HOTA in flags[b] (or-ed in; nothing else of flags is touched): that
 * stream's outputs are then unspecified but written, the other streams are unaffected.  Reads the log, rec_score and threshold and
 * writes only its three outputs. */
RTK_EXPORT int rtk_score_hota(int B, int T, const rtk_score_log_t *log, const double *rec_score /* (B,R) or NULL */,
                              const double *threshold /* device scalar, or NULL: nothing removed */, int alphas,
                              long long *counters /* (alphas,B,6) */, double *sums /* (alphas,B,4) */, int *flags /* (B) */,
                              rtk_stream_t stream);

/* ---- Identity: IDF1, IDP, IDR (csrc/track_identity.hip, csrc/lds_assignment.h, TrackScorer.identity) ---------------------------------
 *
 * The identity metrics of Ristani et al., "Performance Measures and a Data Set for Multi-Target, Multi-Camera Tracking", over the
 * same log, under this module's rules and the reference's point IoU.  The arrangement is TrackEval's `Identity`: every pair above the
 * threshold counts, then ONE GLOBAL ASSIGNMENT of whole trajectories per sequence (here: per clip).  TrackEval's own numbers use box
 * IoU at 0.5: these are NOT those.
 *   levels       `count` of them (1..63), explicit float64 values handed over by the caller (TrackScorer.identity: the single
 *                level 0.5 by default -- IDF1 is a one-threshold metric by convention; HOTA's levels work as well).
 *   removal      clip, log, track score and the removal by a threshold t are the sweep's and HOTA's: a detection whose track score
 *                is < t is removed.  No rec_score, no threshold or t = -infinity removes nothing.
 *   candidate    per (stream, level alpha), in every frame: a remaining detection whose rec_best is not -1 AND IS ONE OF THE FRAME'S
 *                KEPT LABELS, with rec_iou >= alpha (float64 >=, as in HOTA: an IoU of 3/5 is a candidate at 0.6).  THERE IS NO
 *                GREEDY PASS: two detections of one frame that share a best label are both candidates, as TrackEval counts every
 *                pair above the threshold and not only the matched ones.  The log holds only a detection's BEST object, so a second
 *                object above alpha is not seen: a detection is a candidate for at most one label per frame.
 *   per clip     n[g,t] the frames in which a candidate with track id t has best label g (track ids are unique within a frame: a
 *                frame adds at most 1 to a pair, and a log that repeats a track id within a frame still adds 1); gt gains every
 *                frame's kept-label count and pred its remaining detections.  A clip closes at a reset frame or at the end of the
 *                log, and idtp then gains THE WEIGHT OF A MAXIMUM-WEIGHT ONE-TO-ONE MATCHING between the clip's labels and its track
 *                ids under the weights n.  That is TrackEval's minimisation of fn_mat + fp_mat: with cg, ct the frames of a label
 *                and the detections of a track, a matching costs sum cg + sum ct - 2 sum n(matched).
 *   counters     running over the stream: frames | clips | gt | pred | idtp | pairs = the distinct (g,t) with n > 0.  The optimum
 *                WEIGHT is unique even where the optimal matching is not, so every output is an integer and the same on every run;
 *                the matching itself and the number of matched pairs are not unique and are not delivered.
 *   host         float64, the streams pooled: idfn = gt - idtp, idfp = pred - idtp, IDR = idtp / gt, IDP = idtp / pred,
 *                IDF1 = 2 idtp / (gt + pred); a ratio without a denominator is NaN (track_score.py, identity_values).
 * The solver is exact integer arithmetic in LDS (csrc/lds_assignment.h states its contract); no floating point enters a counter. */
#define RTK_SCORE_ID_COUNTERS 6      /* frames | clips | gt | pred | idtp | pairs */
/* Most distinct (label id, track id) pairs of one clip of one stream: the edges of the assignment. */
#define RTK_SCORE_ID_PAIRS 1024

/* LDS bytes of one workgroup of rtk_score_identity for T label ids per clip (a host function: no device is touched); -1 for a T
 * below 1.  The kernel is built for two label capacities, 1024 and the largest that fits RTK_SCORE_LDS_LIMIT, and a T takes the
 * smaller one that holds it: this is that instance's figure, or for a larger T what its tables would need. */
RTK_EXPORT int rtk_score_identity_lds_bytes(int T);

/* Grid (stream, level index): counters (count,B,6) of level alphas[index].  T bounds the label ids of one clip (rtk_track_score's T; a
 * T whose tables do not fit RTK_SCORE_LDS_LIMIT is refused, and so is a log of more than 2^28 frames per stream: a pair's weight is a
 * frame count and the solver's sums stay in an int), RTK_SCORE_SWEEP_TRACKS its track ids and RTK_SCORE_ID_PAIRS its pairs.  A clip of
 * stream b beyond one of the three raises RTK_SCORE_FLAG_IDENTITY in flags[b] (or-ed in; nothing else of flags is touched): that
 * stream's outputs are then unspecified but written, the other streams are unaffected.  Reads the log, rec_score, threshold and alphas
 * and writes only counters and flags. */
RTK_EXPORT int rtk_score_identity(int B, int T, const rtk_score_log_t *log, const double *rec_score /* (B,R) or NULL */,
                                  const double *threshold /* device scalar, or NULL: nothing removed */, const double *alphas /* device, (count) */,
                                  int count, long long *counters /* (count,B,6) */, int *flags /* (B) */, rtk_stream_t stream);

/* ---- Per-frame optimal matching at an IoU threshold (csrc/track_score.hip, csrc/track_optimal.hip, csrc/lds_assignment.h,
 *      TrackScorer(sweep_pairs=...), TrackScorer.sweep(matching="optimal"), TrackScorer.clear_optimal) ------------------------------
 *
 * Everything above rests on rtk_track_score's matching rule: each detection takes its single best object, first come first served,
 * no threshold, no second choice.  The KITTI / AB3DMOT evaluation matches otherwise: per frame ONE ASSIGNMENT of detections to
 * ground-truth objects that refuses pairs below an IoU threshold, and on top of it id switches, fragmentations, MT / ML and the
 * sweep over recall levels.  This section is that matching scheme on the reference's point IoU, at a threshold THE CALLER CHOOSES
 * (there is no default: the threshold of the reference's evaluation is not known).  It is still NOT a reproduction of the reference
 * README's table, whose threshold and evaluator are not distributed.  HOTA and the identity metrics have their own section on the
 * pair log, at the end of this file: rtk_score_hota and rtk_score_identity stay under the greedy rule, rtk_score_hota_optimal and
 * rtk_score_identity_pairs follow TrackEval's arrangement.
 *
 * The main log keeps only each detection's best object, from which no assignment can be computed afterwards; the pair log keeps
 * every overlap.  Per frame of the main log (same frame index), for every detection i and kept object j with common > 0, in
 * (i, then j) order: */
typedef struct {
    int Q;                        /* pairs per stream */
    int *cursor;                  /* (B) pairs logged so far */
    int *frame_pair;              /* (B,F,2) first pair | pair count of the frame in the main log's slot of the same index */
    int *pair_key;                /* (B,Q) i << 8 | j: i the detection's index in the frame, j the index into the frame's kept labels */
    int *pair_common;             /* (B,Q) the pair's `common` count (> 0) */
    int *rec_size;                /* (B,R) the detection's point count, aligned with the main log's records */
    int *label_size;              /* (B,R) the kept object's size, aligned with the main log's label entries */
} rtk_score_pairs_t;

/* rtk_track_score_logged (mem == NULL) or rtk_track_score_memory with a log, bit for bit -- every counter, state tensor, output and
 * tensor of rtk_score_log_t -- in the same single launch, which also appends the frame's pairs.  A frame is logged whole or not at
 * all: the fit test of the main log gains "its pairs fit Q", and a frame that does not fit is in neither log and raises
 * RTK_SCORE_FLAG_LOG (the only way the main log can differ from rtk_track_score_logged's).  Every word has one writer (detection i's
 * thread writes row i's pairs behind an ordered prefix of the rows' pair counts) and plain stores: the same bits on every run.  LDS:
 * rtk_track_score_lds_bytes / rtk_track_score_memory_lds_bytes, nothing more.  The caller zero-initialises the block; only this
 * entry point writes it. */
RTK_EXPORT int rtk_track_score_pairs(const rtk_track_score_in_t *in, const rtk_track_score_state_t *state, const rtk_track_score_out_t *out,
                                     const rtk_score_log_t *log, const rtk_score_memory_t *mem /* NULL: no track memory */,
                                     const rtk_score_pairs_t *pairs, rtk_stream_t stream);

/* The replay under the optimal matching, per (stream, threshold t), frames in log order:
 *   removal      the sweep's: a detection whose track score is < t is removed (equal stays).
 *   candidates   every logged pair (i, j, c) whose detection remains and whose IoU = (double)c / (double)(|i| + |j| - c) -- the
 *                logged integers, as rtk_track_score computes it -- is >= min_iou (float64 >=: an IoU equal to min_iou stays).  A
 *                pair whose denominator is not positive is no candidate (coincident points count once per PAIR, so c can exceed
 *                a size, and the IoU can exceed 1).
 *   assignment   la_solve (csrc/lds_assignment.h) with rows = detections, columns = kept objects and weight
 *                (1 << 23) + min(floor(iou * 65536), 65536): an IoU above 1 weighs as 1.  With at most 64 columns the IoU parts sum to at most 2^22, so the optimum is "most
 *                matches first, then the largest quantised IoU sum": the KITTI cost matrix with its max_cost sentinel.  The total
 *                weight is tp * 2^23 + iou_q: tp, fp, fn and iou_q are unique even where the optimal matching is not; which
 *                matching comes out is the solver's documented choice (rows enter in order, ties go to the smaller column).
 *   counters     frames | gt | pred (the remaining detections) | tp | fp | fn | idsw | frag | tracks | mt | pt | ml.  The per-clip
 *                track table is rtk_track_score's (append on first sight, 0.8 / 0.2 at the clip's close, idsw against the entry's
 *                last matched track id; clips still open are closed at the end).  frag += 1 for an entry that is matched now, was
 *                matched at some earlier frame, and was seen but unmatched in its previous seen frame.
 *   outputs      iou_q (count,B) int64 the sum of the quantised IoUs of the matches; iou_sum (count,B) float64 the matched IoUs
 *                added in kept-object order, frames in order, from 0; tp_mask as rtk_score_replay writes it (index 0 only).
 * Integers and ordered float64 sums only: the same bits on every run. */
#define RTK_SCORE_OPTIMAL_COUNTERS 12
/* Most candidate pairs of one frame: the edges of the assignment, sized from the LDS budget. */
#define RTK_SCORE_PAIR_EDGES 2048

/* LDS bytes of one workgroup of rtk_score_replay_optimal for T track-table entries (a host function: no device is touched); -1 for a
 * T below 1.  Built for two capacities, 1024 and the largest that fits RTK_SCORE_LDS_LIMIT; a T takes the smaller one that holds it:
 * this is that instance's figure, or for a larger T what its tables would need. */
RTK_EXPORT int rtk_score_optimal_lds_bytes(int T);

/* Grid (stream, threshold index), one wave each; the arguments rtk_score_replay takes, plus the pair log, min_iou (finite, > 0),
 * iou_q and flags.  The log is walked with rtk_score_replay's clamps, and a pair whose indices, sizes or count do not describe its
 * frame is skipped, so a foreign buffer is never read out of bounds.  A frame of stream b with more candidates than
 * RTK_SCORE_PAIR_EDGES raises RTK_SCORE_FLAG_OPTIMAL in flags[b] (or-ed in; nothing else of flags is touched): that stream's outputs
 * are then unspecified but written, the other streams are unaffected.  A T whose tables do not fit RTK_SCORE_LDS_LIMIT is refused. */
RTK_EXPORT int rtk_score_replay_optimal(int B, int T, const rtk_score_log_t *log, const rtk_score_pairs_t *pairs, const double *rec_score,
                                        const double *thresholds, const int *reached, int count, double min_iou,
                                        long long *counters /* (count,B,12) */, long long *iou_q /* (count,B) */,
                                        double *iou_sum /* (count,B) */, unsigned char *tp_mask /* NULL or (B,R) */, int *flags /* (B) */,
                                        rtk_stream_t stream);

/* ---- HOTA and the identity metrics under TrackEval's matching (csrc/track_hota_optimal.hip, csrc/track_identity_pairs.hip,
 *      csrc/lds_assignment.h, TrackScorer.hota(matching="optimal"), TrackScorer.identity(pairs="all")) ---------------------------------
 *
 * rtk_score_hota matches each detection to its single best object, first come first served, again at every alpha, and
 * rtk_score_identity sees only a detection's best object.  TrackEval does neither: its HOTA matches every frame ONCE, by a Hungarian
 * assignment over similarity x global alignment score, and thresholds the matched pairs at each alpha afterwards; its Identity counts
 * every pair above the threshold.  This section is that arrangement over the pair log.  WHAT NOW AGREES WITH TrackEval: the
 * arrangement of HOTA (alignment pass, one matching per frame for all alpha, the association sums) and of Identity (every pair, one
 * global assignment).  WHAT STILL DOES NOT: the similarity is the reference's POINT IoU, not a box IoU (the reference's result files
 * hold points: its own choice), and the frame's assignment is solved on scores truncated to 28 BITS (below).  rtk_score_hota and
 * rtk_score_identity are unchanged.
 *
 * HOTA under the optimal matching.  Per stream, per clip (the frames from one reset to the next), frames in log order.
 *   removal      the sweep's: with rec_score and a threshold t a detection whose track score is < t is removed before anything else,
 *                the alignment pass included (TrackEval filters the tracker data first).
 *   valid pair   a logged pair (i, j, c) of a frame whose key and indices describe the frame, with c > 0, whose detection i remains,
 *                and with den = |i| + |j| - c > 0.  Its similarity is s = (double)c / (double)den and sbar = min(s, 1.0): coincident
 *                points count once per PAIR, so the point IoU can exceed 1 -- the sums below and the weights take sbar, the alpha test
 *                and LocA take s unclamped, as rtk_score_hota takes rec_iou.
 *   alignment    per clip.  Every sum is float64, starts from 0.0 and adds one term after the other, no FMA.  Per frame r_i = the sum
 *                of sbar over detection i's valid pairs in pair-log order (j ascending) and k_j = the sum of sbar over object j's
 *                valid pairs in pair-log order (i ascending); per valid pair q = sbar / ((r_i + k_j) - sbar) (TrackEval's sim_iou).
 *                pmc[g,t] += q for g the label id of object j and t the track id of detection i: frames in order, then pairs in
 *                pair-log order.  cg[g] the frames of the clip whose kept labels contain g, ct[t] the remaining detections of the
 *                clip with track id t.  At the clip's close A[g,t] = pmc / ((double)(cg + ct) - pmc).
 *   matching     per frame, ONE MATCHING FOR ALL ALPHA: la_solve (csrc/lds_assignment.h) with rows = detections, columns = kept
 *                objects, one edge per valid pair of weight max(1, (int)floor(min(A[g,t] * sbar, 1.0) * 2^28)).  The matching is the
 *                solver's documented one (rows enter in order, ties go to the smaller column).  This is the one departure from
 *                TrackEval's arrangement: the float64 score is truncated to 28 bits so that the optimum is an integer, and the
 *                max(1, ...) keeps a positive overlap from vanishing; the float score of the optimum found therefore lies within
 *                min(P, G) * 2^-28 of the untruncated optimum -- that bound follows from the truncation, it is not measured.
 *   per level    alpha_a = (double)a / (double)(A + 1) as in rtk_score_hota.  A matched pair is a true positive iff s >= alpha
 *                (float64 >=: an IoU of 3/5 counts at 12/20).  tp += 1; loc += s, added in kept-object order within the frame,
 *                frames in order; n_a[g,t] += 1.  gt = sum cg and pred = sum ct.
 *   clip close   the clip's (g,t) with n_a > 0 IN ORDER OF FIRST APPEARANCE AMONG THE VALID PAIRS (frame order, then pair-log order):
 *                ass += N / (double)(cg + ct - n), ass_re += N / (double)cg, ass_pr += N / (double)ct with N = (double)(n*n) from the
 *                integer product, as rtk_score_hota adds them.  pairs = the number of those (g,t); frames and clips as there; clips
 *                still open are closed at the end.
 * Counters, sums and the host arithmetic are rtk_score_hota's (RTK_SCORE_HOTA_COUNTERS, RTK_SCORE_HOTA_SUMS, hota_values).
 *
 * Two launches.  rtk_score_alignment, one workgroup per stream, walks the log with a label table, a track table and the
 * insertion-ordered list of the clip's potential (g,t) -- those with a valid pair -- and walks every clip a second time at its close.
 * It leaves three tables, so that the second launch needs neither a label table nor a track table:
 *   pair_a       (B,Q) float64, aligned with pair_key: A[g,t] of every logged pair (0 where the pair is not valid);
 *   pair_index   (B,Q) int32, aligned with pair_key: the index of the pair's (g,t) in the stream's table of clip-pairs -- the clips'
 *                potential pairs one clip after the other, each clip's in order of first appearance -- or -1: removed or not valid;
 *   clip_cg, clip_ct   (B,Q) int32: cg and ct of every clip-pair (a clip-pair has a valid logged pair, so Q bounds their number).
 * rtk_score_hota_optimal, grid (stream, alpha index), then solves every frame and folds the sums.  Every level re-solves the same
 * assignment: the kernel is latency bound and the grid fills the device with it. */

/* Most potential (label id, track id) pairs of one clip of one stream in rtk_score_alignment: the list with its float64 sums and its
 * lookup take 24 bytes each, which next to a 1024-entry label table and the track table leaves room for these in RTK_SCORE_LDS_LIMIT
 * (62 496 bytes in all).  rtk_score_hota_optimal counts per clip-pair in the same number of words. */
#define RTK_SCORE_ALIGN_PAIRS 1024

/* LDS bytes of one workgroup of rtk_score_alignment for T label ids per clip (a host function: no device is touched); -1 for a T below
 * 1.  Built for two label capacities, 1024 and the largest that fits RTK_SCORE_LDS_LIMIT (1404); a T takes the smaller one that holds
 * it: this is that instance's figure, or for a larger T what its tables would need. */
RTK_EXPORT int rtk_score_alignment_lds_bytes(int T);

/* One workgroup per stream.  T bounds the label ids of one clip (rtk_track_score's T; a T whose tables do not fit RTK_SCORE_LDS_LIMIT is
 * refused), RTK_SCORE_SWEEP_TRACKS its track ids and RTK_SCORE_ALIGN_PAIRS its potential pairs.  A clip of stream b beyond one of the
 * three raises RTK_SCORE_FLAG_HOTA in flags[b] (or-ed in; nothing else of flags is touched): that stream's outputs are then
 * unspecified but written, the other streams are unaffected.  The logs are walked with rtk_score_replay_optimal's clamps, so a foreign
 * buffer is never read out of bounds.  Reads the logs, rec_score and threshold; writes its four tables -- for every logged pair of
 * every logged frame, and for every clip-pair -- and flags. */
RTK_EXPORT int rtk_score_alignment(int B, int T, const rtk_score_log_t *log, const rtk_score_pairs_t *pairs,
                                   const double *rec_score /* (B,R) or NULL */, const double *threshold /* device scalar, or NULL */,
                                   double *pair_a /* (B,Q) */, int *pair_index /* (B,Q) */, int *clip_cg /* (B,Q) */, int *clip_ct /* (B,Q) */,
                                   int *flags /* (B) */, rtk_stream_t stream);

/* Grid (stream, alpha index), one wave each: counters (alphas,B,6) and sums (alphas,B,4) of level a = index + 1 of `alphas` levels
 * (1..63), in rtk_score_hota's layouts.  rec_score and threshold must be those rtk_score_alignment was given.  A pair whose index does
 * not belong to its clip is skipped, so foreign tables are never read out of bounds.  A frame of stream b with more valid pairs than
 * RTK_SCORE_PAIR_EDGES raises RTK_SCORE_FLAG_OPTIMAL in flags[b] (or-ed in): that stream's outputs are then unspecified but written, the
 * other streams are unaffected.  Static LDS: 44 068 bytes.  Reads the logs and the four tables and writes only its three outputs. */
RTK_EXPORT int rtk_score_hota_optimal(int B, const rtk_score_log_t *log, const rtk_score_pairs_t *pairs,
                                      const double *rec_score /* (B,R) or NULL */, const double *threshold /* device scalar, or NULL */,
                                      int alphas, const double *pair_a, const int *pair_index, const int *clip_cg, const int *clip_ct,
                                      long long *counters /* (alphas,B,6) */, double *sums /* (alphas,B,4) */, int *flags /* (B) */,
                                      rtk_stream_t stream);

/* Identity over every pair.  rtk_score_identity with one change, in what a frame adds: n[g,t] is the number of frames of the clip in
 * which SOME REMAINING DETECTION with track id t has a VALID PAIR (above) with an object of label g and s >= alpha (float64 >=, s
 * unclamped).  A frame adds at most 1 to a pair; there is no best-object restriction, so a detection that overlaps two objects above
 * alpha counts for both, as TrackEval counts every pair above the threshold.  Everything after that is rtk_score_identity's: the
 * per-clip maximum-weight one-to-one matching by la_solve, gt, pred, the counters (RTK_SCORE_ID_COUNTERS; pairs = the distinct (g,t)
 * with n > 0), the limits and RTK_SCORE_FLAG_IDENTITY, and the host arithmetic (identity_values). */

/* LDS bytes of one workgroup of rtk_score_identity_pairs for T label ids per clip: rtk_score_identity_lds_bytes' rules and figures (the
 * words the pair walk adds lie where the solver's tables are larger). */
RTK_EXPORT int rtk_score_identity_pairs_lds_bytes(int T);

/* Grid (stream, level index): rtk_score_identity's arguments plus the pair log, which is walked with rtk_score_replay_optimal's
 * clamps.  Reads the logs, rec_score, threshold and alphas and writes only counters and flags. */
RTK_EXPORT int rtk_score_identity_pairs(int B, int T, const rtk_score_log_t *log, const rtk_score_pairs_t *pairs,
                                        const double *rec_score /* (B,R) or NULL */, const double *threshold /* device scalar, or NULL */,
                                        const double *alphas /* device, (count) */, int count, long long *counters /* (count,B,6) */,
                                        int *flags /* (B) */, rtk_stream_t stream);

/* ---- TrackEval's centre-distance similarity on the pair log (csrc/track_score.hip, csrc/track_optimal.hip and its siblings,
 *      TrackScorer(similarity="centre")) ----------------------------------------------------------------------------------------------
 *
 * The two sections above say that what still does not agree with TrackEval is the similarity: a point IoU where TrackEval has a box IoU.
 * The box IoU is the next section's (the detections have boxes: rtk_fused.h, "Oriented boxes"); this one is the similarity TrackEval
 * has for detections that are positions, _calculate_euclidean_similarity: sim = max(0, 1 - |a - b| / zero_distance), zero_distance = 2.0 by
 * default.  This section writes the pair log under that similarity and replays it with the four kernels above, unchanged in every other
 * respect.  The point IoU is harsh on radar clusters of two to five points (one missed point halves it); this one asks whether the
 * detection sits on its object.  DEPARTURES FROM TrackEval AFTER THIS: the 28-bit assignment weights, and the positions, which are point
 * centroids rather than label-box centres.
 *
 * Per active stream b and frame, with n the clamped n_valid, P detections and G kept objects, as in rtk_track_score.
 *   centre       of detection i: over the columns p < n with obj[b][p] == i, in ascending p, three float64 sums sx += (double)x_p, sy,
 *                sz, each from 0.0; c_i = (sx / m, sy / m, sz / m) with m the (double) number of such columns (the row's rec_size).  A
 *                detection with m == 0 has no pairs.  This is the rule rtk_gt_objects states for its own centres.
 *   position     of kept object j: gt_centre[b][j][0..2], float64 -- the tensor rtk_gt_objects writes as `centre`, in the kept order of
 *                gt_label_id: the mean of the points of the object's own box.  A merged rider does not move it.
 *   similarity   dx = c_i.x - g_j.x, dy, dz likewise; d2 = (dx * dx + dy * dy) + dz * dz; d = sqrt(d2); s = 1.0 - d / zero_distance.  All
 *                float64, every operation rounded on its own, no contraction.  (The device's double sqrt is the compiler's expansion;
 *                DESIGN section 4.9 has what was measured of it.)
 *   logging      the pair (i, j) is logged iff s > 0.0; a NaN is not logged.  The common point count does not matter: a pair with
 *                common == 0 and d < zero_distance is logged, a pair with common points whose centres are zero_distance apart is not.
 *   the log      pairs in (i, then j) order; pair_key = i << 8 | j as above; pair_common the pair's `common` count, which may now be 0;
 *                pair_sim (B,Q) float64, aligned with pair_key, is s.  rec_size, label_size, frame_pair and cursor as above.  A frame is
 *                logged whole or not at all, with the fit rule and RTK_SCORE_FLAG_LOG of rtk_track_score_pairs.
 *   replays      a logged pair is VALID iff its key describes its frame, its detection remains, and s = pair_sim[q] > 0.0.  pair_common
 *                and the sizes are not read.  Everything else in the replay sections above holds as written with "IoU" read as s:
 *                candidates s >= min_iou; weight (1 << 23) + min(floor(s * 65536), 65536); HOTA's sbar = min(s, 1.0), sim_iou, the
 *                alignment score and the 28-bit weights; Identity s >= alpha.
 *
 * rtk_score_pairs_t keeps its seven fields (its layout is pinned); the similarity travels beside it as one more argument, and a log has
 * ONE similarity: a block written by rtk_track_score_pairs_centre goes to the *_sim replays with its pair_sim, a block written by
 * rtk_track_score_pairs to the plain ones, which launch the kernels they always launched.  (Fed to the plain replays, a centre log would be
 * read as point IoUs of its integers: the caller keeps the two apart, as TrackScorer does by building one scorer per similarity.) */

/* rtk_track_score_pairs, bit for bit -- every counter, state tensor, output and tensor of the main log -- in the same single launch,
 * with the pair log written by the rules above.  Every word has one writer (detection i's thread forms its centre in registers and
 * writes row i's pairs behind the ordered prefix of the rows' pair counts), plain stores, no floating-point atomics: the same bits on
 * every run.  LDS: rtk_track_score_centre_lds_bytes -- the figure of rtk_track_score_lds_bytes / rtk_track_score_memory_lds_bytes rounded
 * up to 8 bytes, plus 24 K + 16: the kept objects' positions, zero_distance and the stream's pair_sim address are staged there at the
 * start, so that the three arguments are not carried in scalar registers through the body (with them carried, the compiler reserved a
 * private segment).  A column's detection index rides in the unused fourth word of its coordinates.  Refuses a NULL pair_sim, a NULL
 * gt_centre and a zero_distance that is not finite and > 0. */
RTK_EXPORT int rtk_track_score_centre_lds_bytes(int Kobj, int K, int N, int memory /* 0: no track memory */);
RTK_EXPORT int rtk_track_score_pairs_centre(const rtk_track_score_in_t *in, const rtk_track_score_state_t *state, const rtk_track_score_out_t *out,
                                            const rtk_score_log_t *log, const rtk_score_memory_t *mem /* NULL: no track memory */,
                                            const rtk_score_pairs_t *pairs, double *pair_sim /* (B,Q) */, const double *gt_centre /* (B,K,3) */,
                                            double zero_distance, rtk_stream_t stream);

/* The four replays on a log that carries its similarity: the arguments, grids, limits, flags, outputs and static LDS figures
 * (rtk_score_optimal_lds_bytes, rtk_score_alignment_lds_bytes, 44 068 bytes, rtk_score_identity_pairs_lds_bytes) of the entry points
 * without _sim, plus pair_sim (B,Q), which must not be NULL.  One wave of 64 threads per workgroup, kernels with names of their own. */
RTK_EXPORT int rtk_score_replay_optimal_sim(int B, int T, const rtk_score_log_t *log, const rtk_score_pairs_t *pairs, const double *pair_sim,
                                            const double *rec_score, const double *thresholds, const int *reached, int count, double min_iou,
                                            long long *counters /* (count,B,12) */, long long *iou_q /* (count,B) */,
                                            double *iou_sum /* (count,B) */, unsigned char *tp_mask /* NULL or (B,R) */, int *flags /* (B) */,
                                            rtk_stream_t stream);
RTK_EXPORT int rtk_score_alignment_sim(int B, int T, const rtk_score_log_t *log, const rtk_score_pairs_t *pairs, const double *pair_sim,
                                       const double *rec_score /* (B,R) or NULL */, const double *threshold /* device scalar, or NULL */,
                                       double *pair_a /* (B,Q) */, int *pair_index /* (B,Q) */, int *clip_cg /* (B,Q) */, int *clip_ct /* (B,Q) */,
                                       int *flags /* (B) */, rtk_stream_t stream);
RTK_EXPORT int rtk_score_hota_optimal_sim(int B, const rtk_score_log_t *log, const rtk_score_pairs_t *pairs, const double *pair_sim,
                                          const double *rec_score /* (B,R) or NULL */, const double *threshold /* device scalar, or NULL */,
                                          int alphas, const double *pair_a, const int *pair_index, const int *clip_cg, const int *clip_ct,
                                          long long *counters /* (alphas,B,6) */, double *sums /* (alphas,B,4) */, int *flags /* (B) */,
                                          rtk_stream_t stream);
RTK_EXPORT int rtk_score_identity_pairs_sim(int B, int T, const rtk_score_log_t *log, const rtk_score_pairs_t *pairs, const double *pair_sim,
                                            const double *rec_score /* (B,R) or NULL */, const double *threshold /* device scalar, or NULL */,
                                            const double *alphas /* device, (count) */, int count, long long *counters /* (count,B,6) */,
                                            int *flags /* (B) */, rtk_stream_t stream);

/* ---- The oriented-box IoU on the pair log, in three dimensions and in the bird's-eye view (csrc/track_score.hip,
 *      TrackScorer(similarity="box") / TrackScorer(similarity="box_bev")) --------------------------------------------------------------
 *
 * The evaluators the result files are written for (the KITTI devkit, AB3DMOT, TrackEval's loaders, the VoD devkit) match detections to
 * label boxes by a box overlap.  This section writes the pair log under that overlap -- between the box rtk_object_boxes fits to each
 * detection and the label box of each kept object -- and replays it with the four *_sim kernels above, unchanged.  DEPARTURES FROM
 * TrackEval AFTER THIS: the 28-bit assignment weights; THE UPRIGHT READING of the label box (below); and the detections' boxes, which
 * are fitted from their points (a minimum-area rectangle, not a regressed box).
 *
 * All arithmetic is float64, every operation rounded on its own, no contraction.  Per active stream b and frame, with P detections
 * and G kept objects as in rtk_track_score:
 *   detection    box i < P is row i of rtk_object_boxes' output for the same step: det_box (B,Kobj,8) float64 = cx, cy, cz, l, w, h, yaw,
 *                area; det_valid (B,Kobj) int32.  The detection HAS A BOX iff det_valid > 0, its first seven words are finite, l > 0 and
 *                w > 0, and under RTK_SCORE_BOX_3D also h > 0.  A detection without a box has no pairs: a cluster of two points, or of
 *                collinear points, fitted with min_extent = 0 has w = 0 and therefore none (fit with a positive min_extent).  L = 0.5 * l,
 *                W = 0.5 * w; the footprint is the l x w rectangle about (cx, cy) with its length along (c, s) = (cos yaw, sin yaw); its
 *                z range is [cz - 0.5 * h, cz + 0.5 * h].  (The device's sincos and sqrt are the compiler's expansions: not correctly
 *                rounded, which is why pair_sim is compared within a bound -- DESIGN section 4.9.)
 *   object       box j < G is entry gt_slot[b][j] of gt_boxes (B,K,16) float64, the frame-1 table of rtk_gt_boxes_t (centre | R | half-
 *                extent): the box whose membership test defined the object; a merged rider does not change it.  It is read UPRIGHT IN
 *                THE RADAR FRAME: u = (R[0][0], R[1][0]), n = sqrt(u.x * u.x + u.y * u.y), heading (hx, hy) = (u.x / n, u.y / n);
 *                footprint 2 h0 x 2 h1 about (c.x, c.y), a = h0 along the heading and b = h1 across; z range [c.z - h2, c.z + h2].  A
 *                slot outside [0, K), n == 0 or not finite, a half-extent that is not > 0, or one of the eight words read that is not
 *                finite: the object has no pairs.  THE DEPARTURE: the label box carries the radar-lidar calibration's small tilt
 *                (arccos(R[2][2]), about half a degree on the VoD calibration); the upright reading drops it, and the centre's z is
 *                whatever the table holds -- one reason the bird's-eye-view variant exists.
 *   prefilter    (part of the definition) dx = cx - c.x, dy = cy - c.y; ri = sqrt(L * L + W * W), rj = sqrt(a * a + b * b),
 *                rr = ri + rj; a pair with (dx * dx + dy * dy) > rr * rr has s = 0.
 *   z overlap    (RTK_SCORE_BOX_3D only) zo = min(top_i, top_j) - max(bottom_i, bottom_j); zo <= 0: s = 0.
 *   frame        coordinates relative to the object's centre, in the object's own frame: D = (dx * hx + dy * hy, dy * hx - dx * hy),
 *                E = (ex, ey) = (c * hx + s * hy, s * hx - c * hy), E' = (-ey, ex).  The detection's corners, counter-clockwise:
 *                D + LE + WE', D - LE + WE', D - LE - WE', D + LE - WE' with LE = (L * ex, L * ey) and WE' = (-(W * ey), W * ex), each
 *                coordinate (D + LE) then WE', in that order of additions.  The object's rectangle there is |x| <= a, |y| <= b.
 *   cut          Sutherland-Hodgman: the detection's outline is cut by the four half-planes x <= a, x >= -a, y <= b, y >= -b in this
 *                order.  The outline is kept as directed edges in eight slots: the four edges corner k -> corner k + 1 in slots 0..3,
 *                and slot 4 + k for the edge cut k adds.  Cut k, with sigma(P) = a - P.x, P.x + a, b - P.y, P.y + b, looks at every
 *                edge P0 -> P1 present, in slot order: both ends have sigma >= 0: it stays; both have sigma < 0: it goes; otherwise
 *                t = sigma(P0) / (sigma(P0) - sigma(P1)) and the crossing point X has its cut coordinate SET TO THE BOUND ITSELF (a,
 *                -a, b, -b) and the other one P0 + t * (P1 - P0) (that coordinate's); an edge that leaves (sigma(P0) >= 0) ends at X,
 *                an edge that comes back starts at X.  If an edge left and an edge came back, slot 4 + k is the edge from the point
 *                where the outline left to the point where it came back (of several, the last in slot order).  Every crossing point is
 *                formed once and serves both edges that meet in it, so edges that nearly coincide with a bound cost rounding, not
 *                area; boxes touching along an edge or at a corner have I2 = 0 exactly when they are parallel to the axes.
 *   I2           Green's theorem: acc = the sum, from 0.0 in slot order, over the edges present of (P0.x * P1.y - P1.x * P0.y);
 *                I2 = 0.5 * acc.  With yaw = 0, R = identity and dyadic coordinates and extents every operation up to here is exact.
 *   value        A_i = l * w, A_j = (2a) * (2b).  BEV: s = I2 / ((A_i + A_j) - I2).  3D: I3 = I2 * zo, V_i = A_i * h,
 *                V_j = A_j * (top_j - bottom_j), s = I3 / ((V_i + V_j) - I3).  Then s = min(s, 1.0): unlike the point IoU, a box IoU
 *                above 1 is only rounding.
 *   logging      the pair (i, j) is logged iff s > 0.0; a NaN is not logged.  Order, pair_key, pair_common (which may be 0), rec_size,
 *                label_size, frame_pair, the cursor, the whole-frame fit rule and RTK_SCORE_FLAG_LOG are those of
 *                rtk_track_score_pairs_centre, and the replays' validity rule is the centre section's: a log written here goes to the
 *                *_sim replays with its pair_sim.  */
#define RTK_SCORE_BOX_3D 0
#define RTK_SCORE_BOX_BEV 1

/* rtk_track_score_pairs, bit for bit -- every counter, state tensor, output and tensor of the main log -- in the same single launch,
 * with the pair log written by the rules above.  Thread j stages kept object j's upright box in LDS; the P G decisions s > 0 are spread
 * over the workgroup's 256 threads, each raising a bit of its row's 64-bit mask in LDS (an integer OR); thread i then writes row i's
 * pairs behind the ordered prefix of the rows' pair counts, forming each s again by the same operations: one writer per word of the
 * log, plain stores, no floating-point atomics, the same bits on every run.  LDS: rtk_track_score_box_lds_bytes -- the figure of rtk_track_score_lds_bytes /
 * rtk_track_score_memory_lds_bytes rounded up to 8 bytes, plus 64 K + 16 (eight float64 per kept object, the mode and the stream's
 * pair_sim address).  Refuses a NULL pair_sim, det_box, det_valid or gt_boxes and a mode that is neither of the two. */
RTK_EXPORT int rtk_track_score_box_lds_bytes(int Kobj, int K, int N, int memory /* 0: no track memory */);
RTK_EXPORT int rtk_track_score_pairs_box(const rtk_track_score_in_t *in, const rtk_track_score_state_t *state, const rtk_track_score_out_t *out,
                                         const rtk_score_log_t *log, const rtk_score_memory_t *mem /* NULL: no track memory */,
                                         const rtk_score_pairs_t *pairs, double *pair_sim /* (B,Q) */, const double *det_box /* (B,Kobj,8) */,
                                         const int *det_valid /* (B,Kobj) */, const double *gt_boxes /* (B,K,16) */, int mode,
                                         rtk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RTK_SCORE_H */
