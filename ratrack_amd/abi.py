"""The C ABI of librtk_hip.so (include/*.h), restated for ctypes: this module is the only place where that is done.

STRUCTS maps every struct typedef of the headers to its ctypes mirror, SIGNATURES every compute entry point to its argtypes (restype is
always int); both follow the headers, header by header and in header order.  tests/test_abi_cpu.py checks both against the headers: the
kind of every argument, and every struct's field names, order, offsets and size as a C compiler lays them out.  A new entry point or
struct is added here and nowhere else.  stream(), ptr() and view() build the argument values that have no Python type of their own.
"""
import ctypes

import torch

_i, _l, _f, _d, _p = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_double, ctypes.c_void_p
_ip, _fp, _pp, P = ctypes.POINTER(_i), ctypes.POINTER(_f), ctypes.POINTER(_p), ctypes.POINTER


# ---- include/rtk_fused.h --------------------------------------------------------------------------------------------------------

class Src(ctypes.Structure):
    _fields_ = [("ptr", _p), ("pitch", _i), ("channels", _i), ("per_sample", _i)]


class Layer(ctypes.Structure):
    _fields_ = [("w_packed", _p), ("bias", _p), ("cin16", _i), ("cout16", _i), ("act", _i), ("inv_scale", _f)]


class Interp(ctypes.Structure):
    _fields_ = [("known_feats", _p), ("pitch", _i), ("channels", _i), ("m", _i), ("idx", _p), ("dist2", _p), ("nuniq", _p)]


class GtermJob(ctypes.Structure):
    _fields_ = [("wt", _p), ("bias", _p), ("out", _p), ("cout", _i), ("s0", _i), ("count", _i), ("out_pitch", _i), ("wt2", _p), ("s2", _i)]


class CopyJob(ctypes.Structure):
    _fields_ = [("src", _p), ("dst", _p), ("bytes", _l)]


class LayoutJob(ctypes.Structure):
    _fields_ = [("src", _p), ("dst", _p), ("channels", _i), ("src_pitch", _i), ("per_sample", _i), ("dst_channels", _i),
                ("dst_channel_offset", _i)]


class View(ctypes.Structure):
    _fields_ = [("ptr", _p), ("sb", ctypes.c_longlong), ("sc", ctypes.c_longlong), ("sp", ctypes.c_longlong)]


class TrackFrame(ctypes.Structure):
    _fields_ = [("B", _i), ("N", _i), ("pc1", View), ("flow", View), ("feature1", View), ("prop", View), ("cls", View), ("n_valid", _p),
                ("active", _p)]


class ResultLog(ctypes.Structure):
    _fields_ = [("F", _i), ("R", _i), ("P", _i)] + [(n, _p) for n in ("cursor", "frame", "tag", "rec_track", "rec_conf", "rec_hits", "rec_size",
                                                                      "points", "flags")]


class BoxFilter(ctypes.Structure):
    _fields_ = [(n, _d) for n in ("r_pos", "r_yaw", "r_size", "q_pos", "q_vel", "q_yaw", "q_size", "p0", "p0_vel")] + \
               [(n, _i) for n in ("symmetry", "max_gap", "smooth", "size_rule", "size_percent")]


# ---- include/rtk_gt.h -----------------------------------------------------------------------------------------------------------

class GtBoxes(ctypes.Structure):
    _fields_ = [("boxes", _p), ("box_id", _p), ("count", _p)]


class GtIn(ctypes.Structure):
    _fields_ = [("B", _i), ("N", _i), ("N2", _i), ("K", _i), ("pc1", View), ("pc2", View), ("n_valid", _p), ("frame1", GtBoxes),
                ("frame2", GtBoxes), ("pair", _p), ("motion", _p), ("ego", _p)]


class GtOut(ctypes.Structure):
    _fields_ = [(n, _p) for n in ("gt_cls", "box_index", "obj_id", "gt_warp", "pc1_comp", "counts1", "counts2", "flags")]


class EvalIn(ctypes.Structure):
    _fields_ = [("B", _i), ("N", _i), ("pc1", View), ("warp", View), ("gt_warp", View), ("cls", View), ("mask", _p), ("gt_cls", _p),
                ("threshold", _f), ("n_valid", _p), ("active", _p)]


# ---- include/rtk_score.h --------------------------------------------------------------------------------------------------------

class GtObjectsIn(ctypes.Structure):
    _fields_ = [("B", _i), ("N", _i), ("K", _i), ("pc1", View), ("n_valid", _p), ("frame1", GtBoxes), ("types", _p), ("min_obj_points", _i)]


class GtObjectsOut(ctypes.Structure):
    _fields_ = [(n, _p) for n in ("slot", "label_id", "count", "size", "members", "centre", "flags")]


class ScoreIn(ctypes.Structure):
    _fields_ = [("B", _i), ("N", _i), ("Kobj", _i), ("K", _i), ("T", _i), ("pc1", View)] + \
               [(n, _p) for n in ("obj", "num_objects", "object_ids", "n_valid", "gt_slot", "gt_label_id", "gt_count", "gt_size", "gt_members",
                                  "reset", "active")]


class ScoreState(ctypes.Structure):
    _fields_ = [(n, _p) for n in ("counters", "iou_sum", "table_key", "table_last", "table_seen", "table_matched", "table_used", "prev_gt_id",
                                  "prev_count", "prev_gt", "flags")]


class ScoreOut(ctypes.Structure):
    _fields_ = [(n, _p) for n in ("pred_gt_slot", "pred_gt_id", "gt_pred", "iou", "aff_target", "aff_defined")]


class ScoreLog(ctypes.Structure):
    _fields_ = [("F", _i), ("R", _i)] + [(n, _p) for n in ("object_conf", "cursor", "frame", "label", "rec_track", "rec_best", "rec_conf",
                                                            "rec_iou")]


class ScoreMemory(ctypes.Structure):
    _fields_ = [(n, _p) for n in ("table_ids", "table_count", "row_track", "labelled_coasted")]


class ScorePairs(ctypes.Structure):
    _fields_ = [("Q", _i)] + [(n, _p) for n in ("cursor", "frame_pair", "pair_key", "pair_common", "rec_size", "label_size")]


# ---- include/rtk_train.h --------------------------------------------------------------------------------------------------------

class BnFin(ctypes.Structure):
    _fields_ = [("sums", _p), ("count", _d), ("gamma", _p), ("beta", _p), ("eps", _f), ("momentum", _f), ("running_mean", _p),
                ("running_var", _p), ("num_batches_tracked", _p), ("group_counts", _p)]


class TnJob(ctypes.Structure):
    _fields_ = [("x", _p), ("y", _p), ("out", _p), ("out_pitch", _i), ("x_amax", _p), ("y_amax", _p)]


class PackJob(ctypes.Structure):
    _fields_ = [("src", _p), ("src2", _p), ("dst", _p), ("rows", _i), ("cols", _i), ("pitch", _i), ("transpose", _i), ("kind", _i)]


class InverseIndexJob(ctypes.Structure):
    _fields_ = [("n_src", _i), ("positions", _i), ("idx", _p), ("off", _p), ("inv", _p), ("live", _p), ("live_mult", _i)]


class PoolSrc(ctypes.Structure):
    _fields_ = [("dout", _p), ("karg", _p), ("par", _p), ("sums2", _p), ("dgamma_dbeta", _p)]


class PwOperand(ctypes.Structure):
    _fields_ = [("ptr", _p), ("sample_stride", _l), ("pitch", _i), ("channels", _i), ("layout", _i), ("col0", _i)]


class PwWgradJob(ctypes.Structure):
    _fields_ = [("samples", _i), ("positions", _i), ("dz", P(PwOperand)), ("nsrc", _i), ("srcs", P(PwOperand)), ("dw", _p), ("w_pitch", _i),
                ("dbias", _p)]


STRUCTS = {
    "rtk_src_t": Src, "rtk_layer_t": Layer, "rtk_interp_t": Interp, "rtk_gterm_job_t": GtermJob, "rtk_copy_job_t": CopyJob,
    "rtk_layout_job_t": LayoutJob, "rtk_bcn_view_t": View, "rtk_track_frame_t": TrackFrame,
    "rtk_result_log_t": ResultLog, "rtk_box_filter_t": BoxFilter,
    "rtk_gt_boxes_t": GtBoxes, "rtk_gt_in_t": GtIn, "rtk_gt_out_t": GtOut, "rtk_eval_in_t": EvalIn,
    "rtk_gt_objects_in_t": GtObjectsIn, "rtk_gt_objects_out_t": GtObjectsOut, "rtk_track_score_in_t": ScoreIn,
    "rtk_track_score_state_t": ScoreState, "rtk_track_score_out_t": ScoreOut, "rtk_score_log_t": ScoreLog,
    "rtk_score_memory_t": ScoreMemory, "rtk_score_pairs_t": ScorePairs,
    "rtk_bn_fin_t": BnFin, "rtk_tn_job_t": TnJob, "rtk_pack_job_t": PackJob, "rtk_inverse_index_job_t": InverseIndexJob,
    "rtk_pool_src_t": PoolSrc, "rtk_pw_operand_t": PwOperand, "rtk_pw_wgrad_job_t": PwWgradJob,
}

# name -> argtypes.  A struct pointer that callers pass as ctypes.addressof() is _p; one they pass as an array or byref() is typed.
# The argument blocks of rtk_gt.h and rtk_score.h (GtIn, GtOut, EvalIn, GtObjectsIn, ..., ScoreOut, ScoreLog, ScoreMemory, ScorePairs), rtk_track_frame_t, rtk_result_log_t and rtk_box_filter_t go by
# address; the *_lds_bytes are host functions that return a byte count.
SIGNATURES = {
    # ---- include/rtk_pointnet2.h
    "rtk_furthest_point_sampling": [_i] * 3 + [_p] * 3 + [_p],
    "rtk_gather_points": [_i] * 4 + [_p] * 3 + [_p],
    "rtk_gather_points_grad": [_i] * 4 + [_p] * 3 + [_p],
    "rtk_ball_query": [_i] * 3 + [_f, _i] + [_p] * 3 + [_p],
    "rtk_group_points": [_i] * 5 + [_p] * 3 + [_p],
    "rtk_group_points_grad": [_i] * 5 + [_p] * 3 + [_p],
    "rtk_group_points_grad_set": [_i] * 5 + [_p] * 3 + [_p],
    "rtk_three_nn": [_i] * 3 + [_p] * 4 + [_p],
    "rtk_knn": [_i] * 4 + [_p] * 4 + [_p],
    "rtk_three_interpolate": [_i] * 4 + [_p] * 4 + [_p],
    "rtk_three_interpolate_grad": [_i] * 4 + [_p] * 4 + [_p],
    "rtk_three_interpolate_grad_set": [_i] * 4 + [_p] * 4 + [_p],
    "rtk_knn_point": [_i] * 4 + [_p] * 3 + [_p],
    # ---- include/rtk_fused.h
    "rtk_pointwise_mlp": [_i, _i, P(Interp), _i, P(Src), _p, _i, P(Layer), _p, _i, _i, _i, _p, _p, _p],
    "rtk_pointwise_mlp_pipelined": [_i, _i, P(Interp), _i, P(Src), _p, _i, P(Layer), _p, _i, _i, _i, _p, _p, _p],
    "rtk_pointwise_mlp_tap": [_i, _i, P(Interp), P(Layer), _p, _i, _p, P(Layer), _i, _p, _i, _p],
    "rtk_pointwise_mlp_tap_pipelined": [_i, _i, P(Interp), P(Layer), _p, _i, _p, P(Layer), _i, _p, _i, _p],
    "rtk_pointwise_mlp_pair": [_i, _i, _i, P(Src), _p, P(Layer), _p, _i, _i, _i, P(Layer), _p, _i, _p],
    "rtk_sa_scale": [_i] * 4 + [_p] * 4 + [_i, _i, _p, _i, P(Layer), _p, _i, _i, _p, _p, _p],
    "rtk_sa_scale_serial": [_i] * 4 + [_p] * 4 + [_i, _i, _p, _i, P(Layer), _p, _i, _i, _p, _p, _p],
    "rtk_cost_volume": [_i] * 3 + [_p] * 6 + [P(Layer), P(Layer), _p, _i, _p],
    "rtk_patch_cost": [_i] * 2 + [_p] * 3 + [_i, P(Layer), _p, _i, _i, _p],
    "rtk_patch_cost_wave16": [_i] * 2 + [_p] * 3 + [_i, P(Layer), _p, _i, _i, _p],
    "rtk_pack_split_layer": [_i, _i, _p, _i, _p, _p, _p],
    "rtk_cost_volume_split": [_i] * 3 + [_p] * 10 + [P(Layer), _p, _i, _p],
    "rtk_cost_volume_split_shared": [_i] * 3 + [_p] * 10 + [P(Layer), _p, _i, _i, _p],
    "rtk_cost_volume_split_gconst": [_i] * 3 + [_p] * 10 + [P(Layer), _p, _i, _i, _p],
    "rtk_cost_volume_split_term": [_i] * 3 + [_p] * 11 + [P(Layer), _p, _i, _i, _p],
    "rtk_pack_split_layer16": [_i, _i, _p, _i, _p, _p, _p],
    "rtk_cost_volume_split16_shared": [_i] * 3 + [_p] * 10 + [P(Layer), _p, _i, _i, _p],
    "rtk_cost_volume_split16_term": [_i] * 3 + [_p] * 11 + [P(Layer), _p, _i, _i, _p],
    "rtk_sa_scale_split": [_i] * 4 + [_p] * 4 + [_i, _i, _p, _p, _p, _p, _p, _i, _i, _p, _p, _p],
    "rtk_sa_scale_split_serial": [_i] * 4 + [_p] * 4 + [_i, _i, _p, _p, _p, _p, _p, _i, _i, _p, _p, _p],
    "rtk_split_mlp2": [_i, _p, _p, _p, _p, _p, _p, _p],
    "rtk_prepare_inputs": [_i] * 2 + [_p] * 6 + [_p],
    "rtk_fps_centroids": [_i] * 3 + [_p] * 8 + [_p],
    "rtk_knn_point_masked": [_i] * 4 + [_p] * 4 + [_p],
    "rtk_fps_relevel": [_i] * 3 + [_p] * 9 + [_i, _p, _p],
    "rtk_gru_step": [_i] * 3 + [_p] * 8 + [_p],
    "rtk_gru_step_head": [_i] * 3 + [_p] * 11 + [_i, _p],
    "rtk_global_terms": [_i, _i, _p, _i, P(GtermJob), _p, _i, _i, _p],
    "rtk_copy_multi": [_i, P(CopyJob), _p],
    "rtk_to_channel_major": [_i] * 3 + [_p, _i, _i, _p, _i, _i, _p],
    "rtk_ball_query_pair": [_i] * 3 + [_f, _i, _f, _i] + [_p] * 5 + [_p],
    "rtk_three_nn_masked": [_i] * 3 + [_p] * 6 + [_p],
    "rtk_geometry_front": [_i] * 4 + [_p, _p, _i] + [_p] * 13 + [_p, _p, _i, _p],
    "rtk_geometry_tables": [_i] * 3 + [_p] * 3 + [_fp, _ip, _pp, _pp, _pp, _p],
    "rtk_to_channel_major_multi": [_i] * 3 + [_p, _p],
    "rtk_log_sinkhorn": [_i, _i, _p, _f, _i, _p, _p],
    "rtk_dbscan": [_i, _p, _i, _p, _p, _f, _d, _i, _p, _p],
    "rtk_dbscan_batched": [_p, _f, _d, _i, _i, _p, _p, _p, _p, _p, _l, _p],
    "rtk_object_descriptors": [_p, _i, _p, _p, _p, _p, _p, _p],
    "rtk_affinity_pairs": [_i, _i] + [_p] * 7 + [_p],
    "rtk_associate_batched": [_i] * 3 + [_p] * 7 + [_f, _i] + [_p] * 9 + [_p],
    "rtk_associate_optimal": [_i] * 3 + [_p] * 7 + [_d] + [_p] * 9 + [_p],
    "rtk_associate_optimal_lds_bytes": [_i],
    "rtk_track_memory": [_i] * 3 + [_p] * 21 + [_p],
    "rtk_track_memory_motion": [_i] * 3 + [_f] + [_p] * 24 + [_p],
    "rtk_track_max_objects": [],
    "rtk_result_log_append": [_i] * 3 + [_p] * 12 + [_p],
    "rtk_result_log_select": [_i, _p, _p, _d, _i, _i, _p, _p, _p, _p, _p],
    "rtk_result_log_boxes": [_i, _p, _p, _d] + [_p] * 4 + [_p],
    "rtk_object_boxes": [_i] * 3 + [_p] * 4 + [_d] + [_p] * 4 + [_p],
    "rtk_result_log_filter_boxes": [_i] + [_p] * 12 + [_p],
    "rtk_track_box_filter_step": [_i] * 2 + [_p] * 17 + [_p],
    # ---- include/rtk_gt.h
    "rtk_gt_labels": [_p, _p, _p],
    "rtk_eval_frame": [_p, _p, _p, _p],
    # ---- include/rtk_score.h
    "rtk_gt_objects_lds_bytes": [_i, _i],
    "rtk_track_score_lds_bytes": [_i, _i, _i],
    "rtk_track_score_memory_lds_bytes": [_i, _i, _i],
    "rtk_gt_objects": [_p, _p, _p],
    "rtk_track_score": [_p, _p, _p, _p],
    "rtk_track_score_logged": [_p, _p, _p, _p, _p],
    "rtk_track_score_memory": [_p, _p, _p, _p, _p, _p],
    "rtk_score_track_means": [_i, _p, _p, _p, _p],
    "rtk_score_thresholds": [_p, _p, _p, _i, _p, _p, _p],
    "rtk_score_replay": [_i, _i, _p, _p, _p, _p, _i, _p, _p, _p, _p],
    "rtk_score_hota": [_i, _i, _p, _p, _p, _i, _p, _p, _p, _p],
    "rtk_score_identity_lds_bytes": [_i],
    "rtk_score_identity": [_i, _i, _p, _p, _p, _p, _i, _p, _p, _p],
    "rtk_track_score_pairs": [_p, _p, _p, _p, _p, _p, _p],
    "rtk_score_optimal_lds_bytes": [_i],
    "rtk_score_replay_optimal": [_i, _i, _p, _p, _p, _p, _p, _i, _d, _p, _p, _p, _p, _p, _p],
    "rtk_score_alignment_lds_bytes": [_i],
    "rtk_score_alignment": [_i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p],
    "rtk_score_hota_optimal": [_i, _p, _p, _p, _p, _i, _p, _p, _p, _p, _p, _p, _p, _p],
    "rtk_score_identity_pairs_lds_bytes": [_i],
    "rtk_score_identity_pairs": [_i, _i, _p, _p, _p, _p, _p, _i, _p, _p, _p],
    "rtk_track_score_centre_lds_bytes": [_i, _i, _i, _i],
    "rtk_track_score_pairs_centre": [_p, _p, _p, _p, _p, _p, _p, _p, _d, _p],
    "rtk_track_score_box_lds_bytes": [_i, _i, _i, _i],
    "rtk_track_score_pairs_box": [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _p],
    "rtk_score_replay_optimal_sim": [_i, _i, _p, _p, _p, _p, _p, _p, _i, _d, _p, _p, _p, _p, _p, _p],
    "rtk_score_alignment_sim": [_i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p],
    "rtk_score_hota_optimal_sim": [_i, _p, _p, _p, _p, _p, _i, _p, _p, _p, _p, _p, _p, _p, _p],
    "rtk_score_identity_pairs_sim": [_i, _i, _p, _p, _p, _p, _p, _p, _i, _p, _p, _p],
    # ---- include/rtk_train.h
    "rtk_bn_train_stats": [_i] * 5 + [_p] * 3 + [_p],
    "rtk_bn_relu_fwd": [_i] * 5 + [_p, _p, _i, _p, _p],
    "rtk_bn_relu_fwd_fin": [_i] * 5 + [_p, _p, _p, _i, _p, _p],
    "rtk_bn_relu_pool_fwd_fin_arg": [_i] * 5 + [_p, _p, _p, _p, _p, _p, _p],
    "rtk_pool_bwd_stats_arg": [_i] * 4 + [_p] * 5 + [_p],
    "rtk_bn_relu_bwd_stats": [_i] * 5 + [_p, _p, _p, _i, _p, _p],
    "rtk_bn_relu_bwd_apply": [_i] * 5 + [_p] * 5 + [_d, _p, _i, _p, _p, _p],
    "rtk_bn_relu_bwd_small": [_i] * 4 + [_p] * 4 + [_d, _p, _p, _p, _i, _p],
    "rtk_sa_first_layer": [_i] * 6 + [_p] * 4 + [_i] + [_p] * 3 + [_p],
    "rtk_tn_gemm256_split": [_i, P(TnJob), _l, _p, _l, _p],
    "rtk_absmax": [_p, _l, _p, _p],
    "rtk_pack_weights": [_i, _p, _p],
    "rtk_group_inverse_index": [_i] * 3 + [_p] * 3 + [_p],
    "rtk_group_inverse_index_multi": [_i, _i, P(InverseIndexJob), _p],
    "rtk_three_interpolate_grad_gather": [_i] * 4 + [_p] * 6 + [_p],
    "rtk_sa_first_layer_bwd": [_i] * 5 + [_p] * 6 + [_i, _p, _p],
    "rtk_conv_bn_fwd": [_i] * 6 + [_p] * 7 + [_p],
    "rtk_conv_bn_fwd_fin": [_i] * 6 + [_p] * 8 + [_p],
    "rtk_conv_bn_bwd": [_i] * 6 + [_p] * 6 + [_d, _i, _p, _p, _p],
    "rtk_conv_wgrad": [_i] * 6 + [_p] * 5 + [_l, _p],
    "rtk_conv_wgrad_stats": [_i] * 6 + [_p, P(PoolSrc), _p, _p, _p, _d, _p, _p, _p, _p, _p, _p, _l, _p],
    "rtk_conv_bn_bwd_apply": [_i] * 6 + [_p, P(PoolSrc), _p, _p, _p, _p, _p, _d, _p, _p, _p],
    "rtk_pw_conv": [_i, _i, _i, P(PwOperand), _i, P(PwOperand), _p, _i, _i, _p, _i, _p, _i, _p, _i, _p],
    "rtk_pw_wgrad": [_i, _i, P(PwOperand), _i, P(PwOperand), _p, _i, _p, _p, _l, _p],
    "rtk_pw_wgrad_multi": [_i, P(PwWgradJob), _p, _l, _p],
    "rtk_cost_volume_train": [_i] * 3 + [_p] * 6 + [P(Layer), P(Layer), _p, _i, _p, _p, _p, _p, _p, _p],
    "rtk_cost_volume_bwd": [_i] * 3 + [_p] * 3 + [P(Layer), P(Layer), _p, _p, _i] + [_p] * 12 + [_p],
    "rtk_cost_volume_split_train": [_i] * 3 + [_p] * 10 + [P(Layer), _p, _i, _p, _p, _p, _p, _p, _p, _p],
    "rtk_cost_volume_bwd_split": [_i] * 3 + [_p] * 5 + [P(Layer), _p, _i] + [_p] * 13 + [_p],
    "rtk_patch_cost_bwd": [_i, _i, _p, _p, _p, _i, P(Layer), _p, _p, _i, _p, _p, _p, _p, _p, _p],
    "rtk_patch_dfeat_gather": [_i, _i, _p, _p, _p, _p, _p, _p, _i, _p, _p, _p, _p],
    "rtk_train_group_geometry": [_i] * 5 + [_p] * 3 + [_i] + [_p] * 3 + [_p],
    "rtk_train_interp_weights": [_i] * 3 + [_p] * 5 + [_p],
    "rtk_train_row_weights": [_i] * 3 + [_p] * 2 + [_p],
    "rtk_train_point_weights": [_i] * 3 + [_p] * 3 + [_p],
    "rtk_gru_pack_params": [_i, _i, _pp] + [_p] * 6 + [_p],
    "rtk_gru_step_bwd": [_i] * 3 + [_p] * 15 + [_p],
    "rtk_gru_wgrad": [_i] * 3 + [_p] * 9 + [_p],
    "rtk_scatter_add_rows": [_i] * 4 + [_p] * 3 + [_p],
    "rtk_weightnet_bwd": [_l, _i] + [_p] * 14 + [_l, _p],
    "rtk_gmax_cat_fwd": [_i, _i, _i, _p, _p, _p, _p],
    "rtk_gmax_cat_bwd": [_i, _i, _i, _p, _p, _p, _p],
    "rtk_backbone_loss": [_i, _i, _p, _p, _p, _p, _p, _i, _i, _p, _p, _p, _p, _p],
    "rtk_adam_multi": [_i, _p, _l, _p, _f, _f, _f, _f, _f, _p, _p],
    "rtk_affinity_train": [_i, _i] + [_p] * 12 + [_i] + [_p] * 5 + [_l, _p],
    "rtk_affinity_wgrad": [_i, _i, _p, _p, _l, _p, _p],
    "rtk_object_descriptors_bwd": [_p, _i] + [_p] * 6 + [_p],
}


# ---- argument values ------------------------------------------------------------------------------------------------------------

def stream():
    """rtk_stream_t: the current HIP stream."""
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    """A tensor's device address, or NULL for None (an optional argument)."""
    return t.data_ptr() if t is not None else None


def view(t):
    """(B,C,N) or (B,N) fp32 CUDA tensor, any strides -> rtk_bcn_view_t (read in place: no copy)."""
    assert t.is_cuda and t.dtype == torch.float32, (t.device, t.dtype)
    if t.dim() == 2:
        return View(t.data_ptr(), t.stride(0), 0, t.stride(1))
    return View(t.data_ptr(), t.stride(0), t.stride(1), t.stride(2))
