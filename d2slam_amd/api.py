"""Host-side mirror of the reference's operator interface for the feature hot path, on top of the C ABI
(include/d2fe.h, libd2fe_hip.so).

Mirrors (names / argument meaning / error behaviour):
  * SuperPointConfig + SuperPoint.build()/infer()   d2frontend/include/d2frontend/CNN/superpoint_tensorrt.h:17-48
  * matchKNN(desc_a, desc_b, knn_match_ratio, pts_a, pts_b, search_local_dist)   d2frontend/include/d2frontend/feature_matcher.h:6-11
  * cv::BFMatcher(NORM_L2, crossCheck=True).match    loop_cam.cpp:167-170
  * getFeatureHalfImg                                d2frontend/src/d2featuretracker.cpp:1051-1075

There is NO CPU fallback: if libd2fe_hip.so is missing or no GPU is visible these calls raise.
"""
import ctypes as C
import os
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from .weights import SP_LAYERS

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libd2fe_hip.so")
DEV_LIB_PATH = os.path.join(_HERE, "lib", "libd2fe_hip_dev.so")      # -DD2FE_DEVTOOLS: d2fe_debug_* test hooks, phase stamps, D2FE_* schedule switches
if os.environ.get("D2FE_LIB"):      # developer knob: same-box A/B of two builds of the library (tools/gpu_run.sh ab)
    LIB_PATH = os.path.abspath(os.environ["D2FE_LIB"])

POSTPROC_B, POSTPROC_A = 0, 1
PREC_F32, PREC_F16X2, PREC_F32_WINO, PREC_F16 = 0, 1, 2, 3
PREC_I8 = 5      # int8 operands, int32 accumulation (4 is unassigned); needs FrontEnd.set_int8_ranges after load_superpoint
ERR_TRUNCATED = -4            # d2fe_status: output capacity too small, n_out holds what was written
KEEP_ALL_CAP = 1024           # host-pointer staging capacity of a keep-all handle (max_keypoints = -1)
PROF_STAGES = ["conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b", "convPaDa",
               "convPb", "convDb", "softmax_cand", "select", "sample", "match", "netvlad", "lk"]


class D2FEError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("d2fe error %d: %s" % (code, msg))
        self.code = code


class _Config(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("device_id", C.c_int32), ("max_width", C.c_int32),
                ("max_height", C.c_int32), ("max_batch", C.c_int32), ("max_keypoints", C.c_int32),
                ("remove_borders", C.c_int32), ("keypoint_threshold", C.c_float), ("postproc", C.c_int32),
                ("nms_dist", C.c_int32), ("precision", C.c_int32), ("keep_score_map", C.c_int32),
                ("dense_descriptors", C.c_int32), ("async_tail", C.c_int32), ("variant_b_pca", C.c_int32), ("reserved", C.c_int32 * 4),
                ("exact_order", C.c_int32), ("exact_order_eps", C.c_float), ("exact_order_crops", C.c_int32)]


class _ConvParams(C.Structure):
    _fields_ = [("weight", C.c_void_p), ("bias", C.c_void_p), ("cout", C.c_int32), ("cin", C.c_int32),
                ("ksize", C.c_int32)]


class _SPWeights(C.Structure):
    _fields_ = [("layer", _ConvParams * 12)]


class _NvLayer(C.Structure):
    _fields_ = [("kind", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32), ("stride", C.c_int32), ("act", C.c_int32),
                ("res", C.c_int32), ("weight", C.c_void_p), ("bias", C.c_void_p)]


class _NvWeights(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("layers", C.c_void_p), ("feat_dim", C.c_int32), ("proj_dim", C.c_int32),
                ("n_clusters", C.c_int32), ("pre_w", C.c_void_p), ("pre_b", C.c_void_p), ("assign_w", C.c_void_p),
                ("assign_b", C.c_void_p), ("centroids", C.c_void_p)]


class _MatchBatch(C.Structure):
    _fields_ = [("d_a", C.c_void_p), ("d_b", C.c_void_p), ("d_pts_a", C.c_void_p), ("d_pts_b", C.c_void_p),
                ("d_a_off", C.c_void_p), ("d_b_off", C.c_void_p), ("d_a_cnt", C.c_void_p), ("d_b_cnt", C.c_void_p),
                ("npairs", C.c_int32), ("dim", C.c_int32), ("max_n", C.c_int32), ("mode", C.c_int32),
                ("ratio", C.c_double), ("radius", C.c_double),
                ("d_q_idx", C.c_void_p), ("d_t_idx", C.c_void_p), ("d_dist", C.c_void_p), ("d_n_out", C.c_void_p)]


ALL_GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)      # d2fe_all_gather_fn


class _ExchangeConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("world", C.c_int32), ("rank", C.c_int32), ("wire", C.c_int32), ("loopback", C.c_int32), ("slots", C.c_int32),
                ("own_stream", C.c_int32), ("timing", C.c_int32), ("gate_thres", C.c_double), ("ratio", C.c_double), ("all_gather", ALL_GATHER_FN),
                ("all_gather_user", C.c_void_p), ("reserved", C.c_int32 * 6)]


class _ExchangeResult(C.Structure):
    _fields_ = [("ticket", C.c_int64), ("npairs", C.c_int32), ("cap", C.c_int32), ("q_idx", C.c_void_p), ("t_idx", C.c_void_p), ("dist", C.c_void_p),
                ("n_match", C.c_void_p), ("gate_pass", C.c_void_p), ("gate_sims", C.c_void_p), ("gate_n", C.c_int32), ("phase_ms", C.c_float * 5)]


class _PipeConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("lanes", C.c_int32), ("frames", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("cap", C.c_int32), ("netvlad", C.c_int32), ("match_lr", C.c_int32), ("match_prev", C.c_int32), ("pinned_input", C.c_int32),
                ("ratio", C.c_double), ("radius_lr", C.c_double), ("radius_prev", C.c_double), ("cu_partition", C.c_int32), ("netvlad_inline", C.c_int32), ("coalesce", C.c_int32), ("lane_cus", C.c_int32), ("netvlad_group", C.c_int32), ("coalesce_depth", C.c_int32), ("lr_lk", C.c_int32), ("sp_lk", C.c_int32)]


class _PipeCamera(C.Structure):
    """d2fe_pipe_camera: the one-camera configurations of a pipe (d2fe_pipe_create_camera)"""
    _fields_ = [("struct_size", C.c_int32), ("mono", C.c_int32), ("depth", C.c_int32), ("reserved", C.c_int32)]


class _PipeResult(C.Structure):
    _fields_ = [("frames", C.c_int32), ("cap", C.c_int32), ("desc_dim", C.c_int32), ("netvlad_dim", C.c_int32),
                ("kps_xy", C.c_void_p), ("scores", C.c_void_p), ("desc", C.c_void_p), ("n_kp", C.c_void_p), ("netvlad", C.c_void_p),
                ("lr_q", C.c_void_p), ("lr_t", C.c_void_p), ("lr_dist", C.c_void_p), ("lr_n", C.c_void_p),
                ("prev_q", C.c_void_p), ("prev_t", C.c_void_p), ("prev_dist", C.c_void_p), ("prev_n", C.c_void_p)]


class _PipeLKResult(C.Structure):
    _fields_ = [("frames", C.c_int32), ("cap", C.c_int32), ("pts_xy", C.c_void_p), ("status", C.c_void_p)]


class _TrackParams(C.Structure):
    """d2fe_track_params: the tracker parameters of the LK-carried landmark list (sp_track_use_lk)"""
    _fields_ = [("total_feature_num", C.c_int32), ("levels", C.c_int32), ("win", C.c_int32), ("iters", C.c_int32), ("near_lk_thread_rate", C.c_float),
                ("reserved", C.c_int32), ("feature_min_dist", C.c_double)]


class _FlowParams(C.Structure):
    """d2fe_flow_params: the parameters of the flow landmarks (enable_lk_optical_flow without sp_track_use_lk)"""
    _fields_ = [("struct_size", C.c_int32), ("superpoint", C.c_int32), ("track", _TrackParams), ("fast_cols", C.c_int32), ("fast_rows", C.c_int32),
                ("fast_threshold", C.c_int32), ("reserved", C.c_int32)]


class _PipeFlowResult(C.Structure):
    """d2fe_pipe_flow_result: the flow lists of a ticket (d2fe_pipe_flow_enable)"""
    _fields_ = [("frames", C.c_int32), ("cap_tracks", C.c_int32), ("list_words", C.c_int32), ("reserved", C.c_int32),
                ("n", C.c_void_p), ("n_tracked_in", C.c_void_p), ("n_lost", C.c_void_p), ("n_removed_near", C.c_void_p), ("n_new", C.c_void_p), ("lack", C.c_void_p),
                ("num", C.c_void_p), ("n_cand", C.c_void_p), ("pts_xy", C.c_void_p), ("id", C.c_void_p), ("src", C.c_void_p), ("right_xy", C.c_void_p),
                ("right_status", C.c_void_p), ("depth_mm", C.c_void_p)]


class _PipeTrackResult(C.Structure):
    _fields_ = [("frames", C.c_int32), ("cap_tracks", C.c_int32), ("desc_dim", C.c_int32), ("list_words", C.c_int32),
                ("n", C.c_void_p), ("n_tracked_in", C.c_void_p), ("n_lost", C.c_void_p), ("n_removed_near", C.c_void_p), ("n_new", C.c_void_p),
                ("pts_xy", C.c_void_p), ("id", C.c_void_p), ("src", C.c_void_p), ("kp", C.c_void_p), ("desc", C.c_void_p), ("scores", C.c_void_p),
                ("right_xy", C.c_void_p), ("right_status", C.c_void_p)]


class _PipeDepthResult(C.Structure):
    _fields_ = [("frames", C.c_int32), ("cap", C.c_int32), ("cap_tracks", C.c_int32), ("reserved", C.c_int32), ("kp_depth_mm", C.c_void_p),
                ("track_depth_mm", C.c_void_p)]


class _Camera(C.Structure):
    """d2fe_camera: kind (CAM_PINHOLE / CAM_MEI / CAM_CYLINDRICAL) and its nine doubles (camera_pinhole / camera_mei / camera_cylindrical)"""
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("p", C.c_double * 9)]


class _PipeBearings(C.Structure):
    """d2fe_pipe_bearings: the bearings mode of a stereo / mono pipe (d2fe_pipe_bearings_enable)"""
    _fields_ = [("struct_size", C.c_int32), ("lk_use_pred", C.c_int32), ("cam", _Camera * 2), ("T_right_left", C.c_double * 12), ("distance", C.c_double),
                ("radius_lk", C.c_double)]


class _PipeBearingsResult(C.Structure):
    _fields_ = [("frames", C.c_int32), ("cap", C.c_int32), ("cap_tracks", C.c_int32), ("reserved", C.c_int32), ("kp_bearing", C.c_void_p), ("kp_pred_xy", C.c_void_p),
                ("lk_right_bearing", C.c_void_p), ("lk_pred_ok", C.c_void_p), ("list_bearing", C.c_void_p), ("list_pred_xy", C.c_void_p),
                ("list_right_bearing", C.c_void_p), ("list_pred_ok", C.c_void_p)]


class _QuadBearings(C.Structure):
    """d2fe_quad_bearings: the bearings mode of a quad pipe (d2fe_quad_bearings_enable)"""
    _fields_ = [("struct_size", C.c_int32), ("lk_use_pred", C.c_int32), ("cam", _Camera * 4), ("T_nb", C.c_double * 48), ("distance", C.c_double),
                ("radius_lk", C.c_double)]


class _QuadBearingsResult(C.Structure):
    _fields_ = [("quads", C.c_int32), ("cap", C.c_int32), ("cap_tracks", C.c_int32), ("reserved", C.c_int32), ("kp_bearing", C.c_void_p), ("list_bearing", C.c_void_p),
                ("nb_pred_xy", C.c_void_p), ("nb_bearing", C.c_void_p), ("nb_pred_ok", C.c_void_p)]


class _PipeDeviceResult(C.Structure):
    _fields_ = [("frames", C.c_int32), ("cap", C.c_int32), ("desc_dim", C.c_int32), ("netvlad_dim", C.c_int32),
                ("d_kps_xy", C.c_void_p), ("d_scores", C.c_void_p), ("d_desc", C.c_void_p), ("d_n_kp", C.c_void_p), ("d_netvlad", C.c_void_p)]


class _QuadPipeConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("lanes", C.c_int32), ("quads", C.c_int32), ("raw_width", C.c_int32), ("raw_height", C.c_int32),
                ("width", C.c_int32), ("height", C.c_int32), ("cap", C.c_int32), ("netvlad", C.c_int32), ("match_neighbour", C.c_int32),
                ("match_prev", C.c_int32), ("pinned_input", C.c_int32), ("ratio", C.c_double), ("radius_neighbour", C.c_double),
                ("radius_prev", C.c_double), ("undistort_fov", C.c_double), ("reserved", C.c_int32 * 8)]


class _QuadMaps(C.Structure):
    _fields_ = [("mapx", C.c_void_p * 4), ("mapy", C.c_void_p * 4), ("gain", C.c_void_p * 4), ("device", C.c_int32)]


class _QuadPipeResult(C.Structure):
    _fields_ = [("quads", C.c_int32), ("cap", C.c_int32), ("desc_dim", C.c_int32), ("netvlad_dim", C.c_int32),
                ("kps_xy", C.c_void_p), ("scores", C.c_void_p), ("desc", C.c_void_p), ("n_kp", C.c_void_p), ("netvlad", C.c_void_p),
                ("nb_q", C.c_void_p), ("nb_t", C.c_void_p), ("nb_dist", C.c_void_p), ("nb_n", C.c_void_p),
                ("prev_q", C.c_void_p), ("prev_t", C.c_void_p), ("prev_dist", C.c_void_p), ("prev_n", C.c_void_p)]


class _QuadTrackResult(C.Structure):
    """d2fe_quad_track_result: the landmark lists, neighbour tracks and list matches of a quad ticket (d2fe_quad_track_enable)"""
    _fields_ = [("quads", C.c_int32), ("cap_tracks", C.c_int32), ("desc_dim", C.c_int32), ("list_words", C.c_int32),
                ("n", C.c_void_p), ("n_tracked_in", C.c_void_p), ("n_lost", C.c_void_p), ("n_removed_near", C.c_void_p), ("n_new", C.c_void_p),
                ("pts_xy", C.c_void_p), ("id", C.c_void_p), ("src", C.c_void_p), ("kp", C.c_void_p), ("desc", C.c_void_p), ("scores", C.c_void_p),
                ("nb_lk_xy", C.c_void_p), ("nb_lk_status", C.c_void_p),
                ("lnb_q", C.c_void_p), ("lnb_t", C.c_void_p), ("lnb_dist", C.c_void_p), ("lnb_n", C.c_void_p)]


class _QuadFlowResult(C.Structure):
    """d2fe_quad_flow_result: the flow lists and neighbour tracks of a quad ticket (d2fe_quad_flow_enable)"""
    _fields_ = [("quads", C.c_int32), ("cap_tracks", C.c_int32), ("list_words", C.c_int32), ("reserved", C.c_int32),
                ("n", C.c_void_p), ("n_tracked_in", C.c_void_p), ("n_lost", C.c_void_p), ("n_removed_near", C.c_void_p), ("n_new", C.c_void_p), ("lack", C.c_void_p),
                ("num", C.c_void_p), ("n_cand", C.c_void_p), ("pts_xy", C.c_void_p), ("id", C.c_void_p), ("src", C.c_void_p),
                ("nb_lk_xy", C.c_void_p), ("nb_lk_status", C.c_void_p)]


class _QuadDeviceResult(C.Structure):
    _fields_ = [("quads", C.c_int32), ("cap", C.c_int32), ("desc_dim", C.c_int32), ("netvlad_dim", C.c_int32),
                ("d_kps_xy", C.c_void_p), ("d_scores", C.c_void_p), ("d_desc", C.c_void_p), ("d_n_kp", C.c_void_p), ("d_netvlad", C.c_void_p)]


class _QuadExchangeConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("world", C.c_int32), ("rank", C.c_int32), ("wire", C.c_int32), ("loopback", C.c_int32), ("slots", C.c_int32),
                ("own_stream", C.c_int32), ("timing", C.c_int32), ("mode", C.c_int32), ("reserved0", C.c_int32), ("gate_thres", C.c_double), ("ratio", C.c_double),
                ("all_gather", ALL_GATHER_FN), ("all_gather_user", C.c_void_p), ("reserved", C.c_int32 * 6)]


class _QuadExchangeResult(C.Structure):
    _fields_ = [("ticket", C.c_int64), ("njobs", C.c_int32), ("npairs", C.c_int32), ("pairs_per_job", C.c_int32), ("cap", C.c_int32),
                ("job_rank", C.c_void_p), ("job_quad", C.c_void_p), ("q_idx", C.c_void_p), ("t_idx", C.c_void_p), ("dist", C.c_void_p), ("n_match", C.c_void_p),
                ("local_view", C.c_void_p), ("remote_view", C.c_void_p), ("dir_prev", C.c_void_p), ("gate_sims", C.c_void_p), ("gate_n", C.c_int32),
                ("phase_ms", C.c_float * 5)]


class _LoopConfig(C.Structure):
    """d2fe_loop_config"""
    _fields_ = [("struct_size", C.c_int32), ("capacity_keyframes", C.c_int32), ("max_index", C.c_int32), ("mode", C.c_int32), ("slots", C.c_int32),
                ("timing", C.c_int32), ("max_queries", C.c_int32), ("reserved0", C.c_int32), ("thres", C.c_double), ("ratio", C.c_double), ("reserved", C.c_int32 * 6)]


class _WindowConfig(C.Structure):
    """d2fe_window_config"""
    _fields_ = [("struct_size", C.c_int32), ("capacity", C.c_int32), ("mode", C.c_int32), ("slots", C.c_int32), ("timing", C.c_int32), ("max_queries", C.c_int32),
                ("thres", C.c_double), ("ratio", C.c_double), ("reserved", C.c_int32 * 6)]


class _WindowResult(C.Structure):
    """d2fe_window_result"""
    _fields_ = [("nq", C.c_int32), ("views", C.c_int32), ("cap", C.c_int32), ("capacity", C.c_int32), ("n_window", C.c_int32), ("reserved", C.c_int32),
                ("keyframe_tag", C.c_void_p), ("keyframe_pos", C.c_void_p), ("dir_a", C.c_void_p), ("dir_b", C.c_void_p), ("sim", C.c_void_p), ("sims", C.c_void_p),
                ("local_view", C.c_void_p), ("remote_view", C.c_void_p), ("n_match", C.c_void_p), ("q_idx", C.c_void_p), ("t_idx", C.c_void_p), ("dist", C.c_void_p),
                ("phase_ms", C.c_float * 3), ("reserved1", C.c_int32)]


class _LoopResult(C.Structure):
    """d2fe_loop_result"""
    _fields_ = [("ticket", C.c_int64), ("frames", C.c_int32), ("views", C.c_int32), ("cap", C.c_int32), ("reserved", C.c_int32),
                ("queried", C.c_void_p), ("label", C.c_void_p), ("sim", C.c_void_p), ("keyframe", C.c_void_p), ("dir_old", C.c_void_p), ("ntotal_at_query", C.c_void_p),
                ("added_label", C.c_void_p), ("dir_a", C.c_void_p), ("dir_b", C.c_void_p), ("n_match", C.c_void_p), ("q_idx", C.c_void_p), ("t_idx", C.c_void_p),
                ("dist", C.c_void_p), ("phase_ms", C.c_float * 4)]


def _quad_maps(maps, device):
    """d2fe_quad_maps from four (mapx, mapy, gain or None) raw addresses"""
    m = _QuadMaps()
    for c, (mx, my, g) in enumerate(maps):
        m.mapx[c], m.mapy[c], m.gain[c] = mx, my, g
    m.device = int(bool(device))
    return m


_lib = None
_dev_lib = None

EXPORTS = [
    "d2fe_last_error", "d2fe_version", "d2fe_default_config", "d2fe_create", "d2fe_destroy", "d2fe_load_superpoint", "d2fe_set_superpoint_pca", "d2fe_set_superpoint_int8_ranges",
    "d2fe_calib_create", "d2fe_calib_collect", "d2fe_calib_freeze", "d2fe_calib_stats_get", "d2fe_calib_ranges", "d2fe_calib_destroy",
    "d2fe_desc_dim", "d2fe_superpoint_extract", "d2fe_superpoint_extract_batch", "d2fe_superpoint_extract_device", "d2fe_extract_all",
    "d2fe_extract_all_batch", "d2fe_tail_stream", "d2fe_superpoint_wait_tail", "d2fe_load_netvlad", "d2fe_set_netvlad_pca", "d2fe_netvlad_dim",
    "d2fe_netvlad", "d2fe_netvlad_batch", "d2fe_netvlad_device", "d2fe_match_knn", "d2fe_match_crosscheck", "d2fe_match_batch_device",
    "d2fe_match_fallback_rows", "d2fe_block_words", "d2fe_block_field_offset", "d2fe_pack_blocks_device", "d2fe_gate_pairs_device",
    "d2fe_quad_gate_device", "d2fe_block_bytes_int8", "d2fe_pack_blocks_int8_device", "d2fe_unpack_blocks_int8_device", "d2fe_half_move_cols",
    "d2fe_block_words_d", "d2fe_block_field_offset_d", "d2fe_pack_blocks_device_d", "d2fe_block_bytes_int8_d", "d2fe_pack_blocks_int8_device_d",
    "d2fe_unpack_blocks_int8_device_d",
    "d2fe_half_image_compact_device", "d2fe_remap_matches_device", "d2fe_half_image_filter", "d2fe_undistort", "d2fe_undistort_device",
    "d2fe_db_create", "d2fe_db_destroy", "d2fe_db_ntotal", "d2fe_db_add", "d2fe_db_search", "d2fe_db_query_gated", "d2fe_quantize_int8",
    "d2fe_dequantize_int8", "d2fe_sync", "d2fe_exact_order_stats", "d2fe_profile_enable", "d2fe_profile_read", "d2fe_prepare_gray", "d2fe_prepare_gray_device",
    "d2fe_gen_cylinder_map", "d2fe_gen_cylinder_map_device", "d2fe_gen_pinhole_map", "d2fe_gen_pinhole_map_device", "d2fe_lk_frame_create",
    "d2fe_lk_frame_create_device", "d2fe_lk_frame_destroy", "d2fe_lk_frame_read_level", "d2fe_lk_track", "d2fe_lk_track_batch",
    "d2fe_lk_stereo_workspace_bytes", "d2fe_lk_track_stereo_device", "d2fe_pipe_lk_result_get",
    "d2fe_track_default_params", "d2fe_lk_carry_list_bytes", "d2fe_lk_carry_list_offset", "d2fe_lk_carry_step_device", "d2fe_pipe_track_result_get",
    "d2fe_pipe_set_track_params", "d2fe_pipe_camera_default", "d2fe_pipe_create_camera", "d2fe_pipe_submit_depth", "d2fe_pipe_depth_result_get", "d2fe_depth_at_device", "d2fe_lk_carry_quad_step_device", "d2fe_lk_carry_neighbour_device", "d2fe_quad_track_enable", "d2fe_quad_track_result_get",
    "d2fe_flow_default_params", "d2fe_lk_flow_list_bytes", "d2fe_lk_flow_list_offset", "d2fe_lk_flow_scratch_bytes", "d2fe_detect_fast_device", "d2fe_lk_flow_step_device",
    "d2fe_pipe_flow_enable", "d2fe_pipe_flow_result_get",
    "d2fe_relative_extrinsic", "d2fe_bearings_device", "d2fe_pipe_bearings_default", "d2fe_pipe_bearings_enable", "d2fe_pipe_bearings_result_get",
    "d2fe_lk_flow_quad_step_device", "d2fe_lk_flow_neighbour_device", "d2fe_quad_flow_enable", "d2fe_quad_flow_result_get",
    "d2fe_cylinder_camera", "d2fe_quad_bearings_default", "d2fe_quad_bearings_enable", "d2fe_quad_bearings_result_get",
    "d2fe_detect_fast_by_region", "d2fe_good_features_to_track", "d2fe_pipe_default_config", "d2fe_pipe_create", "d2fe_pipe_destroy",
    "d2fe_pipe_lanes", "d2fe_pipe_stream_placement", "d2fe_pipe_classify_stream", "d2fe_pipe_submit", "d2fe_pipe_wait", "d2fe_pipe_profile_enable", "d2fe_pipe_profile_read",
    "d2fe_pipe_device_view", "d2fe_pipe_device_release", "d2fe_pipe_lane_stream", "d2fe_pipe_geometry", "d2fe_pipe_handle",
    "d2fe_quad_pipe_default_config", "d2fe_quad_pipe_create", "d2fe_quad_pipe_destroy", "d2fe_quad_pipe_submit", "d2fe_quad_pipe_wait",
    "d2fe_quad_pipe_lanes", "d2fe_quad_pipe_geometry", "d2fe_quad_undistort_device",
    "d2fe_quad_device_view", "d2fe_quad_device_release", "d2fe_quad_lane_stream", "d2fe_quad_handle",
    "d2fe_quad_exchange_default_config", "d2fe_quad_exchange_create", "d2fe_quad_exchange_destroy", "d2fe_quad_exchange_enqueue", "d2fe_quad_exchange_collect",
    "d2fe_quad_exchange_jobs", "d2fe_quad_exchange_pairs", "d2fe_quad_exchange_block_bytes", "d2fe_quad_exchange_stream", "d2fe_quad_exchange_gathered", "d2fe_quad_exchange_job_layout",
    "d2fe_exchange_default_config", "d2fe_exchange_create", "d2fe_exchange_destroy", "d2fe_exchange_enqueue", "d2fe_exchange_collect", "d2fe_exchange_pairs",
    "d2fe_exchange_block_bytes", "d2fe_exchange_stream", "d2fe_exchange_gathered",
    "d2fe_window_default_config", "d2fe_window_create", "d2fe_window_create_quad", "d2fe_window_destroy", "d2fe_window_stream", "d2fe_window_push",
    "d2fe_window_push_host", "d2fe_window_retain", "d2fe_window_retain_plan", "d2fe_window_size", "d2fe_window_tags", "d2fe_window_track_device", "d2fe_window_collect",
    "d2fe_loop_default_config", "d2fe_loop_create", "d2fe_loop_create_quad", "d2fe_loop_destroy", "d2fe_loop_enqueue", "d2fe_loop_collect", "d2fe_loop_ntotal",
    "d2fe_loop_keyframes", "d2fe_loop_stream", "d2fe_loop_query_device", "d2fe_loop_add_host", "d2fe_rccl_load", "d2fe_rccl_path", "d2fe_rccl_unique_id", "d2fe_rccl_comm_init_rank", "d2fe_rccl_comm_destroy"]
# the development library (lib/libd2fe_hip_dev.so, include/d2fe_debug.h) exports these on top: test hooks and kernel diagnostics
DEBUG_EXPORTS = [
    "d2fe_debug_graph_count", "d2fe_debug_read", "d2fe_debug_netvlad_layer", "d2fe_debug_netvlad_stamps", "d2fe_debug_pack_wino",
    "d2fe_debug_pack_netvlad", "d2fe_debug_netvlad_tile", "d2fe_debug_conv3x3_wino", "d2fe_debug_match_stamps",
    "d2fe_debug_netvlad_plan", "d2fe_debug_netvlad_shapes", "d2fe_debug_netvlad_features", "d2fe_debug_netvlad_groups", "d2fe_debug_netvlad_slots", "d2fe_debug_regime_counts", "d2fe_debug_regime_reset",
    "d2fe_debug_softmax_cand", "d2fe_debug_select_b", "d2fe_debug_sample_b", "d2fe_debug_sample_b_pca", "d2fe_debug_nms2_a",
    "d2fe_debug_desc_head_sparse", "d2fe_debug_sample_a", "d2fe_debug_conv_layer", "d2fe_debug_conv_layer_q", "d2fe_debug_conv1a",
    "d2fe_debug_calib_ranges_from_hist", "d2fe_debug_calib_stats", "d2fe_debug_calib_conv1a"]
# enum d2fe_regime of include/d2fe_debug.h, in order: launches per size-dependent code path (the last two entries are the grid and the item count of the
# most recent Winograd launch, not counts)
REGIMES = ["wino_nt1_one", "wino_nt1_static", "wino_nt1_claimed", "wino_nt2_one", "wino_nt2_static", "wino_nt2_claimed_ring", "wino_nt2_claimed_fused1b",
           "match_nw4", "match_nw2", "nv_gmerge", "nv_front_tpw", "wino_last_grid", "wino_last_total"]


def _preload_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm bundles its own libamdhip64 (same SONAME as /opt/rocm's): whichever copy
    is loaded first serves both, and torch cannot see the GPU through the system copy.  If torch is installed but not yet
    imported, load ITS runtime first (located without importing torch) so that a later `import torch` stays consistent."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is not None and spec.origin:
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            try:
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
            except OSError:
                pass


def load_library(dev=False):
    """dlopen the C-ABI library (dev=True: the development library with the d2fe_debug_* hooks, include/d2fe_debug.h).  Raises if it has not
    been built (python -m d2slam_amd.build [--dev])."""
    global _lib, _dev_lib
    if dev:
        if _dev_lib is None:
            _dev_lib = _open_library(DEV_LIB_PATH, True)
        return _dev_lib
    if _lib is None:
        _lib = _open_library(LIB_PATH, False)
    return _lib


def _open_library(path, dev):
    if True:
        _preload_hip_runtime()
        if not os.path.exists(path):
            raise D2FEError(-100, "%s not built: run `python __graft_entry__.py` or `python -m d2slam_amd.build%s` "
                                  "(no CPU fallback exists)" % (os.path.basename(path), " --dev" if dev else ""))
        lib = C.CDLL(path)
        lib.d2fe_last_error.restype = C.c_char_p
        lib.d2fe_version.restype = C.c_char_p
        if dev:
            lib.d2fe_debug_read.restype = C.c_long
            lib.d2fe_debug_read.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t]
            for nm in ("d2fe_debug_netvlad_layer", "d2fe_debug_netvlad_stamps", "d2fe_debug_pack_wino", "d2fe_debug_pack_netvlad", "d2fe_debug_match_stamps"):
                getattr(lib, nm).restype = C.c_long
            lib.d2fe_debug_regime_counts.argtypes = [C.c_void_p, C.c_int]
            lib.d2fe_debug_regime_reset.argtypes = []; lib.d2fe_debug_regime_reset.restype = None
            vp, ci = C.c_void_p, C.c_int
            lib.d2fe_debug_softmax_cand.argtypes = [vp, vp, ci, ci, ci, ci, C.c_float, ci, ci, vp, vp, vp]
            lib.d2fe_debug_select_b.argtypes = [vp, vp, vp, C.c_long, ci, ci, ci, ci, ci, ci, vp, C.c_float, ci, vp, vp, vp, vp]
            lib.d2fe_debug_sample_b.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, vp, ci, vp, ci, vp]
            lib.d2fe_debug_sample_b_pca.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, vp, ci, vp, ci, vp, vp, ci, vp]
            lib.d2fe_debug_nms2_a.argtypes = [vp, vp, ci, ci, ci, C.c_float, ci, ci, ci, vp, vp, vp, vp]
            lib.d2fe_debug_desc_head_sparse.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp]
            lib.d2fe_debug_sample_a.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, vp, ci, ci, vp, ci, vp, vp, ci, vp]
            lib.d2fe_debug_conv_layer.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
            lib.d2fe_debug_conv_layer_q.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_float]
            lib.d2fe_debug_conv1a.argtypes = [vp, ci, vp, ci, C.c_longlong, C.c_longlong, ci, ci, ci, vp, vp, vp, C.c_longlong]
            lib.d2fe_debug_calib_ranges_from_hist.argtypes = [vp, ci, C.c_float, ci, C.c_double, vp, vp]
            lib.d2fe_debug_calib_stats.argtypes = [vp, vp, C.c_longlong, ci, ci, ci, C.c_float, ci, ci, ci, vp, vp, vp, vp]
            lib.d2fe_debug_calib_conv1a.argtypes = [vp, vp, ci, C.c_longlong, C.c_longlong, ci, ci, ci, vp, vp, C.c_float, ci, ci, vp, vp, vp, vp]
        lib.d2fe_destroy.restype = None
        lib.d2fe_calib_create.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.d2fe_calib_collect.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_int]
        lib.d2fe_calib_freeze.argtypes = [C.c_void_p]
        lib.d2fe_calib_stats_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.d2fe_calib_ranges.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p]
        lib.d2fe_calib_destroy.argtypes = [C.c_void_p]; lib.d2fe_calib_destroy.restype = None
        lib.d2fe_half_move_cols.restype = C.c_float
        lib.d2fe_half_move_cols.argtypes = [C.c_int, C.c_double]
        lib.d2fe_default_config.restype = None
        lib.d2fe_superpoint_extract_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                      C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        lib.d2fe_superpoint_extract_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                       C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_int, C.c_void_p, C.c_void_p]
        lib.d2fe_extract_all_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        lib.d2fe_extract_all.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                         C.c_void_p, C.c_void_p]
        lib.d2fe_superpoint_extract.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        lib.d2fe_match_knn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double,
                                       C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                       C.c_void_p]
        lib.d2fe_match_crosscheck.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        lib.d2fe_match_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.d2fe_half_image_filter.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
        lib.d2fe_create.argtypes = [C.c_void_p, C.c_void_p]
        lib.d2fe_destroy.argtypes = [C.c_void_p]
        lib.d2fe_load_superpoint.argtypes = [C.c_void_p, C.c_void_p]
        lib.d2fe_sync.argtypes = [C.c_void_p]
        lib.d2fe_exact_order_stats.argtypes = [C.c_void_p, C.c_void_p]
        lib.d2fe_match_fallback_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.d2fe_match_fallback_rows.restype = C.c_long
        lib.d2fe_tail_stream.argtypes = [C.c_void_p]
        lib.d2fe_tail_stream.restype = C.c_void_p
        lib.d2fe_superpoint_wait_tail.argtypes = [C.c_void_p, C.c_void_p]
        lib.d2fe_undistort.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_int, C.c_int, C.c_void_p]
        lib.d2fe_undistort_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        lib.d2fe_db_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        lib.d2fe_db_destroy.argtypes = [C.c_void_p]
        lib.d2fe_db_destroy.restype = None
        lib.d2fe_db_ntotal.argtypes = [C.c_void_p]
        lib.d2fe_db_add.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        lib.d2fe_db_search.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        lib.d2fe_db_query_gated.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
        lib.d2fe_quantize_int8.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        lib.d2fe_dequantize_int8.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        lib.d2fe_load_netvlad.argtypes = [C.c_void_p, C.c_void_p]
        lib.d2fe_set_netvlad_pca.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        lib.d2fe_netvlad_dim.argtypes = [C.c_void_p]
        lib.d2fe_netvlad_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p]
        lib.d2fe_netvlad.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        lib.d2fe_netvlad_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p]
        lib.d2fe_set_superpoint_pca.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        lib.d2fe_desc_dim.argtypes = [C.c_void_p]
        lib.d2fe_set_superpoint_int8_ranges.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        lib.d2fe_profile_enable.argtypes = [C.c_void_p, C.c_int]
        lib.d2fe_profile_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.d2fe_prepare_gray.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        lib.d2fe_prepare_gray_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int,
                                                 C.c_int, C.c_void_p, C.c_void_p]
        lib.d2fe_gen_cylinder_map.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
        lib.d2fe_gen_cylinder_map_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.d2fe_gen_pinhole_map.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
        lib.d2fe_gen_pinhole_map_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p,
                                                    C.c_void_p, C.c_void_p]
        lib.d2fe_lk_frame_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        lib.d2fe_lk_frame_create_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        lib.d2fe_lk_frame_destroy.argtypes = [C.c_void_p]
        lib.d2fe_lk_frame_destroy.restype = None
        lib.d2fe_lk_frame_read_level.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        lib.d2fe_lk_frame_read_level.restype = C.c_long
        lib.d2fe_lk_track.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float,
                                      C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        lib.d2fe_lk_track_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                            C.c_void_p, C.c_void_p]
        lib.d2fe_lk_stereo_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
        lib.d2fe_lk_stereo_workspace_bytes.restype = C.c_size_t
        lib.d2fe_lk_track_stereo_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p,
                                                    C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.d2fe_pipe_lk_result_get.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        lib.d2fe_track_default_params.argtypes = [C.c_void_p]
        lib.d2fe_track_default_params.restype = None
        lib.d2fe_lk_carry_list_bytes.argtypes = [C.c_int, C.c_int]
        lib.d2fe_lk_carry_list_bytes.restype = C.c_size_t
        lib.d2fe_lk_carry_list_offset.argtypes = [C.c_int, C.c_int, C.c_int]
        lib.d2fe_lk_carry_list_offset.restype = C.c_long
        lib.d2fe_lk_carry_step_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.d2fe_pipe_track_result_get.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        lib.d2fe_lk_carry_quad_step_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int,
                                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.d2fe_lk_carry_neighbour_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_size_t, C.c_int,
                                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.d2fe_flow_default_params.argtypes = [C.c_void_p]
        lib.d2fe_flow_default_params.restype = None
        lib.d2fe_lk_flow_list_bytes.argtypes = [C.c_int]
        lib.d2fe_lk_flow_list_bytes.restype = C.c_size_t
        lib.d2fe_lk_flow_list_offset.argtypes = [C.c_int, C.c_int]
        lib.d2fe_lk_flow_list_offset.restype = C.c_long
        lib.d2fe_lk_flow_scratch_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        lib.d2fe_lk_flow_scratch_bytes.restype = C.c_size_t
        lib.d2fe_detect_fast_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                C.c_void_p, C.c_void_p, C.c_void_p]
        lib.d2fe_lk_flow_step_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]
        lib.d2fe_pipe_flow_enable.argtypes = [C.c_void_p, C.c_void_p]
        lib.d2fe_pipe_flow_result_get.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        lib.d2fe_lk_flow_quad_step_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                                      C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.d2fe_lk_flow_neighbour_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_size_t, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.c_void_p]
        lib.d2fe_quad_flow_enable.argtypes = [C.c_void_p, C.c_void_p]
        lib.d2fe_quad_flow_result_get.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        lib.d2fe_quad_track_enable.argtypes = [C.c_void_p, C.c_void_p]
        lib.d2fe_quad_track_result_get.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        lib.d2fe_pipe_set_track_params.argtypes = [C.c_void_p, C.c_void_p]
        lib.d2fe_detect_fast_by_region.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                   C.c_void_p, C.c_int, C.c_void_p]
        lib.d2fe_good_features_to_track.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p,
                                                    C.c_int, C.c_void_p]
        lib.d2fe_pipe_default_config.argtypes = [C.c_void_p]
        lib.d2fe_pipe_default_config.restype = None
        lib.d2fe_pipe_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.d2fe_pipe_destroy.argtypes = [C.c_void_p]
        lib.d2fe_pipe_destroy.restype = None
        lib.d2fe_pipe_lanes.argtypes = [C.c_void_p]
        lib.d2fe_pipe_stream_placement.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        lib.d2fe_pipe_classify_stream.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
        lib.d2fe_pipe_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
        lib.d2fe_pipe_wait.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        lib.d2fe_pipe_camera_default.argtypes = [C.c_void_p]
        lib.d2fe_pipe_camera_default.restype = None
        lib.d2fe_pipe_create_camera.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.d2fe_pipe_submit_depth.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p]
        lib.d2fe_pipe_depth_result_get.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        lib.d2fe_depth_at_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int,
                                             C.c_void_p, C.c_void_p]
        lib.d2fe_relative_extrinsic.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.d2fe_bearings_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.d2fe_pipe_bearings_default.argtypes = [C.c_void_p]
        lib.d2fe_pipe_bearings_default.restype = None
        lib.d2fe_pipe_bearings_enable.argtypes = [C.c_void_p, C.c_void_p]
        lib.d2fe_pipe_bearings_result_get.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        lib.d2fe_cylinder_camera.argtypes = [C.c_int, C.c_int, C.c_double, C.c_void_p]
        lib.d2fe_quad_bearings_default.argtypes = [C.c_void_p]
        lib.d2fe_quad_bearings_default.restype = None
        lib.d2fe_quad_bearings_enable.argtypes = [C.c_void_p, C.c_void_p]
        lib.d2fe_quad_bearings_result_get.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        lib.d2fe_pipe_device_view.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        lib.d2fe_pipe_device_release.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        lib.d2fe_pipe_profile_enable.argtypes = [C.c_void_p, C.c_int]
        lib.d2fe_pipe_profile_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.d2fe_pipe_lane_stream.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        lib.d2fe_pipe_geometry.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.d2fe_pipe_handle.argtypes = [C.c_void_p]; lib.d2fe_pipe_handle.restype = C.c_void_p
        lib.d2fe_quad_pipe_default_config.argtypes = [C.c_void_p]; lib.d2fe_quad_pipe_default_config.restype = None
        lib.d2fe_quad_pipe_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.d2fe_quad_pipe_destroy.argtypes = [C.c_void_p]; lib.d2fe_quad_pipe_destroy.restype = None
        lib.d2fe_quad_pipe_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p]
        lib.d2fe_quad_pipe_wait.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        lib.d2fe_quad_pipe_lanes.argtypes = [C.c_void_p]
        lib.d2fe_quad_pipe_geometry.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.d2fe_quad_undistort_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p,
                                                   C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        lib.d2fe_quad_device_view.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        lib.d2fe_quad_device_release.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        lib.d2fe_quad_lane_stream.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        lib.d2fe_quad_handle.argtypes = [C.c_void_p]; lib.d2fe_quad_handle.restype = C.c_void_p
        lib.d2fe_quad_exchange_default_config.argtypes = [C.c_void_p]; lib.d2fe_quad_exchange_default_config.restype = None
        lib.d2fe_quad_exchange_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.d2fe_quad_exchange_destroy.argtypes = [C.c_void_p]; lib.d2fe_quad_exchange_destroy.restype = None
        lib.d2fe_quad_exchange_enqueue.argtypes = [C.c_void_p, C.c_int64, C.c_int]
        lib.d2fe_quad_exchange_collect.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        for nm in ("d2fe_quad_exchange_jobs", "d2fe_quad_exchange_pairs", "d2fe_quad_exchange_block_bytes"):
            getattr(lib, nm).argtypes = [C.c_void_p]
        lib.d2fe_quad_exchange_stream.argtypes = [C.c_void_p]; lib.d2fe_quad_exchange_stream.restype = C.c_void_p
        lib.d2fe_quad_exchange_gathered.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        lib.d2fe_quad_exchange_job_layout.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        lib.d2fe_exchange_default_config.argtypes = [C.c_void_p]; lib.d2fe_exchange_default_config.restype = None
        lib.d2fe_exchange_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.d2fe_exchange_destroy.argtypes = [C.c_void_p]; lib.d2fe_exchange_destroy.restype = None
        lib.d2fe_exchange_enqueue.argtypes = [C.c_void_p, C.c_int64, C.c_int]
        lib.d2fe_exchange_collect.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.d2fe_exchange_pairs.argtypes = [C.c_void_p]
        lib.d2fe_exchange_block_bytes.argtypes = [C.c_void_p]
        lib.d2fe_exchange_stream.argtypes = [C.c_void_p]; lib.d2fe_exchange_stream.restype = C.c_void_p
        lib.d2fe_exchange_gathered.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        lib.d2fe_window_default_config.argtypes = [C.c_void_p]; lib.d2fe_window_default_config.restype = None
        lib.d2fe_window_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.d2fe_window_create_quad.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.d2fe_window_destroy.argtypes = [C.c_void_p]; lib.d2fe_window_destroy.restype = None
        lib.d2fe_window_stream.argtypes = [C.c_void_p]; lib.d2fe_window_stream.restype = C.c_void_p
        lib.d2fe_window_push.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int64]
        lib.d2fe_window_push_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
        lib.d2fe_window_retain.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        lib.d2fe_window_retain_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        lib.d2fe_window_size.argtypes = [C.c_void_p]
        lib.d2fe_window_tags.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        lib.d2fe_window_track_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
        lib.d2fe_window_collect.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.d2fe_loop_default_config.argtypes = [C.c_void_p]; lib.d2fe_loop_default_config.restype = None
        lib.d2fe_loop_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.d2fe_loop_create_quad.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.d2fe_loop_destroy.argtypes = [C.c_void_p]; lib.d2fe_loop_destroy.restype = None
        lib.d2fe_loop_enqueue.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int]
        lib.d2fe_loop_collect.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        lib.d2fe_loop_ntotal.argtypes = [C.c_void_p]
        lib.d2fe_loop_keyframes.argtypes = [C.c_void_p]
        lib.d2fe_loop_stream.argtypes = [C.c_void_p]; lib.d2fe_loop_stream.restype = C.c_void_p
        lib.d2fe_loop_add_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        lib.d2fe_loop_query_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        lib.d2fe_rccl_load.argtypes = [C.c_char_p]
        lib.d2fe_rccl_path.restype = C.c_char_p
        lib.d2fe_rccl_unique_id.argtypes = [C.c_void_p]
        lib.d2fe_rccl_comm_init_rank.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        lib.d2fe_rccl_comm_destroy.argtypes = [C.c_void_p]
    return lib


class _DebugConv(C.Structure):      # d2fe_debug_conv of include/d2fe_debug.h
    _fields_ = [(k, C.c_int32) for k in ("family", "precision", "shape", "conv64_tile", "pool", "relu", "n", "H", "W", "cout", "in_cstride", "in_coff",
                                         "out_cstride", "out_coff", "img_stride", "ncu")] + \
               [(k, C.c_int64) for k in ("in_img_stride", "in_floats", "out_img_stride", "out_floats", "img_istride", "img_bytes")]


def _check(rc):
    if rc != 0:
        raise D2FEError(rc, load_library().d2fe_last_error().decode())


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


@dataclass
class SuperPointConfig:
    """Field-for-field SuperPointConfig (superpoint_tensorrt.h:17-33); TensorRT-only fields are kept for
    source compatibility and ignored (onnx_path/engine_path/tensor names/dla_core/fp_16)."""
    max_keypoints: int = 100
    remove_borders: int = 1
    dla_core: int = 0
    fp_16: int = 0
    input_width: int = 640
    input_height: int = 480
    superpoint_pca_dims: int = -1
    keypoint_threshold: float = 0.015
    input_tensor_names: List[str] = field(default_factory=lambda: ["input"])
    output_tensor_names: List[str] = field(default_factory=lambda: ["scores", "descriptors"])
    onnx_path: str = ""
    engine_path: str = ""
    pca_mean_path: str = ""
    pca_comp_path: str = ""
    enable_pca: bool = False
    # device-side additions
    device_id: int = 0
    max_batch: int = 2
    postproc: int = POSTPROC_B
    nms_dist: int = 10
    precision: int = PREC_F32
    keep_score_map: bool = False   # debug: also write the dense score map
    dense_descriptors: bool = False  # debug: dense descriptor map instead of the sparse descriptor head (variant B)
    async_tail: bool = False         # extract_device: post-processing on the handle's tail stream, under the next call's convolutions


class FrontEnd:
    """One device context (== one LoopCam's networks, loop_cam.cpp:24-70)."""

    def __init__(self, cfg: SuperPointConfig, dev: bool = False, exact_order: bool = False, exact_order_eps: float = 0.0, exact_order_crops: int = 0,
                 variant_b_pca: bool = False):
        """dev=True: a handle of the development library (d2fe_debug_* hooks, D2FE_* schedule switches); the product library otherwise.
        exact_order (PREC_F32_WINO, variant B, max_keypoints >= 1): the keypoint lists equal those of a PREC_F32 handle position by position
        (include/d2fe.h, d2fe_config::exact_order); exact_order_eps / exact_order_crops: 0 = the library defaults.  Pipes created from the handle inherit it.
        variant_b_pca (variant B only): set_pca is accepted and every extract call, pipe, list, store and exchange of the handle carries rows of pca_dims
        floats (include/d2fe.h, d2fe_config::variant_b_pca); False: variant B refuses a PCA, as the reference's live path ignores it."""
        lib = load_library(dev)
        self.dev = bool(dev)
        c = _Config()
        lib.d2fe_default_config(C.byref(c))
        c.device_id = cfg.device_id
        c.max_width = cfg.input_width
        c.max_height = cfg.input_height
        c.max_batch = cfg.max_batch
        c.max_keypoints = cfg.max_keypoints
        c.remove_borders = cfg.remove_borders
        c.keypoint_threshold = cfg.keypoint_threshold
        c.postproc = cfg.postproc
        c.nms_dist = cfg.nms_dist
        c.precision = cfg.precision
        c.keep_score_map = int(cfg.keep_score_map)
        c.dense_descriptors = int(cfg.dense_descriptors)
        c.async_tail = int(cfg.async_tail)
        c.exact_order = int(bool(exact_order))
        c.exact_order_eps = float(exact_order_eps)
        c.exact_order_crops = int(exact_order_crops)
        c.variant_b_pca = int(bool(variant_b_pca))
        self.cfg = cfg
        self._h = C.c_void_p()
        _check(lib.d2fe_create(C.byref(c), C.byref(self._h)))
        self._lib = lib
        self._keep = None

    def _need_dev(self, what):
        if not self.dev:
            raise D2FEError(-5, "%s is a test hook of the development library: create the handle with FrontEnd(cfg, dev=True) / DevFrontEnd(cfg) "
                                "(include/d2fe_debug.h; the product library exports no d2fe_debug_* symbol)" % what)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            # pipes run on this handle's packed weights; the library refuses to destroy a handle that still has live pipes (d2fe_destroy), so they go first
            for p in list(getattr(self, "_pipes", ())):
                p.close()
            self._lib.d2fe_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def load_superpoint(self, weights):
        """weights: {layer: (W [cout,cin,k,k], b [cout])} for the 12 layers of superpoint.ipynb:306-321."""
        sw = _SPWeights()
        keep = []
        for i, name in enumerate(SP_LAYERS):
            W, b = weights[name]
            W = np.ascontiguousarray(W, np.float32); b = np.ascontiguousarray(b, np.float32)
            keep += [W, b]
            sw.layer[i].weight = W.ctypes.data
            sw.layer[i].bias = b.ctypes.data
            sw.layer[i].cout, sw.layer[i].cin, sw.layer[i].ksize = W.shape[0], W.shape[1], W.shape[2]
        _check(self._lib.d2fe_load_superpoint(self._h, C.byref(sw)))

    def set_pca(self, comp, mean):
        """comp [pca_dims,256] (CSV layout of superpoint_onnx.cpp:47-53), mean [256]; comp=None switches the PCA off.  Variant A (pca_dims 1..256), or a
        variant-B handle created with variant_b_pca=True (pca_dims 4..256, a multiple of 4); any other variant-B handle raises D2FE_ERR_UNSUPPORTED.
        desc_dim is pca_dims afterwards.  Refused while pipes of the handle are alive."""
        if comp is None:
            _check(self._lib.d2fe_set_superpoint_pca(self._h, None, None, 0))
            return
        comp = np.ascontiguousarray(comp, np.float32); mean = np.ascontiguousarray(mean, np.float32)
        _check(self._lib.d2fe_set_superpoint_pca(self._h, _ptr(comp), _ptr(mean), comp.shape[0]))

    def set_int8_ranges(self, ranges):
        """PREC_I8 handles, after load_superpoint: the dynamic range of every layer's OUTPUT tensor -- a {layer name: range} dict or 12 numbers in SP_LAYERS
        order (calibrate.measure_ranges gives the dict).  The entries of convPb and convDb are ignored (a dict may leave them out).  A later load_superpoint clears
        the ranges; refused while pipes of the handle are alive."""
        if isinstance(ranges, dict):
            ranges = [ranges.get(name, 1.0) if name in ("convPb", "convDb") else ranges[name] for name in SP_LAYERS]
        r = np.ascontiguousarray(ranges, np.float32)
        _check(self._lib.d2fe_set_superpoint_int8_ranges(self._h, _ptr(r), int(r.size)))

    @property
    def desc_dim(self):
        return int(self._lib.d2fe_desc_dim(self._h))

    # ---- extractor ---------------------------------------------------------------------------------------------
    def extract_batch(self, images, cap=None):
        """images: u8 [n,H,W].  Returns list of (kps [k,2], scores [k], desc [k,256])."""
        images = np.ascontiguousarray(images, np.uint8)
        if images.ndim == 2:
            images = images[None]
        n, H, W = images.shape
        if not cap:      # keep-all handles (max_keypoints = -1) have no configured cap: the library's staging capacity applies
            cap = self.cfg.max_keypoints if self.cfg.max_keypoints > 0 else KEEP_ALL_CAP
        kps = np.zeros((n, cap, 2), np.float32); sc = np.zeros((n, cap), np.float32)
        desc = np.zeros((n, cap, self.desc_dim), np.float32); cnt = np.zeros(n, np.int32)
        rc = self._lib.d2fe_superpoint_extract_batch(self._h, _ptr(images), n, W, H, W, H * W, _ptr(kps), _ptr(sc),
                                                     _ptr(desc), cap, _ptr(cnt))
        # D2FE_ERR_TRUNCATED: the first `cap` keypoints in raster order were written and n_out is valid -- report it, keep the results
        self.last_truncated = rc == ERR_TRUNCATED
        if rc != 0 and rc != ERR_TRUNCATED:
            _check(rc)
        return [(kps[i, :cnt[i]].copy(), sc[i, :cnt[i]].copy(), desc[i, :cnt[i]].copy()) for i in range(n)]

    def extract_all_batch(self, images, n_netvlad, cap=None):
        """d2fe_extract_all_batch: SuperPoint on all images + NetVLAD on the first n_netvlad, one upload, two streams.
        Returns (list of (kps, scores, desc), netvlad [n_netvlad, G])."""
        images = np.ascontiguousarray(images, np.uint8)
        if images.ndim == 2:
            images = images[None]
        n, H, W = images.shape
        if not cap:
            cap = self.cfg.max_keypoints if self.cfg.max_keypoints > 0 else KEEP_ALL_CAP
        kps = np.zeros((n, cap, 2), np.float32); sc = np.zeros((n, cap), np.float32)
        desc = np.zeros((n, cap, self.desc_dim), np.float32); cnt = np.zeros(n, np.int32)
        g = np.zeros((max(n_netvlad, 1), self.netvlad_dim), np.float32)
        rc = self._lib.d2fe_extract_all_batch(self._h, _ptr(images), n, W, H, W, H * W, _ptr(kps), _ptr(sc), _ptr(desc), cap, _ptr(cnt),
                                              int(n_netvlad), _ptr(g))
        self.last_truncated = rc == ERR_TRUNCATED
        if rc != 0 and rc != ERR_TRUNCATED:
            _check(rc)
        return [(kps[i, :cnt[i]].copy(), sc[i, :cnt[i]].copy(), desc[i, :cnt[i]].copy()) for i in range(n)], g[:n_netvlad].copy()

    def graph_count(self):
        """(cached hipGraphs of host-pointer launch sequences, geometries whose capture was rejected) -- include/d2fe.h."""
        self._need_dev("graph_count")
        bad = C.c_int(0)
        self._lib.d2fe_debug_graph_count.argtypes = [C.c_void_p, C.c_void_p]
        n = int(self._lib.d2fe_debug_graph_count(self._h, C.byref(bad)))
        return n, int(bad.value)

    def match_fallback_rows(self, reset=True, full=False):
        """Queries that needed more than the matcher's first four candidates since the last reset (include/d2fe.h); full=True returns
        (that count, the number that took the exact scan of all train rows)."""
        fs = C.c_long(0)
        r = int(self._lib.d2fe_match_fallback_rows(self._h, int(bool(reset)), C.byref(fs)))
        if r < 0:
            _check(r)
        return (r, int(fs.value)) if full else r

    def extract_device(self, d_gray, n, W, H, d_kps, d_scores, d_desc, d_idx, cap, d_n, stream=None, stride=None,
                       image_stride=None):
        """Device-resident form; arguments are raw device addresses (ints)."""
        _check(self._lib.d2fe_superpoint_extract_device(self._h, d_gray, n, W, H, stride or W, image_stride or H * W,
                                                        d_kps, d_scores, d_desc, d_idx, cap, d_n, stream))

    def tail_stream(self):
        """async_tail mode: raw hipStream_t on which the outputs of extract_device become valid (0 when the mode is off)."""
        return int(self._lib.d2fe_tail_stream(self._h) or 0)

    def wait_tail(self, stream=None):
        _check(self._lib.d2fe_superpoint_wait_tail(self._h, C.c_void_p(stream or 0)))

    def debug_read(self, name, shape):
        self._need_dev("debug_read")
        out = np.empty(shape, np.float32)
        r = self._lib.d2fe_debug_read(self._h, name.encode(), _ptr(out), out.nbytes)
        if r < 0:
            _check(int(r))
        if r != out.nbytes:
            raise D2FEError(-1, "debug_read size mismatch %d vs %d" % (r, out.nbytes))
        return out

    def debug_conv3x3_wino(self, x, weight, bias, pool=False, relu=True, iters=0):
        """One 3x3 layer through the Winograd kernels: x [n,H,W,Cin] NHWC, weight [Cout,Cin,3,3].  Returns (out, ms_per_launch)."""
        self._need_dev("debug_conv3x3_wino")
        x = np.ascontiguousarray(x, np.float32); weight = np.ascontiguousarray(weight, np.float32)
        bias = np.ascontiguousarray(bias, np.float32)
        n, H, W, cin = x.shape
        cout = weight.shape[0]
        out = np.empty((n, H // 2, W // 2, cout) if pool else (n, H, W, cout), np.float32)
        ms = C.c_float(0.0)
        _check(self._lib.d2fe_debug_conv3x3_wino(self._h, _ptr(x), n, H, W, cin, _ptr(weight), _ptr(bias), cout, int(pool),
                                                 int(relu), _ptr(out), int(iters), C.byref(ms)))
        return out, float(ms.value)

    def sync(self):
        _check(self._lib.d2fe_sync(self._h))

    def exact_order_stats(self):
        """Cumulative exact_order counters of the handle and its pipe lanes: dict(marked, cells, dropped, calls); zeros when the option is off."""
        v = (C.c_int64 * 4)()
        _check(self._lib.d2fe_exact_order_stats(self._h, v))
        return dict(marked=int(v[0]), cells=int(v[1]), dropped=int(v[2]), calls=int(v[3]))

    def profile_enable(self, mode):
        """0 off, 1 dominant kernel (conv1b) only, 2 every stage (HIP events on the launch stream)."""
        _check(self._lib.d2fe_profile_enable(self._h, int(mode)))

    def profile_read(self):
        ms = np.zeros(len(PROF_STAGES), np.float32); cnt = np.zeros(len(PROF_STAGES), np.int32)
        _check(self._lib.d2fe_profile_read(self._h, _ptr(ms), _ptr(cnt)))
        return {n: (float(ms[i]), int(cnt[i])) for i, n in enumerate(PROF_STAGES)}

    # ---- NetVLAD (MobileNetVLADONNX, mobilenetvlad_onnx.h:18-74) ---------------------------------------------------------
    def load_netvlad(self, nv):
        """nv: dict(layers=[dict(kind, cin, cout, stride, act, res, weight, bias)...], head=dict(pre_w, pre_b, assign_w,
        assign_b, centroids)) as produced by d2slam_amd.netvlad.synthetic_netvlad_weights()."""
        kinds = {"conv": 0, "pw": 1, "dw": 2}
        n = len(nv["layers"])
        arr = (_NvLayer * n)()
        keep = []
        for i, l in enumerate(nv["layers"]):
            w = np.ascontiguousarray(l["weight"], np.float32); b = np.ascontiguousarray(l["bias"], np.float32)
            keep += [w, b]
            arr[i] = _NvLayer(kinds[l["kind"]], l["cin"], l["cout"], l["stride"], l["act"], l["res"], w.ctypes.data, b.ctypes.data)
        hd = {k: np.ascontiguousarray(v, np.float32) for k, v in nv["head"].items()}
        ws = _NvWeights(n, C.cast(arr, C.c_void_p), hd["pre_w"].shape[1], hd["pre_w"].shape[0], hd["assign_w"].shape[0],
                        hd["pre_w"].ctypes.data, hd["pre_b"].ctypes.data, hd["assign_w"].ctypes.data,
                        hd["assign_b"].ctypes.data, hd["centroids"].ctypes.data)
        _check(self._lib.d2fe_load_netvlad(self._h, C.byref(ws)))

    def load_netvlad_onnx(self, path):
        """MobileNetVLADONNX's constructor takes an ONNX file (mobilenetvlad_onnx.h:18-47): graph -> layer list -> d2fe_load_netvlad."""
        from . import onnx_graph
        self.load_netvlad(onnx_graph.load_netvlad_onnx(path))

    def set_netvlad_pca(self, comp, mean):
        if comp is None:
            _check(self._lib.d2fe_set_netvlad_pca(self._h, None, None, 0))
            return
        comp = np.ascontiguousarray(comp, np.float32); mean = np.ascontiguousarray(mean, np.float32)
        _check(self._lib.d2fe_set_netvlad_pca(self._h, _ptr(comp), _ptr(mean), comp.shape[0]))

    @property
    def netvlad_dim(self):
        r = int(self._lib.d2fe_netvlad_dim(self._h))
        if r < 0:
            _check(r)
        return r

    def debug_netvlad_layer(self, layer, shape):
        """Output of one layer of the last netvlad call ([n,h,w,c] fp32) or None when it only exists inside a fused block."""
        self._need_dev("debug_netvlad_layer")
        out = np.empty(shape, np.float32)
        self._lib.d2fe_debug_netvlad_layer.restype = C.c_long
        r = self._lib.d2fe_debug_netvlad_layer(self._h, int(layer), int(shape[0]), _ptr(out), C.c_size_t(out.nbytes))
        if r == -3:      # D2FE_ERR_NOT_READY
            return None
        if r < 0:
            _check(int(r))
        assert r == out.nbytes, (r, out.nbytes)
        return out

    def debug_netvlad_stamps(self, max_wgs=32768):
        """[workgroups][32] uint64 phase stamps of the plan step named by D2FE_NV_STAMP_STEP (see include/d2fe.h)."""
        self._need_dev("debug_netvlad_stamps")
        out = np.zeros((max_wgs, 32), np.uint64)
        self._lib.d2fe_debug_netvlad_stamps.restype = C.c_long
        r = int(self._lib.d2fe_debug_netvlad_stamps(self._h, _ptr(out), C.c_long(max_wgs)))
        if r < 0:
            _check(r)
        return out[:r]

    def netvlad(self, images):
        """MobileNetVLADONNX::inference for a batch of u8 images [n,H,W] -> [n, netvlad_dim]."""
        images = np.ascontiguousarray(images, np.uint8)
        if images.ndim == 2:
            images = images[None]
        n, H, W = images.shape
        out = np.zeros((n, self.netvlad_dim), np.float32)
        _check(self._lib.d2fe_netvlad_batch(self._h, _ptr(images), n, W, H, W, H * W, _ptr(out)))
        return out

    def netvlad_device(self, d_gray, n, W, H, d_out, stream=None, stride=None, image_stride=None):
        _check(self._lib.d2fe_netvlad_device(self._h, d_gray, n, W, H, stride or W, image_stride or H * W, d_out, stream))

    # ---- SURVEY 8(f) next rows ------------------------------------------------------------------------------------------------
    def undistort(self, src, mapx, mapy, gain=None):
        """FisheyeUndist::undist_id_cuda (fisheye_undistort.h:152-176): remap(INTER_LINEAR) [+ photometric gain] -> u8."""
        src = np.ascontiguousarray(src, np.uint8); mapx = np.ascontiguousarray(mapx, np.float32); mapy = np.ascontiguousarray(mapy, np.float32)
        g = np.ascontiguousarray(gain, np.float32) if gain is not None else None
        dst = np.empty(mapx.shape, np.uint8)
        _check(self._lib.d2fe_undistort(self._h, _ptr(src), src.shape[1], src.shape[0], src.shape[1], _ptr(mapx), _ptr(mapy),
                                        _ptr(g), mapx.shape[1], mapx.shape[0], _ptr(dst)))
        return dst

    def undistort_device(self, d_src, n, sw, sh, d_mapx, d_mapy, d_gain, dw, dh, d_dst, stream=None, sstride=None,
                         src_image_stride=None):
        """Device-resident undistort of n frames sharing one map set (raw addresses)."""
        _check(self._lib.d2fe_undistort_device(self._h, d_src, n, sw, sh, sstride or sw, src_image_stride if src_image_stride is not None else sw * sh,
                                               d_mapx, d_mapy, d_gain, dw, dh, d_dst, stream))

    def quad_undistort_device(self, d_raw, quads, sw, sh, maps, dw, dh, d_dst, stream=None, sstride=None, camera_stride=None, quad_stride=None):
        """The quad pipe's undistort step on its own (d2fe_quad_undistort_device): 4 cameras x quads raw frames in ONE launch.  maps: per camera
        (d_mapx, d_mapy, d_gain or None), raw device addresses, 16-byte aligned; view (q, c) is written to d_dst + (q * 4 + c) * dw * dh."""
        st = int(sstride or sw)
        cs = int(camera_stride if camera_stride is not None else st * sh)
        qs = int(quad_stride if quad_stride is not None else 4 * cs)
        m = _quad_maps(maps, True)
        _check(self._lib.d2fe_quad_undistort_device(self._h, C.c_void_p(d_raw), int(quads), int(sw), int(sh), st, cs, qs, C.byref(m), int(dw), int(dh),
                                                    C.c_void_p(d_dst), C.c_void_p(stream or 0)))

    def prepare_gray(self, img, width, height):
        """cv::cvtColor(BGR2GRAY) if 3 channels + cv::resize to (width, height) if the size differs (superpoint_onnx.cpp:76-83)."""
        img = np.ascontiguousarray(img, np.uint8)
        ch = 1 if img.ndim == 2 else img.shape[2]
        sh, sw = img.shape[:2]
        out = np.zeros((height, width), np.uint8)
        _check(self._lib.d2fe_prepare_gray(self._h, _ptr(img), ch, sw, sh, sw * ch, int(width), int(height), _ptr(out)))
        return out

    @staticmethod
    def _mei(cam):
        """cam: dict(xi,k1,k2,p1,p2,gamma1,gamma2,u0,v0) or the 9 values in that order (kalibr 'omni' + 'radtan')."""
        keys = ("xi", "k1", "k2", "p1", "p2", "gamma1", "gamma2", "u0", "v0")
        vals = [cam[k] for k in keys] if isinstance(cam, dict) else list(cam)
        return (C.c_double * 9)(*[float(v) for v in vals])

    def gen_cylinder_map(self, cam, width, height, fov_deg):
        """FisheyeUndist::generateCylinderMap (fisheye_undistort.h:458-500) -> (mapx, mapy) float32 [height, width]."""
        mx = np.zeros((height, width), np.float32); my = np.zeros((height, width), np.float32)
        _check(self._lib.d2fe_gen_cylinder_map(self._h, self._mei(cam), int(width), int(height), float(fov_deg), _ptr(mx), _ptr(my)))
        return mx, my

    def gen_cylinder_map_device(self, cam, width, height, fov_deg, d_mapx, d_mapy, stream=None):
        _check(self._lib.d2fe_gen_cylinder_map_device(self._h, self._mei(cam), int(width), int(height), float(fov_deg),
                                                      C.c_void_p(d_mapx), C.c_void_p(d_mapy), C.c_void_p(stream or 0)))

    def gen_pinhole_map(self, cam, q_wxyz, width, height, f):
        """genOneUndistMap(id, cam, rotation, w, h, f) (fisheye_undistort.h:615-660) -> (mapx, mapy)."""
        mx = np.zeros((height, width), np.float32); my = np.zeros((height, width), np.float32)
        q = (C.c_double * 4)(*[float(v) for v in q_wxyz])
        _check(self._lib.d2fe_gen_pinhole_map(self._h, self._mei(cam), q, int(width), int(height), float(f), _ptr(mx), _ptr(my)))
        return mx, my

    def quantize_int8(self, x, double_max=False):
        x = np.ascontiguousarray(x, np.float32).reshape(-1)
        out = np.empty(x.shape[0], np.int8)
        _check(self._lib.d2fe_quantize_int8(self._h, _ptr(x), x.shape[0], int(double_max), _ptr(out)))
        return out

    def dequantize_int8(self, q, landmark_num=-1):
        q = np.ascontiguousarray(q, np.int8).reshape(-1)
        out = np.empty(q.shape[0], np.float32)
        _check(self._lib.d2fe_dequantize_int8(self._h, _ptr(q), q.shape[0], int(landmark_num), _ptr(out)))
        return out

    # ---- matcher -------------------------------------------------------------------------------------------------
    def match_knn(self, desc_a, desc_b, knn_match_ratio=0.8, pts_a=None, pts_b=None, search_local_dist=-1.0):
        a = np.ascontiguousarray(desc_a, np.float32); b = np.ascontiguousarray(desc_b, np.float32)
        na = a.shape[0] if a.ndim == 2 else 0
        nb = b.shape[0] if b.ndim == 2 else 0
        dim = a.shape[1] if na else (b.shape[1] if nb else 256)
        cap = max(na, 1)
        q = np.zeros(cap, np.int32); t = np.zeros(cap, np.int32); d = np.zeros(cap, np.float32); n = C.c_int(0)
        pa = np.ascontiguousarray(pts_a, np.float32) if pts_a is not None and len(pts_a) else None
        pb = np.ascontiguousarray(pts_b, np.float32) if pts_b is not None and len(pts_b) else None
        _check(self._lib.d2fe_match_knn(self._h, _ptr(a), na, _ptr(b), nb, dim, float(knn_match_ratio), _ptr(pa), _ptr(pb),
                                        float(search_local_dist), _ptr(q), _ptr(t), _ptr(d), cap, C.byref(n)))
        return q[:n.value].copy(), t[:n.value].copy(), d[:n.value].copy()

    def match_crosscheck(self, desc_a, desc_b):
        a = np.ascontiguousarray(desc_a, np.float32); b = np.ascontiguousarray(desc_b, np.float32)
        na, nb = a.shape[0], b.shape[0]
        dim = a.shape[1]
        cap = max(na, 1)
        q = np.zeros(cap, np.int32); t = np.zeros(cap, np.int32); d = np.zeros(cap, np.float32); n = C.c_int(0)
        _check(self._lib.d2fe_match_crosscheck(self._h, _ptr(a), na, _ptr(b), nb, dim, _ptr(q), _ptr(t), _ptr(d), cap,
                                               C.byref(n)))
        return q[:n.value].copy(), t[:n.value].copy(), d[:n.value].copy()

    def pack_blocks_device(self, d_desc, d_kps, d_scores, d_n, d_netvlad, row0, row_step, nframes, cap, netvlad_dim, d_blocks, stream=None, desc_dim=256):
        """One exchange block per frame (desc | kps | scores | netvlad | n), raw device addresses; desc_dim: floats per descriptor row; see include/d2fe.h."""
        _check(self._lib.d2fe_pack_blocks_device_d(self._h, C.c_void_p(d_desc), C.c_void_p(d_kps), C.c_void_p(d_scores), C.c_void_p(d_n),
                                                   C.c_void_p(d_netvlad or 0), int(row0), int(row_step), int(nframes), int(cap), int(desc_dim), int(netvlad_dim),
                                                   C.c_void_p(d_blocks), C.c_void_p(stream or 0)))

    def pack_blocks_int8_device(self, d_desc, d_kps, d_n, d_netvlad, row0, row_step, nframes, cap, netvlad_dim, d_blocks, stream=None, desc_dim=256):
        """Exchange blocks in the reference's int8 wire precision (VisualImageDesc::toLCM); raw device addresses."""
        V = C.c_void_p
        _check(self._lib.d2fe_pack_blocks_int8_device_d(self._h, V(d_desc), V(d_kps), V(d_n), V(d_netvlad or 0), int(row0), int(row_step), int(nframes),
                                                        int(cap), int(desc_dim), int(netvlad_dim), V(d_blocks), V(stream or 0)))

    def unpack_blocks_int8_device(self, d_blocks_int8, nblocks, cap, netvlad_dim, d_blocks, renorm=0, stream=None, desc_dim=256):
        """Gathered int8 blocks -> fp32 block layout with the reference's decode (renorm 0) or every descriptor re-normalised over its row (1)."""
        V = C.c_void_p
        _check(self._lib.d2fe_unpack_blocks_int8_device_d(self._h, V(d_blocks_int8), int(nblocks), int(cap), int(desc_dim), int(netvlad_dim), int(renorm),
                                                          V(d_blocks), V(stream or 0)))

    def gate_pairs_device(self, d_q, q_stride, d_db, db_stride, dim, d_pair_q, d_pair_db, npairs, thres, d_cnt_inout=None, d_pass=None,
                          d_sims=None, d_n_pass=None, stream=None):
        """NetVLAD gate of a pair list (getMatchedPrevKeyframe's similarity test), raw device addresses."""
        _check(self._lib.d2fe_gate_pairs_device(self._h, C.c_void_p(d_q), C.c_size_t(q_stride), C.c_void_p(d_db), C.c_size_t(db_stride), int(dim),
                                                C.c_void_p(d_pair_q), C.c_void_p(d_pair_db), int(npairs), C.c_double(thres),
                                                C.c_void_p(d_cnt_inout or 0), C.c_void_p(d_pass or 0), C.c_void_p(d_sims or 0),
                                                C.c_void_p(d_n_pass or 0), C.c_void_p(stream or 0)))

    def quad_gate_device(self, d_local, local_stride, d_remote, remote_stride, dim, d_job_local_row0, d_job_remote_row0, local_view_step,
                         remote_view_step, njobs, thres, d_dir_prev=None, d_sims=None, d_cnt_inout=None, d_n_pass=None, stream=None):
        """The FOURCORNER_FISHEYE gate of getMatchedPrevKeyframe + the view pairing of trackRemoteFrames (include/d2fe.h)."""
        V = C.c_void_p
        _check(self._lib.d2fe_quad_gate_device(self._h, V(d_local), C.c_size_t(local_stride), V(d_remote), C.c_size_t(remote_stride), int(dim),
                                               V(d_job_local_row0), V(d_job_remote_row0), int(local_view_step), int(remote_view_step),
                                               int(njobs), C.c_double(thres), V(d_dir_prev or 0), V(d_sims or 0), V(d_cnt_inout or 0),
                                               V(d_n_pass or 0), V(stream or 0)))

    def half_image_compact_device(self, d_desc, d_pts, d_n, d_job_row, d_job_left, d_job_shift, njobs, cap, dim, width_undistort, undistort_fov,
                                  d_out_desc, d_out_pts, d_out_map, d_out_n, stream=None):
        """getFeatureHalfImg for a batch of jobs + the a-side x shift (d2featuretracker.cpp:1051-1075,1161-1170); raw device addresses."""
        V = C.c_void_p
        _check(self._lib.d2fe_half_image_compact_device(self._h, V(d_desc), V(d_pts), V(d_n), V(d_job_row), V(d_job_left), V(d_job_shift), int(njobs),
                                                        int(cap), int(dim), int(width_undistort), C.c_double(undistort_fov), V(d_out_desc), V(d_out_pts),
                                                        V(d_out_map), V(d_out_n), V(stream or 0)))

    def half_move_cols(self, width_undistort, undistort_fov):
        """move_cols of getFeatureHalfImg: (float)(width_undistort * 90.0 / undistort_fov)."""
        return float(self._lib.d2fe_half_move_cols(int(width_undistort), float(undistort_fov)))

    def remap_matches_device(self, d_q, d_t, d_n_match, d_map_a_job, d_map_b_job, d_maps, npairs, cap_match, cap_map, stream=None):
        """Index remap of matchLocalFeatures (d2featuretracker.cpp:1178-1181) for a batch of pairs; raw device addresses."""
        V = C.c_void_p
        _check(self._lib.d2fe_remap_matches_device(self._h, V(d_q), V(d_t), V(d_n_match), V(d_map_a_job), V(d_map_b_job), V(d_maps), int(npairs),
                                                   int(cap_match), int(cap_map), V(stream or 0)))

    def match_batch_device(self, d_a, d_b, d_a_off, d_b_off, d_a_cnt, d_b_cnt, npairs, dim, max_n, d_q, d_t, d_dist,
                           d_n, mode=0, ratio=0.8, radius=-1.0, d_pts_a=None, d_pts_b=None, stream=None):
        mb = _MatchBatch(d_a, d_b, d_pts_a, d_pts_b, d_a_off, d_b_off, d_a_cnt, d_b_cnt, npairs, dim, max_n, mode,
                         ratio, radius, d_q, d_t, d_dist, d_n)
        _check(self._lib.d2fe_match_batch_device(self._h, C.byref(mb), stream))


class DevFrontEnd(FrontEnd):
    """FrontEnd on the development library (lib/libd2fe_hip_dev.so): the d2fe_debug_* test hooks and the D2FE_* schedule switches exist only there."""

    def __init__(self, cfg: SuperPointConfig):
        super().__init__(cfg, dev=True)

    # ---- the SuperPoint tail kernels of csrc/postproc.hip on injected tensors (include/d2fe_debug.h; tests/test_postproc_edges.py) ----
    def debug_softmax_cand(self, logits, thr, border, want_semi=True):
        """softmax_cand_kernel on logits [n, Hc, Wc, lstride >= 65] (channels 65.. are padding).  Returns (semi [n, 8Hc, 8Wc] or None,
        [the u64 candidate keys of image i, in the order the kernel left them], counts [n])."""
        logits = np.ascontiguousarray(logits, np.float32)
        n, Hc, Wc, lstride = logits.shape
        semi = np.empty((n, Hc * 8, Wc * 8), np.float32) if want_semi else None
        cand = np.empty((n, 64 * Hc * Wc), np.uint64); cnt = np.empty(n, np.int32)
        _check(self._lib.d2fe_debug_softmax_cand(self._h, _ptr(logits), lstride, n, Hc, Wc, float(thr), int(border), int(bool(want_semi)), _ptr(semi),
                                                 _ptr(cand), _ptr(cnt)))
        return semi, [cand[i, :min(int(cnt[i]), cand.shape[1])].copy() for i in range(n)], cnt

    def debug_select_b(self, keys, W, H, max_kp, cap, always_sort=False, semi=None, thr=0.0, border=0, counts=None):
        """select_b_kernel on injected keys: `keys` is a list of u64 arrays, one per image (counts: the cand_count entries, the lists' lengths by default).
        Returns one (kps_xy [m, 2], scores [m], idx [m]) per image, m = the kernel's n_out."""
        n = len(keys)
        cand_cap = max(1, max(len(k) for k in keys))
        cand = np.zeros((n, cand_cap), np.uint64)
        for i, k in enumerate(keys):
            cand[i, :len(k)] = k
        cnt = np.ascontiguousarray([len(k) for k in keys] if counts is None else counts, np.int32)
        if semi is not None:
            semi = np.ascontiguousarray(semi, np.float32).reshape(n, H, W)
        kps = np.empty((n, cap, 2), np.float32); sc = np.empty((n, cap), np.float32); idx = np.empty((n, cap), np.int32); m = np.empty(n, np.int32)
        _check(self._lib.d2fe_debug_select_b(self._h, _ptr(cand), _ptr(cnt), cand_cap, n, W, H, int(max_kp), int(cap), int(bool(always_sort)), _ptr(semi),
                                             float(thr), int(border), _ptr(kps), _ptr(sc), _ptr(idx), _ptr(m)))
        return [(kps[i, :m[i]].copy(), sc[i, :m[i]].copy(), idx[i, :m[i]].copy()) for i in range(n)]

    def debug_sample_b(self, desc_raw, kps_xy, n_kp, dcoff=0, slotmap=None):
        """sample_b_kernel.  Dense form: desc_raw [n, Hc, Wc, dstride], read at channel offset dcoff.  Sparse form: desc_raw [n, max_slots, 256] and
        slotmap [n, Hc, Wc].  kps_xy [n, cap, 2], n_kp [n].  Returns desc [n, cap, 256] (rows at and beyond n_kp are not written)."""
        desc_raw = np.ascontiguousarray(desc_raw, np.float32); kps_xy = np.ascontiguousarray(kps_xy, np.float32)
        n_kp = np.ascontiguousarray(n_kp, np.int32)
        n, cap = kps_xy.shape[0], kps_xy.shape[1]
        if slotmap is None:
            _, Hc, Wc, dstride = desc_raw.shape
            max_slots = 0
        else:
            slotmap = np.ascontiguousarray(slotmap, np.int32)
            _, Hc, Wc = slotmap.shape
            dstride, max_slots = 256, desc_raw.shape[1]
        out = np.empty((n, cap, 256), np.float32)
        _check(self._lib.d2fe_debug_sample_b(self._h, _ptr(desc_raw), dstride, int(dcoff), n, Hc, Wc, _ptr(kps_xy), _ptr(n_kp), cap, _ptr(slotmap), max_slots,
                                             _ptr(out)))
        return out

    def debug_sample_b_pca(self, desc_raw, kps_xy, n_kp, comp, mean, dcoff=0, slotmap=None):
        """sample_b_pca_kernel: debug_sample_b's arguments plus comp [pca_dims, 256] and mean [256].  Returns desc [n, cap, pca_dims]."""
        self._need_dev("debug_sample_b_pca")
        desc_raw = np.ascontiguousarray(desc_raw, np.float32); kps_xy = np.ascontiguousarray(kps_xy, np.float32)
        n_kp = np.ascontiguousarray(n_kp, np.int32)
        comp = np.ascontiguousarray(comp, np.float32); mean = np.ascontiguousarray(mean, np.float32)
        assert comp.ndim == 2 and comp.shape[1] == 256 and mean.shape == (256,)
        n, cap = kps_xy.shape[0], kps_xy.shape[1]
        if slotmap is None:
            _, Hc, Wc, dstride = desc_raw.shape
            max_slots = 0
        else:
            slotmap = np.ascontiguousarray(slotmap, np.int32)
            _, Hc, Wc = slotmap.shape
            dstride, max_slots = 256, desc_raw.shape[1]
        out = np.empty((n, cap, comp.shape[0]), np.float32)
        _check(self._lib.d2fe_debug_sample_b_pca(self._h, _ptr(desc_raw), dstride, int(dcoff), n, Hc, Wc, _ptr(kps_xy), _ptr(n_kp), cap, _ptr(slotmap), max_slots,
                                                 _ptr(comp), _ptr(mean), comp.shape[0], _ptr(out)))
        return out

    def debug_nms2_a(self, semi, thr, dist, max_kp, cap):
        """Variant A's keypoint selection on semi [n, H, W]: nms2_a_kernel, select_b_kernel (always_sort) and the CV_16UC1 wrap.
        Returns one (kps_xy, scores, idx) per image."""
        semi = np.ascontiguousarray(semi, np.float32)
        n, H, W = semi.shape
        kps = np.empty((n, cap, 2), np.float32); sc = np.empty((n, cap), np.float32); idx = np.empty((n, cap), np.int32); m = np.empty(n, np.int32)
        _check(self._lib.d2fe_debug_nms2_a(self._h, _ptr(semi), n, H, W, float(thr), int(dist), int(max_kp), int(cap), _ptr(kps), _ptr(sc), _ptr(idx), _ptr(m)))
        return [(kps[i, :m[i]].copy(), sc[i, :m[i]].copy(), idx[i, :m[i]].copy()) for i in range(n)]

    # ---- the sparse descriptor head and variant A's descriptor tail on injected tensors (include/d2fe_debug.h; tests/test_desc_head_edges.py) ----
    def debug_desc_head_sparse(self, x, kps_xy, n_kp, max_slots, w_da, b_da, w_db, b_db, with_mid=False, img_w=0, img_h=0):
        """launch_desc_head_sparse on x [n, Hc, Wc, x_cstride >= 128] (channels 128.. are padding), kps_xy [n, cap, 2], n_kp [n]; w_da [256, 128, 3, 3],
        w_db [256, 256, 1, 1].  img_w = 0: variant B's corners, else variant A's.  Returns (store [n, max_slots, 256], slotmap [n, Hc, Wc], cells [n, max_slots],
        count [n]); what the kernels did not write holds all-ones words."""
        x = np.ascontiguousarray(x, np.float32); kps_xy = np.ascontiguousarray(kps_xy, np.float32); n_kp = np.ascontiguousarray(n_kp, np.int32)
        w_da = np.ascontiguousarray(w_da, np.float32); b_da = np.ascontiguousarray(b_da, np.float32)
        w_db = np.ascontiguousarray(w_db, np.float32); b_db = np.ascontiguousarray(b_db, np.float32)
        assert w_da.shape == (256, 128, 3, 3) and w_db.shape == (256, 256, 1, 1) and b_da.shape == (256,) and b_db.shape == (256,)
        n, Hc, Wc, xs = x.shape
        cap = kps_xy.shape[1]
        assert kps_xy.shape == (n, cap, 2) and n_kp.shape == (n,)
        ms = max(int(max_slots), 1)
        store = np.empty((n, ms, 256), np.float32); slotmap = np.empty((n, Hc, Wc), np.int32)
        cells = np.empty((n, ms), np.int32); count = np.empty(n, np.int32)
        _check(self._lib.d2fe_debug_desc_head_sparse(self._h, _ptr(x), xs, n, Hc, Wc, _ptr(kps_xy), _ptr(n_kp), cap, int(max_slots), int(bool(with_mid)),
                                                     int(img_w), int(img_h), _ptr(w_da), _ptr(b_da), _ptr(w_db), _ptr(b_db), _ptr(slotmap), _ptr(cells),
                                                     _ptr(count), _ptr(store)))
        return store, slotmap, cells, count

    def debug_sample_a(self, desc_raw, kps_xy, n_kp, img_w, img_h, scap=None, dcoff=0, slotmap=None, comp=None, mean=None):
        """Variant A's computeDescriptors (sample_a_kernel, chan_norm_a_kernel, finish_a_kernel); desc_raw / slotmap as for debug_sample_b, scap = keypoints
        per image of the sampling scratch (cap by default), comp [pca_dims, 256] with mean [256] or None.  Returns desc [n, cap, pca_dims or 256]."""
        desc_raw = np.ascontiguousarray(desc_raw, np.float32); kps_xy = np.ascontiguousarray(kps_xy, np.float32)
        n_kp = np.ascontiguousarray(n_kp, np.int32)
        n, cap = kps_xy.shape[0], kps_xy.shape[1]
        if slotmap is None:
            _, Hc, Wc, dstride = desc_raw.shape
            max_slots = 0
        else:
            slotmap = np.ascontiguousarray(slotmap, np.int32)
            _, Hc, Wc = slotmap.shape
            dstride, max_slots = 256, desc_raw.shape[1]
        pd = 0
        if comp is not None:
            comp = np.ascontiguousarray(comp, np.float32); mean = np.ascontiguousarray(mean, np.float32)
            assert comp.ndim == 2 and comp.shape[1] == 256 and mean.shape == (256,)
            pd = comp.shape[0]
        out = np.empty((n, cap, pd or 256), np.float32)
        _check(self._lib.d2fe_debug_sample_a(self._h, _ptr(desc_raw), dstride, int(dcoff), n, Hc, Wc, int(img_w), int(img_h), _ptr(kps_xy), _ptr(n_kp), cap,
                                             int(cap if scap is None else scap), _ptr(slotmap), max_slots, _ptr(comp), _ptr(mean), pd, _ptr(out)))
        return out

    # ---- one layer of the direct SuperPoint conv kernels on injected tensors (include/d2fe_debug.h; tests/test_conv_layer_edges.py) ----
    def debug_conv_layer(self, family, precision, shape, weight, bias, n, H, W, out, out_cstride, out_coff, out_img_stride, x=None, in_cstride=0, in_coff=0,
                         in_img_stride=0, pool=False, relu=True, conv64_tile=1, ncu=0, frames=None, img_stride=0, img_istride=0, w1a=None, b1a=None,
                         status=False, in_range=None):
        """d2fe_debug_conv_layer (in_range given: d2fe_debug_conv_layer_q, see debug_conv_layer_q).  x: the WHOLE input buffer (any shape, fp32), out: the WHOLE pre-filled output buffer -- a copy comes back with what the
        kernels wrote and the caller's values everywhere else.  weight [cout, cin, k, k], bias [cout]; shape 4 (CONV1B_FUSED) takes frames (u8, whole buffer) with
        w1a [64, 1, 3, 3] and b1a [64] instead of x.  Raises D2FEError (code -1 refused, -5 family 3: the launcher does not take the tensors); status=True returns (code, out) instead."""
        weight = np.ascontiguousarray(weight, np.float32); bias = np.ascontiguousarray(bias, np.float32)
        assert weight.ndim == 4 and bias.shape == (weight.shape[0],)
        out = np.array(out, np.float32, order="C")
        if x is not None:
            x = np.ascontiguousarray(x, np.float32)
        if frames is not None:
            frames = np.ascontiguousarray(frames, np.uint8)
            w1a = np.ascontiguousarray(w1a, np.float32); b1a = np.ascontiguousarray(b1a, np.float32)
            assert w1a.shape == (64, 1, 3, 3) and b1a.shape == (64,)
        p = _DebugConv(int(family), int(precision), int(shape), int(conv64_tile), int(bool(pool)), int(bool(relu)), int(n), int(H), int(W), weight.shape[0],
                       int(in_cstride), int(in_coff), int(out_cstride), int(out_coff), int(img_stride), int(ncu), int(in_img_stride),
                       0 if x is None else x.size, int(out_img_stride), out.size, int(img_istride), 0 if frames is None else frames.size)
        if in_range is None:
            rc = int(self._lib.d2fe_debug_conv_layer(self._h, C.byref(p), _ptr(weight), _ptr(bias), _ptr(x), _ptr(out), _ptr(frames), _ptr(w1a), _ptr(b1a)))
        else:
            rc = int(self._lib.d2fe_debug_conv_layer_q(self._h, C.byref(p), _ptr(weight), _ptr(bias), _ptr(x), _ptr(out), _ptr(frames), _ptr(w1a), _ptr(b1a),
                                                       float(in_range)))
        if status:
            return rc, out
        _check(rc)
        return out

    def debug_conv_layer_q(self, family, precision, shape, weight, bias, n, H, W, out, out_cstride, out_coff, out_img_stride, in_range, **kw):
        """d2fe_debug_conv_layer_q: debug_conv_layer with the dynamic range of the layer's INPUT tensor -- the only entry that takes precision PREC_I8 (one-tile
        kernels: family 0 or 1).  For shape 4 in_range is the range of conv1a's output."""
        return self.debug_conv_layer(family, precision, shape, weight, bias, n, H, W, out, out_cstride, out_coff, out_img_stride, in_range=in_range, **kw)

    def debug_conv1a(self, kernel, frames, img_stride, img_istride, n, H, W, w1a, b1a, out):
        """d2fe_debug_conv1a: kernel 0 conv1a_mfma_kernel, 1 conv1a_kernel, -1 launch_conv1a's pick.  frames: the whole u8 buffer; out: the whole pre-filled
        buffer of at least n * H * W * 64 floats, returned as a copy with what the kernel wrote."""
        frames = np.ascontiguousarray(frames, np.uint8)
        w1a = np.ascontiguousarray(w1a, np.float32); b1a = np.ascontiguousarray(b1a, np.float32)
        assert w1a.shape == (64, 1, 3, 3) and b1a.shape == (64,)
        out = np.array(out, np.float32, order="C")
        _check(self._lib.d2fe_debug_conv1a(self._h, int(kernel), _ptr(frames), int(img_stride), int(img_istride), frames.size, int(n), int(H), int(W), _ptr(w1a),
                                           _ptr(b1a), _ptr(out), out.size))
        return out

    # ---- the calibration session's parts on injected data (include/d2fe_debug.h; tests/test_calib_cpu.py, tests/test_calib_edges.py) ----
    @staticmethod
    def calib_ranges_from_hist(hist, t, method, param=None):
        """d2fe_debug_calib_ranges_from_hist: the host rule of d2fe_calib_ranges on one histogram (u64 [n_bins]) of a tensor with range t.  -> (range as
        np.float32, index: ENTROPY the winning candidate, PERCENTILE b + 1, MINMAX and an empty histogram n_bins).  Needs no handle and no GPU."""
        lib = load_library(dev=True)
        hist = np.ascontiguousarray(hist, np.uint64)
        r, k = C.c_float(), C.c_int()
        _check(lib.d2fe_debug_calib_ranges_from_hist(_ptr(hist), int(hist.size), float(t), calib_method(method), float(0.0 if param is None else param),
                                                     C.byref(r), C.byref(k)))
        return np.float32(r.value), int(k.value)

    @staticmethod
    def _calib_out(n_bins, acc):
        if acc is not None:
            return [np.array(a, dt).reshape(-1) for a, dt in zip(acc, (np.uint32, np.uint64, np.uint64, np.uint64))]
        return [np.zeros(1, np.uint32), np.zeros(int(n_bins), np.uint64), np.zeros(1, np.uint64), np.zeros(1, np.uint64)]

    def debug_calib_stats(self, tensor, ch_off, channels, t, n_bins, phase, wgs=0, acc=None):
        """d2fe_debug_calib_stats: calib_stats_kernel on tensor [pixels, ch_stride] f32, channels ch_off .. ch_off + channels.  phase 0: the range phase, 1: the
        histogram phase with T = t.  acc: the (t_max_bits, hist, n_zero, n_over) of an earlier call to accumulate into.  -> (t_max_bits, hist, n_zero, n_over)"""
        self._need_dev("debug_calib_stats")
        tensor = np.ascontiguousarray(tensor, np.float32)
        assert tensor.ndim == 2
        o = self._calib_out(n_bins, acc)
        _check(self._lib.d2fe_debug_calib_stats(self._h, _ptr(tensor), tensor.shape[0], int(ch_off), int(channels), tensor.shape[1], float(t), int(n_bins), int(phase),
                                                int(wgs), *[_ptr(a) for a in o]))
        return int(o[0][0]), o[1], int(o[2][0]), int(o[3][0])

    def debug_calib_conv1a(self, frames, img_stride, img_istride, n, H, W, w1a, b1a, t, n_bins, phase, acc=None):
        """d2fe_debug_calib_conv1a: calib_conv1a_stats_kernel on injected frames and weights (as debug_conv1a takes them); outputs as debug_calib_stats"""
        self._need_dev("debug_calib_conv1a")
        frames = np.ascontiguousarray(frames, np.uint8)
        w1a = np.ascontiguousarray(w1a, np.float32); b1a = np.ascontiguousarray(b1a, np.float32)
        assert w1a.shape == (64, 1, 3, 3) and b1a.shape == (64,)
        o = self._calib_out(n_bins, acc)
        _check(self._lib.d2fe_debug_calib_conv1a(self._h, _ptr(frames), int(img_stride), int(img_istride), frames.size, int(n), int(H), int(W), _ptr(w1a), _ptr(b1a),
                                                 float(t), int(n_bins), int(phase), *[_ptr(a) for a in o]))
        return int(o[0][0]), o[1], int(o[2][0]), int(o[3][0])

    # ---- NetVLAD inspection (include/d2fe_debug.h; tests/test_netvlad_shapes*.py) ----
    @staticmethod
    def netvlad_shapes(family):
        """[(NK, NT)] nv_pblock_kernel is compiled for: family 0 every shape, 1 the shapes that also exist with merged groups.  Needs no handle and no GPU."""
        lib = load_library(dev=True)
        n = int(lib.d2fe_debug_netvlad_shapes(int(family), None, 0))
        if n < 0:
            raise D2FEError(n, "d2fe_debug_netvlad_shapes(%d)" % family)
        out = (C.c_int * (2 * max(n, 1)))()
        assert int(lib.d2fe_debug_netvlad_shapes(int(family), out, n)) == n
        return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n)]

    @staticmethod
    def netvlad_plan(layers, proj_dim):
        """[(kind, first layer, last layer, halves)] of the execution plan d2fe_load_netvlad builds for this layer list (dicts of kind, cin, cout, stride, act,
        res; weights not needed) under the D2FE_NV_* switches of the environment.  Needs no handle and no GPU."""
        lib = load_library(dev=True)
        kinds = {"conv": 0, "pw": 1, "dw": 2}
        arr = (_NvLayer * len(layers))(*[_NvLayer(kinds[l["kind"]], l["cin"], l["cout"], l["stride"], l["act"], l["res"], None, None) for l in layers])
        out = (C.c_int * (4 * 64))()
        n = int(lib.d2fe_debug_netvlad_plan(arr, len(layers), int(proj_dim), out, 64))
        if n < 0:
            _check(n)
        return [tuple(int(v) for v in out[4 * i:4 * i + 4]) for i in range(min(n, 64))]

    def debug_netvlad_features(self, shape):
        """The pre-projected features [n, positions, proj_dim] the VLAD stage of the last netvlad call read (partial slabs added in slab order)."""
        self._need_dev("debug_netvlad_features")
        out = np.empty(shape, np.float32)
        self._lib.d2fe_debug_netvlad_features.restype = C.c_long
        r = int(self._lib.d2fe_debug_netvlad_features(self._h, int(shape[0]), _ptr(out), C.c_size_t(out.nbytes)))
        if r < 0:
            _check(r)
        assert r == out.nbytes, (r, out.nbytes)
        return out

    def debug_netvlad_groups(self, layer):
        """(hidden-channel groups that wrote `layer` in the last netvlad call, partial slabs left in memory: 1 once the slab sum ran); layer -1: the features"""
        self._need_dev("debug_netvlad_groups")
        out = (C.c_int * 2)()
        _check(int(self._lib.d2fe_debug_netvlad_groups(self._h, int(layer), out)))
        return int(out[0]), int(out[1])

    @staticmethod
    def netvlad_slots(cin, cout, ncu, nbuf=1):
        """nv_pblock_slots: resident workgroups of the pixel-pair block shape on a device of ncu compute units.  Needs no handle and no GPU."""
        lib = load_library(dev=True)
        lib.d2fe_debug_netvlad_slots.restype = C.c_long
        r = int(lib.d2fe_debug_netvlad_slots(int(cin), int(cout), int(ncu), int(nbuf)))
        if r < 0:
            raise D2FEError(r, "d2fe_debug_netvlad_slots")
        return r

    @staticmethod
    def regime_counts(reset=False):
        """{regime name: launches since the last reset} of the development library's process-wide launch-regime record (REGIMES; include/d2fe_debug.h):
        which size-dependent code path the Winograd, matcher and NetVLAD launchers took.  Needs no handle (pipes and handles of this process share it)."""
        lib = load_library(dev=True)
        n = int(lib.d2fe_debug_regime_counts(None, 0))
        if n != len(REGIMES):
            raise D2FEError(-1, "api.REGIMES (%d names) out of sync with enum d2fe_regime (%d entries)" % (len(REGIMES), n))
        out = (C.c_longlong * n)()
        lib.d2fe_debug_regime_counts(out, n)
        if reset:
            lib.d2fe_debug_regime_reset()
        return {k: int(out[i]) for i, k in enumerate(REGIMES)}

    @staticmethod
    def regime_reset():
        load_library(dev=True).d2fe_debug_regime_reset()


class _Owned:
    """An object that owns one library object: _HANDLE names the attribute that holds it (a C.c_void_p), _DESTROY the library call that gives it back."""
    _HANDLE = _DESTROY = None

    def close(self):
        h = getattr(self, self._HANDLE, None)
        if h is not None and h.value:
            getattr(self._lib, self._DESTROY)(h)
            setattr(self, self._HANDLE, C.c_void_p())

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


CALIB_METHODS = {"minmax": 0, "entropy": 1, "percentile": 2}      # d2fe_calib_method of include/d2fe.h
CALIB_PERCENTILE_DEFAULT = 99.99


def calib_method(method):
    return CALIB_METHODS[method] if isinstance(method, str) else int(method)


class Int8Calibrator(_Owned):
    """An int8 calibration session (include/d2fe.h, d2fe_calib_*) on a PREC_F32 handle with dense_descriptors and weights loaded; product library.  collect()
    images (range phase), freeze(), collect() again (histogram phase), then ranges("entropy") -> the dict FrontEnd.set_int8_ranges takes.  n_bins 0: 2048."""
    _HANDLE, _DESTROY = "_c", "d2fe_calib_destroy"

    def __init__(self, fe: FrontEnd, n_bins=0):
        self._lib = fe._lib
        self._fe = fe           # the session borrows the handle
        self._c = C.c_void_p()
        _check(self._lib.d2fe_calib_create(fe.handle, int(n_bins), C.byref(self._c)))
        self.n_bins = int(n_bins) or 2048
        if not hasattr(fe, "_pipes"):      # closed with the handle's pipes, before the handle (FrontEnd.close)
            import weakref
            fe._pipes = weakref.WeakSet()
        fe._pipes.add(self)

    def collect(self, images):
        """images: u8 [n, H, W] or [H, W]; n may exceed the handle's max_batch"""
        images = np.ascontiguousarray(images, np.uint8)
        if images.ndim == 2:
            images = images[None]
        n, H, W = images.shape
        _check(self._lib.d2fe_calib_collect(self._c, _ptr(images), W, H, W, H * W, n))

    def freeze(self):
        _check(self._lib.d2fe_calib_freeze(self._c))

    def stats(self, layer, hist=True):
        """layer: a name of SP_LAYERS or its index.  -> {"t_max": np.float32, "hist": u64 [n_bins] (None before freeze() or with hist=False), "n_zero", "n_over",
        "n_total"}"""
        li = SP_LAYERS.index(layer) if isinstance(layer, str) else int(layer)
        t = C.c_float()
        h = np.zeros(self.n_bins, np.uint64) if hist else None
        z, o, tot = C.c_uint64(), C.c_uint64(), C.c_uint64()
        rc = self._lib.d2fe_calib_stats_get(self._c, li, C.byref(t), _ptr(h), C.byref(z), C.byref(o), C.byref(tot))
        if rc == -3 and hist:      # D2FE_ERR_NOT_READY: no histogram before the freeze
            h = None
            rc = self._lib.d2fe_calib_stats_get(self._c, li, C.byref(t), None, C.byref(z), C.byref(o), C.byref(tot))
        _check(rc)
        return {"t_max": np.float32(t.value), "hist": h, "n_zero": int(z.value), "n_over": int(o.value), "n_total": int(tot.value)}

    def ranges(self, method="entropy", param=None):
        """method: "minmax" | "entropy" | "percentile" (param: the percentile, default 99.99).  -> {layer name: range} in SP_LAYERS order, np.float32 values as floats"""
        m = calib_method(method)
        if param is None:
            param = CALIB_PERCENTILE_DEFAULT if m == CALIB_METHODS["percentile"] else 0.0
        r = np.zeros(len(SP_LAYERS), np.float32)
        _check(self._lib.d2fe_calib_ranges(self._c, m, float(param), _ptr(r)))
        return {name: float(r[i]) for i, name in enumerate(SP_LAYERS)}


class StereoPipe(_Owned):
    """Frames in flight (include/d2fe.h, d2fe_pipe_*): the per-frame work of D2Frontend::processStereoframe (SuperPoint on both images, NetVLAD on
    the left one, matchKNN L<->R and L<->previous L) for `frames` stereo frames per submit with up to `lanes` submits in flight.
    lr_lk=True (needs match_lr=False): the reference's default stereo path (lr_match_use_lk) -- SuperPoint on the left images only, every left keypoint
    tracked into the right image with pyramidal LK inside the pass; wait() then also returns "lk_pts" [F, cap, 2] and "lk_status" [F, cap].
    flow_lk=True | "only" (d2fe_pipe_flow_enable; needs lr_lk=True or mono=True, excludes sp_lk; flow_params: a dict of flow_params() keywords or a _FlowParams): the
    flow landmarks, the FAST-replenished LK list, beside SuperPoint or ("only": superpoint = 0, needs netvlad=False, match_prev=False) as the whole front end.  wait()
    then also returns per frame f "flow_n", "flow_n_tracked_in", "flow_n_lost", "flow_n_removed_near", "flow_n_new", "flow_lack", "flow_num", "flow_n_cand" [F],
    "flow_pts" [F, cap_tracks, 2], "flow_id" / "flow_src" [F, cap_tracks], "flow_right_pts" / "flow_right_status" (None on a mono pipe), "flow_depth_mm" (None without depth).
    sp_lk=True (needs lr_lk=True; together the reference's defaults, sp_track_use_lk): the LK-carried landmark list of D2FeatureTracker::trackLK is kept on the
    device and carried across frames, passes and lanes; track_params (a dict of d2fe_track_params fields, or track_params()) replaces the reference's defaults.
    wait() then returns, instead of lk_*, per frame f: "track_n" [F], "track_pts" [F, cap_tracks, 2], "track_id" / "track_src" / "track_kp" [F, cap_tracks],
    "track_desc" [F, cap_tracks, D], "track_scores", "track_right_pts" [F, cap_tracks, 2], "track_right_status" [F, cap_tracks] and the counts
    "track_n_tracked_in", "track_n_lost", "track_n_removed_near", "track_n_new" [F] (include/d2fe.h, d2fe_pipe_track_result).
    mono=True (needs match_lr=False, lr_lk=False): ONE camera per frame, the reference's MONOCULAR configuration -- submit(left) without a right image; the result
    keeps its [2 F] rows, the right ones with n_kp = 0.  With sp_lk=True the list is carried on the one image and "track_right_pts" / "track_right_status" are None.
    depth=True (needs mono=True): PINHOLE_DEPTH -- submit(left, depth=...) with a uint16 depth frame per gray frame; wait() then also returns "kp_depth_mm"
    [F, cap] uint16 (the value under every keypoint, 0 beyond n_kp) and, with sp_lk, "track_depth_mm" [F, cap_tracks] (None otherwise).
    bearings=dict(cam_left=..., cam_right=..., T_right_left=..., distance=100.0, lk_use_pred=True, radius_lk=...) (d2fe_pipe_bearings_enable; every pipe shape): unit
    bearings, extrinsic predictions and the lk_lk_use_pred gate on the device; wait() then also returns "bearing_kp" [2 F, cap, 3] float64, "bearing_kp_pred" [F, cap, 2],
    "bearing_lk_right" [F, cap, 3] / "bearing_lk_pred_ok" [F, cap] (lr_lk without lists) and "bearing_list" / "bearing_list_pred" / "bearing_list_right" /
    "bearing_list_pred_ok" over the entries of the list the pipe carries; None for what the pipe's shape does not produce.  With match_lr and radius_lr > 0 the
    L <-> R radius gate compares the predicted points.
    submit() enqueues and returns a ticket; wait() returns views into the lane's pinned result block (copy what must outlive 2 * lanes submits)."""
    _HANDLE, _DESTROY = "_p", "d2fe_pipe_destroy"

    def __init__(self, fe: FrontEnd, lanes=4, frames=1, width=640, height=480, cap=None, netvlad=True, match_lr=True, match_prev=True,
                 ratio=0.8, radius_lr=-1.0, radius_prev=-1.0, pinned_input=False, cu_partition=False, netvlad_inline=None, coalesce=1, lane_cus=0, netvlad_group=1, coalesce_depth=0,
                 lr_lk=False, sp_lk=False, track_params=None, mono=False, depth=False, flow_lk=False, flow_params=None, bearings=None):
        self._lib = fe._lib
        self._fe = fe           # the pipe borrows the handle's weights
        c = _PipeConfig()
        self._lib.d2fe_pipe_default_config(C.byref(c))
        c.lanes, c.frames, c.width, c.height = int(lanes), int(frames), int(width), int(height)
        c.cap = int(cap or fe.cfg.max_keypoints)
        c.netvlad, c.match_lr, c.match_prev, c.pinned_input = int(bool(netvlad)), int(bool(match_lr)), int(bool(match_prev)), int(bool(pinned_input))
        c.ratio, c.radius_lr, c.radius_prev = float(ratio), float(radius_lr), float(radius_prev)
        c.cu_partition = int(bool(cu_partition)); c.coalesce = int(coalesce); c.lane_cus = int(lane_cus); c.netvlad_group = int(netvlad_group); c.coalesce_depth = int(coalesce_depth)
        c.netvlad_inline = 2 if netvlad_inline is None else int(bool(netvlad_inline))      # None: auto (inline when lanes > 2)
        c.lr_lk = int(bool(lr_lk))
        c.sp_lk = int(bool(sp_lk))
        cam = _PipeCamera()
        self._lib.d2fe_pipe_camera_default(C.byref(cam))
        cam.mono, cam.depth = int(bool(mono)), int(bool(depth))
        self._mono, self._depth = bool(mono), bool(depth)
        self._depth_res = _PipeDepthResult()
        self._lr_lk = bool(lr_lk)
        self._sp_lk = bool(sp_lk)
        self._lk_res = _PipeLKResult()
        self._track_res = _PipeTrackResult()
        self._p = C.c_void_p()
        if mono or depth:
            _check(self._lib.d2fe_pipe_create_camera(fe.handle, C.byref(c), C.byref(cam), C.byref(self._p)))
        else:
            _check(self._lib.d2fe_pipe_create(fe.handle, C.byref(c), C.byref(self._p)))
        self._flow = False
        self._flow_res = _PipeFlowResult()
        self._bearings = False
        self._bear_res = _PipeBearingsResult()
        try:
            if track_params is not None:
                self.set_track_params(track_params)
            if flow_lk:
                if flow_lk not in (True, "only"):
                    raise ValueError('flow_lk is False, True (beside SuperPoint) or "only" (superpoint = 0)')
                self.flow_enable(flow_params, superpoint=0 if flow_lk == "only" else 1)
            if bearings is not None:
                self.bearings_enable(**bearings)
        except Exception:
            self.close()
            raise
        if not hasattr(fe, "_pipes"):
            import weakref
            fe._pipes = weakref.WeakSet()
        fe._pipes.add(self)
        self.lanes, self.frames, self.width, self.height = int(lanes), int(frames), int(width), int(height)
        self._pinned_input = bool(pinned_input)
        self._res = _PipeResult()

    def profile_enable(self, mode):
        _check(self._lib.d2fe_pipe_profile_enable(self._p, int(mode)))

    def profile_read(self):
        ms = (C.c_float * len(PROF_STAGES))(); n = (C.c_int32 * len(PROF_STAGES))()
        _check(self._lib.d2fe_pipe_profile_read(self._p, ms, n))
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(PROF_STAGES)}

    def submit_ptr(self, left_ptr, right_ptr, stride=None, image_stride=None):
        """raw host addresses (e.g. of pinned torch tensors)"""
        t = C.c_int64()
        _check(self._lib.d2fe_pipe_submit(self._p, C.c_void_p(left_ptr), C.c_void_p(right_ptr), int(stride or self.width),
                                          int(image_stride or self.width * self.height), C.byref(t)))
        return int(t.value)

    def submit_depth_ptr(self, gray_ptr, depth_ptr, stride=None, depth_stride=None, image_stride=None, depth_image_stride=None):
        """d2fe_pipe_submit_depth on raw host addresses; the depth strides are in bytes"""
        t = C.c_int64()
        ds = int(depth_stride or 2 * self.width)
        _check(self._lib.d2fe_pipe_submit_depth(self._p, C.c_void_p(gray_ptr), C.c_void_p(depth_ptr), int(stride or self.width), ds,
                                                int(image_stride or self.width * self.height), int(depth_image_stride or ds * self.height), C.byref(t)))
        return int(t.value)

    def submit(self, left, right=None, depth=None):
        """left, right: u8 [frames, H, W] (or [H, W] when frames == 1); a mono pipe takes right=None, a depth pipe depth = u16 [frames, H, W] (a view whose rows are
        further apart than the image is wide is passed on with its strides).  The library copies the frames into its own pinned staging before this returns
        (pinned_input = 0), so the arrays -- and any contiguous temporaries made here -- are not referenced afterwards.  A pipe created with
        pinned_input=True DMAs straight from the caller's memory until the ticket has been waited for: that contract (page-locked memory that
        stays alive and unchanged) cannot be kept for numpy arrays, so it is refused here -- use submit_ptr with memory you own."""
        if self._pinned_input:
            raise ValueError("StereoPipe(pinned_input=True): submit() takes numpy arrays, which are neither page-locked nor kept alive until wait(); "
                             "use submit_ptr() with page-locked memory that outlives the ticket")
        left = np.ascontiguousarray(left, np.uint8)
        if depth is not None:
            if right is not None:
                raise ValueError("submit(left, depth=...) belongs to a mono pipe: no right image")
            depth = np.asarray(depth)
            if depth.dtype != np.uint16:
                raise TypeError("depth frames are uint16")
            d3 = depth if depth.ndim == 3 else depth[None]
            if d3.strides[2] != 2 or d3.strides[1] < 2 * d3.shape[2] or (d3.shape[0] > 1 and d3.strides[0] < d3.strides[1] * d3.shape[1]):
                d3 = np.ascontiguousarray(d3)
            return self.submit_depth_ptr(left.ctypes.data, d3.ctypes.data, depth_stride=d3.strides[1], depth_image_stride=max(d3.strides[0], d3.strides[1] * d3.shape[1]))
        if right is not None:
            right = np.ascontiguousarray(right, np.uint8)
        return self.submit_ptr(left.ctypes.data, None if right is None else right.ctypes.data)

    def stream_placement(self):
        """(classes, n_classes) of d2fe_pipe_stream_placement: classes[k] = (hardware-pipe class of lane k's own stream, of its second stream)."""
        K = self.lanes
        arr = (C.c_int32 * (2 * K))(); n = C.c_int32(0)
        _check(self._lib.d2fe_pipe_stream_placement(self._p, arr, C.byref(n)))
        return [(arr[2 * k], arr[2 * k + 1]) for k in range(K)], n.value

    def classify_stream(self, stream):
        """d2fe_pipe_classify_stream: the class of the pipe's streams `stream` (a hipStream_t as int) takes turns with on the device, -1: none.  Idle pipe only."""
        c = C.c_int32(-1)
        _check(self._lib.d2fe_pipe_classify_stream(self._p, C.c_void_p(int(stream)), C.byref(c)))
        return int(c.value)

    def pick_consumer_stream(self, make, handle=lambda s: s, tries=4):
        """A stream for a device-side consumer of this pipe's results that disturbs the lanes least: `make()` creates candidate streams one at a time (`handle(stream)` = its
        hipStream_t as int) until one takes turns with none of the lanes' streams, or only with second (NetVLAD) streams; after `tries` candidates the best seen.  One at a
        time because every stream a process creates costs it a hardware queue for good."""
        placement, n = self.stream_placement()
        own = {a for a, _ in placement}
        best = None
        for _ in range(tries if n >= 2 else 1):
            st = make()
            if n < 2:
                return st
            c = self.classify_stream(handle(st))
            rank = 0 if c < 0 else 1 if c not in own else 2
            if best is None or rank < best[0]:
                best = (rank, st)
            if rank < 2:
                break
        return best[1]

    def device_view(self, ticket, stream):
        """DEVICE pointers into the ticket's result block for a consumer on `stream` (a raw hipStream_t, not 0): the stream is made to wait for the ticket's SuperPoint
        and NetVLAD results; release with device_release(ticket, stream) once the consumer's work is queued (include/d2fe.h, d2fe_pipe_device_view)."""
        r = _PipeDeviceResult()
        _check(self._lib.d2fe_pipe_device_view(self._p, C.c_int64(ticket), C.c_void_p(stream), C.byref(r)))
        return r

    def device_release(self, ticket, stream):
        _check(self._lib.d2fe_pipe_device_release(self._p, C.c_int64(ticket), C.c_void_p(stream)))

    def wait_raw(self, ticket):
        _check(self._lib.d2fe_pipe_wait(self._p, C.c_int64(ticket), C.byref(self._res)))
        return self._res

    def wait(self, ticket):
        """dict of numpy VIEWS into the pinned result block"""
        r = self.wait_raw(ticket)
        F, cap, D, G = r.frames, r.cap, r.desc_dim, r.netvlad_dim

        def view(ptr, shape, dt):
            if not ptr:
                return None
            n = int(np.prod(shape))
            buf = (C.c_float * n).from_address(ptr) if dt == np.float32 else (C.c_int32 * n).from_address(ptr)
            return np.frombuffer(buf, dtype=dt).reshape(shape)
        out = {"kps_xy": view(r.kps_xy, (2 * F, cap, 2), np.float32), "scores": view(r.scores, (2 * F, cap), np.float32),
               "desc": view(r.desc, (2 * F, cap, D), np.float32), "n_kp": view(r.n_kp, (2 * F,), np.int32),
               "netvlad": view(r.netvlad, (F, G), np.float32) if G else None}
        for k in ("lr", "prev"):
            out[k + "_q"] = view(getattr(r, k + "_q"), (F, cap), np.int32); out[k + "_t"] = view(getattr(r, k + "_t"), (F, cap), np.int32)
            out[k + "_dist"] = view(getattr(r, k + "_dist"), (F, cap), np.float32); out[k + "_n"] = view(getattr(r, k + "_n"), (F,), np.int32)
        if self._sp_lk:
            t = self.track_result_raw(ticket)
            T, lw, base = t.cap_tracks, t.list_words, t.n          # the header of frame 0's list is the lowest address of the lists
            words = np.frombuffer((C.c_int32 * (F * lw)).from_address(base), dtype=np.int32).reshape(F, lw)

            def per_list(ptr, shape, dt):
                o = (ptr - base) // 4
                return words[:, o:o + int(np.prod(shape))].view(dt).reshape((F,) + tuple(shape))
            for k in ("n", "n_tracked_in", "n_lost", "n_removed_near", "n_new"):
                out["track_" + k] = per_list(getattr(t, k), (1,), np.int32)[:, 0]
            out["track_pts"] = per_list(t.pts_xy, (T, 2), np.float32); out["track_desc"] = per_list(t.desc, (T, D), np.float32)
            out["track_scores"] = per_list(t.scores, (T,), np.float32)
            for k in ("id", "src", "kp"):
                out["track_" + k] = per_list(getattr(t, k), (T,), np.int32)
            out["track_right_pts"] = view(t.right_xy, (F, T, 2), np.float32)
            out["track_right_status"] = np.frombuffer((C.c_uint8 * (F * T)).from_address(t.right_status), dtype=np.uint8).reshape(F, T) if t.right_status else None
        elif self._lr_lk:
            lk = self.lk_result_raw(ticket)
            out["lk_pts"] = view(lk.pts_xy, (F, cap, 2), np.float32)
            out["lk_status"] = np.frombuffer((C.c_uint8 * (F * cap)).from_address(lk.status), dtype=np.uint8).reshape(F, cap)
        if self._flow:
            t = self.flow_result_raw(ticket)
            T, lw, base = t.cap_tracks, t.list_words, t.n          # the header of frame 0's list is the lowest address of the lists
            words = np.frombuffer((C.c_int32 * (F * lw)).from_address(base), dtype=np.int32).reshape(F, lw)
            flist = lambda ptr, shape, dt: words[:, (ptr - base) // 4:(ptr - base) // 4 + int(np.prod(shape))].view(dt).reshape((F,) + tuple(shape))
            for k in ("n", "n_tracked_in", "n_lost", "n_removed_near", "n_new", "lack", "num", "n_cand"):
                out["flow_" + k] = flist(getattr(t, k), (1,), np.int32)[:, 0]
            out["flow_pts"] = flist(t.pts_xy, (T, 2), np.float32); out["flow_id"] = flist(t.id, (T,), np.int32); out["flow_src"] = flist(t.src, (T,), np.int32)
            out["flow_right_pts"] = view(t.right_xy, (F, T, 2), np.float32)
            out["flow_right_status"] = np.frombuffer((C.c_uint8 * (F * T)).from_address(t.right_status), dtype=np.uint8).reshape(F, T) if t.right_status else None
            out["flow_depth_mm"] = np.frombuffer((C.c_uint16 * (F * T)).from_address(t.depth_mm), dtype=np.uint16).reshape(F, T) if t.depth_mm else None
        if self._depth:
            d = self.depth_result_raw(ticket)
            out["kp_depth_mm"] = np.frombuffer((C.c_uint16 * (F * cap)).from_address(d.kp_depth_mm), dtype=np.uint16).reshape(F, cap)
            T = d.cap_tracks
            out["track_depth_mm"] = np.frombuffer((C.c_uint16 * (F * T)).from_address(d.track_depth_mm), dtype=np.uint16).reshape(F, T) if d.track_depth_mm else None
        if self._bearings:
            b = self.bearings_result_raw(ticket)
            T = b.cap_tracks

            def raw(ptr, shape, ct, dt):
                return np.frombuffer((ct * int(np.prod(shape))).from_address(ptr), dtype=dt).reshape(shape) if ptr else None
            out["bearing_kp"] = raw(b.kp_bearing, (2 * F, cap, 3), C.c_double, np.float64)
            out["bearing_kp_pred"] = view(b.kp_pred_xy, (F, cap, 2), np.float32)
            out["bearing_lk_right"] = raw(b.lk_right_bearing, (F, cap, 3), C.c_double, np.float64)
            out["bearing_lk_pred_ok"] = raw(b.lk_pred_ok, (F, cap), C.c_uint8, np.uint8)
            out["bearing_list"] = raw(b.list_bearing, (F, T, 3), C.c_double, np.float64)
            out["bearing_list_pred"] = view(b.list_pred_xy, (F, T, 2), np.float32)
            out["bearing_list_right"] = raw(b.list_right_bearing, (F, T, 3), C.c_double, np.float64)
            out["bearing_list_pred_ok"] = raw(b.list_pred_ok, (F, T), C.c_uint8, np.uint8)
        return out

    def bearings_enable(self, cam_left, cam_right=None, T_right_left=None, distance=100.0, lk_use_pred=True, radius_lk=0.0):
        """d2fe_pipe_bearings_enable: once, before the first submit.  cam_left / cam_right: camera_pinhole() / camera_mei(); T_right_left: 12 doubles, [3][4] row-major
        (relative_extrinsic); radius_lk = search_local_max_dist_lr * width.  A mono pipe takes cam_left alone."""
        b = _PipeBearings()
        self._lib.d2fe_pipe_bearings_default(C.byref(b))
        b.cam[0] = cam_left
        b.cam[1] = cam_right if cam_right is not None else cam_left
        if T_right_left is not None:
            b.T_right_left = (C.c_double * 12)(*[float(v) for v in np.asarray(T_right_left, np.float64).reshape(-1)])
        b.distance, b.lk_use_pred, b.radius_lk = float(distance), int(bool(lk_use_pred)), float(radius_lk)
        _check(self._lib.d2fe_pipe_bearings_enable(self._p, C.byref(b)))
        self._bearings = True

    def bearings_result_raw(self, ticket):
        """d2fe_pipe_bearings_result_get: the bearings of a ticket that wait() has returned (D2FE_ERR_UNSUPPORTED without the mode)"""
        _check(self._lib.d2fe_pipe_bearings_result_get(self._p, C.c_int64(ticket), C.byref(self._bear_res)))
        return self._bear_res

    def depth_result_raw(self, ticket):
        """d2fe_pipe_depth_result_get: the depth values of a ticket that wait() has returned (depth pipes)"""
        _check(self._lib.d2fe_pipe_depth_result_get(self._p, C.c_int64(ticket), C.byref(self._depth_res)))
        return self._depth_res

    def lk_result_raw(self, ticket):
        """d2fe_pipe_lk_result_get: the left -> right LK tracks of a ticket that wait() has returned (lr_lk pipes)"""
        _check(self._lib.d2fe_pipe_lk_result_get(self._p, C.c_int64(ticket), C.byref(self._lk_res)))
        return self._lk_res


    def flow_enable(self, fp=None, superpoint=None):
        """d2fe_pipe_flow_enable: once, before the first submit (fp: a dict of flow_params() keywords, a _FlowParams, or None for the reference's defaults)"""
        fp = flow_params(**fp) if isinstance(fp, dict) else fp if fp is not None else flow_params()
        if superpoint is not None:
            fp.superpoint = int(superpoint)
        _check(self._lib.d2fe_pipe_flow_enable(self._p, C.byref(fp)))
        self._flow = True

    def flow_result_raw(self, ticket):
        """d2fe_pipe_flow_result_get: the flow lists of a ticket that wait() has returned (D2FE_ERR_UNSUPPORTED without the mode)"""
        _check(self._lib.d2fe_pipe_flow_result_get(self._p, C.c_int64(ticket), C.byref(self._flow_res)))
        return self._flow_res

    def track_result_raw(self, ticket):
        """d2fe_pipe_track_result_get: the landmark lists of a ticket that wait() has returned (sp_lk pipes)"""
        _check(self._lib.d2fe_pipe_track_result_get(self._p, C.c_int64(ticket), C.byref(self._track_res)))
        return self._track_res

    def set_track_params(self, tp):
        """d2fe_pipe_set_track_params: only before the first submit"""
        _check(self._lib.d2fe_pipe_set_track_params(self._p, C.byref(track_params(**tp) if isinstance(tp, dict) else tp)))


def depth_at_device(fe, d_depth, width, height, depth_stride, depth_image_stride, d_pts_xy, pts_stride, d_n, n_lists, cap, d_out, stream=None):
    """d2fe_depth_at_device on raw device addresses (ints): n_lists point lists [cap][2] float32 (pts_stride floats apart) against n_lists uint16 depth images (strides
    in bytes), counts d_n [n_lists] int32, values to d_out [n_lists][cap] uint16 -- depth[cvRound(y)][cvRound(x)], 0 outside the image, for NaN and for slots >= n.
    Asynchronous on `stream` (None: the handle's)."""
    _check(fe._lib.d2fe_depth_at_device(fe.handle, C.c_void_p(d_depth), int(width), int(height), int(depth_stride), int(depth_image_stride), C.c_void_p(d_pts_xy),
                                        int(pts_stride), C.c_void_p(d_n), int(n_lists), int(cap), C.c_void_p(d_out), C.c_void_p(stream or 0)))


CAM_PINHOLE, CAM_MEI, CAM_CYLINDRICAL = 0, 1, 3


def camera_pinhole(fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0):
    """d2fe_camera of camodocal's PinholeCamera (pinhole + radtan)"""
    return _Camera(CAM_PINHOLE, 0, (C.c_double * 9)(float(fx), float(fy), float(cx), float(cy), float(k1), float(k2), float(p1), float(p2), 0.0))


def camera_mei(cam):
    """d2fe_camera of camodocal's CataCamera; cam: dict(xi,k1,k2,p1,p2,gamma1,gamma2,u0,v0) or the nine values in that order"""
    return _Camera(CAM_MEI, 0, FrontEnd._mei(cam))


def camera_cylindrical(fx, fy, cx, cy):
    """d2fe_camera of camodocal's CylindricalCamera (the undistorted quadcam views)"""
    return _Camera(CAM_CYLINDRICAL, 0, (C.c_double * 9)(float(fx), float(fy), float(cx), float(cy), 0.0, 0.0, 0.0, 0.0, 0.0))


def cylinder_camera(width, height, fov_deg):
    """d2fe_cylinder_camera (host only): the virtual camera gen_cylinder_map assumes for a width x height view of fov_deg degrees"""
    c = _Camera()
    _check(load_library().d2fe_cylinder_camera(int(width), int(height), float(fov_deg), C.byref(c)))
    return c


def relative_extrinsic(q_a_wxyz, t_a, q_b_wxyz, t_b):
    """d2fe_relative_extrinsic (host only): T_b_a [3, 4] = [R_b^T R_a | R_b^T (t_a - t_b)] from two poses (unit quaternion w x y z, translation) in a common frame"""
    lib = load_library()
    a = [np.ascontiguousarray(v, np.float64).reshape(-1) for v in (q_a_wxyz, t_a, q_b_wxyz, t_b)]
    if [len(v) for v in a] != [4, 3, 4, 3]:
        raise ValueError("relative_extrinsic takes (q[4], t[3], q[4], t[3])")
    T = np.zeros(12, np.float64)
    _check(lib.d2fe_relative_extrinsic(_ptr(a[0]), _ptr(a[1]), _ptr(a[2]), _ptr(a[3]), _ptr(T)))
    return T.reshape(3, 4)


def bearings_device(fe, cam, d_pts_xy, pts_stride, d_n, n_lists, cap, d_bearing, cam_other=None, T=None, distance=100.0, d_pred_xy=None, d_other_xy=None,
                    d_other_status=None, radius=0.0, d_other_bearing=None, d_pred_ok=None, stream=None):
    """d2fe_bearings_device on raw device addresses (ints): n_lists point lists [cap][2] float32 (pts_stride floats apart), counts d_n [n_lists] int32 -> unit bearings
    d_bearing [n_lists][cap][3] float64.  T (12 host doubles) and d_pred_xy [n_lists][cap][2] float32: the extrinsic prediction.  The four gate arrays (d_other_xy
    [n_lists][cap][2], d_other_status [n_lists][cap] uint8 -> d_other_bearing [n_lists][cap][3] float64, d_pred_ok [n_lists][cap] uint8) are given together, with cam_other.
    Asynchronous on `stream` (None: the handle's)."""
    Tc = None if T is None else (C.c_double * 12)(*[float(v) for v in np.asarray(T, np.float64).reshape(-1)])
    _check(fe._lib.d2fe_bearings_device(fe.handle, C.byref(cam), None if cam_other is None else C.byref(cam_other), Tc, float(distance), C.c_void_p(d_pts_xy),
                                        int(pts_stride), C.c_void_p(d_n), int(n_lists), int(cap), C.c_void_p(d_bearing), C.c_void_p(d_pred_xy or 0),
                                        C.c_void_p(d_other_xy or 0), C.c_void_p(d_other_status or 0), float(radius), C.c_void_p(d_other_bearing or 0),
                                        C.c_void_p(d_pred_ok or 0), C.c_void_p(stream or 0)))


def _pinned_view(ptr, shape, dt):
    if not ptr:
        return None
    n = int(np.prod(shape))
    buf = (C.c_float * n).from_address(ptr) if dt == np.float32 else (C.c_int32 * n).from_address(ptr)
    return np.frombuffer(buf, dtype=dt).reshape(shape)


class QuadPipe(_Owned):
    """Quadcam frames in flight (include/d2fe.h, d2fe_quad_pipe_*): per submit `quads` quad frames of four raw fisheye frames -> ONE undistort launch ->
    SuperPoint and NetVLAD of every view -> the four neighbour pairs (0,1) (1,2) (2,3) (0,3) and the temporal pairs, with up to `lanes` submits in flight.
    maps: per camera (mapx, mapy, gain or None) as [height][width] float32 numpy arrays or device tensors (anything with .data_ptr()); the pipe copies them.
    submit() enqueues and returns a ticket; wait() returns views into the lane's pinned result block (copy what must outlive 2 * lanes submits).
    Temporal pairs: view c of quad frame q against view c of quad frame q - 1 (q = 0: the last quad frame of the previous submit).
    sp_lk=True (d2fe_quad_track_enable; track_params: a dict of d2fe_track_params fields, a _TrackParams or None for the reference's defaults): the LK-carried
    landmark lists of the four cameras, the neighbour LK tracks and the neighbour matches of the lists; wait() then carries the track_* keys.
    flow_lk=True (d2fe_quad_flow_enable; excludes sp_lk; flow_params: a dict of flow_params() keywords, a _FlowParams or None for the reference's defaults): the flow
    landmarks of the four cameras beside SuperPoint and their neighbour LK tracks; wait() then also returns per list (q, c) "flow_n", "flow_n_tracked_in",
    "flow_n_lost", "flow_n_removed_near", "flow_n_new", "flow_lack", "flow_num", "flow_n_cand" [quads, 4], "flow_pts" [quads, 4, cap_tracks, 2], "flow_id" /
    "flow_src" [quads, 4, cap_tracks], and "flow_nb_lk_xy" [quads, 4, cap_tracks, 2] / "flow_nb_lk_status" [quads, 4, cap_tracks] per neighbour pair.
    bearings=dict(cams=[4 cameras], T_nb=[4 x 12 doubles], distance=100.0, lk_use_pred=True, radius_lk=...) (d2fe_quad_bearings_enable; with or without a list mode):
    unit bearings, neighbour predictions and the lk_lk_use_pred gate on the device; wait() then also returns "bear_kp" [quads, 4, cap, 3] float64 and, with lists,
    "bear_list" [quads, 4, cap_tracks, 3] float64, "bear_nb_pred" [quads, 4, cap_tracks, 2], "bear_nb" [quads, 4, cap_tracks, 3] float64 and "bear_nb_pred_ok"
    [quads, 4, cap_tracks] uint8 per neighbour pair (None without lists)."""
    _HANDLE, _DESTROY = "_p", "d2fe_quad_pipe_destroy"

    def __init__(self, fe: FrontEnd, maps, lanes=4, quads=1, raw_width=1280, raw_height=800, width=800, height=400, cap=None, netvlad=True,
                 match_neighbour=True, match_prev=True, ratio=0.8, radius_neighbour=None, radius_prev=-1.0, undistort_fov=200.0, pinned_input=False,
                 sp_lk=False, track_params=None, flow_lk=False, flow_params=None, bearings=None):
        self._lib = fe._lib
        self._fe = fe           # the pipe borrows the handle's weights
        c = _QuadPipeConfig()
        self._lib.d2fe_quad_pipe_default_config(C.byref(c))
        c.lanes, c.quads, c.raw_width, c.raw_height, c.width, c.height = int(lanes), int(quads), int(raw_width), int(raw_height), int(width), int(height)
        c.cap = int(cap or fe.cfg.max_keypoints)
        c.netvlad, c.match_neighbour, c.match_prev, c.pinned_input = int(bool(netvlad)), int(bool(match_neighbour)), int(bool(match_prev)), int(bool(pinned_input))
        c.ratio = float(ratio)
        c.radius_neighbour = float(0.2 * width if radius_neighbour is None else radius_neighbour)      # search_local_max_dist_lr * width
        c.radius_prev, c.undistort_fov = float(radius_prev), float(undistort_fov)
        device = all(hasattr(m, "data_ptr") for mm in maps for m in mm if m is not None)
        keep = []

        def addr(a):
            if a is None:
                return None
            if device:
                return int(a.data_ptr())
            a = np.ascontiguousarray(a, np.float32)
            if a.size != width * height:
                raise ValueError("QuadPipe: every map must hold width * height floats")
            keep.append(a)
            return a.ctypes.data
        m = _quad_maps([tuple(addr(a) for a in mm) for mm in maps], device)
        self._p = C.c_void_p()
        _check(self._lib.d2fe_quad_pipe_create(fe.handle, C.byref(c), C.byref(m), C.byref(self._p)))
        if not hasattr(fe, "_pipes"):
            import weakref
            fe._pipes = weakref.WeakSet()
        fe._pipes.add(self)
        self.lanes, self.quads, self.raw_width, self.raw_height = int(lanes), int(quads), int(raw_width), int(raw_height)
        self._pinned_input = bool(pinned_input)
        self._res = _QuadPipeResult()
        self._track_res = _QuadTrackResult()
        self._flow_res = _QuadFlowResult()
        self._bear_res = _QuadBearingsResult()
        self._sp_lk = False
        self._flow = False
        self._bearings = False
        try:
            if sp_lk:
                self.track_enable(track_params)
            if flow_lk:
                self.flow_enable(flow_params)
            if bearings is not None:
                self.bearings_enable(**bearings)
        except Exception:
            self.close()
            raise

    def flow_enable(self, fp=None):
        """d2fe_quad_flow_enable: once, before the first submit (fp: a dict of flow_params() keywords, a _FlowParams, or None for the reference's defaults)"""
        fp = flow_params(**fp) if isinstance(fp, dict) else fp
        _check(self._lib.d2fe_quad_flow_enable(self._p, C.byref(fp) if fp is not None else None))
        self._flow = True

    def flow_result_raw(self, ticket):
        """d2fe_quad_flow_result_get: the flow lists of a ticket that wait() has returned (D2FE_ERR_UNSUPPORTED without the mode)"""
        _check(self._lib.d2fe_quad_flow_result_get(self._p, C.c_int64(ticket), C.byref(self._flow_res)))
        return self._flow_res

    def bearings_enable(self, cams, T_nb=None, distance=100.0, lk_use_pred=True, radius_lk=0.0):
        """d2fe_quad_bearings_enable: once, before the first submit, in any order with track_enable / flow_enable.  cams: four cameras (cylinder_camera() for the
        undistorted views); T_nb: [4][12] doubles, pair n of (0,1) (1,2) (2,3) (0,3) as [3][4] row-major (relative_extrinsic); radius_lk = search_local_max_dist_lr *
        width."""
        b = _QuadBearings()
        self._lib.d2fe_quad_bearings_default(C.byref(b))
        if len(cams) != 4:
            raise ValueError("QuadPipe.bearings_enable takes four cameras")
        for c in range(4):
            b.cam[c] = cams[c]
        if T_nb is not None:
            T = np.asarray(T_nb, np.float64).reshape(-1)
            if T.size != 48:
                raise ValueError("QuadPipe.bearings_enable: T_nb is [4][12] doubles")
            b.T_nb = (C.c_double * 48)(*[float(v) for v in T])
        b.distance, b.lk_use_pred, b.radius_lk = float(distance), int(bool(lk_use_pred)), float(radius_lk)
        _check(self._lib.d2fe_quad_bearings_enable(self._p, C.byref(b)))
        self._bearings = True

    def bearings_result_raw(self, ticket):
        """d2fe_quad_bearings_result_get: the bearings of a ticket that wait() has returned (D2FE_ERR_UNSUPPORTED without the mode)"""
        _check(self._lib.d2fe_quad_bearings_result_get(self._p, C.c_int64(ticket), C.byref(self._bear_res)))
        return self._bear_res

    def track_enable(self, tp=None):
        """d2fe_quad_track_enable: once, before the first submit (tp: dict of d2fe_track_params fields, a _TrackParams, or None for the defaults)"""
        tp = track_params(**tp) if isinstance(tp, dict) else tp
        _check(self._lib.d2fe_quad_track_enable(self._p, C.byref(tp) if tp is not None else None))
        self._sp_lk = True

    def track_result_raw(self, ticket):
        """d2fe_quad_track_result_get: the lists of a ticket that wait() has returned"""
        _check(self._lib.d2fe_quad_track_result_get(self._p, C.c_int64(ticket), C.byref(self._track_res)))
        return self._track_res

    def submit_ptr(self, raw_ptr, stride=None, camera_stride=None, quad_stride=None):
        """raw host address (e.g. of a pinned torch tensor); image (q, c) at raw_ptr + q * quad_stride + c * camera_stride"""
        t = C.c_int64()
        st = int(stride or self.raw_width)
        cs = int(camera_stride if camera_stride is not None else st * self.raw_height)
        qs = int(quad_stride if quad_stride is not None else 4 * cs)
        _check(self._lib.d2fe_quad_pipe_submit(self._p, C.c_void_p(raw_ptr), st, cs, qs, C.byref(t)))
        return int(t.value)

    def submit(self, raw):
        """raw: u8 [quads][4][raw_height][raw_width].  The library copies the frames into its pinned staging before this returns (pinned_input = 0);
        a pipe with pinned_input=True takes page-locked memory that outlives the ticket: use submit_ptr."""
        if self._pinned_input:
            raise ValueError("QuadPipe(pinned_input=True): submit() takes numpy arrays, which are neither page-locked nor kept alive until wait(); use submit_ptr()")
        raw = np.ascontiguousarray(raw, np.uint8)
        if raw.shape != (self.quads, 4, self.raw_height, self.raw_width):
            raise ValueError("QuadPipe.submit: expected [%d][4][%d][%d] u8, got %s" % (self.quads, self.raw_height, self.raw_width, raw.shape))
        return self.submit_ptr(raw.ctypes.data)

    def device_view(self, ticket, stream):
        """DEVICE pointers into the ticket's result block (quad-major rows q * 4 + c) for a consumer on `stream` (a raw hipStream_t, not 0): the stream is made to
        wait for the ticket's SuperPoint and NetVLAD results; release with device_release(ticket, stream) once the consumer's work is queued (d2fe_quad_device_view)."""
        r = _QuadDeviceResult()
        _check(self._lib.d2fe_quad_device_view(self._p, C.c_int64(ticket), C.c_void_p(stream), C.byref(r)))
        return r

    def device_release(self, ticket, stream):
        _check(self._lib.d2fe_quad_device_release(self._p, C.c_int64(ticket), C.c_void_p(stream)))

    def lane_stream(self, ticket):
        """the hipStream_t (int) of the lane that ran the ticket's submit"""
        st = C.c_void_p()
        _check(self._lib.d2fe_quad_lane_stream(self._p, C.c_int64(ticket), C.byref(st)))
        return st.value

    def wait_raw(self, ticket):
        _check(self._lib.d2fe_quad_pipe_wait(self._p, C.c_int64(ticket), C.byref(self._res)))
        return self._res

    def wait(self, ticket):
        """dict of numpy VIEWS into the pinned result block, quad-major: [quads][4 views]..."""
        r = self.wait_raw(ticket)
        Q, cap, D, G = r.quads, r.cap, r.desc_dim, r.netvlad_dim
        f, i = np.float32, np.int32
        out = {"kps_xy": _pinned_view(r.kps_xy, (Q, 4, cap, 2), f), "scores": _pinned_view(r.scores, (Q, 4, cap), f),
               "desc": _pinned_view(r.desc, (Q, 4, cap, D), f), "n_kp": _pinned_view(r.n_kp, (Q, 4), i),
               "netvlad": _pinned_view(r.netvlad, (Q, 4, G), f) if G else None}
        for k in ("nb", "prev"):
            out[k + "_q"] = _pinned_view(getattr(r, k + "_q"), (Q, 4, cap), i); out[k + "_t"] = _pinned_view(getattr(r, k + "_t"), (Q, 4, cap), i)
            out[k + "_dist"] = _pinned_view(getattr(r, k + "_dist"), (Q, 4, cap), f); out[k + "_n"] = _pinned_view(getattr(r, k + "_n"), (Q, 4), i)
        if self._sp_lk:
            t = self.track_result_raw(ticket)
            T, lw = t.cap_tracks, t.list_words

            def per_list(ptr, shape, dt):      # [quads][4] + shape views of a per-list array: list (q, c) is (q * 4 + c) * list_words words further on
                base = _pinned_view(ptr, ((Q * 4 - 1) * lw + int(np.prod(shape or (1,))),), dt)
                return np.lib.stride_tricks.as_strided(base, (Q, 4) + tuple(shape), (16 * lw, 4 * lw) + tuple(np.zeros(shape, dt).strides), writeable=False)
            for k in ("n", "n_tracked_in", "n_lost", "n_removed_near", "n_new"):
                out["track_" + k] = per_list(getattr(t, k), (), i)
            out["track_pts"] = per_list(t.pts_xy, (T, 2), f); out["track_scores"] = per_list(t.scores, (T,), f); out["track_desc"] = per_list(t.desc, (T, D), f)
            for k in ("id", "src", "kp"):
                out["track_" + k] = per_list(getattr(t, k), (T,), i)
            out["track_nb_lk_xy"] = _pinned_view(t.nb_lk_xy, (Q, 4, T, 2), f)
            out["track_nb_lk_status"] = np.frombuffer((C.c_uint8 * (Q * 4 * T)).from_address(t.nb_lk_status), dtype=np.uint8).reshape(Q, 4, T)
            for k in ("q", "t"):
                out["track_lnb_" + k] = _pinned_view(getattr(t, "lnb_" + k), (Q, 4, T), i)
            out["track_lnb_dist"] = _pinned_view(t.lnb_dist, (Q, 4, T), f); out["track_lnb_n"] = _pinned_view(t.lnb_n, (Q, 4), i)
        if self._flow:
            t = self.flow_result_raw(ticket)
            T, lw = t.cap_tracks, t.list_words

            def flist(ptr, shape, dt):         # as per_list above, over the flow-list blocks
                base = _pinned_view(ptr, ((Q * 4 - 1) * lw + int(np.prod(shape or (1,))),), dt)
                return np.lib.stride_tricks.as_strided(base, (Q, 4) + tuple(shape), (16 * lw, 4 * lw) + tuple(np.zeros(shape, dt).strides), writeable=False)
            for k in ("n", "n_tracked_in", "n_lost", "n_removed_near", "n_new", "lack", "num", "n_cand"):
                out["flow_" + k] = flist(getattr(t, k), (), i)
            out["flow_pts"] = flist(t.pts_xy, (T, 2), f); out["flow_id"] = flist(t.id, (T,), i); out["flow_src"] = flist(t.src, (T,), i)
            out["flow_nb_lk_xy"] = _pinned_view(t.nb_lk_xy, (Q, 4, T, 2), f)
            out["flow_nb_lk_status"] = np.frombuffer((C.c_uint8 * (Q * 4 * T)).from_address(t.nb_lk_status), dtype=np.uint8).reshape(Q, 4, T)
        if self._bearings:
            b = self.bearings_result_raw(ticket)
            T = b.cap_tracks

            def raw(ptr, shape, ct, dt):
                return np.frombuffer((ct * int(np.prod(shape))).from_address(ptr), dtype=dt).reshape(shape) if ptr else None
            out["bear_kp"] = raw(b.kp_bearing, (Q, 4, cap, 3), C.c_double, np.float64)
            out["bear_list"] = raw(b.list_bearing, (Q, 4, T, 3), C.c_double, np.float64)
            out["bear_nb_pred"] = _pinned_view(b.nb_pred_xy, (Q, 4, T, 2), f)
            out["bear_nb"] = raw(b.nb_bearing, (Q, 4, T, 3), C.c_double, np.float64)
            out["bear_nb_pred_ok"] = raw(b.nb_pred_ok, (Q, 4, T), C.c_uint8, np.uint8)
        return out


def block_words(cap, netvlad_dim, desc_dim=256):
    """Float words of one exchange block (include/d2fe.h, d2fe_block_words_d); callable without a GPU."""
    return int(load_library().d2fe_block_words_d(int(cap), int(desc_dim), int(netvlad_dim)))


def block_bytes_int8(cap, netvlad_dim, desc_dim=256):
    """Bytes of one int8 exchange block (include/d2fe.h, d2fe_block_bytes_int8_d)."""
    return int(load_library().d2fe_block_bytes_int8_d(int(cap), int(desc_dim), int(netvlad_dim)))


def block_field_offset(cap, netvlad_dim, field, desc_dim=256):
    """Word offset of a block field: 'desc', 'kps', 'scores', 'netvlad', 'n'."""
    return int(load_library().d2fe_block_field_offset_d(int(cap), int(desc_dim), int(netvlad_dim), ["desc", "kps", "scores", "netvlad", "n"].index(field)))


class FlatIPDatabase(_Owned):
    """faiss::IndexFlatIP stand-in for the NetVLAD keyframe database (loop_detector.h:71-72, loop_detector.cpp:254-263,300-350)."""
    _HANDLE, _DESTROY = "_db", "d2fe_db_destroy"

    def __init__(self, fe: FrontEnd, dim: int, capacity: int = 65536):
        self._lib = fe._lib
        self._db = C.c_void_p()
        self._fe = fe
        _check(self._lib.d2fe_db_create(fe.handle, dim, capacity, C.byref(self._db)))
        self.dim = dim

    @property
    def ntotal(self):
        return int(self._lib.d2fe_db_ntotal(self._db))

    def add(self, vecs):
        v = np.ascontiguousarray(vecs, np.float32).reshape(-1, self.dim)
        r = int(self._lib.d2fe_db_add(self._db, _ptr(v), v.shape[0]))
        if r < 0:
            _check(r)
        return r

    def search(self, q, k):
        q = np.ascontiguousarray(q, np.float32).reshape(-1, self.dim)
        sims = np.zeros((q.shape[0], k), np.float32); labels = np.zeros((q.shape[0], k), np.int32)
        _check(self._lib.d2fe_db_search(self._db, _ptr(q), q.shape[0], k, _ptr(sims), _ptr(labels)))
        return sims, labels

    def query_gated(self, q, max_index, thres):
        """LoopDetector::queryIndexFromDatabase (loop_detector.cpp:300-350) -> (label or -1, similarity)."""
        q = np.ascontiguousarray(q, np.float32).reshape(self.dim)
        label = C.c_int32(-1); sim = C.c_float(0)
        _check(self._lib.d2fe_db_query_gated(self._db, _ptr(q), int(max_index), float(thres), C.byref(label), C.byref(sim)))
        return int(label.value), float(sim.value)


# ---- LK optical-flow tracker (d2frontend/src/opticaltrack_utils.cpp) ---------------------------------
PYR_LEVEL = 2            # opticaltrack_utils.h:10
WIN_SIZE = 21            # opticaltrack_utils.cpp:25
LK_ITERS = 30            # SparsePyrLKOpticalFlow::create(WIN_SIZE, PYR_LEVEL, 30, true), :239
WHOLE_IMG_MATCH, LEFT_RIGHT_IMG_MATCH, RIGHT_LEFT_IMG_MATCH = 0, 1, 2   # TrackLRType


class LKFrame(_Owned):
    """Device-resident image pyramid = LKImageInfoGPU::pyr (opticaltrack_utils.h:16-23), built by buildImagePyramid
    (opticaltrack_utils.cpp:526-542)."""
    _HANDLE, _DESTROY = "_f", "d2fe_lk_frame_destroy"

    def __init__(self, fe: FrontEnd, gray=None, levels=PYR_LEVEL, d_gray=None, width=None, height=None, stride=None, stream=None):
        self._lib = fe._lib
        self._fe = fe
        self._f = C.c_void_p()
        self.levels = levels
        if gray is not None:
            img = np.ascontiguousarray(gray, np.uint8)
            self.height, self.width = img.shape
            _check(self._lib.d2fe_lk_frame_create(fe.handle, _ptr(img), self.width, self.height, self.width, levels, C.byref(self._f)))
        else:
            self.width, self.height = int(width), int(height)
            _check(self._lib.d2fe_lk_frame_create_device(fe.handle, C.c_void_p(d_gray), self.width, self.height,
                                                         int(stride or width), levels, C.c_void_p(stream or 0), C.byref(self._f)))

    def level(self, l):
        w, h = self.width, self.height
        for _ in range(l):
            w, h = (w + 1) // 2, (h + 1) // 2
        out = np.zeros((h, w), np.uint8)
        r = self._lib.d2fe_lk_frame_read_level(self._f, int(l), _ptr(out), out.nbytes, None, None)
        if r < 0:
            _check(int(r))
        return out


def buildImagePyramid(fe: FrontEnd, gray, maxLevel=PYR_LEVEL) -> LKFrame:
    """buildImagePyramid(GpuMat, maxLevel) (opticaltrack_utils.cpp:526-542)."""
    return LKFrame(fe, gray, maxLevel)


def lk_track(fe: FrontEnd, prev: LKFrame, cur: LKFrame, prev_pts, cur_init, track_type=WHOLE_IMG_MATCH, move_cols=0.0,
             win=WIN_SIZE, iters=LK_ITERS):
    """Forward + reverse SparsePyrLK with the 0.5 px and inBorder tests (opticaltrack_utils.cpp:236-272) -> (cur_pts, status)."""
    pp = np.ascontiguousarray(prev_pts, np.float32).reshape(-1, 2)
    ci = np.ascontiguousarray(cur_init, np.float32).reshape(-1, 2)
    n = pp.shape[0]
    out = np.zeros((max(n, 1), 2), np.float32); st = np.zeros(max(n, 1), np.uint8)
    _check(fe._lib.d2fe_lk_track(fe.handle, prev._f, cur._f, _ptr(pp), _ptr(ci), n, int(track_type), float(move_cols), int(win),
                                 int(iters), _ptr(out), _ptr(st)))
    return out[:n], st[:n]


def lk_stereo_workspace_bytes(n_frames, width, height, levels=PYR_LEVEL):
    """d2fe_lk_stereo_workspace_bytes (host arithmetic): the pyramids of n_frames left and n_frames right frames"""
    return int(load_library().d2fe_lk_stereo_workspace_bytes(int(n_frames), int(width), int(height), int(levels)))


def lk_track_stereo_device(fe: FrontEnd, d_left, d_right, n_frames, width, height, d_kps_xy, d_n_kp, cap, d_workspace, d_pts_xy, d_status,
                           stream=None, stride=None, image_stride=None, levels=PYR_LEVEL, win=WIN_SIZE, iters=LK_ITERS):
    """Device-resident stereo tracks (d2fe_lk_track_stereo_device); arguments are raw device addresses (ints), as for FrontEnd.extract_device: the keypoints
    [n_frames, cap, 2] and counts [n_frames] are the ones extract_device left; only enqueues on `stream`."""
    _check(fe._lib.d2fe_lk_track_stereo_device(fe.handle, d_left, d_right, int(n_frames), int(width), int(height), int(stride or width),
                                               int(image_stride or (stride or width) * height), d_kps_xy, d_n_kp, int(cap), int(levels), int(win), int(iters),
                                               d_workspace, d_pts_xy, d_status, stream))


LKC_FIELDS = ["hdr", "pts", "id", "src", "kp", "scores", "desc", "trk_xy", "trk_status"]      # enum D2FE_LKC_* of include/d2fe.h, in order


def track_params(**kw):
    """d2fe_track_params with the reference's defaults (d2fe_track_default_params), fields replaced by keyword"""
    tp = _TrackParams()
    load_library().d2fe_track_default_params(C.byref(tp))
    for k, v in kw.items():
        if k not in dict(_TrackParams._fields_) or k == "reserved":
            raise TypeError("d2fe_track_params has no field %r" % k)
        setattr(tp, k, v)
    return tp


def lk_carry_list_bytes(cap_tracks, desc_dim=256):
    """d2fe_lk_carry_list_bytes (host arithmetic): one landmark-list block"""
    return int(load_library().d2fe_lk_carry_list_bytes(int(cap_tracks), int(desc_dim)))


def lk_carry_list_offset(cap_tracks, desc_dim, field):
    """d2fe_lk_carry_list_offset: 32-bit words from the block base to `field` (a name of LKC_FIELDS or its index)"""
    return int(load_library().d2fe_lk_carry_list_offset(int(cap_tracks), int(desc_dim), LKC_FIELDS.index(field) if isinstance(field, str) else int(field)))


def lk_carry_list_views(block, cap_tracks, desc_dim=256):
    """dict of numpy views into a HOST copy of one list block (a 4-byte-aligned uint8 / int32 / float32 array of lk_carry_list_bytes bytes)"""
    w = np.ascontiguousarray(block).view(np.int32).reshape(-1)
    T, D = int(cap_tracks), int(desc_dim)
    shapes = {"hdr": ((64,), np.int32), "pts": ((T, 2), np.float32), "id": ((T,), np.int32), "src": ((T,), np.int32), "kp": ((T,), np.int32),
              "scores": ((T,), np.float32), "desc": ((T, D), np.float32), "trk_xy": ((T, 2), np.float32)}
    out = {}
    for k, (shape, dt) in shapes.items():
        o = lk_carry_list_offset(T, D, k)
        out[k] = w[o:o + int(np.prod(shape))].view(dt).reshape(shape)
    o = lk_carry_list_offset(T, D, "trk_status")
    out["trk_status"] = w[o:o + (T + 3) // 4].view(np.uint8)[:T]
    out.update(n=int(out["hdr"][0]), n_tracked_in=int(out["hdr"][1]), n_lost=int(out["hdr"][2]), n_removed_near=int(out["hdr"][3]), n_new=int(out["hdr"][4]))
    return out


def lk_carry_step(fe: FrontEnd, d_prev_pyr, d_cur_pyr, width, height, d_prev_list, d_cur_list, d_kps_xy, d_kp_scores, d_kp_desc, d_n_kp, kp_cap, d_next_id,
                  tp=None, desc_dim=256, stream=None):
    """One frame of the LK-carried landmark list on the device (d2fe_lk_carry_step_device); arguments are raw device addresses (ints), as for
    lk_track_stereo_device: the pyramids (one image of the stereo workspace, or an LKFrame's), the previous and the current list block (zeroed once), the outputs
    extract_device left for the current frame, one int32 next_id.  Only enqueues on `stream`."""
    tp = tp if tp is not None else track_params()
    _check(fe._lib.d2fe_lk_carry_step_device(fe.handle, d_prev_pyr, d_cur_pyr, int(width), int(height), d_prev_list, d_cur_list, int(desc_dim), d_kps_xy or None,
                                             d_kp_scores or None, d_kp_desc or None, d_n_kp or None, int(kp_cap), C.byref(tp), d_next_id, stream))


def lk_carry_quad_step(fe: FrontEnd, d_prev_pyr, d_cur_pyr, pyr_stride, width, height, d_prev_lists, d_cur_lists, list_stride, d_kps_xy, d_kp_scores, d_kp_desc,
                       d_n_kp, kp_cap, d_next_id, tp=None, desc_dim=256, stream=None):
    """The four cameras' lists of one quad frame in ONE launch (d2fe_lk_carry_quad_step_device): camera c's lists / pyramids are c * list_stride words /
    c * pyr_stride bytes behind the bases, its keypoints row c of the dense [4][kp_cap] extract outputs.  The bits of four lk_carry_step calls in camera order."""
    tp = tp if tp is not None else track_params()
    _check(fe._lib.d2fe_lk_carry_quad_step_device(fe.handle, d_prev_pyr, d_cur_pyr, int(pyr_stride), int(width), int(height), d_prev_lists, d_cur_lists, int(list_stride),
                                                  int(desc_dim), d_kps_xy or None, d_kp_scores or None, d_kp_desc or None, d_n_kp or None, int(kp_cap), C.byref(tp),
                                                  d_next_id, stream))


def lk_carry_neighbour(fe: FrontEnd, d_pyr, pyr_stride, quads, width, height, undistort_fov, d_lists, list_stride, d_nb_xy, d_nb_status, tp=None, desc_dim=256,
                       stream=None):
    """trackLK(left, right, type) of the four neighbour pairs of `quads` quad frames over device-resident lists, ONE launch (d2fe_lk_carry_neighbour_device):
    d_nb_xy [quads][4][cap_tracks][2] float32, d_nb_status [quads][4][cap_tracks] uint8, written for every slot."""
    tp = tp if tp is not None else track_params()
    _check(fe._lib.d2fe_lk_carry_neighbour_device(fe.handle, d_pyr, int(pyr_stride), int(quads), int(width), int(height), float(undistort_fov), d_lists,
                                                  int(list_stride), int(desc_dim), C.byref(tp), d_nb_xy, d_nb_status, stream))


# ---- the flow landmarks (enable_lk_optical_flow without sp_track_use_lk): the FAST-replenished LK list on the device ----
FLOW_FIELDS = ["hdr", "pts", "id", "src", "trk_xy", "trk_status"]      # the fields of LKC_FIELDS a flow list has


def flow_params(**kw):
    """d2fe_flow_params with the reference's defaults (d2fe_flow_default_params); keywords replace its own fields (superpoint, fast_cols, fast_rows,
    fast_threshold) or those of its d2fe_track_params (total_feature_num, levels, win, iters, near_lk_thread_rate, feature_min_dist)"""
    fp = _FlowParams()
    load_library().d2fe_flow_default_params(C.byref(fp))
    for k, v in kw.items():
        if k in ("superpoint", "fast_cols", "fast_rows", "fast_threshold"):
            setattr(fp, k, int(v))
        elif k in dict(_TrackParams._fields_) and k != "reserved":
            setattr(fp.track, k, v)
        else:
            raise TypeError("d2fe_flow_params has no field %r" % k)
    return fp


def lk_flow_cap_tracks(fp):
    """the capacity of the list d2fe_lk_flow_step_device keeps for these parameters: max(total_feature_num, 1)"""
    return max(int(fp.track.total_feature_num), 1)


def lk_flow_list_bytes(cap_tracks):
    """d2fe_lk_flow_list_bytes (host arithmetic): one flow-list block"""
    return int(load_library().d2fe_lk_flow_list_bytes(int(cap_tracks)))


def lk_flow_list_offset(cap_tracks, field):
    """d2fe_lk_flow_list_offset: 32-bit words from the block base to `field` (a name of LKC_FIELDS or its index); -1 for a field a flow list lacks"""
    return int(load_library().d2fe_lk_flow_list_offset(int(cap_tracks), LKC_FIELDS.index(field) if isinstance(field, str) else int(field)))


def lk_flow_scratch_bytes(width, height, cap_tracks, cols=3, rows=4):
    """d2fe_lk_flow_scratch_bytes (host arithmetic): score map + candidate pool of the device detector"""
    return int(load_library().d2fe_lk_flow_scratch_bytes(int(width), int(height), int(cap_tracks), int(cols), int(rows)))


def lk_flow_list_views(block, cap_tracks):
    """dict of numpy views into a HOST copy of one flow-list block (lk_flow_list_bytes bytes), and the header's counts by name"""
    w = np.ascontiguousarray(block).view(np.int32).reshape(-1)
    T = int(cap_tracks)
    shapes = {"hdr": ((64,), np.int32), "pts": ((T, 2), np.float32), "id": ((T,), np.int32), "src": ((T,), np.int32), "trk_xy": ((T, 2), np.float32)}
    out = {}
    for k, (shape, dt) in shapes.items():
        o = lk_flow_list_offset(T, k)
        out[k] = w[o:o + int(np.prod(shape))].view(dt).reshape(shape)
    o = lk_flow_list_offset(T, "trk_status")
    out["trk_status"] = w[o:o + (T + 3) // 4].view(np.uint8)[:T]
    h = out["hdr"]
    out.update(n=int(h[0]), n_tracked_in=int(h[1]), n_lost=int(h[2]), n_removed_near=int(h[3]), n_new=int(h[4]), next_id=int(h[6]), lack=int(h[7]), num=int(h[8]),
               n_cand=int(h[9]))
    return out


def detect_fast_device(fe: FrontEnd, d_pyr, width, height, d_features, cap_tracks, d_xy, d_response, cap, d_n, d_scratch, cols=3, rows=4, threshold=10, stream=None):
    """detectFastByRegion without the host (d2fe_detect_fast_device); arguments are raw device addresses (ints): level 0 of a pyramid, ONE int32 `features`,
    the outputs xy [cap, 2] float32, response [cap] int32 (or None), n [1] int32, and lk_flow_scratch_bytes of 16-byte aligned scratch.  Only enqueues on `stream`."""
    _check(fe._lib.d2fe_detect_fast_device(fe.handle, d_pyr, int(width), int(height), d_features, int(cap_tracks), int(cols), int(rows), int(threshold), d_xy,
                                           d_response or None, int(cap), d_n, d_scratch, stream))


def lk_flow_step_device(fe: FrontEnd, d_prev_pyr, d_cur_pyr, width, height, d_prev_list, d_cur_list, d_kps_xy, d_n_kp, kp_cap, d_next_id, d_scratch, fp=None,
                        stream=None):
    """One frame of the flow landmarks on the device (d2fe_lk_flow_step_device); arguments are raw device addresses (ints), as for lk_carry_step: the pyramids, the
    previous and the current flow-list block (zeroed once), the keypoints extract_device left for the current frame (or None / kp_cap = 0), one int32 next_id,
    the detector's scratch.  Five launches, only enqueued on `stream`."""
    fp = fp if fp is not None else flow_params()
    _check(fe._lib.d2fe_lk_flow_step_device(fe.handle, d_prev_pyr, d_cur_pyr, int(width), int(height), d_prev_list, d_cur_list, d_kps_xy or None, d_n_kp or None,
                                            int(kp_cap), C.byref(fp), d_next_id, d_scratch, stream))


def lk_flow_quad_step_device(fe: FrontEnd, d_prev_pyr, d_cur_pyr, pyr_stride, width, height, d_prev_lists, d_cur_lists, list_stride, d_kps_xy, d_n_kp, kp_cap,
                             d_next_id, d_scratch, scratch_stride, fp=None, stream=None):
    """The four cameras' flow lists of one quad frame in FIVE launches (d2fe_lk_flow_quad_step_device): camera c's lists / pyramids / detector scratch are
    c * list_stride words / c * pyr_stride bytes / c * scratch_stride bytes behind the bases, its keypoints row c of the dense [4][kp_cap] extract outputs.  The bytes
    of four lk_flow_step_device calls in camera order."""
    fp = fp if fp is not None else flow_params()
    _check(fe._lib.d2fe_lk_flow_quad_step_device(fe.handle, d_prev_pyr, d_cur_pyr, int(pyr_stride), int(width), int(height), d_prev_lists, d_cur_lists, int(list_stride),
                                                 d_kps_xy or None, d_n_kp or None, int(kp_cap), C.byref(fp), d_next_id, d_scratch, int(scratch_stride), stream))


def lk_flow_neighbour_device(fe: FrontEnd, d_pyr, pyr_stride, quads, width, height, undistort_fov, d_lists, list_stride, d_nb_xy, d_nb_status, tp=None, stream=None):
    """trackLK(left, right, type) of the four neighbour pairs of `quads` quad frames over device-resident FLOW lists, ONE launch (d2fe_lk_flow_neighbour_device):
    d_nb_xy [quads][4][cap_tracks][2] float32, d_nb_status [quads][4][cap_tracks] uint8 with cap_tracks = max(total_feature_num, 1), written for every slot."""
    tp = tp if tp is not None else track_params()
    _check(fe._lib.d2fe_lk_flow_neighbour_device(fe.handle, d_pyr, int(pyr_stride), int(quads), int(width), int(height), float(undistort_fov), d_lists,
                                                 int(list_stride), C.byref(tp), d_nb_xy, d_nb_status, stream))


class _LKPair(C.Structure):
    _fields_ = [("prev", C.c_void_p), ("cur", C.c_void_p), ("first", C.c_int32), ("count", C.c_int32), ("type", C.c_int32),
                ("move_cols", C.c_float)]


def lk_track_batch(fe: FrontEnd, jobs, win=WIN_SIZE, iters=LK_ITERS):
    """jobs: list of (prev LKFrame, cur LKFrame, prev_pts, cur_init, track_type, move_cols) -> list of (cur_pts, status);
    all tracks run in one kernel launch (d2fe_lk_track_batch)."""
    pairs = (_LKPair * max(len(jobs), 1))()
    pp, ci, first = [], [], 0
    for k, (prev, cur, p, c, t, mv) in enumerate(jobs):
        p = np.ascontiguousarray(p, np.float32).reshape(-1, 2); c = np.ascontiguousarray(c, np.float32).reshape(-1, 2)
        pairs[k] = _LKPair(prev._f, cur._f, first, len(p), int(t), float(mv))
        pp.append(p); ci.append(c); first += len(p)
    n = first
    allp = np.concatenate(pp) if n else np.zeros((0, 2), np.float32)
    alli = np.concatenate(ci) if n else np.zeros((0, 2), np.float32)
    out = np.zeros((max(n, 1), 2), np.float32); st = np.zeros(max(n, 1), np.uint8)
    _check(fe._lib.d2fe_lk_track_batch(fe.handle, pairs, len(jobs), _ptr(np.ascontiguousarray(allp)), _ptr(np.ascontiguousarray(alli)),
                                       n, int(win), int(iters), _ptr(out), _ptr(st)))
    res = []
    for k in range(len(jobs)):
        a, cnt = pairs[k].first, pairs[k].count
        res.append((out[a:a + cnt].copy(), st[a:a + cnt].copy()))
    return res


def opticalflowTrackPyr(fe: FrontEnd, cur_img, prev_lk: dict, track_type=WHOLE_IMG_MATCH, undistort_fov=200.0):
    """opticalflowTrackPyr(cur_img, prev_lk, type) (opticaltrack_utils.cpp:173-279).  prev_lk / the return value are dicts with
    the LKImageInfoGPU fields: lk_pts [n,2], lk_ids, lk_local_index, lk_types, pyr (LKFrame)."""
    cur_img = np.ascontiguousarray(cur_img, np.uint8)
    cur_pyr = buildImagePyramid(fe, cur_img, PYR_LEVEL)
    prev_pts = np.asarray(prev_lk.get("lk_pts", np.zeros((0, 2))), np.float32).reshape(-1, 2)
    ids = np.asarray(prev_lk.get("lk_ids", np.arange(len(prev_pts))))
    types = np.asarray(prev_lk.get("lk_types", np.zeros(len(prev_pts), np.int32)))
    local = np.asarray(prev_lk.get("lk_local_index", np.arange(len(prev_pts))))
    empty = {"lk_pts": np.zeros((0, 2), np.float32), "lk_ids": ids[:0], "lk_local_index": local[:0], "lk_types": types[:0], "pyr": cur_pyr}
    if len(prev_pts) == 0:
        return empty
    move_cols = np.float32(cur_img.shape[1] * 90.0 / undistort_fov)
    if track_type == WHOLE_IMG_MATCH:
        cur_pts = prev_pts.copy()
    else:
        if track_type == LEFT_RIGHT_IMG_MATCH:
            keep = prev_pts[:, 0] < np.float32(cur_img.shape[1]) - move_cols
            cur_pts = prev_pts[keep].copy(); cur_pts[:, 0] += move_cols
        else:
            keep = prev_pts[:, 0] >= move_cols
            cur_pts = prev_pts[keep].copy(); cur_pts[:, 0] -= move_cols
        prev_pts, ids, types, local = prev_pts[keep], ids[keep], types[keep], local[keep]
    if len(cur_pts) == 0:
        return empty
    out, st = lk_track(fe, prev_lk["pyr"], cur_pyr, prev_pts, cur_pts, track_type, float(move_cols))
    k = st.astype(bool)
    return {"lk_pts": out[k], "lk_ids": ids[k], "lk_local_index": local[k], "lk_types": types[k], "pyr": cur_pyr}


def detectFastByRegion(fe: FrontEnd, frame: LKFrame, features, cols, rows, threshold=10, with_response=False):
    """detectFastByRegion(img, mask, features, cols, rows) (opticaltrack_utils.cpp:444-493)."""
    cap = max(int(features), 1)
    xy = np.zeros((cap, 2), np.float32); resp = np.zeros(cap, np.int32); n = C.c_int(0)
    _check(fe._lib.d2fe_detect_fast_by_region(fe.handle, frame._f, int(features), int(cols), int(rows), int(threshold), _ptr(xy),
                                              _ptr(resp), cap, C.byref(n)))
    return (xy[:n.value].copy(), resp[:n.value].copy()) if with_response else xy[:n.value].copy()


def goodFeaturesToTrack(fe: FrontEnd, frame: LKFrame, max_corners, quality=0.01, min_dist=20.0):
    """cv::cuda::createGoodFeaturesToTrackDetector(type, max_corners, quality, min_dist)->detect (opticaltrack_utils.cpp:404-412)."""
    cap = max(int(max_corners), 1) if max_corners > 0 else frame.width * frame.height // 4
    xy = np.zeros((cap, 2), np.float32); n = C.c_int(0)
    _check(fe._lib.d2fe_good_features_to_track(fe.handle, frame._f, int(max_corners), float(quality), float(min_dist), _ptr(xy), cap,
                                               C.byref(n)))
    return xy[:n.value].copy()


def detectPoints(fe: FrontEnd, frame: LKFrame, cur_pts, require_pts, use_fast=False, fast_rows=3, fast_cols=4,
                 feature_min_dist=20.0):
    """detectPoints (opticaltrack_utils.cpp:375-442): detect only when more than a quarter of the points are missing, ask for
    twice the shortfall when some points exist, drop candidates closer than feature_min_dist to an accepted point."""
    cur_pts = np.asarray(cur_pts, np.float32).reshape(-1, 2)
    lack = int(require_pts) - len(cur_pts)
    if not lack > int(require_pts) // 4:
        return np.zeros((0, 2), np.float32)
    num = lack * 2 if len(cur_pts) > 0 else lack
    if use_fast:
        cand = detectFastByRegion(fe, frame, num, fast_rows, fast_cols)   # (sic) the reference passes rows as `cols`, :391-392
    else:
        cand = goodFeaturesToTrack(fe, frame, num, 0.01, feature_min_dist)
    all_pts = [p for p in cur_pts]
    out = []
    for p in cand:
        near = False
        for q in all_pts:
            d = p - q
            if np.sqrt(np.float64(d[0]) * d[0] + np.float64(d[1]) * d[1]) < feature_min_dist:
                near = True
                break
        if not near:
            out.append(p); all_pts.append(p)
        if len(out) >= lack:
            break
    return np.asarray(out, np.float32).reshape(-1, 2)


class SuperPoint:
    """Mirror of class SuperPoint (superpoint_tensorrt.h:36-93): build() then infer()."""

    def __init__(self, super_point_config: SuperPointConfig, weights=None):
        self.super_point_config_ = super_point_config
        self._weights = weights
        self._fe: Optional[FrontEnd] = None

    def build(self) -> bool:
        """SuperPoint::build (superpoint_tensorrt.cpp:22-107): returns False instead of raising, like the reference."""
        try:
            self._fe = FrontEnd(self.super_point_config_)
            if self._weights is None:
                raise D2FEError(-3, "no weights given (the reference would fail to parse onnx_path)")
            self._fe.load_superpoint(self._weights)
            return True
        except D2FEError as e:
            self.last_error = str(e)
            self._fe = None
            return False

    def infer(self, image):
        """bool SuperPoint::infer(const cv::Mat&, vector<Point2f>& keypoints, vector<float>& descriptors,
        vector<float>& scores) (superpoint_tensorrt.cpp:161-183).  Returns (ok, keypoints [k,2], descriptors
        flat [k*256], scores [k]); on failure all three are empty, as the reference clears them."""
        empty = (False, np.zeros((0, 2), np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32))
        if self._fe is None:
            return empty
        try:
            (kps, sc, desc), = self._fe.extract_batch(np.asarray(image)[None])
            return True, kps, desc.reshape(-1), sc
        except D2FEError as e:
            self.last_error = str(e)
            return empty

    @property
    def frontend(self):
        return self._fe


def matchKNN(fe: FrontEnd, desc_a, desc_b, knn_match_ratio=0.8, pts_a=None, pts_b=None, search_local_dist=-1.0):
    """D2FrontEnd::matchKNN (feature_matcher.cpp:4-42) -> list of (queryIdx, trainIdx, distance)."""
    q, t, d = fe.match_knn(desc_a, desc_b, knn_match_ratio, pts_a, pts_b, search_local_dist)
    return list(zip(q.tolist(), t.tolist(), d.tolist()))


def get_feature_half_img(pts, desc, require_left, width_undistort, undistort_fov, dims=256):
    """getFeatureHalfImg (d2featuretracker.cpp:1051-1075): returns (desc_half, pts_new, tmp_to_idx)."""
    lib = load_library()
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    n = pts.shape[0]
    m = np.zeros(max(n, 1), np.int32); cnt = C.c_int(0)
    _check(lib.d2fe_half_image_filter(_ptr(pts), n, int(require_left), int(width_undistort), float(undistort_fov),
                                      _ptr(m), C.byref(cnt)))
    idx = m[:cnt.value].copy()
    desc = np.asarray(desc, np.float32).reshape(-1, dims)
    return desc[idx].copy(), pts[idx].copy(), idx


# ---- cross-agent exchange behind a pipe (include/d2fe.h, d2fe_exchange_* / d2fe_rccl_*; csrc/exchange.hip) ---------------------------------------------
WIRE = {"fp32": 0, "int8": 1, "int8-renorm256": 2}
EXCHANGE_PHASES = ("pack_blocks", "all_gather", "decode_counts_gate", "match_remote", "release_and_d2h")


def rccl_unique_id():
    """128 bytes from ncclGetUniqueId (rank 0 makes it; every rank needs the same bytes)"""
    buf = (C.c_char * 128)()
    _check(load_library().d2fe_rccl_unique_id(buf))
    return bytes(buf.raw)


def rccl_comm_init_rank(uid, world, rank, device=0):
    """ncclCommInitRank through the library's own dlopen of librccl -> an opaque ncclComm_t (int address)"""
    assert len(uid) == 128
    comm = C.c_void_p()
    _check(load_library().d2fe_rccl_comm_init_rank(C.create_string_buffer(uid, 128), int(world), int(rank), int(device), C.byref(comm)))
    return comm.value


def rccl_comm_destroy(comm):
    if comm:
        _check(load_library().d2fe_rccl_comm_destroy(C.c_void_p(comm)))


class Exchange(_Owned):
    """d2fe_exchange_*: pack -> ONE all-gather -> gate -> remote matchKNN -> D2H per ticket of a StereoPipe, queued on the stream of the lane that produced the
    ticket (own_stream=False) or on one stream of its own.  comm: an ncclComm_t address (rccl_comm_init_rank, or D2SLAM's own) or None with `all_gather` =
    a Python callable (user, d_send, d_recv, bytes_per_rank, stream) -> 0 (tests over gloo)."""
    _HANDLE, _DESTROY = "_x", "d2fe_exchange_destroy"

    def __init__(self, pipe, comm=None, world=1, rank=0, wire="fp32", loopback=False, slots=4, own_stream=False, timing=False, gate_thres=0.8, ratio=0.8, all_gather=None):
        self._lib = pipe._lib
        self._pipe = pipe
        c = _ExchangeConfig()
        self._lib.d2fe_exchange_default_config(C.byref(c))
        c.world, c.rank, c.wire, c.loopback, c.slots = int(world), int(rank), WIRE[wire], int(bool(loopback)), int(slots)
        c.own_stream, c.timing, c.gate_thres, c.ratio = int(bool(own_stream)), int(bool(timing)), float(gate_thres), float(ratio)
        self._cb = ALL_GATHER_FN(all_gather) if all_gather is not None else ALL_GATHER_FN()
        c.all_gather = self._cb
        self._x = C.c_void_p()
        _check(self._lib.d2fe_exchange_create(pipe._p, C.c_void_p(comm) if comm else None, C.byref(c), C.byref(self._x)))
        self.npairs = int(self._lib.d2fe_exchange_pairs(self._x))
        self.block_bytes = int(self._lib.d2fe_exchange_block_bytes(self._x))
        self.world, self.rank = int(world), int(rank)
        self.slots, self.timing = int(slots), bool(timing)
        self._res = _ExchangeResult()

    @property
    def stream(self):
        """own_stream=True: that hipStream_t (int), else None"""
        return self._lib.d2fe_exchange_stream(self._x)

    def gathered(self, slot):
        """(fp32 blocks, wire blocks): device addresses of the slot's gathered blocks [world][frames] (d2fe_exchange_gathered)"""
        a, b = C.c_void_p(), C.c_void_p()
        _check(self._lib.d2fe_exchange_gathered(self._x, int(slot), C.byref(a), C.byref(b)))
        return a.value, b.value

    def enqueue(self, ticket, slot):
        _check(self._lib.d2fe_exchange_enqueue(self._x, int(ticket), int(slot)))

    def collect(self, slot):
        """blocks until the slot's results are in host memory; numpy VIEWS into the pinned slot (valid until the slot is enqueued again)"""
        r = self._res
        _check(self._lib.d2fe_exchange_collect(self._x, int(slot), C.byref(r)))
        n, cap = int(r.npairs), int(r.cap)

        def view(addr, ct, shape):
            if not addr:
                return None
            cnt = int(np.prod(shape)) if len(shape) else 1
            return np.ctypeslib.as_array(C.cast(addr, C.POINTER(ct)), shape=(max(cnt, 1),))[:cnt].reshape(shape)
        return {"ticket": int(r.ticket), "mq": view(r.q_idx, C.c_int32, (n, cap)), "mt": view(r.t_idx, C.c_int32, (n, cap)), "md": view(r.dist, C.c_float, (n, cap)),
                "mn": view(r.n_match, C.c_int32, (n,)), "gate_pass": view(r.gate_pass, C.c_int32, (n,)), "sims": view(r.gate_sims, C.c_float, (n,)),
                "gate_n": int(r.gate_n), "phase_ms": [float(v) for v in r.phase_ms] if self.timing else None}


QUAD_MODE = {"all2all": 0, "gated": 1}
QUAD_EXCHANGE_PHASES = ("pack_blocks", "all_gather", "decode_prepare", "match_remote", "release_and_d2h")


def quad_exchange_job_layout(world, rank, quads, loopback=False):
    """d2fe_quad_exchange_job_layout: ([remote rank], [quad frame]) of every job of one rank; needs no device"""
    lib = load_library()
    n = int(lib.d2fe_quad_exchange_job_layout(int(world), int(rank), int(quads), int(bool(loopback)), None, None, 0))
    _check(n if n < 0 else 0)
    jr, jq = (C.c_int32 * max(n, 1))(), (C.c_int32 * max(n, 1))()
    lib.d2fe_quad_exchange_job_layout(int(world), int(rank), int(quads), int(bool(loopback)), jr, jq, n)
    return list(jr[:n]), list(jq[:n])


class QuadExchange(_Owned):
    """d2fe_quad_exchange_*: device view -> pack one block per view -> ONE all-gather -> [int8: decode] -> ONE prepare launch (gate, matcher table, counter) ->
    ONE matcher launch -> release -> ONE D2H per ticket of a QuadPipe, on one stream of its own (own_stream=True) or on the producing lane's stream.  comm: an
    ncclComm_t address (rccl_comm_init_rank, or D2SLAM's own) or None with `all_gather` = a Python callable (user, d_send, d_recv, bytes_per_rank, stream) -> 0.
    Job j = (remote rank, quad frame), rank-major; all2all: problem j * 16 + lv * 4 + rv, gated: problem j * 4 + k (include/d2fe.h has the layout)."""
    _HANDLE, _DESTROY = "_x", "d2fe_quad_exchange_destroy"

    def __init__(self, quad_pipe, comm=None, world=1, rank=0, wire="fp32", mode="all2all", loopback=False, slots=4, own_stream=True, timing=False, gate_thres=0.8,
                 ratio=0.8, all_gather=None):
        self._lib = quad_pipe._lib
        self._pipe = quad_pipe
        c = _QuadExchangeConfig()
        self._lib.d2fe_quad_exchange_default_config(C.byref(c))
        c.world, c.rank, c.wire, c.mode, c.loopback, c.slots = int(world), int(rank), WIRE[wire], QUAD_MODE[mode], int(bool(loopback)), int(slots)
        c.own_stream, c.timing, c.gate_thres, c.ratio = int(bool(own_stream)), int(bool(timing)), float(gate_thres), float(ratio)
        self._cb = ALL_GATHER_FN(all_gather) if all_gather is not None else ALL_GATHER_FN()
        c.all_gather = self._cb
        self._x = C.c_void_p()
        _check(self._lib.d2fe_quad_exchange_create(quad_pipe._p, C.c_void_p(comm) if comm else None, C.byref(c), C.byref(self._x)))
        self.njobs = int(self._lib.d2fe_quad_exchange_jobs(self._x))
        self.npairs = int(self._lib.d2fe_quad_exchange_pairs(self._x))
        self.block_bytes = int(self._lib.d2fe_quad_exchange_block_bytes(self._x))
        self.world, self.rank = int(world), int(rank)
        self.slots, self.timing, self.mode = int(slots), bool(timing), mode
        self._res = _QuadExchangeResult()

    @property
    def stream(self):
        """own_stream=True: that hipStream_t (int), else None"""
        return self._lib.d2fe_quad_exchange_stream(self._x)

    def gathered(self, slot):
        """(fp32 blocks, wire blocks): device addresses of the slot's gathered blocks [world][4 quads] (d2fe_quad_exchange_gathered)"""
        a, b = C.c_void_p(), C.c_void_p()
        _check(self._lib.d2fe_quad_exchange_gathered(self._x, int(slot), C.byref(a), C.byref(b)))
        return a.value, b.value

    def enqueue(self, ticket, slot):
        _check(self._lib.d2fe_quad_exchange_enqueue(self._x, int(ticket), int(slot)))

    def collect(self, slot):
        """blocks until the slot's results are in host memory; numpy VIEWS into the pinned slot (valid until the slot is enqueued again)"""
        r = self._res
        _check(self._lib.d2fe_quad_exchange_collect(self._x, int(slot), C.byref(r)))
        nj, n, cap = int(r.njobs), int(r.npairs), int(r.cap)
        f, i = np.float32, np.int32
        return {"ticket": int(r.ticket), "njobs": nj, "npairs": n, "pairs_per_job": int(r.pairs_per_job), "cap": cap,
                "job_rank": _pinned_view(r.job_rank, (nj,), i), "job_quad": _pinned_view(r.job_quad, (nj,), i),
                "mq": _pinned_view(r.q_idx, (n, cap), i), "mt": _pinned_view(r.t_idx, (n, cap), i), "md": _pinned_view(r.dist, (n, cap), f),
                "mn": _pinned_view(r.n_match, (n,), i), "local_view": _pinned_view(r.local_view, (n,), i), "remote_view": _pinned_view(r.remote_view, (n,), i),
                "dir_prev": _pinned_view(r.dir_prev, (nj,), i), "sims": _pinned_view(r.gate_sims, (nj, 4), f), "gate_n": int(r.gate_n),
                "phase_ms": [float(v) for v in r.phase_ms] if self.timing else None}


# ---- loop query behind a pipe (include/d2fe.h, d2fe_loop_*; csrc/loop.hip) -----------------------------------------------------------------------------------
LOOP_QUERY, LOOP_ADD = 1, 2      # enum D2FE_LOOP_*
LOOP_PHASES = ("search_gate_prepare", "match", "append", "release_and_d2h")


def loop_select(sims, ntotal, max_index, thres):
    """The selection of the search kernel in numpy: the best row by (similarity descending, label ascending) among the rows with label <= ntotal - max_index,
    accepted when its similarity exceeds thres -> (label or -1, similarity).  sims: the similarities of rows 0 .. ntotal - 1."""
    s = np.asarray(sims, np.float32)[:ntotal]
    lab = np.arange(len(s))
    ok = lab <= ntotal - max_index
    if not ok.any():
        return -1, 0.0
    best = int(lab[ok][np.argmax(s[ok])])      # argmax returns the first (lowest label) of equal similarities
    return (best, float(s[best])) if float(s[best]) > thres else (-1, 0.0)


def loop_dirs(views, main_dir, dir_old):
    """[(dir_a, dir_b)] of the `views` matcher problems of a hit (loop_detector.cpp:461-476 with main_dir_a = main_dir, main_dir_b = dir_old)"""
    return [((main_dir + i) % views, ((dir_old - main_dir + views) % views + main_dir + i) % views) for i in range(views)]


class LoopQuery(_Owned):
    """d2fe_loop_*: the device keyframe store behind a StereoPipe or a QuadPipe and, per ticket, search + gate -> matchKNN against the stored keyframe -> add, on
    one stream of its own (LoopDetector::processImageArray, loop_detector.cpp:23-215).  Destroy it before the pipe."""
    _HANDLE, _DESTROY = "_x", "d2fe_loop_destroy"

    def __init__(self, pipe, capacity_keyframes=4096, max_index=10, thres=0.6, ratio=0.8, mode=0, slots=4, timing=False, max_queries=64):
        self._lib = pipe._lib
        self._pipe = pipe
        c = _LoopConfig()
        self._lib.d2fe_loop_default_config(C.byref(c))
        c.capacity_keyframes, c.max_index, c.mode, c.slots, c.timing, c.max_queries = int(capacity_keyframes), int(max_index), int(mode), int(slots), int(bool(timing)), int(max_queries)
        c.thres, c.ratio = float(thres), float(ratio)
        self._x = C.c_void_p()
        quad = isinstance(pipe, QuadPipe)
        _check((self._lib.d2fe_loop_create_quad if quad else self._lib.d2fe_loop_create)(pipe._p, C.byref(c), C.byref(self._x)))
        self.views, self.main_dir = (4, 2) if quad else (1, 0)
        self.slots, self.timing = int(slots), bool(timing)
        self._res = _LoopResult()

    @property
    def stream(self):
        return self._lib.d2fe_loop_stream(self._x)

    @property
    def ntotal(self):
        r = int(self._lib.d2fe_loop_ntotal(self._x))
        if r < 0:
            _check(r)
        return r

    @property
    def keyframes(self):
        r = int(self._lib.d2fe_loop_keyframes(self._x))
        if r < 0:
            _check(r)
        return r

    def enqueue(self, ticket, slot, is_keyframe=None, flags=LOOP_QUERY | LOOP_ADD):
        m = None if is_keyframe is None else np.ascontiguousarray(is_keyframe, np.uint8)
        _check(self._lib.d2fe_loop_enqueue(self._x, int(ticket), int(slot), _ptr(m) if m is not None else None, int(flags)))

    def add_host(self, netvlad, desc, n_kp):
        """keyframes from host arrays [n][views][netvlad_dim], [n][views][cap][desc_dim] (or None when every count is 0), [n][views] -> ordinal of the first"""
        n_kp = np.ascontiguousarray(n_kp, np.int32).reshape(-1, self.views)
        nv = np.ascontiguousarray(netvlad, np.float32); d = None if desc is None else np.ascontiguousarray(desc, np.float32)
        r = int(self._lib.d2fe_loop_add_host(self._x, _ptr(nv), _ptr(d), _ptr(n_kp), n_kp.shape[0]))
        if r < 0:
            _check(r)
        return r

    def query_device(self, d_netvlad, d_desc, d_n_kp, nq, max_index, slot, stream=None):
        """query only, raw device addresses (ints) in the pipe's row order: [nq][views][netvlad_dim], [nq][views][cap][desc_dim], [nq][views]"""
        _check(self._lib.d2fe_loop_query_device(self._x, C.c_void_p(d_netvlad), C.c_void_p(d_desc), C.c_void_p(d_n_kp), int(nq), int(max_index), int(slot),
                                                C.c_void_p(stream or 0)))

    def collect(self, slot):
        """blocks until the slot's results are in host memory; numpy VIEWS into the pinned slot (valid until the slot is enqueued again)"""
        r = self._res
        _check(self._lib.d2fe_loop_collect(self._x, int(slot), C.byref(r)))
        F, V, cap = int(r.frames), int(r.views), int(r.cap)
        f, i = np.float32, np.int32
        out = {"ticket": int(r.ticket), "frames": F, "views": V, "cap": cap, "sim": _pinned_view(r.sim, (F,), f)}
        for k in ("queried", "label", "keyframe", "dir_old", "ntotal_at_query"):
            out[k] = _pinned_view(getattr(r, k), (F,), i)
        for k in ("added_label", "dir_a", "dir_b", "n_match"):
            out[k] = _pinned_view(getattr(r, k), (F, V), i)
        out["q_idx"] = _pinned_view(r.q_idx, (F, V, cap), i); out["t_idx"] = _pinned_view(r.t_idx, (F, V, cap), i); out["dist"] = _pinned_view(r.dist, (F, V, cap), f)
        out["phase_ms"] = [float(v) for v in r.phase_ms] if self.timing else None
        return out


# ---- remote tracking against the keyframe window (include/d2fe.h, d2fe_window_*; csrc/window.hip) ---------------------------------------------------------------
WINDOW_PHASES = ("gate", "match", "d2h")
WINDOW_DIRS = (2, 3, 0, 1)       # getMatchedPrevKeyframe's view order of a quadcam keyframe (d2featuretracker.cpp:207)


def window_retain_plan(tags, keep):
    """d2fe_window_retain_plan: [True for every keyframe updatebySldWin's erase loop (:47-57) drops]; tags oldest first.  Needs no device."""
    t = np.ascontiguousarray(tags, np.int64).reshape(-1); k = np.ascontiguousarray(keep, np.int64).reshape(-1)
    ev = np.zeros(max(len(t), 1), np.uint8)
    n = int(load_library().d2fe_window_retain_plan(_ptr(t) if len(t) else None, len(t), _ptr(k) if len(k) else None, len(k), _ptr(ev)))
    if n < 0:
        _check(n)
    assert n == int(ev[:len(t)].sum())
    return [bool(v) for v in ev[:len(t)]]


def window_select(sims, thres):
    """The gate kernel's selection, restated: sims [n][V] in window order (oldest first) and `dirs` order -> (pos, j) of the smallest (n - 1 - pos) * V + j among the
    pairs with !(sim < thres), or None"""
    sims = np.asarray(sims, np.float32)
    n, V = sims.shape if sims.ndim == 2 else (0, 1)
    best = None
    for pos in range(n):
        for j in range(V):
            if not (float(sims[pos, j]) < thres):
                key = (n - 1 - pos) * V + j
                if best is None or key < best:
                    best = key
    return None if best is None else (n - 1 - best // V, best % V)


def window_views(views, dir_b):
    """[(remote view, local view)] of the `views` matcher problems of a hit (trackRemoteFrames :273-284 with dir_cur = 2)"""
    if views == 1:
        return [(0, 0)]
    return [((2 + k) % 4, (dir_b - 2 + (2 + k) % 4) % 4) for k in range(4)]


class KeyframeWindow(_Owned):
    """d2fe_window_*: the tracker's keyframe window on the device behind a StereoPipe or a QuadPipe, and D2FeatureTracker::trackRemoteFrames for a batch of remote
    frames -- the NetVLAD walk of getMatchedPrevKeyframe (newest keyframe first, the first pass wins) and matchKNN(keyframe, remote) -- as gate -> match -> D2H on one
    stream of its own (d2featuretracker.cpp:166-310).  Destroy it before the pipe."""
    _HANDLE, _DESTROY = "_x", "d2fe_window_destroy"

    def __init__(self, pipe, capacity=12, thres=0.8, ratio=0.8, mode=0, slots=4, timing=False, max_queries=64):
        self._lib = pipe._lib
        self._pipe = pipe
        c = _WindowConfig()
        self._lib.d2fe_window_default_config(C.byref(c))
        c.capacity, c.mode, c.slots, c.timing, c.max_queries = int(capacity), int(mode), int(slots), int(bool(timing)), int(max_queries)
        c.thres, c.ratio = float(thres), float(ratio)
        self._x = C.c_void_p()
        quad = isinstance(pipe, QuadPipe)
        _check((self._lib.d2fe_window_create_quad if quad else self._lib.d2fe_window_create)(pipe._p, C.byref(c), C.byref(self._x)))
        self.views, self.gate_view = (4, 2) if quad else (1, 0)
        g = [C.c_int32() for _ in range(4)]
        _check((self._lib.d2fe_quad_pipe_geometry if quad else self._lib.d2fe_pipe_geometry)(pipe._p, *[C.byref(v) for v in g]))
        self.frames, self.cap, self.desc_dim, self.netvlad_dim = (int(v.value) for v in g)
        self.capacity, self.slots, self.timing = int(capacity), int(slots), bool(timing)
        self._res = _WindowResult()

    @property
    def stream(self):
        return self._lib.d2fe_window_stream(self._x)

    def __len__(self):
        r = int(self._lib.d2fe_window_size(self._x))
        if r < 0:
            _check(r)
        return r

    def tags(self):
        """the window's tags, oldest first"""
        t = np.zeros(self.capacity, np.int64)
        n = int(self._lib.d2fe_window_tags(self._x, _ptr(t), self.capacity))
        if n < 0:
            _check(n)
        return [int(v) for v in t[:n]]

    def push(self, ticket, frame, tag):
        """frame `frame` of a ticket of the pipe becomes the newest keyframe (asynchronous, device to device); the newest tag again is a no-op"""
        _check(self._lib.d2fe_window_push(self._x, int(ticket), int(frame), int(tag)))

    def push_host(self, netvlad, desc, n_kp, tag):
        """the same from host arrays [views][netvlad_dim], [views][cap][desc_dim] (or None when every count is 0), [views]; blocking"""
        n_kp = np.ascontiguousarray(n_kp, np.int32).reshape(self.views)
        nv = np.ascontiguousarray(netvlad, np.float32); d = None if desc is None else np.ascontiguousarray(desc, np.float32)
        _check(self._lib.d2fe_window_push_host(self._x, _ptr(nv), _ptr(d), _ptr(n_kp), int(tag)))

    def retain(self, tags):
        """updatebySldWin: drops every keyframe whose tag is not listed, except the newest -> how many were dropped (host bookkeeping only)"""
        t = np.ascontiguousarray(tags, np.int64).reshape(-1)
        r = int(self._lib.d2fe_window_retain(self._x, _ptr(t) if len(t) else None, len(t)))
        if r < 0:
            _check(r)
        return r

    def track_device(self, d_netvlad, nv_stride, d_desc, desc_stride, d_n_kp, nkp_stride, nq, slot, stream=None):
        """raw device addresses (ints); row q * views + v of each array is view v of remote frame q, strides in 32-bit words between rows"""
        _check(self._lib.d2fe_window_track_device(self._x, C.c_void_p(d_netvlad), C.c_size_t(nv_stride), C.c_void_p(d_desc), C.c_size_t(desc_stride), C.c_void_p(d_n_kp),
                                                  C.c_size_t(nkp_stride), int(nq), int(slot), C.c_void_p(stream or 0)))

    def _track_blocks(self, d_blocks, world, first, nq, slot, stream):
        cap, G, D = self.cap, self.netvlad_dim, self.desc_dim
        blk = block_words(cap, G, D)
        if nq is None:
            nq = world * self.frames - first
        base = d_blocks + 4 * blk * first * self.views
        self.track_device(base + 4 * block_field_offset(cap, G, "netvlad", D), blk, base + 4 * block_field_offset(cap, G, "desc", D), blk,
                          base + 4 * block_field_offset(cap, G, "n", D), blk, nq, slot, stream)
        return nq

    def track_exchange(self, exchange, xslot, slot, first=0, nq=None):
        """the gathered fp32 blocks [world][frames] of slot `xslot` of an Exchange, read in place: frames first .. first + nq of them (default: all of them, this
        rank's own included), ordered behind what is queued on the exchange's stream (own_stream=False: collect the exchange first).  Returns nq."""
        return self._track_blocks(exchange.gathered(xslot)[0], exchange.world, first, nq, slot, exchange.stream)

    def track_quad_exchange(self, exchange, xslot, slot, first=0, nq=None):
        """the same for a QuadExchange: blocks [world][quads][4 views], quad frames first .. first + nq"""
        return self._track_blocks(exchange.gathered(xslot)[0], exchange.world, first, nq, slot, exchange.stream)

    def collect(self, slot):
        """blocks until the slot's results are in host memory; numpy VIEWS into the pinned slot (valid until the slot is queued again)"""
        r = self._res
        _check(self._lib.d2fe_window_collect(self._x, int(slot), C.byref(r)))
        nq, V, cap, K = int(r.nq), int(r.views), int(r.cap), int(r.capacity)
        f, i = np.float32, np.int32
        out = {"nq": nq, "views": V, "cap": cap, "capacity": K, "n_window": int(r.n_window),
               "keyframe_tag": _pinned_view(r.keyframe_tag, (2 * nq,), i).view(np.int64), "sim": _pinned_view(r.sim, (nq,), f), "sims": _pinned_view(r.sims, (nq, K, V), f)}
        for k in ("keyframe_pos", "dir_a", "dir_b"):
            out[k] = _pinned_view(getattr(r, k), (nq,), i)
        for k in ("local_view", "remote_view", "n_match"):
            out[k] = _pinned_view(getattr(r, k), (nq, V), i)
        out["q_idx"] = _pinned_view(r.q_idx, (nq, V, cap), i); out["t_idx"] = _pinned_view(r.t_idx, (nq, V, cap), i); out["dist"] = _pinned_view(r.dist, (nq, V, cap), f)
        out["phase_ms"] = [float(v) for v in r.phase_ms] if self.timing else None
        return out

