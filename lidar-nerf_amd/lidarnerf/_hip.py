"""ctypes binding of liblidarnerf_hip.so (C ABI: include/lidarnerf_hip.h).

PyTorch is used only for device memory and streams: every call passes raw device pointers + sizes + the current HIP
stream.  There is NO CPU fallback: if the library is missing or a call fails, a RuntimeError is raised.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# LNH_LIB_PATH: developer override (A/B builds of the same library, tools/); still no fallback if it is missing
_LIB_PATH = os.environ.get("LNH_LIB_PATH") or os.path.join(os.path.dirname(_HERE), "lib", "liblidarnerf_hip.so")

P, U32, I32, F32 = C.c_void_p, C.c_uint32, C.c_int, C.c_float
# the bucketed grid backward's arguments up to the workspace, shared by its five entry points
_GRID_BWD_WS = [P, P, P, P, U32, U32, U32, U32, F32, U32, U32, I32, U32, I32, P, C.c_uint64]

# name -> argument ctypes (stream is appended automatically)
_SIGS = {
    "lnh_grid_encode_forward": [P, P, P, P, U32, U32, U32, U32, F32, U32, P, U32, I32, U32, I32],
    "lnh_grid_encode_backward": [P, P, P, P, P, U32, U32, U32, U32, F32, U32, P, P, U32, I32, U32, I32],
    "lnh_grid_encode_backward_ws": _GRID_BWD_WS,
    "lnh_grid_encode_backward_ws_levels": _GRID_BWD_WS + [U32, U32],
    "lnh_grid_encode_backward_ws_begin": _GRID_BWD_WS,
    "lnh_grid_encode_backward_ws_finish": _GRID_BWD_WS + [U32, U32],
    "lnh_grid_encode_backward_ws_ex": _GRID_BWD_WS + [U32, U32, I32, U32],
    "lnh_grad_total_variation": [P, P, P, P, F32, U32, U32, U32, U32, F32, U32, U32, I32, I32],
    "lnh_grid_corner_indices": [P, P, P, U32, U32, U32, U32, F32, U32, U32, I32],
    "lnh_freq_encode_forward": [P, U32, U32, U32, U32, P],
    "lnh_freq_encode_backward": [P, P, U32, U32, U32, U32, P],
    "lnh_sh_encode_forward": [P, P, U32, U32, U32, P],
    "lnh_sh_encode_backward": [P, P, U32, U32, U32, P, P],
    "lnh_mlp_forward": [P, P, U32, U32, U32, U32, U32, U32, U32, P, P],
    "lnh_mlp_backward": [P, P, P, U32, U32, U32, U32, U32, U32, U32, P, P, P, C.c_uint64],
    "lnh_mlp_backward_data": [P, P, P, U32, U32, U32, U32, U32, U32, P, P],
    "lnh_mlp_wgrad": [P, P, U32, U32, U32, P, P, C.c_uint64],
    "lnh_near_far_from_aabb": [P, P, P, U32, F32, P, P],
    "lnh_sph_from_ray": [P, P, F32, U32, P],
    "lnh_morton3D": [P, U32, P],
    "lnh_morton3D_invert": [P, U32, P],
    "lnh_packbits": [P, U32, F32, P],
    "lnh_occupancy_lookup": [P, P, P, F32, U32, U32, U32, P, P],
    "lnh_march_rays_train": [P, P, P, F32, F32, U32, U32, U32, U32, U32, P, P, P, P, P, P, P, P],
    "lnh_march_rays_train_ordered": [P, P, P, F32, F32, U32, U32, U32, U32, U32, P, P, P, P, P, P, P, P],
    "lnh_composite_rays_train_forward": [P, P, P, P, U32, U32, F32, P, P, P],
    "lnh_composite_rays_train_backward": [P, P, P, P, P, P, P, P, U32, U32, F32, P, P],
    "lnh_lidar_composite_rays_train_forward": [P, P, P, P, P, P, P, U32, U32, U32, F32, P, P, P],
    "lnh_lidar_composite_rays_train_backward": [P, P, P, P, P, P, P, P, P, P, P, P, P, U32, U32, U32, F32, P, P],
    "lnh_march_rays": [U32, U32, P, P, P, P, F32, F32, U32, U32, U32, P, P, P, P, P, P, P],
    "lnh_composite_rays": [U32, U32, F32, P, P, P, P, P, P, P, P],
    "lnh_lidar_march_rays": [U32, U32, U32, P, P, P, P, P, P, P, F32, F32, U32, U32, U32, P, P, P, P, P],
    "lnh_lidar_composite_rays": [U32, U32, U32, U32, F32, P, P, P, P, P, P, P, P, P, P, P, P, P, P],
    "lnh_alive_compact": [U32, P, P, P, P],
    "lnh_lidar_weights": [P, P, P, U32, U32, F32, P],
    "lnh_lidar_composite_forward": [P, P, P, P, U32, U32, U32, F32, P, P, P, P],
    "lnh_lidar_composite_backward": [P, P, P, P, P, P, P, U32, U32, U32, F32, P, P],
    "lnh_lidar_resample": [P, P, P, P, U32, U32, U32, F32, U32, P, P, P],
    "lnh_lidar_resample_strided": [P, P, U32, P, P, U32, U32, U32, F32, U32, P, P, P],
    "lnh_lidar_resample_points": [P, P, U32, P, P, U32, U32, U32, F32, P, P, P, P, P, P, F32, P],
    "lnh_lidar_sample_points": [P, P, P, P, F32, U32, U32, U32, U32, P],
    "lnh_lidar_coarse_sample_points": [P, P, P, P, F32, U32, U32, U32, F32, F32, P, P],
    "lnh_grid_encode_forward_mapped": [P, P, P, P, U32, U32, U32, U32, U32, U32, U32, F32, U32, I32],
    "lnh_grid_encode_forward_mapped_ex": [P, P, P, P, U32, U32, U32, U32, U32, U32, U32, F32, U32, U32, I32],
    "lnh_density_mlp_forward": [P, P, U32, U32, U32, U32, U32, P, P],
    "lnh_density_mlp_backward": [P, P, P, U32, U32, U32, U32, P, P, P, C.c_uint64],
    "lnh_lidar_merge_weights": [P, P, P, P, U32, U32, F32, P, P],
    "lnh_lidar_color_forward": [P, P, P, P, P, U32, U32, P],
    "lnh_lidar_color_composite_forward": [P, P, P, P, P, P, P, U32, U32, F32, P, P, P, P, P, P],
    "lnh_lidar_color_composite_forward_train": [P, P, P, P, P, P, P, U32, U32, F32, P, F32, F32, F32, P, P, P, P, P, P, P],
    "lnh_lidar_coarse_samples": [P, U32, U32, F32, F32, P],
    "lnh_lidar_dir_term": [P, P, U32, U32, U32, P, P],
    "lnh_lidar_dir_term_freq": [P, U32, P, U32, U32, P, P],
    "lnh_lidar_dir_term_backward": [P, P, U32, U32, P, P, U32, P, C.c_uint64],
    "lnh_lidar_pack_weights": [P, U32, P, U32, P, U32, U32, P, U32, P, U32, P, P],
    "lnh_lidar_to_pano": [P, U32, U32, U32, F32, F32, F32, P, P, P],
    "lnh_pano_to_lidar": [P, P, U32, U32, F32, F32, P, P],
    "lnh_lidar_to_pano_masked": [P, U32, U32, U32, F32, F32, F32, U32, U32, U32, U32, F32, P, P, P],
    "lnh_lidar_to_pano_fpa": [P, C.c_uint64, U32, U32, F32, F32, F32, U32, C.c_double, P, C.c_uint64, P, P],
    "lnh_marching_cubes_count": [P, U32, U32, U32, F32, P, C.c_uint64, P],
    "lnh_marching_cubes_emit": [P, U32, U32, U32, F32, P, C.c_uint64, P, U32, P, U32],
    "lnh_tsdf_integrate": [P, P, U32, U32, U32, F32, F32, F32, P, P, U32, U32, U32, F32, P, P],
    "lnh_tsdf_finalize": [P, P, U32, U32, U32, U32, P],
    "lnh_mesh_vertex_observed": [P, U32, P, U32, U32, U32, U32, P],
    "lnh_mesh_filter_count": [P, U32, P, U32, P, C.c_uint64, P],
    "lnh_mesh_filter_emit": [P, P, U32, P, U32, P, C.c_uint64, P, U32, P, U32],
    "lnh_raycast_bounds": [P, U32, P, U32, P, C.c_uint64, P, P],
    "lnh_raycast_build_count": [P, U32, P, U32, P, U32, U32, U32, P, C.c_uint64, P, P],
    "lnh_raycast_build_fill": [P, U32, P, U32, P, U32, U32, U32, P, C.c_uint64, P, P, C.c_uint64],
    "lnh_raycast_cast": [P, U32, P, U32, P, U32, U32, U32, P, P, C.c_uint64, P, P, U32, P, P, P, P],
    "lnh_knn_bounds": [P, U32, P, C.c_uint64, P],
    "lnh_knn_build_count": [P, U32, P, U32, U32, U32, P, C.c_uint64, P, P],
    "lnh_knn_build_fill": [P, U32, P, U32, U32, U32, P, C.c_uint64, P, P],
    "lnh_knn_search": [P, U32, P, U32, U32, U32, P, P, P, P, P, U32, U32, P, P, P, P],
    "lnh_raydrop_forward": [P, U32, U32, P, U32, U32, P],
    "lnh_raydrop_grad": [P, U32, U32, P, U32, U32, P, C.c_uint64, P, P],
    "lnh_raydrop_adam": [P, P, P, P, U32, P, U32, P, P, C.c_double, C.c_double, C.c_double],
    "lnh_unet_input": [P, U32, U32, U32, U32, P],
    "lnh_unet_conv3x3": [P, U32, U32, U32, U32, P, U32, U32, U32, P, P, P, U32, U32, U32, P],
    "lnh_unet_upconv2x2": [P, U32, U32, U32, U32, P, P, U32, P],
    "lnh_unet_head": [P, U32, U32, U32, P, P, P, P],
    "lnh_unet_pool_backward": [P, U32, U32, U32, U32, P, P, U32, P],
    "lnh_unet_head_backward": [P, U32, U32, U32, P, P, P, C.c_uint64, P, P, P],
    "lnh_unet_pack_upconv": [P, U32, U32, P, P],
    "lnh_unet_upconv2x2_backward_data": [P, U32, U32, U32, U32, U32, U32, U32, U32, U32, P, P],
    "lnh_unet_upconv2x2_backward_weight": [P, P, U32, U32, U32, U32, U32, U32, U32, U32, U32, P, C.c_uint64, P, P],
    "lnh_unet_pack_conv3x3": [P, U32, U32, P, P],
    "lnh_unet_conv3x3_raw": [P, U32, U32, U32, U32, P, U32, U32, U32, P, U32, U32, U32, P],
    "lnh_unet_bn_stats": [P, C.c_uint64, U32, P, P, C.c_double, C.c_double, P, C.c_uint64, P, P, P, P, P, P],
    "lnh_unet_bn_relu": [P, C.c_uint64, U32, P, P, P],
    "lnh_unet_bn_relu_backward": [P, P, P, C.c_uint64, U32, P, P, P, P, C.c_uint64, P, P, P],
    "lnh_unet_conv3x3_backward_weight": [P, U32, U32, U32, U32, P, U32, U32, U32, P, U32, U32, U32, U32, P, C.c_uint64, P],
    "lnh_unet_loss_grad": [P, P, U32, C.c_uint64, C.c_double, P, C.c_uint64, P, P],
    "lnh_unet_grad_sumsq": [P, U32, P, C.c_uint64, P],
    "lnh_unet_rmsprop_step": [P, U32, P, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double],
    "lnh_chamfer_nn": [P, U32, P, U32, P, P],
    "lnh_grad_check_f16": [P, C.c_uint64, P],
    "lnh_adam_table_step": [P, P, P, P, P, C.c_uint64, C.c_double, C.c_double, C.c_double, C.c_double, P, P, P, P],
    "lnh_adam_table_step_dlr": [P, P, P, P, P, C.c_uint64, P, C.c_double, C.c_double, C.c_double, P, P, P, P],
    "lnh_lidar_step_prologue": [P, U32, P, U32, P, U32, U32, P, U32, P, U32, P, P, P, P, P, P, F32, U32, U32, U32, F32, F32, P, P, P,
                                P],
    "lnh_lidar_loss": [P, P, P, U32, F32, F32, F32, P, P, P, P],
    "lnh_lidar_loss_patch": [P, P, P, U32, U32, U32, F32, F32, F32, F32, F32, P, P, P, P],
    "lnh_train_check": [P, P, C.c_uint64, P, P, U32, F32, F32, C.c_double, C.c_double],
    "lnh_train_step": [P, P, P, P, P, P, C.c_uint64, P, P, P, U32, P, P, C.c_double, C.c_double, C.c_double, C.c_double,
                       C.c_double, U32],
    "lnh_zero_regions": [P, P, U32],
    "lnh_ema_update": [P, P, C.c_uint64, P, P, P, U32, F32],
    "lnh_ema_swap": [P, P, P, C.c_uint64, P, P, P, U32],
    "lnh_lidar_march_prologue": [P, P, P, U32, F32, F32, P, P, P, P, U32],
    "lnh_lidar_color_backward": [P, P, P, P, P, P, P, U32, U32, P, P, P, P, C.c_uint64],
    "lnh_lidar_color_backward_image": [P, P, P, P, P, P, P, U32, U32, P, P, P, P, C.c_uint64],
    "lnh_ragged_color_forward": [P, P, P, P, U32, U32, P],
    "lnh_ragged_color_backward": [P, P, F32, P, P, P, P, U32, U32, P, P, P, P, C.c_uint64],
    "lnh_ragged_points": [P, F32, U32, P],
    "lnh_ragged_pack_weights": [P, U32, P, U32, P, U32, U32, P, U32, P, U32, P, P],
    "lnh_ragged_color_input": [P, P, U32, U32, P],
    "lnh_ragged_color_input_rays": [P, P, P, P, U32, U32, U32, P],
    "lnh_ragged_color_output": [P, U32, P],
    "lnh_ragged_color_output_backward": [P, P, U32, P],
    "lnh_ragged_grad_rows": [P, F32, P, P, U32, U32, P],
    "lnh_lidar_loss_ex": [P, P, P, U32, P, P, P, C.c_uint64, P, P, P],
    "lnh_lidar_eval_frame": [P, P, P, U32, U32, P, F32, I32, I32, P, C.c_uint64, P, P, P],
    "lnh_lidar_eval_ssim": [P, P, U32, U32, F32, I32, P, C.c_uint64],
    "lnh_lidar_eval_finalize": [U32, U32, P, I32, I32, P, C.c_uint64, P, P, U32],
    "lnh_eval_points_project": [P, P, U32, U32, F32, F32, F32, I32, P, C.c_uint64, P, P, P],
    "lnh_eval_points_nn": [P, P, P, U32, P, C.c_uint64, P, P, P, P],
    "lnh_eval_points_finalize": [P, P, P, U32, F32, P, P, U32],
    "lnh_nvs_eval_frame": [P, P, P, P, P, U32, U32, F32, P, C.c_uint64],
    "lnh_nvs_eval_ssim": [P, P, P, U32, U32, P, C.c_uint64],
    "lnh_nvs_eval_finalize": [U32, U32, P, C.c_uint64, P, P, P, U32],
    "lnh_lidar_sample_batch": [P, P, I32, I32, U32, U32, F32, F32, P, P, U32, U32, I32, I32, I32, I32, I32, P, P, P, P],
    "lnh_lidar_frame_rays": [P, I32, I32, U32, U32, F32, F32, P, P],
}
# entry points added without moving lnh_version(): a library built before them still loads, and the feature is detected
# by symbol (require_symbols)
_OPTIONAL = {"lnh_lidar_eval_frame": "frame evaluation", "lnh_lidar_eval_ssim": "frame evaluation",
             "lnh_lidar_eval_finalize": "frame evaluation", "lnh_lidar_eval_workspace_bytes": "frame evaluation",
             "lnh_eval_points_project": "points evaluation", "lnh_eval_points_nn": "points evaluation",
             "lnh_eval_points_finalize": "points evaluation", "lnh_eval_points_workspace_bytes": "points evaluation",
             "lnh_nvs_eval_frame": "NVS evaluation", "lnh_nvs_eval_ssim": "NVS evaluation",
             "lnh_nvs_eval_finalize": "NVS evaluation", "lnh_nvs_eval_workspace_bytes": "NVS evaluation",
             "lnh_lidar_sample_batch": "batch sampling", "lnh_lidar_frame_rays": "batch sampling",
             "lnh_march_rays_train_ordered": "ordered marching",
             "lnh_lidar_to_pano_masked": "bbox-mask conversion", "lnh_lidar_to_pano_fpa": "fpa conversion",
             "lnh_lidar_to_pano_fpa_workspace_size": "fpa conversion",
             "lnh_marching_cubes_count": "mesh export", "lnh_marching_cubes_emit": "mesh export",
             "lnh_marching_cubes_workspace_size": "mesh export",
             "lnh_tsdf_integrate": "TSDF fusion", "lnh_tsdf_finalize": "TSDF fusion",
             "lnh_mesh_vertex_observed": "TSDF fusion", "lnh_mesh_filter_count": "TSDF fusion",
             "lnh_mesh_filter_emit": "TSDF fusion", "lnh_mesh_filter_workspace_size": "TSDF fusion",
             "lnh_raycast_bounds": "mesh ray casting", "lnh_raycast_build_count": "mesh ray casting",
             "lnh_raycast_build_fill": "mesh ray casting", "lnh_raycast_cast": "mesh ray casting",
             "lnh_raycast_workspace_size": "mesh ray casting",
             "lnh_knn_bounds": "nearest-neighbour search", "lnh_knn_build_count": "nearest-neighbour search",
             "lnh_knn_build_fill": "nearest-neighbour search", "lnh_knn_search": "nearest-neighbour search",
             "lnh_knn_workspace_size": "nearest-neighbour search",
             "lnh_raydrop_forward": "ray-drop MLP", "lnh_raydrop_grad": "ray-drop MLP", "lnh_raydrop_adam": "ray-drop MLP",
             "lnh_raydrop_workspace_size": "ray-drop MLP", "lnh_raydrop_param_count": "ray-drop MLP",
             "lnh_unet_input": "ray-drop U-Net", "lnh_unet_conv3x3": "ray-drop U-Net", "lnh_unet_upconv2x2": "ray-drop U-Net",
             "lnh_unet_head": "ray-drop U-Net", "lnh_unet_workspace_size": "ray-drop U-Net",
             "lnh_unet_pool_backward": "U-Net training", "lnh_unet_head_backward": "U-Net training",
             "lnh_unet_head_backward_workspace_size": "U-Net training",
             "lnh_unet_pack_upconv": "U-Net training", "lnh_unet_upconv2x2_backward_data": "U-Net training",
             "lnh_unet_upconv2x2_backward_weight": "U-Net training",
             "lnh_unet_upconv2x2_backward_weight_workspace_size": "U-Net training",
             "lnh_unet_pack_conv3x3": "U-Net training", "lnh_unet_conv3x3_raw": "U-Net training", "lnh_unet_bn_stats": "U-Net training",
             "lnh_unet_bn_relu": "U-Net training", "lnh_unet_bn_relu_backward": "U-Net training",
             "lnh_unet_bn_stats_workspace_size": "U-Net training", "lnh_unet_bn_relu_backward_workspace_size": "U-Net training",
             "lnh_unet_conv3x3_backward_weight": "U-Net training",
             "lnh_unet_conv3x3_backward_weight_workspace_size": "U-Net training",
             "lnh_unet_loss_grad": "U-Net training", "lnh_unet_loss_grad_workspace_size": "U-Net training",
             "lnh_unet_grad_sumsq": "U-Net training", "lnh_unet_grad_sumsq_workspace_size": "U-Net training",
             "lnh_unet_rmsprop_step": "U-Net training",
             "lnh_lidar_color_composite_forward_train": "training forward tail",
             "lnh_lidar_color_composite_forward_train_bf16": "training forward tail"}
for _n in ("lnh_mlp_forward", "lnh_mlp_backward", "lnh_mlp_backward_data", "lnh_mlp_wgrad", "lnh_density_mlp_forward", "lnh_density_mlp_backward",
           "lnh_lidar_dir_term", "lnh_lidar_pack_weights", "lnh_lidar_step_prologue", "lnh_lidar_color_forward", "lnh_lidar_color_backward",
           "lnh_lidar_color_composite_forward", "lnh_lidar_color_composite_forward_train", "lnh_lidar_color_backward_image",
           "lnh_lidar_dir_term_freq",
           "lnh_ragged_pack_weights", "lnh_ragged_color_input", "lnh_ragged_color_input_rays", "lnh_ragged_color_output",
           "lnh_ragged_color_output_backward", "lnh_ragged_grad_rows", "lnh_ragged_color_forward", "lnh_ragged_color_backward"):
    _SIGS[_n + "_bf16"] = _SIGS[_n]  # bf16-operand build of the MLP kernels (include/lidarnerf_hip.h, last section)
EXPORTS = sorted(list(_SIGS) + ["lnh_version", "lnh_last_error", "lnh_arch", "lnh_build_variant",
                                 "lnh_grid_backward_workspace_size", "lnh_grid_backward_workspace_size_min",
                                 "lnh_grid_backward_plan_info", "lnh_grid_backward_workspace_clear_bytes",
                                 "lnh_grid_backward_set_slice_entries", "lnh_grid_forward_set_schedule",
                                 "lnh_wgrad_workspace_bytes",
                                 "lnh_lidar_loss_ex_workspace_bytes", "lnh_lidar_eval_workspace_bytes",
                                 "lnh_eval_points_workspace_bytes", "lnh_nvs_eval_workspace_bytes",
                                 "lnh_lidar_to_pano_fpa_workspace_size",
                                 "lnh_marching_cubes_workspace_size", "lnh_raycast_workspace_size",
                                 "lnh_mesh_filter_workspace_size",
                                 "lnh_knn_workspace_size", "lnh_raydrop_workspace_size", "lnh_raydrop_param_count",
                                 "lnh_unet_workspace_size", "lnh_unet_head_backward_workspace_size",
                                 "lnh_unet_upconv2x2_backward_weight_workspace_size", "lnh_unet_bn_stats_workspace_size",
                                 "lnh_unet_bn_relu_backward_workspace_size",
                                 "lnh_unet_conv3x3_backward_weight_workspace_size",
                                 "lnh_unet_loss_grad_workspace_size", "lnh_unet_grad_sumsq_workspace_size"])

LNH_F32, LNH_F16 = 0, 1
LNH_BWD_WS_CLEARED, LNH_BWD_TABLE_ZERO = 1, 2
# lnh_unet_conv3x3's tile argument (include/lidarnerf_hip.h, LNH_UNET_TILE_*); 0 = chosen from the shape
UNET_TILE_16, UNET_TILE_32, UNET_TILE_64, UNET_TILE_KSPLIT = 1, 2, 4, 8
# lnh_unet_conv3x3_backward_weight's variant argument (LNH_UNET_WGRAD_*); 0 = the default
UNET_WGRAD_GATHER, UNET_WGRAD_TR = 1, 2
# lnh_unet_loss_grad's mask_dtype (LNH_UNET_MASK_*); the table and state of lnh_unet_grad_sumsq / lnh_unet_rmsprop_step (LNH_URS_*)
UNET_MASK_F32, UNET_MASK_U8 = 0, 1
URS_MAX_TENSORS, URS_TENSOR_WORDS, URS_SLOTS = 64, 5, 8  # a table record: param, grad, square_avg, momentum_buffer, numel (int64 each)
URS_LR, URS_STEP, URS_SKIPPED, URS_SUMSQ, URS_NORM, URS_COEF, URS_NONFINITE = range(7)

_lib = None


def lib_path():
    return _LIB_PATH


def lib():
    """Load the shared library (fails loudly: the HIP extension IS the product path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(
                f"{_LIB_PATH} not found — build it with `python lidar-nerf_amd/build.py` "
                "(hipcc --offload-arch=gfx950); there is no CPU fallback.")
        L = C.CDLL(_LIB_PATH)
        for name, sig in _SIGS.items():
            if name in _OPTIONAL and not hasattr(L, name):
                continue
            fn = getattr(L, name)
            fn.argtypes = sig + [P]
            fn.restype = C.c_int
        for fn in (L.lnh_grid_backward_workspace_size, L.lnh_grid_backward_workspace_size_min):
            fn.argtypes, fn.restype = [P, U32, U32, U32, U32, F32, U32, U32, I32, I32], C.c_uint64
        L.lnh_grid_backward_workspace_clear_bytes.argtypes = [P, U32, U32, U32, U32, F32, U32, U32, I32, U32, I32, C.c_uint64]
        L.lnh_grid_backward_workspace_clear_bytes.restype = C.c_uint64
        L.lnh_grid_backward_plan_info.argtypes = [P, U32, U32, U32, U32, F32, U32, U32, I32, I32, U32, P]
        L.lnh_grid_backward_plan_info.restype = C.c_int
        L.lnh_grid_backward_set_slice_entries.argtypes = [U32]
        L.lnh_grid_backward_set_slice_entries.restype = None
        if hasattr(L, "lnh_grid_forward_set_schedule"):
            L.lnh_grid_forward_set_schedule.argtypes = [U32, U32]
            L.lnh_grid_forward_set_schedule.restype = None
        L.lnh_wgrad_workspace_bytes.argtypes = []
        L.lnh_wgrad_workspace_bytes.restype = C.c_uint64
        L.lnh_lidar_loss_ex_workspace_bytes.argtypes = [U32]
        L.lnh_lidar_loss_ex_workspace_bytes.restype = C.c_uint64
        if hasattr(L, "lnh_lidar_eval_workspace_bytes"):
            L.lnh_lidar_eval_workspace_bytes.argtypes = [U32, U32]
            L.lnh_lidar_eval_workspace_bytes.restype = C.c_uint64
        if hasattr(L, "lnh_eval_points_workspace_bytes"):
            L.lnh_eval_points_workspace_bytes.argtypes = [U32, U32]
            L.lnh_eval_points_workspace_bytes.restype = C.c_uint64
        if hasattr(L, "lnh_nvs_eval_workspace_bytes"):
            L.lnh_nvs_eval_workspace_bytes.argtypes = [U32, U32]
            L.lnh_nvs_eval_workspace_bytes.restype = C.c_uint64
        if hasattr(L, "lnh_lidar_to_pano_fpa_workspace_size"):
            L.lnh_lidar_to_pano_fpa_workspace_size.argtypes = [C.c_uint64, U32, U32]
            L.lnh_lidar_to_pano_fpa_workspace_size.restype = C.c_uint64
        if hasattr(L, "lnh_marching_cubes_workspace_size"):
            L.lnh_marching_cubes_workspace_size.argtypes = [U32, U32, U32]
            L.lnh_marching_cubes_workspace_size.restype = C.c_uint64
        if hasattr(L, "lnh_mesh_filter_workspace_size"):
            L.lnh_mesh_filter_workspace_size.argtypes = [U32, U32]
            L.lnh_mesh_filter_workspace_size.restype = C.c_uint64
        if hasattr(L, "lnh_raycast_workspace_size"):
            L.lnh_raycast_workspace_size.argtypes = [U32, U32, U32, U32, U32, C.c_uint64]
            L.lnh_raycast_workspace_size.restype = C.c_uint64
        if hasattr(L, "lnh_knn_workspace_size"):
            L.lnh_knn_workspace_size.argtypes = [U32, U32, U32, U32]
            L.lnh_knn_workspace_size.restype = C.c_uint64
        if hasattr(L, "lnh_raydrop_workspace_size"):
            L.lnh_raydrop_workspace_size.argtypes = [U32, U32, U32]
            L.lnh_raydrop_workspace_size.restype = C.c_uint64
            L.lnh_raydrop_param_count.argtypes = [U32, U32]
            L.lnh_raydrop_param_count.restype = C.c_uint64
        if hasattr(L, "lnh_unet_workspace_size"):
            L.lnh_unet_workspace_size.argtypes = [U32, U32, U32]
            L.lnh_unet_workspace_size.restype = C.c_uint64
        if hasattr(L, "lnh_unet_head_backward_workspace_size"):
            L.lnh_unet_head_backward_workspace_size.argtypes = [U32, U32, U32]
            L.lnh_unet_head_backward_workspace_size.restype = C.c_uint64
        if hasattr(L, "lnh_unet_upconv2x2_backward_weight_workspace_size"):
            L.lnh_unet_upconv2x2_backward_weight_workspace_size.argtypes = [U32, U32, U32, U32, U32]
            L.lnh_unet_upconv2x2_backward_weight_workspace_size.restype = C.c_uint64
        for name in ("lnh_unet_bn_stats_workspace_size", "lnh_unet_bn_relu_backward_workspace_size"):
            if hasattr(L, name):
                getattr(L, name).argtypes, getattr(L, name).restype = [C.c_uint64, U32], C.c_uint64
        if hasattr(L, "lnh_unet_conv3x3_backward_weight_workspace_size"):
            L.lnh_unet_conv3x3_backward_weight_workspace_size.argtypes = [U32] * 7
            L.lnh_unet_conv3x3_backward_weight_workspace_size.restype = C.c_uint64
        if hasattr(L, "lnh_unet_loss_grad_workspace_size"):
            L.lnh_unet_loss_grad_workspace_size.argtypes, L.lnh_unet_loss_grad_workspace_size.restype = [C.c_uint64], C.c_uint64
        if hasattr(L, "lnh_unet_grad_sumsq_workspace_size"):
            L.lnh_unet_grad_sumsq_workspace_size.argtypes, L.lnh_unet_grad_sumsq_workspace_size.restype = [], C.c_uint64
        L.lnh_last_error.restype = C.c_char_p
        L.lnh_arch.restype = C.c_char_p
        L.lnh_build_variant.restype = C.c_char_p
        L.lnh_version.restype = C.c_int
        # A library that is not the product build (tools/probe_variants.py: phases compiled out, fake cursors, ...) gives
        # WRONG results by construction; LNH_LIB_PATH may point at one only together with LNH_ALLOW_VARIANT=1.
        tag = L.lnh_build_variant().decode()
        if tag != "product" and os.environ.get("LNH_ALLOW_VARIANT") != "1":
            raise RuntimeError(f"{_LIB_PATH} is the timing-probe build '{tag}', not the product library "
                               "(set LNH_ALLOW_VARIANT=1 to time it; its results are wrong by construction)")
        _lib = L
    return _lib


GRIDTYPE_TCNN = 2  # hash on tiny-cuda-nn's lattice (include/lidarnerf_hip.h, lnh_grid_encode_forward)
_GRIDTYPE_MIN_VERSION = {GRIDTYPE_TCNN: 101}
_gridtype_ok = set()


def require_gridtype(gridtype):
    """Refuse a grid type the loaded library predates (gridtype 2 needs lnh_version() >= 101): an older library would
    return LNH_ERR_INVALID_ARG at best, index with the wrong lattice at worst."""
    if gridtype in _gridtype_ok:
        return
    need = _GRIDTYPE_MIN_VERSION.get(gridtype, 100)
    have = lib().lnh_version()
    if have < need:
        raise RuntimeError(f"{_LIB_PATH} reports lnh_version() {have}; gridtype {gridtype} (tiny-cuda-nn lattice) needs "
                           f"{need} or later — rebuild the library (python lidar-nerf_amd/build.py)")
    _gridtype_ok.add(gridtype)


_version_ok = set()


def require_version(need, what):
    """Refuse a feature the loaded library predates (an older library lacks the entry point, or would misread it)."""
    if need in _version_ok:
        return
    have = lib().lnh_version()
    if have < need:
        raise RuntimeError(f"{_LIB_PATH} reports lnh_version() {have}; {what} needs {need} or later — rebuild the library "
                           "(python lidar-nerf_amd/build.py)")
    _version_ok.add(need)


def require_symbols(names, what):
    """Refuse a feature whose entry points the loaded library lacks (they were added without a new lnh_version())."""
    L = lib()
    missing = [n for n in names if not hasattr(L, n)]
    if missing:
        raise RuntimeError(f"{_LIB_PATH} does not export {', '.join(missing)}; {what} needs them — rebuild the library "
                           "(python lidar-nerf_amd/build.py)")


# lnh_lidar_eval_* (include/lidarnerf_hip.h): masking rule, row layout
EVAL_MODES = {"eval": 0, "test": 1}
EVAL_SLOT_NAMES = ("loss", "loss_depth", "loss_raydrop", "loss_intensity", "mae", "rmse", "depth_rmse", "a1", "a2", "a3",
                   "ssim", "masked", "crop_r0", "crop_c0", "crop_h", "crop_w", "valid", "data_range", "frames", "bad")
EVAL_SLOTS = len(EVAL_SLOT_NAMES)
# lnh_eval_points_* (include/lidarnerf_hip.h, LNH_PTS_*): row layout of the fused points meter
PTS_SLOT_NAMES = ("chamfer", "fscore", "precision", "recall", "mean_pred", "mean_gt", "count_pred", "count_gt", "frames",
                  "bad")
PTS_SLOTS = len(PTS_SLOT_NAMES)
# lnh_nvs_eval_* (include/lidarnerf_hip.h, LNH_NVS_*): row layout of the NVS baselines' meters; the first eight are the keys of
# the reference's eval_points_and_pano
NVS_SLOT_NAMES = ("depth_rmse", "depth_a1", "depth_a2", "depth_a3", "depth_ssim", "intensity_mae", "chamfer", "f_score",
                  "crop_r0", "crop_c0", "crop_h", "crop_w", "n", "data_range", "sum_sq", "sum_abs", "frames", "bad")
NVS_SLOTS = len(NVS_SLOT_NAMES)
NVS_METRICS = NVS_SLOT_NAMES[:8]


# lnh_lidar_loss_options (include/lidarnerf_hip.h): criterion codes, flags, the struct
LOSS_CODES = {"l1": 0, "mse": 1, "huber": 2, "bce": 3, "cos": 4}
LOSS_SOBEL, LOSS_GRAD, LOSS_GRAD_NORM_SMOOTH, LOSS_SPATIAL, LOSS_TV = 1, 2, 4, 8, 16


class LidarLossOptionsC(C.Structure):
    _fields_ = [("depth_loss", C.c_int32), ("raydrop_loss", C.c_int32), ("intensity_loss", C.c_int32),
                ("grad_loss", C.c_int32), ("flags", C.c_uint32), ("px", C.c_uint32), ("py", C.c_uint32),
                ("scale", C.c_float), ("huber_delta", C.c_float), ("alpha_d", C.c_float), ("alpha_r", C.c_float),
                ("alpha_i", C.c_float), ("alpha_grad", C.c_float), ("alpha_grad_norm", C.c_float),
                ("alpha_spatial", C.c_float), ("alpha_tv", C.c_float)]


def loss_options(o, px, py, scale, huber_delta, alpha_d, alpha_r, alpha_i, alpha_grad):
    """The C struct of a nerf.loss.LidarLossOptions for one call."""
    flags = ((LOSS_SOBEL if o.sobel_grad else 0) | (LOSS_GRAD if o.grad_loss else 0) |
             (LOSS_GRAD_NORM_SMOOTH if o.grad_norm_smooth else 0) | (LOSS_SPATIAL if o.spatial_smooth else 0) |
             (LOSS_TV if o.tv_loss else 0))
    return LidarLossOptionsC(LOSS_CODES[o.depth_loss], LOSS_CODES[o.raydrop_loss], LOSS_CODES[o.intensity_loss],
                             LOSS_CODES[o.depth_grad_loss], flags, int(px), int(py), float(scale), float(huber_delta),
                             float(alpha_d), float(alpha_r), float(alpha_i), float(alpha_grad), o.alpha_grad_norm,
                             o.alpha_spatial, o.alpha_tv)


def ptr(t):
    """Device (or host) pointer of a tensor, None -> NULL."""
    if t is None:
        return None
    return t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream():
    """hipStream_t of torch's current stream on the current device.  (torch.cuda.current_stream() builds a Stream object
    per call: 9 us of host time, ~45 times per training step — the occupancy-grid step of BASELINE config 4 was host-bound on
    it; the raw-handle accessor torch itself uses costs a fraction of a microsecond.)"""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


# Optional per-entry-point HIP-event timing (bench.py): TIMERS[name] = [(start_event, end_event, tag), ...].
# Events are recorded on the stream the kernel is launched on (torch's current stream).
TIMERS = None


def enable_timers(names=None):
    """Start collecting HIP events around calls (all entry points, or only `names`)."""
    global TIMERS, _TIMED
    TIMERS, _TIMED = {}, (set(names) if names else None)


def disable_timers():
    global TIMERS
    t, TIMERS = TIMERS, None
    return t


_TIMED = None


def call(name, *args, tag=None, timer=None):
    """Invoke an entry point on the current stream; raise on any non-zero status.  `timer`: the name the optional HIP-event
    timing files this call under (an entry point that serves several roles, e.g. lnh_grid_encode_backward_ws_ex)."""
    L = _lib if _lib is not None else lib()
    tname = timer or name
    timed = TIMERS is not None and (_TIMED is None or tname in _TIMED)
    if timed:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    rc = getattr(L, name)(*args, stream())
    if timed:
        e1.record()
        TIMERS.setdefault(tname, []).append((e0, e1, tag))
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc}): {L.lnh_last_error().decode()}")


def zero_regions(tensors):
    """Clear up to 8 device tensors with ONE launch (lnh_zero_regions; zero fills are kernels, never memset nodes)."""
    ts = [t for t in tensors if t is not None and t.numel()]
    if not ts:
        return
    for t in ts:
        if not (t.is_cuda and t.is_contiguous()):
            raise RuntimeError("lidarnerf_hip: zero_regions needs contiguous GPU tensors")
    ptrs = (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    sizes = (C.c_uint64 * len(ts))(*[t.numel() * t.element_size() for t in ts])
    call("lnh_zero_regions", C.cast(ptrs, C.c_void_p), C.cast(sizes, C.c_void_p), len(ts))


_WGRAD_WS = {}


def wgrad_ws(device):
    """(pointer, bytes) of the weight-gradient workspace of `device` for the MLP backward entry points (include/
    lidarnerf_hip.h, lnh_wgrad_workspace_bytes): allocated once per device and kept for the life of the process —
    a captured step keeps its address.  The backward launches of a process use it one after the other (one training stream
    per device, as everywhere in this package); a caller that runs backward passes on several streams of one device at the
    same time must hand each its own workspace."""
    dev = torch.device(device)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    t = _WGRAD_WS.get(key)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("lidarnerf_hip: the weight-gradient workspace must exist before a step is captured "
                               "(run one step eagerly first)")
        t = _WGRAD_WS[key] = torch.empty(int(lib().lnh_wgrad_workspace_bytes()), dtype=torch.uint8,
                                         device=torch.device("cuda", key))
    return t.data_ptr(), t.numel()


def ptr_array(values):
    """Host array of device pointers (None -> NULL) for the entry points that take `T *const *`; keep the returned object
    alive until the call has returned."""
    return (C.c_void_p * max(len(values), 1))(*[(v if v else None) for v in values])


def u32_array(values):
    return (C.c_uint32 * max(len(values), 1))(*[int(v) for v in values])


# indices into the optimizer's device-side scalar buffer (include/lidarnerf_hip.h LNH_TS_*)
TS_SCALE, TS_GROWTH, TS_FOUND, TS_INV, TS_INV_TABLE, TS_LAST_SCALE, TS_T, TS_IT, TS_LR, TS_T_NEXT, TS_IT_NEXT, TS_SKIPPED = range(12)
TRAIN_STATE_FLOATS, TRAIN_MAX_SMALL = 16, 16


def mlp_suffix(dt):
    """Entry-point suffix of the MLP kernels for a torch element type (fp16 build: '', bf16 build: '_bf16')."""
    if dt == torch.float16:
        return ""
    if dt == torch.bfloat16:
        return "_bf16"
    raise RuntimeError(f"lidarnerf_hip: unsupported MLP element type {dt} (float16 / bfloat16)")


def dtype_code(dt):
    if dt == torch.float32:
        return LNH_F32
    if dt == torch.float16:
        return LNH_F16
    raise RuntimeError(f"lidarnerf_hip: unsupported table dtype {dt} (float32 / float16 only)")


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("lidarnerf_hip: tensor must live on the GPU (no CPU path in this library)")
        if t is not None and not t.is_contiguous():
            raise RuntimeError("lidarnerf_hip: tensor must be contiguous")
