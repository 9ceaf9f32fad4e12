"""ctypes binding of libgarmentnets_hip.so (C ABI: include/garmentnets_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C garmentnets_amd/csrc``.  There is NO CPU
fallback: if the shared object is missing or a call fails, an exception is raised.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# GARMENTNETS_HIP_LIB: another build of the same C ABI (deployment layouts; A/B runs of two builds in two processes)
LIB_PATH = os.environ.get("GARMENTNETS_HIP_LIB") or os.path.join(_HERE, "libgarmentnets_hip.so")

GN_OK, GN_EINVAL, GN_ELAUNCH, GN_ECAP = 0, -1, -2, -3

_vp, _i32, _i64, _f32, _f64, _sz = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double,
                                   ctypes.c_size_t)

# name -> argtypes (every function returns int unless listed in _RESTYPES)
PROTOTYPES = {
    "gn_version": [],
    "gn_device_info": [_vp, _vp],
    "gn_segment_ptr": [_vp, _i64, _i32, _vp, _vp],
    "gn_fps": [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp],
    "gn_fps_nested": [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp],
    "gn_fps_workspace_bytes": [_i32, _i32],
    "gn_fps_nested_ws": [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _sz, _vp],
    "gn_ball_query": [_vp, _vp, _vp, _vp, _i32, _i32, _f32, _i32, _vp, _vp, _vp],
    "gn_sa_gather": [_vp, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp],
    "gn_segment_max": [_vp, _i32, _vp, _i32, _i32, _i32, _vp, _i32, _vp],
    "gn_sa_fused_supported": [_i32, _i32, _i32, _i32],
    "gn_sa_fused": [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp],
    "gn_sa_fused_scoped": [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp],
    "gn_sa_fused_group": [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _i32],
    "gn_sa_fused_auto_group": [_i32, _i32, _i32, _i32, _i32],
    "gn_sa_gather_scoped": [_vp, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp],
    "gn_global_max_pool": [_vp, _i32, _vp, _i32, _i32, _vp, _i32, _vp],
    "gn_knn_interpolate": [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp],
    "gn_knn_interpolate_any": [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp],
    "gn_linear": [_vp, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _i64, _i32, _i32, _vp, _i32, _vp],
    "gn_nocs_head": [_vp, _i32, _i64, _i32, _vp, _vp, _vp, _vp],
    "gn_grid_features": [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp],
    "gn_grid_scatter_workspace_bytes": [_i64, _i32, _i32],
    "gn_grid_scatter": [_vp, _i32, _vp, _i64, _i32, _i64, _i32, _vp, _vp, _vp, _sz, _i32, _vp],
    "gn_grid_scatter_ex": [_vp, _i32, _vp, _i64, _i32, _i32, _i64, _i32, _vp, _vp, _vp, _sz, _i32, _vp],
    "gn_channel_stats": [_vp, _i32, _i64, _i32, _vp, _vp, _vp],
    "gn_groupnorm_affine": [_vp, _vp, _i32, _i64, _vp, _vp, _i32, _i64, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _vp],
    "gn_channel_stats_any": [_vp, _i32, _i64, _i32, _vp, _vp, _vp],
    "gn_groupnorm_affine_map": [_vp, _vp, _i32, _i32, _i64, _vp, _vp, _i32, _i32, _i64, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _vp],
    "gn_conv3d_gcr": [_vp, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp],
    "gn_conv3d_gcr_split": [_vp, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _sz, _vp],
    "gn_conv3d_occupancy_workspace_bytes": [_i32, _i32, _i32, _i32],
    "gn_conv_affine_pack_bytes": [_i32, _i32, _i32],
    "gn_conv_affine_pack_workspace_bytes": [_i32, _i32, _i32],
    "gn_conv_affine_pack": [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _i64, _vp, _i32, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    "gn_conv3d_gcr_split_persample": [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _sz, _vp],
    "gn_conv_affine_pack_wino_bytes": [_i32, _i32, _i32],
    "gn_conv_affine_pack_wino": [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _i64, _vp, _i32, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    "gn_conv3d_gcr_split_wino": [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _sz, _vp],
    "gn_conv3d_gcr_split_wino_partial": [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp],
    "gn_weight_pack_split_bytes": [_i32, _i32, _i32],
    "gn_weight_pack_split_wino_bytes": [_i32, _i32],
    "gn_weight_pack_upconv_bytes": [_i32, _i32],
    "gn_weight_pack_split": [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _sz, _vp, _vp],
    "gn_weight_pack_split_wino": [_vp, _i32, _i32, _i32, _i32, _vp, _sz, _vp, _vp],
    "gn_weight_pack_upconv": [_vp, _i32, _i32, _i32, _i32, _vp, _sz, _vp, _vp],
    "gn_affine_act": [_vp, _i32, _i64, _i32, _vp, _vp, _vp, _i32, _vp, _vp],
    "gn_upconv_partial": [_vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp],
    "gn_grid_tile_flags": [_vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp],
    "gn_maxpool3d_2": [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp],
    "gn_grid_stats": [_vp, _vp, _i64, _i32, _i64, _i32, _vp, _vp, _vp, _vp],
    "gn_trilinear_sample": [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _i64, _i64, _vp, _i32, _vp],
    "gn_trilinear_sample_batch": [_vp, _i32, _i64, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _i32, _vp],
    "gn_implicit_decode": [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _i64, _i64, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32,
                           _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp],
    "gn_ggm3d": [_vp, _i32, _i32, _i32, _f64, _vp, _vp, _vp],
    "gn_minmax": [_vp, _i64, _vp, _vp],
    "gn_ggm3d_batch": [_vp, _i32, _i32, _i32, _i32, _f64, _vp, _vp, _vp],
    "gn_ggm3d_range_workspace_bytes": [_i32, _i32, _i32, _i32],
    "gn_ggm3d_batch_ex": [_vp, _i32, _i32, _i32, _i32, _f64, _vp, _vp, _i32, _vp, _vp, _sz, _vp],
    "gn_minmax_batch": [_vp, _i32, _i64, _vp, _vp],
    "gn_mc33_batch_workspace_bytes": [_i32, _i32, _i32, _i32],
    "gn_mc33_batch": [_vp, _i32, _i32, _i32, _i32, _f64, _vp, _sz, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp],
    "gn_mc33_batch_profiled": [_vp, _i32, _i32, _i32, _i32, _f64, _vp, _sz, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp],
    "gn_mc33_workspace_bytes": [_i32, _i32, _i32],
    "gn_mc33": [_vp, _i32, _i32, _i32, _f64, _vp, _sz, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp],
    "gn_gather_nn": [_vp, _i32, _i32, _i32, _vp, _i64, _f64, _vp, _vp],
    "gn_gather_nn_batch": [_vp, _i32, _i32, _i32, _i32, _vp, _i64, _f64, _vp, _vp],
    "gn_mesh_compact_workspace_bytes": [_i64, _i64],
    "gn_mesh_largest_component_workspace_bytes": [_i64],
    "gn_mesh_largest_component": [_vp, _i64, _i64, _vp, _sz, _vp, _vp, _vp, _vp],
    "gn_mesh_compact": [_vp, _i32, _vp, _vp, _i64, _i64, _vp, _sz, _vp, _vp, _vp, _vp],
    "gn_scale_verts": [_vp, _i64, _f64, _vp, _vp],
    "gn_implicit_decode_split": [_vp, _i32, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp],
    "gn_implicit_decode_split_batch": [_vp, _i32, _i64, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp],
    "gn_implicit_decode_batch": [_vp, _i32, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _i32, _vp],
    "gn_implicit_decode_lattice_split": [_vp, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp],
    "gn_decoder_input_scale": [_vp, _i64, _i32, _i32, _f32, _vp, _vp],
    "gn_nearest_neighbor": [_vp, _i64, _vp, _i64, _vp, _vp, _vp],
    "gn_nearest_neighbor_f64_batch": [_vp, _vp, _vp, _i32, _i64, _vp, _vp, _vp],
    "gn_point_mesh_sqdist_batch": [_vp, _vp, _vp, _vp, _i32, _i64, _vp, _vp, _vp, _vp],
    "gn_winding_number_batch": [_vp, _vp, _vp, _vp, _i32, _i64, _vp, _vp, _vp],
    "gn_winding_field_batch": [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp],
    "gn_distance_field_batch": [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp],
    "gn_query_targets_face_chunk": [],
    "gn_query_targets_workspace_bytes": [_i32, _i64, _i64, _i32],
    "gn_query_targets_batch": [_vp, _vp, _vp, _vp, _i32, _i64, _i64, _i32, _i32, _f32, _i32, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp],
    "gn_nocs_bin_metrics_workspace_bytes": [_vp, _i32],
    "gn_nocs_bin_metrics": [_vp, _i32, _i32, _i32, _vp, _sz, _vp, _vp],
    "gn_value_losses_workspace_bytes": [_vp, _i32],
    "gn_value_losses": [_vp, _i32, _vp, _sz, _vp, _vp],
    "gn_nocs_bin_loss_bwd": [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp],
    "gn_value_losses_bwd": [_vp, _i32, _vp, _vp, _vp],
    "gn_adam_step": [_vp, _i32, _i64, _vp, _i32, _vp],
    "gn_grad_pack": [_vp, _i32, _i64, _vp, _i64, _i32, _vp],
    "gn_grid_scatter_bwd_workspace_bytes": [_i64, _i32, _i64, _i32],
    "gn_grid_scatter_bwd": [_vp, _vp, _vp, _i32, _vp, _i64, _i32, _i32, _i64, _i32, _vp, _sz, _vp, _i32, _vp],
    "gn_segment_max_bwd": [_vp, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _i32, _vp],
    "gn_global_max_pool_bwd": [_vp, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _vp, _i32, _vp],
    "gn_sa_gather_bwd_workspace_bytes": [_i64, _i64],
    "gn_sa_gather_bwd": [_vp, _i32, _vp, _i64, _i32, _i64, _vp, _sz, _vp, _i32, _vp],
    "gn_knn_neighbours": [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp],
    "gn_knn_interpolate_bwd_workspace_bytes": [_i64, _i32, _i64],
    "gn_knn_interpolate_bwd": [_vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _vp, _sz, _vp, _i32, _vp],
    "gn_trilinear_sample_bwd_workspace_bytes": [_i32, _i64, _i32, _i32, _i32],
    "gn_trilinear_sample_bwd": [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _sz, _vp, _vp, _vp],
    "gn_conv3d_bwd_weight_workspace_bytes": [_i32, _i32, _i32, _i32, _i32, _i32],
    "gn_conv3d_bwd_weight": [_vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _sz, _vp, _vp],
    "gn_relu_mask": [_vp, _vp, _i64, _vp, _vp],
    "gn_relu_mask_max_workspace_bytes": [_i32],
    "gn_relu_mask_max": [_vp, _vp, _i32, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    "gn_conv3d_bwd_weight_split_workspace_bytes": [_i32, _i32, _i32, _i32, _i32, _i32],
    "gn_conv3d_bwd_weight_split": [_vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _sz, _vp, _vp],
    "gn_groupnorm_bwd_stats_workspace_bytes": [_i32, _i64, _i32],
    "gn_groupnorm_bwd_stats": [_vp, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _sz, _vp, _vp, _vp],
    "gn_groupnorm_bwd_coef": [_vp, _vp, _vp, _vp, _i32, _i32, _i64, _vp, _vp, _vp, _vp, _i32, _i32, _i64, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp,
                              _vp, _vp],
    "gn_groupnorm_bwd_apply": [_vp, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp],
    "gn_maxpool3d_2_bwd": [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp],
    "gn_linear_act_bwd_workspace_bytes": [_i64, _i32],
    "gn_linear_act_bwd": [_vp, _i32, _vp, _i32, _vp, _i64, _i32, _vp, _i32, _vp, _sz, _vp, _vp],
    "gn_linear_bwd_weight_workspace_bytes": [_i64, _i32, _i32],
    "gn_linear_bwd_weight": [_vp, _i32, _vp, _i32, _i64, _i32, _i32, _vp, _sz, _vp, _i32, _vp],
    "gn_row_affine": [_vp, _i32, _vp, _vp, _i64, _i32, _vp, _i32, _vp],
    "gn_col_moments_workspace_bytes": [_i64, _i32],
    "gn_col_moments": [_vp, _i32, _i64, _i32, _vp, _sz, _vp, _vp],
    "gn_col_dots_workspace_bytes": [_i64, _i32],
    "gn_col_dots": [_vp, _i32, _vp, _i32, _i64, _i32, _vp, _sz, _vp, _vp],
    "gn_bn_train_bwd_workspace_bytes": [_i64, _i32],
    "gn_bn_train_bwd": [_vp, _i32, _vp, _i32, _vp, _i64, _i32, _vp, _i32, _vp, _sz, _vp, _vp],
    "gn_resident_points": [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "gn_resident_garment": [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "gn_resident_volume": [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp],
    "gn_resident_volume_queries": [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "gn_resident_query_targets": [_vp, _vp, _i32, _i64, _i32, _i64, _i64, _i32, _i32, _f32, _i32, _vp, _vp, _sz, _vp, _vp, _vp],
    "gn_resident_surface": [_vp, _vp, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp],
    "gn_resident_mc_surface": [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp],
    "gn_render_points_batch": [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp],
    "gn_color_idx_batch": [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp],
    "gn_render_mesh_batch": [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp],
    "gn_color_mesh_batch": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp],
    "gn_depth_render_batch": [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _vp],
    "gn_depth_cloud_offsets": [_vp, _i32, _i32, _vp, _vp, _vp],
    "gn_depth_cloud_write": [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i64, _vp, _vp, _vp, _vp],
    "gn_cloth_simulate_batch": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i64, _i64, _i32, _vp, _i32, _i32, _vp, _vp],
    "gn_cloth_contact_buckets": [_i32],
    "gn_cloth_contact_workspace_bytes": [_i64, _i32, _i32],
    "gn_cloth_contact_lists": [_vp, _vp, _vp, _i32, _i64, _i32, _i32, _vp, _i32, _i32, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp],
    "gn_cloth_simulate_contacts_batch": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i64, _i64, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp,
                                         _i32, _vp, _vp, _vp, _vp],
    "gn_cloth_face_contact_lists": [_vp, _vp, _vp, _vp, _vp, _i32, _i64, _i64, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64,
                                    _vp, _vp, _i64, _vp, _i64, _vp, _vp],
    "gn_cloth_simulate_face_contacts_batch": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i64, _i64, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp,
                                              _i32, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _i32, _vp, _vp, _i64, _vp],
}
_RESTYPES = {"gn_weight_pack_split_bytes": _sz, "gn_weight_pack_split_wino_bytes": _sz, "gn_weight_pack_upconv_bytes": _sz,
             "gn_conv_affine_pack_bytes": _sz, "gn_conv_affine_pack_workspace_bytes": _sz, "gn_conv_affine_pack_wino_bytes": _sz, "gn_conv3d_occupancy_workspace_bytes": _sz, "gn_mc33_workspace_bytes": _sz, "gn_ggm3d_range_workspace_bytes": _sz, "gn_mc33_batch_workspace_bytes": _sz, "gn_grid_scatter_workspace_bytes": _sz, "gn_fps_workspace_bytes": _sz, "gn_mesh_compact_workspace_bytes": _sz, "gn_mesh_largest_component_workspace_bytes": _sz,
             "gn_nocs_bin_metrics_workspace_bytes": _sz, "gn_value_losses_workspace_bytes": _sz,
             "gn_grid_scatter_bwd_workspace_bytes": _sz, "gn_sa_gather_bwd_workspace_bytes": _sz, "gn_knn_interpolate_bwd_workspace_bytes": _sz,
             "gn_trilinear_sample_bwd_workspace_bytes": _sz, "gn_conv3d_bwd_weight_workspace_bytes": _sz, "gn_conv3d_bwd_weight_split_workspace_bytes": _sz, "gn_relu_mask_max_workspace_bytes": _sz, "gn_groupnorm_bwd_stats_workspace_bytes": _sz,
             "gn_linear_act_bwd_workspace_bytes": _sz, "gn_linear_bwd_weight_workspace_bytes": _sz,
             "gn_col_moments_workspace_bytes": _sz, "gn_col_dots_workspace_bytes": _sz, "gn_bn_train_bwd_workspace_bytes": _sz,
             "gn_query_targets_workspace_bytes": _sz, "gn_cloth_contact_workspace_bytes": _sz}

LINEAR_BWD_CHUNK_ROWS = 512                     # GN_LINEAR_BWD_CHUNK_ROWS
LINEAR_ACT_CHUNK_ROWS = 1024                    # GN_LINEAR_ACT_CHUNK_ROWS (gn_linear_act_bwd, gn_col_moments, gn_col_dots, gn_bn_train_bwd)

LOSS_MAX_SETS = 8                               # GN_LOSS_MAX_SETS
LOSS_KINDS = {"l2": 0, "smooth_l1": 1, "bce_logits": 2, "row_norm": 3}


class NocsBinSet(ctypes.Structure):
    """GnNocsBinSet (host table entry of gn_nocs_bin_metrics)"""
    _fields_ = [("logits", _vp), ("gt", _vp), ("n", _i64), ("ldl", _i32), ("pad", _i32)]


class LossSegment(ctypes.Structure):
    """GnLossSegment (host table entry of gn_value_losses)"""
    _fields_ = [("pred", _vp), ("target", _vp), ("count", _i64), ("kind", _i32), ("mirror", _i32)]


class NocsBinGradSet(ctypes.Structure):
    """GnNocsBinGradSet (host table entry of gn_nocs_bin_loss_bwd)"""
    _fields_ = [("logits", _vp), ("gt", _vp), ("grad", _vp), ("n", _i64), ("ldl", _i32), ("ldg", _i32), ("ncols", _i32), ("pad", _i32)]


class LossGradSegment(ctypes.Structure):
    """GnLossGradSegment (host table entry of gn_value_losses_bwd)"""
    _fields_ = [("pred", _vp), ("target", _vp), ("grad", _vp), ("count", _i64), ("coef", _f64), ("kind", _i32), ("mirror", _i32)]


QT_KINDS = {"nocs_winding_number_field": 0, "sim_nocs_winding_number_field": 0, "nocs_distance_field": 1, "nocs_signed_distance_field": 2,
            "nocs_occupancy_grid": 3}             # GN_QT_*: the dataset's volume_group -> the kind of gn_query_targets_batch

ADAM_CHUNK = 4096                               # GN_ADAM_CHUNK
ADAM_MAX_HYPER = 16                             # GN_ADAM_MAX_HYPER


class AdamEntry(ctypes.Structure):
    """GnAdamEntry (DEVICE table entry of gn_adam_step)"""
    _fields_ = [("p", _vp), ("g", _vp), ("exp_avg", _vp), ("exp_avg_sq", _vp), ("numel", _i64), ("blk0", _i64), ("hyper", _i32), ("pad", _i32)]


class PackEntry(ctypes.Structure):
    """GnPackEntry (DEVICE table entry of gn_grad_pack)"""
    _fields_ = [("src", _vp), ("dst_off", _i64), ("numel", _i64), ("blk0", _i64)]


class AdamHyper(ctypes.Structure):
    """GnAdamHyper (host scalars of gn_adam_step)"""
    _fields_ = [("lr", _f64), ("beta1", _f64), ("beta2", _f64), ("eps", _f64), ("weight_decay", _f64), ("bias_correction1", _f64),
                ("bias_correction2_sqrt", _f64)]


RESIDENT_META = ("pc_off", "pc_len", "vert_off", "face_off", "num_faces", "mc_vert_off", "mc_face_off", "num_mc_faces", "dataset_idx",
                 "scale_bits")                  # GN_RESIDENT_* : the int64 columns of GnResidentStore.meta
RESIDENT_ARRAYS = ("pc_sim", "pc_nocs", "pc_rgb", "sim_verts", "nocs_verts", "task_verts", "faces", "cdf_nocs", "cdf_task", "mc_verts", "mc_flags",
                   "mc_faces", "cdf_mc", "volume", "meta", "grip", "aabb")


class ResidentStore(ctypes.Structure):
    """GnResidentStore (host struct of the gn_resident_* calls: device pointers of the resident arrays, NULL for the ones a store does not hold)"""
    _fields_ = [(k, _vp) for k in RESIDENT_ARRAYS] + [("n", _i32), ("D", _i32), ("H", _i32), ("W", _i32)]


CLOTH_MAX_LDS = 160 * 1024                      # CL_MAX_LDS
CLOTH_MAX_BLOCK = 1024                          # CL_MAX_BLOCK
CLOTH_MAX_LIST = 64                             # CL_MAX_LIST
CLOTH_LISTS_TRAVEL, CLOTH_LISTS_BUILD = 1, 2    # CL_LISTS_*: the flags of gn_cloth_contact_lists
CLOTH_FACE_MAX_LIST = 32                        # CL_FACE_MAX_LIST
CLOTH_FACE_MAX_CHUNKS = 1024                    # CL_FACE_MAX_CHUNKS
CLOTH_FACE_BLOCK = 256                          # CL_FACE_BLOCK: vertices per workgroup of the face-list kernels

RENDER_MAX_SIZE = 4096                          # GN_RENDER_MAX_SIZE
RENDER_MAX_OVERLAYS = 3                         # GN_RENDER_MAX_OVERLAYS
RENDER_SIDES = {"front": 0, "top": 1, "left": 2}   # GN_RENDER_*
COLOR_TABLE, COLOR_VIRIDIS = 0, 1               # GN_COLOR_*


class OverlayPoint(ctypes.Structure):
    """GnOverlayPoint"""
    _fields_ = [("xyz", _f32 * 3), ("rgba", _f32 * 4), ("kernel_size", _i32)]


class ColorImage(ctypes.Structure):
    """GnColorImage (table entry of gn_color_idx_batch: the same bytes on the host and on the device)"""
    _fields_ = [("offset", _i64), ("count", _i64), ("mode", _i32), ("side", _i32), ("vmin", _f32), ("vmax", _f32), ("default_color", _f32 * 4),
                ("num_overlays", _i32), ("pad", _i32), ("overlay", OverlayPoint * RENDER_MAX_OVERLAYS)]


class MeshImage(ctypes.Structure):
    """GnMeshImage (table entry of gn_render_mesh_batch / gn_color_mesh_batch: the same bytes on the host and on the device)"""
    _fields_ = [("vert_begin", _i64), ("vert_end", _i64), ("face_begin", _i64), ("face_end", _i64), ("side", _i32), ("ambient", _f32),
                ("default_color", _f32 * 4)]


class DepthImage(ctypes.Structure):
    """GnDepthImage (table entry of gn_depth_render_batch / gn_depth_cloud_write: the same bytes on the host and on the device)"""
    _fields_ = [("vert_begin", _i64), ("vert_end", _i64), ("face_begin", _i64), ("face_end", _i64), ("R", _f64 * 9), ("t", _f64 * 3), ("f", _f64),
                ("c", _f64), ("znear", _f64), ("ambient", _f32), ("base_color", _f32 * 3)]


_lib = None


class GarmentNetsHipError(RuntimeError):
    pass


def load():
    """Load the shared library (once) and declare every prototype of include/garmentnets_hip.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GarmentNetsHipError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C garmentnets_amd/csrc`). garmentnets_amd has no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    lib.gn_last_error.restype = ctypes.c_char_p
    lib.gn_last_error.argtypes = []
    lib.gn_last_kernel.restype = ctypes.c_char_p
    lib.gn_last_kernel.argtypes = []
    for name, argtypes in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.argtypes = argtypes
        fn.restype = _RESTYPES.get(name, ctypes.c_int)
    _lib = lib
    return lib


def call(name, *args):
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != GN_OK:
        msg = lib.gn_last_error().decode(errors="replace")
        if rc == GN_EINVAL:
            raise ValueError(f"{name}: {msg}")
        raise GarmentNetsHipError(f"{name} failed (code {rc}): {msg}")
    return rc
