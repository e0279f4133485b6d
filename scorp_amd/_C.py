"""ctypes binding of libscorp_gs.so (C ABI in include/scorp_gs.h).

There is no CPU or PyTorch fallback: if the HIP library is missing or fails to load, importing the
rasterizer raises.  Build it with `python -m scorp_amd.build` (or __graft_entry__.build()).
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SCORP_GS_LIB", os.path.join(_HERE, "libscorp_gs.so"))   # override: A/B builds of the library

c_float_p = ctypes.c_void_p  # raw device pointers travel as integers


class ScorpGs3dInputs(ctypes.Structure):
    _fields_ = [
        ("num_gaussians", ctypes.c_int32), ("sh_degree", ctypes.c_int32), ("sh_coeffs", ctypes.c_int32),
        ("image_width", ctypes.c_int32), ("image_height", ctypes.c_int32),
        ("tanfovx", ctypes.c_float), ("tanfovy", ctypes.c_float), ("scale_modifier", ctypes.c_float),
        ("prefiltered", ctypes.c_int32), ("debug", ctypes.c_int32),
        ("bg", c_float_p), ("viewmatrix", c_float_p), ("projmatrix", c_float_p), ("campos", c_float_p),
        ("means3D", c_float_p), ("shs", c_float_p), ("colors_precomp", c_float_p), ("opacities", c_float_p),
        ("scales", c_float_p), ("rotations", c_float_p), ("cov3D_precomp", c_float_p),
        ("shs_rest", c_float_p), ("raw_params", ctypes.c_int32), ("num_views", ctypes.c_int32),
    ]


class ScorpGs3dGrads(ctypes.Structure):
    _fields_ = [(n, c_float_p) for n in ("means3D", "means2D", "shs", "colors_precomp", "opacities", "scales",
                                         "rotations", "cov3D_precomp", "shs_rest")]


class ScorpGs3dTrainView(ctypes.Structure):
    _fields_ = [("inputs", ctypes.c_void_p), ("out_radii", ctypes.c_void_p), ("state", ctypes.c_void_p),
                ("state_bytes", ctypes.c_size_t), ("pairs", ctypes.c_void_p), ("capacity", ctypes.c_uint64),
                ("out_color", ctypes.c_void_p), ("out_depth_raw", ctypes.c_void_p), ("out_alpha", ctypes.c_void_p),
                ("out_depth", ctypes.c_void_p), ("out_visible", ctypes.c_void_p), ("gt", ctypes.c_void_p),
                ("mask", ctypes.c_void_p), ("lambda_dssim", ctypes.c_float), ("backward_flags", ctypes.c_uint32),
                ("out_loss3", ctypes.c_void_p), ("loss_workspace", ctypes.c_void_p), ("loss_workspace_bytes", ctypes.c_size_t),
                ("grad_color", ctypes.c_void_p), ("grads", ctypes.c_void_p), ("backward_scratch", ctypes.c_void_p),
                ("backward_scratch_bytes", ctypes.c_size_t), ("out_header", ctypes.c_void_p), ("adam", ctypes.c_void_p)]


class ScorpGs3dViewTerms(ctypes.Structure):
    _fields_ = [("depth_sensor", ctypes.c_void_p), ("depth_est", ctypes.c_void_p), ("lambda_depth_sensor", ctypes.c_float),
                ("weight_depth_est", ctypes.c_float), ("lambda_isotropic", ctypes.c_float), ("_pad", ctypes.c_float),
                ("out_terms4", ctypes.c_void_p), ("grad_depth_raw", ctypes.c_void_p), ("grad_alpha", ctypes.c_void_p),
                ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t)]


class ScorpGs2dViewTerms(ctypes.Structure):
    _fields_ = [("depth_sensor", ctypes.c_void_p), ("depth_est", ctypes.c_void_p), ("lambda_depth_sensor", ctypes.c_float),
                ("weight_depth_est", ctypes.c_float), ("weight_depth_normal", ctypes.c_float), ("lambda_isotropic", ctypes.c_float),
                ("out_terms6", ctypes.c_void_p), ("out_depth", ctypes.c_void_p), ("grad_depth", ctypes.c_void_p),
                ("grad_normal", ctypes.c_void_p), ("workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t)]


class ScorpFusedAdam(ctypes.Structure):
    _fields_ = [("exp_avg", ctypes.c_void_p * 6), ("exp_avg_sq", ctypes.c_void_p * 6), ("lr", ctypes.c_float * 6),
                ("_pad", ctypes.c_float * 2), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double), ("eps", ctypes.c_double),
                ("step", ctypes.c_int32), ("_pad2", ctypes.c_int32), ("skipped_counter", ctypes.c_void_p),
                ("max_radii2D", ctypes.c_void_p), ("xyz_gradient_accum", ctypes.c_void_p), ("denom", ctypes.c_void_p)]


class ScorpGs2dTrainView(ctypes.Structure):
    _fields_ = [("inputs", ctypes.c_void_p), ("out_radii", ctypes.c_void_p), ("state", ctypes.c_void_p),
                ("state_bytes", ctypes.c_size_t), ("pairs", ctypes.c_void_p), ("capacity", ctypes.c_uint64),
                ("out_color", ctypes.c_void_p), ("out_allmap", ctypes.c_void_p), ("gt", ctypes.c_void_p),
                ("mask", ctypes.c_void_p), ("rays_d", ctypes.c_void_p), ("rays_o", ctypes.c_void_p),
                ("lambda_dssim", ctypes.c_float), ("depth_ratio", ctypes.c_float), ("lambda_normal", ctypes.c_float),
                ("lambda_dist", ctypes.c_float), ("out_loss3", ctypes.c_void_p), ("out_reg2", ctypes.c_void_p),
                ("loss_workspace", ctypes.c_void_p), ("loss_workspace_bytes", ctypes.c_size_t),
                ("reg_workspace", ctypes.c_void_p), ("reg_workspace_bytes", ctypes.c_size_t),
                ("grad_color", ctypes.c_void_p), ("grad_allmap", ctypes.c_void_p), ("grads", ctypes.c_void_p),
                ("backward_scratch", ctypes.c_void_p), ("backward_scratch_bytes", ctypes.c_size_t),
                ("backward_flags", ctypes.c_uint32), ("adam", ctypes.c_void_p)]


class ScorpTsdfViews(ctypes.Structure):
    _fields_ = [("depth", c_float_p), ("rgb", c_float_p), ("full_proj", c_float_p), ("num_views", ctypes.c_int32),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("_pad", ctypes.c_int32)]


class ScorpTsdfSamples(ctypes.Structure):
    _fields_ = [("xyz", c_float_p), ("x", c_float_p), ("y", c_float_p), ("z", c_float_p), ("nx", ctypes.c_int32),
                ("ny", ctypes.c_int32), ("nz", ctypes.c_int32), ("_pad", ctypes.c_int32), ("first", ctypes.c_uint64),
                ("count", ctypes.c_uint64)]


class ScorpTsdfParams(ctypes.Structure):
    _fields_ = [("voxel_size", ctypes.c_double), ("center", ctypes.c_float * 3), ("radius", ctypes.c_float),
                ("contracted", ctypes.c_int32), ("_pad", ctypes.c_int32)]


class ScorpTsdfBlockViews(ctypes.Structure):
    _fields_ = [("depth", c_float_p), ("rgb", ctypes.c_void_p), ("cam", c_float_p), ("num_views", ctypes.c_int32),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("_pad", ctypes.c_int32)]


class ScorpRowTensor(ctypes.Structure):
    _fields_ = [("src", c_float_p), ("dst", c_float_p), ("row_floats", ctypes.c_uint32), ("zero_if_fresh", ctypes.c_uint32)]


class ScorpAdamTensor(ctypes.Structure):
    _fields_ = [("param", c_float_p), ("grad", c_float_p), ("exp_avg", c_float_p), ("exp_avg_sq", c_float_p),
                ("numel", ctypes.c_uint64), ("lr", ctypes.c_float), ("_pad", ctypes.c_float)]


EXPORTS = [
    "scorp_version", "scorp_source_sha", "scorp_last_error", "scorp_gs3d_state_bytes", "scorp_gs3d_pairs_bytes",
    "scorp_gs3d_backward_scratch_bytes", "scorp_gs3d_backward_scratch_bytes_ex", "scorp_gs3d_preprocess", "scorp_gs3d_num_pairs", "scorp_gs3d_render",
    "scorp_gs3d_render_image", "scorp_gs3d_render_score",
    "scorp_gs3d_check_overflow", "scorp_gs3d_backward", "scorp_gs3d_backward_ex", "scorp_gs3d_debug_geom", "scorp_gs3d_debug_tiles", "scorp_gs3d_debug_work",
    "scorp_loss_workspace_bytes", "scorp_loss_l1_ssim_forward", "scorp_loss_l1_ssim_backward",
    "scorp_knn_dist2", "scorp_gaussians_transform", "scorp_adam_step", "scorp_adam_step_guarded", "scorp_adam_step_guarded_ex", "scorp_densification_stats", "scorp_densification_stats_ex", "scorp_gather_rows", "scorp_gs3d_render_tail", "scorp_gs3d_render_tail_backward",
    "scorp_gs3d_pose_score_accumulate",
    "scorp_gs2d_state_bytes", "scorp_gs2d_backward_scratch_bytes", "scorp_gs2d_preprocess", "scorp_gs2d_render",
    "scorp_gs2d_render_image", "scorp_gs2d_render_score",
    "scorp_gs2d_backward", "scorp_gs2d_backward_ex", "scorp_gs2d_backward_scratch_bytes_ex", "scorp_gs2d_debug_geom", "scorp_gs2d_debug_tiles", "scorp_gs2d_maps_forward",
    "scorp_gs2d_maps_backward", "scorp_gs2d_regularizers_workspace_bytes", "scorp_gs2d_regularizers_forward",
    "scorp_gs2d_regularizers_backward", "scorp_gs3d_train_view", "scorp_gs2d_train_view",
    "scorp_gs3d_view_terms_workspace_bytes", "scorp_gs3d_train_view_ex", "scorp_gs3d_depth_terms",
    "scorp_gs2d_view_terms_workspace_bytes", "scorp_gs2d_train_view_ex", "scorp_gs2d_surfel_terms",
    "scorp_prof_enable", "scorp_prof_select", "scorp_prof_num_kernels", "scorp_prof_kernel_name", "scorp_prof_collect",
    "scorp_mask_vote_scratch_bytes", "scorp_gs3d_mask_vote", "scorp_gs2d_mask_vote",
    "scorp_icp_workspace_bytes", "scorp_icp_point_to_point",
    "scorp_icp_point_to_plane_workspace_bytes", "scorp_icp_point_to_plane",
    "scorp_icp_generalized_workspace_bytes", "scorp_icp_generalized",
    "scorp_estimate_normals_workspace_bytes", "scorp_estimate_normals",
    "scorp_cloud_workspace_bytes", "scorp_cloud_knn_distance", "scorp_cloud_radius_count", "scorp_cloud_dbscan",
    "scorp_cloud_fpfh_workspace_bytes", "scorp_cloud_fpfh", "scorp_feature_match_tile_rows", "scorp_feature_match_split_rows",
    "scorp_feature_match_workspace_bytes", "scorp_feature_match",
    "scorp_cloud_orient_workspace_bytes", "scorp_cloud_orient_normals",
    "scorp_pose_fit_workspace_bytes", "scorp_pose_ransac", "scorp_pose_adam_9dof",
    "scorp_tsdf_fuse", "scorp_isosurface_count_cells", "scorp_isosurface_emit_vertices", "scorp_isosurface_count_faces",
    "scorp_isosurface_emit_faces",
    "scorp_mesh_cluster_link", "scorp_mesh_cluster_roots", "scorp_mesh_cluster_stats",
    "scorp_mesh_simplify_cells", "scorp_mesh_simplify_roots", "scorp_mesh_simplify_accumulate", "scorp_mesh_simplify_place",
    "scorp_mesh_simplify_faces",
    "scorp_mesh_decimate_quadrics", "scorp_mesh_decimate_flags", "scorp_mesh_decimate_candidates", "scorp_mesh_decimate_hash",
    "scorp_mesh_decimate_select", "scorp_mesh_decimate_apply", "scorp_mesh_decimate_faces",
    "scorp_mesh_distance_workspace_bytes", "scorp_mesh_distance_build", "scorp_mesh_distance_query", "scorp_mesh_sample_points",
    "scorp_nearest_point_workspace_bytes", "scorp_nearest_point_distance",
    "scorp_mesh_render_workspace_bytes", "scorp_mesh_render",
    "scorp_mesh_face_normals", "scorp_mesh_vertex_normals", "scorp_mesh_smooth", "scorp_mesh_normal_map",
    "scorp_tsdf_blocks_touch", "scorp_tsdf_blocks_neighbors", "scorp_tsdf_blocks_integrate",
    "scorp_isosurface_blocks_count_cells", "scorp_isosurface_blocks_emit_vertices", "scorp_isosurface_blocks_count_faces",
    "scorp_isosurface_blocks_emit_faces",
    "scorp_marching_cubes_count_edges", "scorp_marching_cubes_emit_vertices", "scorp_marching_cubes_count_faces",
    "scorp_marching_cubes_emit_faces",
    "scorp_marching_cubes_blocks_count_edges", "scorp_marching_cubes_blocks_emit_vertices", "scorp_marching_cubes_blocks_count_faces",
    "scorp_marching_cubes_blocks_emit_faces",
]

BACKWARD_EXACT_FP32 = 1   # scorp_gs3d_backward_ex flag (include/scorp_gs.h)
BACKWARD_SCRATCH_ZEROED = 2   # scorp_gs3d_backward_ex flag: the caller cleared the accumulator rows already
BACKWARD_DETERMINISTIC = 4    # scorp_gs3d_backward_ex flag: no float atomics (plain partial rows + an ordered per-Gaussian sum)
VOTE_SUMS, VOTE_GRADIENT, VOTE_BINARY = 0, 1, 2   # methods of scorp_gs3d_mask_vote / scorp_gs2d_mask_vote
POSE_UMEYAMA, POSE_KABSCH = 0, 1   # methods of scorp_pose_ransac
MESH_RENDER_CULL_BACKFACES = 1   # flag of scorp_mesh_render (include/scorp_gs.h)
MESH_NORMALS_AREA, MESH_NORMALS_UNIFORM = 0, 1   # weightings of scorp_mesh_vertex_normals
MESH_SMOOTH_UNIFORM, MESH_SMOOTH_INVERSE_DISTANCE = 0, 1   # weights of scorp_mesh_smooth
ORIENT_MAJORITY_AWAY, ORIENT_FIRST = 0, 1   # component_sign of scorp_cloud_orient_normals
ERR_INVALID, ERR_NO_INLIERS = -1, -4   # return codes the Python layer tells apart (include/scorp_gs.h)

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python -m scorp_amd.build` "
            "(needs /opt/rocm/bin/hipcc). scorp_amd has no CPU fallback.")
    # PyTorch-ROCm bundles its own libamdhip64; it must be the HIP runtime already in the process when this library
    # is loaded, or the kernels register with a second runtime that has no device ("no ROCm-capable device").
    import torch  # noqa: F401
    L = ctypes.CDLL(LIB_PATH)
    vp, u64, i32, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int32, ctypes.c_size_t
    L.scorp_version.restype = ctypes.c_int
    L.scorp_last_error.restype = ctypes.c_char_p
    L.scorp_source_sha.restype = ctypes.c_char_p
    L.scorp_gs3d_state_bytes.restype = sz
    L.scorp_gs3d_state_bytes.argtypes = [i32, i32, i32]
    L.scorp_gs3d_pairs_bytes.restype = sz
    L.scorp_gs3d_pairs_bytes.argtypes = [u64]
    L.scorp_gs3d_backward_scratch_bytes.restype = sz
    L.scorp_gs3d_backward_scratch_bytes.argtypes = [i32]
    L.scorp_gs3d_backward_scratch_bytes_ex.restype = sz
    L.scorp_gs3d_backward_scratch_bytes_ex.argtypes = [i32, i32, i32, u64, ctypes.c_uint32]
    L.scorp_gs3d_preprocess.argtypes = [ctypes.POINTER(ScorpGs3dInputs), vp, vp, sz, vp]
    L.scorp_gs3d_num_pairs.argtypes = [vp, vp, ctypes.POINTER(u64)]
    L.scorp_gs3d_render.argtypes = [ctypes.POINTER(ScorpGs3dInputs), vp, vp, u64, vp, vp, vp, vp]
    L.scorp_gs3d_render_image.argtypes = [ctypes.POINTER(ScorpGs3dInputs), vp, vp, u64, vp, vp, vp, vp]
    L.scorp_gs3d_render_score.argtypes = [ctypes.POINTER(ScorpGs3dInputs), vp, vp, u64, vp, vp, i32, ctypes.c_float, vp, vp]
    L.scorp_gs3d_check_overflow.argtypes = [vp, vp, ctypes.POINTER(u64)]
    L.scorp_gs3d_backward.argtypes = [ctypes.POINTER(ScorpGs3dInputs), vp, vp, u64, vp, vp, vp,
                                      ctypes.POINTER(ScorpGs3dGrads), vp, sz, vp]
    L.scorp_gs3d_backward_ex.argtypes = [ctypes.POINTER(ScorpGs3dInputs), vp, vp, u64, vp, vp, vp,
                                         ctypes.POINTER(ScorpGs3dGrads), vp, sz, ctypes.c_uint32, vp]
    L.scorp_gs3d_debug_geom.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    L.scorp_gs3d_debug_tiles.argtypes = [vp, vp, u64, i32, i32, i32, vp, vp, vp]
    L.scorp_gs3d_debug_work.argtypes = [vp, i32, i32, i32, ctypes.POINTER(u64 * 3), vp]
    L.scorp_loss_workspace_bytes.restype = sz
    L.scorp_loss_workspace_bytes.argtypes = [i32, i32, i32]
    L.scorp_loss_l1_ssim_forward.argtypes = [vp, vp, vp, i32, i32, i32, ctypes.c_float, vp, vp, sz, i32, vp]
    L.scorp_loss_l1_ssim_backward.argtypes = [vp, vp, vp, i32, i32, i32, ctypes.c_float, vp, vp, vp, vp]
    L.scorp_gs3d_render_tail.argtypes = [vp, vp, ctypes.c_int64, vp, i32, vp, vp, vp]
    L.scorp_gs3d_render_tail_backward.argtypes = [vp, vp, vp, ctypes.c_int64, vp, vp, vp]
    L.scorp_gs3d_pose_score_accumulate.argtypes = [vp, vp, vp, vp, ctypes.c_int64, ctypes.c_float, vp, vp]
    L.scorp_gs2d_state_bytes.restype = sz
    L.scorp_gs2d_state_bytes.argtypes = [i32, i32, i32]
    L.scorp_gs2d_backward_scratch_bytes.restype = sz
    L.scorp_gs2d_backward_scratch_bytes.argtypes = [i32]
    L.scorp_gs2d_preprocess.argtypes = [ctypes.POINTER(ScorpGs3dInputs), vp, vp, sz, vp]
    L.scorp_gs2d_render.argtypes = [ctypes.POINTER(ScorpGs3dInputs), vp, vp, u64, vp, vp, vp]
    L.scorp_gs2d_render_image.argtypes = [ctypes.POINTER(ScorpGs3dInputs), vp, vp, u64, vp, vp, vp]
    L.scorp_gs2d_render_score.argtypes = [ctypes.POINTER(ScorpGs3dInputs), vp, vp, u64, vp, vp, i32, ctypes.c_float, ctypes.c_float, vp, vp]
    L.scorp_gs2d_backward.argtypes = [ctypes.POINTER(ScorpGs3dInputs), vp, vp, u64, vp, vp, ctypes.POINTER(ScorpGs3dGrads), vp, sz, vp]
    L.scorp_gs2d_backward_ex.argtypes = [ctypes.POINTER(ScorpGs3dInputs), vp, vp, u64, vp, vp, ctypes.POINTER(ScorpGs3dGrads), vp, sz,
                                         ctypes.c_uint32, vp]
    L.scorp_gs2d_backward_scratch_bytes_ex.restype = sz
    L.scorp_gs2d_backward_scratch_bytes_ex.argtypes = [i32, i32, i32, u64, ctypes.c_uint32]
    L.scorp_gs2d_debug_geom.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.scorp_gs2d_debug_tiles.argtypes = [vp, vp, u64, i32, i32, i32, vp, vp, vp]
    L.scorp_gs2d_maps_forward.argtypes = [i32, i32, vp, vp, vp, vp, ctypes.c_float, vp, vp, vp, vp, vp, vp]
    L.scorp_gs2d_maps_backward.argtypes = [i32, i32, vp, vp, vp, vp, ctypes.c_float, vp, vp, vp, vp, vp, vp, vp, vp]
    L.scorp_gs2d_regularizers_workspace_bytes.restype = sz
    L.scorp_gs2d_regularizers_workspace_bytes.argtypes = [i32, i32]
    L.scorp_gs2d_regularizers_forward.argtypes = [i32, i32, vp, vp, vp, vp, ctypes.c_float, ctypes.c_float, ctypes.c_float, vp, vp, sz, vp]
    L.scorp_gs2d_regularizers_backward.argtypes = [i32, i32, vp, vp, vp, vp, ctypes.c_float, ctypes.c_float, ctypes.c_float, vp, vp, vp]
    L.scorp_gs3d_train_view.argtypes = [ctypes.POINTER(ScorpGs3dTrainView), vp]
    L.scorp_gs2d_train_view.argtypes = [ctypes.POINTER(ScorpGs2dTrainView), vp]
    L.scorp_gs3d_view_terms_workspace_bytes.restype = sz
    L.scorp_gs3d_view_terms_workspace_bytes.argtypes = [i32, i32, i32]
    L.scorp_gs3d_train_view_ex.argtypes = [ctypes.POINTER(ScorpGs3dTrainView), ctypes.POINTER(ScorpGs3dViewTerms), vp]
    L.scorp_gs3d_depth_terms.argtypes = [i32, i32, vp, vp, vp, vp, ctypes.c_float, ctypes.c_float, vp, vp, vp, vp, sz, vp]
    L.scorp_gs2d_view_terms_workspace_bytes.restype = sz
    L.scorp_gs2d_view_terms_workspace_bytes.argtypes = [i32, i32, i32]
    L.scorp_gs2d_train_view_ex.argtypes = [ctypes.POINTER(ScorpGs2dTrainView), ctypes.POINTER(ScorpGs2dViewTerms), vp]
    L.scorp_gs2d_surfel_terms.argtypes = [i32, i32, vp, vp, vp, vp, ctypes.c_float, vp, vp, ctypes.c_float, ctypes.c_float,
                                          ctypes.c_float, vp, vp, vp, vp, vp, vp, sz, vp]
    L.scorp_knn_dist2.argtypes = [vp, i32, vp, vp]
    L.scorp_gaussians_transform.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp]
    L.scorp_adam_step.argtypes = [ctypes.POINTER(ScorpAdamTensor), i32, ctypes.c_double, ctypes.c_double, ctypes.c_double, i32, vp]
    L.scorp_adam_step_guarded.argtypes = [ctypes.POINTER(ScorpAdamTensor), i32, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                          i32, vp, vp]
    L.scorp_adam_step_guarded_ex.argtypes = [ctypes.POINTER(ScorpAdamTensor), i32, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                             i32, vp, vp, vp]
    L.scorp_gather_rows.argtypes = [ctypes.POINTER(ScorpRowTensor), i32, vp, u64, vp]
    L.scorp_densification_stats.argtypes = [i32, vp, vp, vp, i32, vp, vp, vp, vp, vp]
    L.scorp_densification_stats_ex.argtypes = [i32, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp]
    L.scorp_mask_vote_scratch_bytes.restype = sz
    L.scorp_mask_vote_scratch_bytes.argtypes = [i32, i32, i32, u64]
    for fn in (L.scorp_gs3d_mask_vote, L.scorp_gs2d_mask_vote):
        fn.argtypes = [ctypes.POINTER(ScorpGs3dInputs), vp, vp, u64, vp, i32, ctypes.c_uint32, ctypes.c_float, vp, vp, sz, vp]
    L.scorp_icp_workspace_bytes.restype = sz
    L.scorp_icp_workspace_bytes.argtypes = [i32, i32, i32]
    f64 = ctypes.c_double
    L.scorp_icp_point_to_point.argtypes = [vp, i32, vp, i32, vp, i32, f64, i32, f64, f64, vp, vp, vp, vp, vp, sz, vp]
    L.scorp_icp_point_to_plane_workspace_bytes.restype = sz
    L.scorp_icp_point_to_plane_workspace_bytes.argtypes = [i32, i32, i32]
    L.scorp_icp_point_to_plane.argtypes = [vp, i32, vp, vp, i32, vp, i32, f64, i32, f64, f64, vp, vp, vp, vp, vp, sz, vp]
    L.scorp_icp_generalized_workspace_bytes.restype = sz
    L.scorp_icp_generalized_workspace_bytes.argtypes = [i32, i32, i32]
    L.scorp_icp_generalized.argtypes = [vp, vp, i32, vp, vp, i32, vp, i32, f64, i32, f64, f64, vp, vp, vp, vp, vp, sz, vp]
    L.scorp_estimate_normals_workspace_bytes.restype = sz
    L.scorp_estimate_normals_workspace_bytes.argtypes = [i32]
    L.scorp_estimate_normals.argtypes = [vp, i32, i32, vp, vp, vp, sz, vp]
    L.scorp_cloud_workspace_bytes.restype = sz
    L.scorp_cloud_workspace_bytes.argtypes = [i32]
    L.scorp_cloud_knn_distance.argtypes = [vp, i32, i32, vp, vp, vp, sz, vp]
    L.scorp_cloud_radius_count.argtypes = [vp, i32, f64, vp, vp, sz, vp]
    L.scorp_cloud_dbscan.argtypes = [vp, i32, f64, i32, vp, vp, vp, vp, vp, sz, vp]
    L.scorp_cloud_fpfh_workspace_bytes.restype = sz
    L.scorp_cloud_fpfh_workspace_bytes.argtypes = [i32, i32]
    L.scorp_cloud_fpfh.argtypes = [vp, vp, i32, f64, i32, vp, vp, vp, vp, vp, sz, vp]
    L.scorp_feature_match_tile_rows.restype = i32
    L.scorp_feature_match_tile_rows.argtypes = []
    L.scorp_feature_match_split_rows.restype = i32
    L.scorp_feature_match_split_rows.argtypes = [i32, i32]
    L.scorp_feature_match_workspace_bytes.restype = sz
    L.scorp_feature_match_workspace_bytes.argtypes = [i32, i32]
    L.scorp_feature_match.argtypes = [vp, i32, vp, i32, vp, vp, vp, sz, vp]
    L.scorp_cloud_orient_workspace_bytes.restype = sz
    L.scorp_cloud_orient_workspace_bytes.argtypes = [i32, i32]
    L.scorp_cloud_orient_normals.argtypes = [vp, vp, vp, i32, i32, ctypes.POINTER(f64), i32, vp, vp, vp, vp, vp, vp, sz, vp]
    L.scorp_pose_fit_workspace_bytes.restype = sz
    L.scorp_pose_fit_workspace_bytes.argtypes = [i32, i32]
    L.scorp_pose_ransac.argtypes = [vp, vp, i32, vp, i32, f64, f64, i32, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.scorp_pose_adam_9dof.argtypes = [vp, vp, i32, i32, f64, f64, f64, f64, f64, ctypes.POINTER(f64), vp, vp, i32, i32, vp, sz, vp]
    L.scorp_tsdf_fuse.argtypes = [ctypes.POINTER(ScorpTsdfViews), ctypes.POINTER(ScorpTsdfSamples), ctypes.POINTER(ScorpTsdfParams),
                                  vp, vp, vp]
    i64 = ctypes.c_int64
    L.scorp_isosurface_count_cells.argtypes = [vp, i32, i32, i32, ctypes.c_float, vp, vp]
    L.scorp_isosurface_emit_vertices.argtypes = [vp, vp, vp, vp, i32, i32, i32, ctypes.c_float, vp, i64, vp, vp]
    L.scorp_isosurface_count_faces.argtypes = [vp, i32, i32, i32, ctypes.c_float, vp, vp]
    L.scorp_isosurface_emit_faces.argtypes = [vp, i32, i32, i32, ctypes.c_float, vp, vp, i64, vp, vp]
    L.scorp_mesh_cluster_link.argtypes = [vp, i64, vp, vp, u64, vp, vp]
    L.scorp_mesh_cluster_roots.argtypes = [vp, i64, vp, vp, vp]
    L.scorp_mesh_cluster_stats.argtypes = [vp, vp, i64, vp, vp, i64, i64, vp, vp, vp, vp]
    L.scorp_mesh_simplify_cells.argtypes = [vp, i64, vp, f64, vp, vp, u64, vp, vp, vp]
    L.scorp_mesh_simplify_roots.argtypes = [vp, u64, vp, i64, vp, vp, vp]
    L.scorp_mesh_simplify_accumulate.argtypes = [vp, vp, i64, vp, i64, vp, f64, vp, vp, i64, i32, vp, vp, vp, vp]
    L.scorp_mesh_simplify_place.argtypes = [vp, vp, i64, vp, f64, i32, vp, vp, vp]
    L.scorp_mesh_simplify_faces.argtypes = [vp, i64, vp, i64, vp, u64, vp, vp, vp]
    L.scorp_mesh_decimate_quadrics.argtypes = [vp, i64, vp, i64, vp, vp, i64, vp, vp, f64, vp, vp]
    L.scorp_mesh_decimate_flags.argtypes = [vp, vp, i64, i64, vp, vp]
    L.scorp_mesh_decimate_candidates.argtypes = [vp, vp, i64, vp, i64, vp, vp, i64, vp, vp, vp, f64, vp, vp, vp]
    L.scorp_mesh_decimate_hash.argtypes = [vp, i64, vp, i64, i64, vp, vp]
    L.scorp_mesh_decimate_select.argtypes = [vp, i64, vp, i64, i64, vp, vp, vp, vp]
    L.scorp_mesh_decimate_apply.argtypes = [vp, i64, vp, vp, i64, vp, i64, vp, vp, vp, vp, vp, vp]
    L.scorp_mesh_decimate_faces.argtypes = [vp, i64, vp, i64, vp, vp, vp]
    L.scorp_mesh_distance_workspace_bytes.restype = sz
    L.scorp_mesh_distance_workspace_bytes.argtypes = [i64, i64]
    L.scorp_mesh_distance_build.argtypes = [vp, i64, vp, i64, vp, sz, vp, vp]
    L.scorp_mesh_distance_query.argtypes = [vp, i64, vp, i64, vp, i64, f64, vp, vp, vp, vp, sz, vp]
    L.scorp_mesh_sample_points.argtypes = [vp, i64, vp, i64, vp, i64, u64, vp, vp, vp, vp]
    L.scorp_nearest_point_workspace_bytes.restype = sz
    L.scorp_nearest_point_workspace_bytes.argtypes = [i32, i32]
    L.scorp_nearest_point_distance.argtypes = [vp, i32, vp, i32, f64, vp, vp, vp, sz, vp]
    L.scorp_mesh_render_workspace_bytes.restype = sz
    L.scorp_mesh_render_workspace_bytes.argtypes = [i64, i64, i32, i32, i32]
    L.scorp_mesh_render.argtypes = [vp, i64, vp, i64, vp, vp, i32, i32, i32, f64, ctypes.c_uint32, vp, ctypes.c_float, vp, vp, vp, vp, vp, vp,
                                    sz, vp]
    L.scorp_mesh_face_normals.argtypes = [vp, i64, vp, i64, i32, vp, vp]
    L.scorp_mesh_vertex_normals.argtypes = [vp, i64, vp, i64, vp, vp, i32, vp, vp]
    L.scorp_mesh_smooth.argtypes = [vp, i64, vp, vp, vp, ctypes.POINTER(f64), i32, i32, vp, vp, vp]
    L.scorp_mesh_normal_map.argtypes = [vp, i64, vp, i64, vp, vp, vp, i32, i32, i32, vp, vp]
    bv, f32 =ctypes.POINTER(ScorpTsdfBlockViews), ctypes.c_float
    L.scorp_tsdf_blocks_touch.argtypes = [bv, f32, f32, i32, vp, vp, u64, vp, vp]
    L.scorp_tsdf_blocks_neighbors.argtypes = [vp, i64, vp, vp]
    L.scorp_tsdf_blocks_integrate.argtypes = [bv, f32, f32, vp, vp, i64, vp, vp, vp, vp]
    L.scorp_isosurface_blocks_count_cells.argtypes = [vp, vp, vp, i64, vp, vp]
    L.scorp_isosurface_blocks_emit_vertices.argtypes = [vp, vp, vp, vp, vp, i64, f32, vp, i64, vp, vp, vp]
    L.scorp_isosurface_blocks_count_faces.argtypes = [vp, vp, vp, i64, vp, vp]
    L.scorp_isosurface_blocks_emit_faces.argtypes = [vp, vp, vp, i64, vp, vp, i64, vp, vp]
    L.scorp_marching_cubes_count_edges.argtypes = [vp, i32, i32, i32, f32, vp, vp, vp]
    L.scorp_marching_cubes_emit_vertices.argtypes = [vp, vp, vp, vp, i32, i32, i32, f32, vp, vp, i64, vp, vp]
    L.scorp_marching_cubes_count_faces.argtypes = [vp, i32, i32, i32, f32, vp, vp]
    L.scorp_marching_cubes_emit_faces.argtypes = [vp, i32, i32, i32, f32, vp, vp, vp, i64, vp, vp]
    L.scorp_marching_cubes_blocks_count_edges.argtypes = [vp, vp, vp, i64, vp, vp, vp]
    L.scorp_marching_cubes_blocks_emit_vertices.argtypes = [vp, vp, vp, vp, vp, i64, f32, vp, vp, i64, vp, vp, vp]
    L.scorp_marching_cubes_blocks_count_faces.argtypes = [vp, vp, vp, i64, vp, vp]
    L.scorp_marching_cubes_blocks_emit_faces.argtypes = [vp, vp, vp, i64, vp, vp, vp, i64, vp, vp]
    L.scorp_prof_enable.argtypes = [ctypes.c_int]
    L.scorp_prof_select.argtypes = [u64]
    L.scorp_prof_kernel_name.restype = ctypes.c_char_p
    L.scorp_prof_kernel_name.argtypes = [ctypes.c_int]
    L.scorp_prof_collect.argtypes = [vp, vp]
    _lib = L
    return L


def current_stream_ptr():
    """The current HIP stream of the current device as an integer.  torch.cuda.current_stream() builds a Stream object through
    three layers of device-index helpers (9 us a call, six calls per training iteration); the raw getter is 0.3 us."""
    import torch
    try:
        return int(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))
    except AttributeError:   # (a torch build without the raw getters)
        return int(torch.cuda.current_stream().cuda_stream)


def prof_enable(on=True, only=None):
    """Start / stop hipEvent bracketing of the library's kernels; `only` = iterable of kernel names to bracket."""
    L = lib()
    mask = (1 << 64) - 1
    if only is not None:
        names = [L.scorp_prof_kernel_name(k).decode() for k in range(L.scorp_prof_num_kernels())]
        mask = sum(1 << names.index(n) for n in only)
    check(L.scorp_prof_select(mask), "scorp_prof_select")
    check(L.scorp_prof_enable(1 if on else 0), "scorp_prof_enable")


def prof_collect():
    """{kernel name: (total ms, launches)} of the kernels timed since prof_enable(True); synchronises."""
    L = lib()
    n = L.scorp_prof_num_kernels()
    ms = (ctypes.c_double * n)()
    cnt = (ctypes.c_uint64 * n)()
    check(L.scorp_prof_collect(ms, cnt), "scorp_prof_collect")
    return {L.scorp_prof_kernel_name(k).decode(): (ms[k], int(cnt[k])) for k in range(n)}


def check(code, what):
    if code != 0:
        msg = lib().scorp_last_error()
        raise RuntimeError(f"{what} failed ({code}): {msg.decode(errors='replace') if msg else ''}")


def call(name, *args):
    """lib().<name>(*args, current stream), checked under its name: a tensor goes as its data_ptr(), a ctypes.Structure by
    reference, None and everything else as given.  For the callers that are not per-iteration hot paths (scorp_amd/mesh)."""
    import torch
    check(getattr(lib(), name)(*[a.data_ptr() if isinstance(a, torch.Tensor) else ctypes.byref(a) if isinstance(a, ctypes.Structure) else a
                                 for a in args], current_stream_ptr()), name)


def call_with_workspace(name, size_name, size_args, *args):
    """call(name, *args, workspace, size) for the entry points that take a one-call workspace as their last two arguments:
    size = lib().<size_name>(*size_args) bytes, allocated as a uint8 tensor on the device of the first tensor of args, under
    that device's guard."""
    import torch
    dev = next(a.device for a in args if isinstance(a, torch.Tensor))
    with torch.cuda.device(dev):
        size = getattr(lib(), size_name)(*size_args)
        workspace = torch.empty(size, dtype=torch.uint8, device=dev)
        call(name, *args, workspace, size)
