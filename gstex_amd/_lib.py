"""ctypes binding of libgstex_hip.so (the C-ABI declared in include/gstex_hip.h).

The shared library is built in-tree (``make -C gstex_amd/csrc`` or ``__graft_entry__.build()``).
There is no fallback: if the library is missing every op raises, so a GPU run can never silently
fall back to a CPU path.  ``torch`` must be imported before the library is loaded so that the HIP
runtime torch ships (soname libamdhip64.so.7) is the one the library binds to.
"""
from __future__ import annotations

import ctypes
import os
import threading
from ctypes import POINTER, c_char_p, c_double, c_float, c_int32, c_int64, c_size_t, c_void_p

import torch  # noqa: F401  (load torch's HIP runtime first)

LIB_PATH = os.environ.get("GSTEX_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libgstex_hip.so")

ABI_VERSION = 19
REC_FLOATS = 32
HP_DOUBLES = 12  # GSTEX_HP_DOUBLES: the fp64 row of a near-edge-on splat (gstex_raster_setup hp_records)
PARTIAL_FLOATS = 32  # GSTEX_PARTIAL_FLOATS: floats between partial rows of a backward with geometry gradients
PARTIAL_FLOATS_PHOTO = 24  # GSTEX_PARTIAL_FLOATS_PHOTO: ... without (the photometric training step)
SETTING_AA_BLUR = 1 << 9
SETTING_DIST_REG = 1 << 10
SETTING_EDIT = 1 << 13
SETTING_EVAL_NORMAL = 1 << 15


class GstexCamera(ctypes.Structure):
    _fields_ = [
        ("viewmat", c_void_p),
        ("c2w", c_void_p),
        ("fx", c_float),
        ("fy", c_float),
        ("cx", c_float),
        ("cy", c_float),
        ("H", c_int32),
        ("W", c_int32),
        ("block", c_int32),
    ]


class GstexAdamTensor(ctypes.Structure):
    _fields_ = [
        ("param", c_void_p),
        ("grad", c_void_p),
        ("exp_avg", c_void_p),
        ("exp_avg_sq", c_void_p),
        ("numel", c_int64),
        ("step_size", c_float),
        ("bias_correction2_sqrt", c_float),
    ]


class GstexPairGuard(ctypes.Structure):
    _fields_ = [
        ("capacity", c_int64),
        ("step_flag", c_void_p),
        ("host_count", c_void_p),
        ("first", c_int32),
    ]


ADAM_MAX_TENSORS = 16


class GstexTrainPrologueArgs(ctypes.Structure):
    """gstex_train_prologue_args (ABI 17): the launches of a training render before its raster forward."""
    _fields_ = [("n", c_int32), ("sh_degree", c_int32), ("n_rest", c_int32), ("map_cols", c_int32),
                ("capacity", c_int64), ("cam", GstexCamera), ("guard", GstexPairGuard)] + [
        (name, c_void_p) for name in (
            "means", "quats", "log_scales", "opac_logits", "mappings", "campos", "features_rest", "texture_dims",
            "quats_n", "scales", "opacities", "uv0", "umap", "vmap", "viewdirs", "depths", "centers", "extents",
            "num_tiles_hit", "rgbs", "offsets", "scan_workspace")] + [("scan_workspace_bytes", c_size_t)] + [
        (name, c_void_p) for name in (
            "records", "tile_ranges", "sorted_ids", "sorted_slots", "tile_order", "bin_workspace")] + [
        ("bin_workspace_bytes", c_size_t), ("raster_aux", c_void_p), ("raster_aux_bytes", c_size_t),
        ("raster_channels", c_int32), ("hp_records", c_void_p)]


class GstexTrainEpilogueArgs(ctypes.Structure):
    """gstex_train_epilogue_args (ABI 17): the training render's backward after the raster backward."""
    _fields_ = [("n", c_int32), ("sh_degree", c_int32), ("n_rest", c_int32), ("cam", GstexCamera)] + [
        (name, c_void_p) for name in (
            "means", "scales", "quats_n", "quats", "log_scales", "opacities", "umap", "vmap", "viewdirs",
            "num_tiles_hit", "offsets", "partials", "v_means", "v_quats", "v_log_scales", "v_opac_logits",
            "v_features_rest", "v_scales_act", "v_quats_n", "v_rgbs", "v_opacities_act", "v_centers", "v_uv0")]


class GstexRasterScene(ctypes.Structure):
    """gstex_raster_scene (ABI 19): what the raster forward and its backward share."""
    _fields_ = [("cam", GstexCamera), ("channels", c_int32), ("settings", c_int32)] + [
        (name, c_void_p) for name in (
            "background", "records", "hp_records", "tile_ranges", "sorted_ids", "texture")] + [
        ("n_texels", c_int64), ("tex_scale", c_float), ("tex_bias", c_float), ("state", c_void_p),
        ("n_isect", c_int64), ("aux", c_void_p)]


class GstexRasterFwdArgs(ctypes.Structure):
    """gstex_raster_fwd_args (ABI 19)."""
    _fields_ = [("scene", GstexRasterScene)] + [
        (name, c_void_p) for name in (
            "tile_order", "out_img", "out_depth", "out_reg", "out_alpha", "out_tex", "out_normal")] + [
        ("zero_buf", c_void_p), ("zero_floats", c_int64), ("zero_buf2", c_void_p), ("zero_floats2", c_int64),
        ("aux_zeroed", c_int32)]


class GstexRasterBwdArgs(ctypes.Structure):
    """gstex_raster_bwd_args (ABI 19)."""
    _fields_ = [("scene", GstexRasterScene)] + [
        (name, c_void_p) for name in (
            "sorted_slots", "v_img", "v_depth", "v_reg", "v_alpha", "v_tex", "v_normal", "partials", "row_flags",
            "v_texture")] + [("zero_buf", c_void_p), ("zero_floats", c_int64)]


class GstexRasterSetupBwdArgs(ctypes.Structure):
    """gstex_raster_setup_bwd_args (ABI 19)."""
    _fields_ = [("n", c_int32), ("glob_scale", c_float), ("row_floats", c_int32), ("fold_aabb", c_int32),
                ("n_rows", c_int64), ("cam", GstexCamera)] + [
        (name, c_void_p) for name in (
            "means", "scales", "quats", "umap", "vmap", "num_tiles_hit", "offsets", "partials", "row_flags",
            "v_means", "v_scales", "v_quats", "v_rgbs", "v_opacities", "v_centers", "v_uv0")]


class GstexRasterViewmatBwdArgs(ctypes.Structure):
    """gstex_raster_viewmat_bwd_args (added within ABI 19): the raster's view-matrix gradient."""
    _fields_ = [("n", c_int32), ("glob_scale", c_float), ("row_floats", c_int32), ("fold_aabb", c_int32),
                ("n_rows", c_int64), ("cam", GstexCamera)] + [
        (name, c_void_p) for name in (
            "means", "scales", "quats", "num_tiles_hit", "offsets", "partials", "row_flags", "v_centers", "workspace",
            "v_viewmat")]


class GstexLossTarget(ctypes.Structure):
    """gstex_loss_target (added within ABI 19): the dataset image and mask of gstex_loss_target_fwd / _bwd."""
    _fields_ = [("gt", c_void_p), ("mask", c_void_p), ("gt_dtype", c_int32), ("gt_channels", c_int32),
                ("mask_dtype", c_int32), ("reserved", c_int32)]


class GstexPaintScatterArgs(ctypes.Structure):
    """gstex_paint_scatter_args (added within ABI 19): a stroke scattered into the texel accumulator."""
    _fields_ = [("cam", GstexCamera), ("settings", c_int32), ("stroke_dtype", c_int32), ("eps", c_float)] + [
        (name, c_void_p) for name in ("records", "tile_ranges", "tile_order", "sorted_ids", "stroke", "depth")] + [
        ("n_texels", c_int64), ("acc", c_void_p)]


class GstexPaintBlendArgs(ctypes.Structure):
    """gstex_paint_blend_args (added within ABI 19): the accumulator blended into the texels."""
    _fields_ = [("n_texels", c_int64), ("acc", c_void_p), ("texture", c_void_p), ("scale", c_float),
                ("shift", c_float)]


class GstexDensityPlanArgs(ctypes.Structure):
    """gstex_density_plan_args (added within ABI 19): one density-control event's decisions."""
    _fields_ = [("n", c_int32), ("size_prune", c_int32), ("prune_only", c_int32)] + [
        (name, c_float) for name in ("grad_threshold", "log_big", "logit_faint", "max_screen_px", "log_world",
                                     "log_split")] + [
        (name, c_void_p) for name in ("log_scales", "opac_logits", "grad_sum", "count", "max_extent", "rows", "kind")]


class GstexDensityTensor(ctypes.Structure):
    """gstex_density_tensor (added within ABI 19): one per-splat tensor of gstex_density_apply."""
    _fields_ = [("src", c_void_p), ("dst", c_void_p), ("width", c_int32), ("role", c_int32)]


class GstexDensityApplyArgs(ctypes.Structure):
    """gstex_density_apply_args (added within ABI 19)."""
    _fields_ = [("n", c_int32), ("n_tensors", c_int32), ("n_new", c_int64), ("log_split", c_float)] + [
        (name, c_void_p) for name in ("rows", "kind", "offsets", "scales", "quats_n", "noise")] + [
        ("tensors", POINTER(GstexDensityTensor))]


class GstexTsdfVolume(ctypes.Structure):
    """gstex_tsdf_volume (added within ABI 19): the dense grid of the mesh-extraction entry points."""
    _fields_ = [("nx", c_int32), ("ny", c_int32), ("nz", c_int32), ("origin", c_float * 3), ("voxel_size", c_float),
                ("tsdf", c_void_p), ("weight", c_void_p), ("color", c_void_p)]


class GstexTsdfView(ctypes.Structure):
    """gstex_tsdf_view (added within ABI 19): one view of gstex_tsdf_integrate."""
    _fields_ = [("cam", GstexCamera), ("depth", c_void_p), ("alpha", c_void_p), ("rgb", c_void_p)]


class GstexTsdfIntegrateArgs(ctypes.Structure):
    """gstex_tsdf_integrate_args (added within ABI 19)."""
    _fields_ = [("vol", GstexTsdfVolume), ("n_views", c_int32), ("sdf_trunc", c_float), ("alpha_min", c_float),
                ("depth_trunc", c_float), ("near_z", c_float), ("views", POINTER(GstexTsdfView))]


class GstexMeshExtractArgs(ctypes.Structure):
    """gstex_mesh_extract_args (added within ABI 19): marching tetrahedra's mark and emit passes."""
    _fields_ = [("vol", GstexTsdfVolume)] + [
        (name, c_void_p) for name in ("table", "edge_mask", "vertex_count", "face_count", "vertex_offsets",
                                      "face_offsets")] + [
        ("n_vertices", c_int64), ("n_faces", c_int64), ("vertices", c_void_p), ("colors", c_void_p),
        ("faces", c_void_p)]


class GstexNnGrid(ctypes.Structure):
    """gstex_nn_grid (added within ABI 19): the uniform grid of the nearest-neighbour entry points."""
    _fields_ = [("origin", c_float * 3), ("cell_size", c_float), ("nx", c_int32), ("ny", c_int32), ("nz", c_int32)]


class GstexNnQueryArgs(ctypes.Structure):
    """gstex_nn_query_args (added within ABI 19)."""
    _fields_ = [("grid", GstexNnGrid), ("n_points", c_int64), ("cell_start", c_void_p), ("records", c_void_p),
                ("n_queries", c_int64), ("queries", c_void_p), ("k", c_int32), ("exclude_self", c_int32),
                ("max_radius", c_float), ("d2", c_void_p), ("index", c_void_p)]


class GstexMeshSampleArgs(ctypes.Structure):
    """gstex_mesh_sample_args (added within ABI 19): the mesh sampler's mark and emit passes."""
    _fields_ = [("n_vertices", c_int64), ("n_faces", c_int64), ("vertices", c_void_p), ("faces", c_void_p),
                ("spacing", c_float), ("count", c_void_p), ("stats", c_void_p), ("offsets", c_void_p),
                ("n_samples", c_int64), ("samples", c_void_p), ("weights", c_void_p), ("face_of", c_void_p)]


class GstexClusterArgs(ctypes.Structure):
    """gstex_cluster_args (added within ABI 19): the walks of the splat clustering (degree, link, assign)."""
    _fields_ = [("grid", GstexNnGrid), ("n", c_int64), ("cell_start", c_void_p), ("records", c_void_p),
                ("shapes", c_void_p), ("eps", c_float), ("min_pts", c_int32), ("degree", c_void_p),
                ("parent", c_void_p), ("offsets", c_void_p), ("labels", c_void_p)]


SELECT_MAX_TENSORS = 4  # GSTEX_SELECT_MAX_TENSORS


class GstexSelectPlanArgs(ctypes.Structure):
    """gstex_select_plan_args (added within ABI 19): the rows and texels a per-splat mask keeps."""
    _fields_ = [("n", c_int32), ("n_texels", c_int64)] + [
        (name, c_void_p) for name in ("keep", "texture_dims", "rows", "texels", "flag")]


class GstexSelectDimsArgs(ctypes.Structure):
    """gstex_select_dims_args (added within ABI 19)."""
    _fields_ = [("n", c_int32), ("n_new", c_int32)] + [
        (name, c_void_p) for name in ("keep", "texture_dims", "row_off", "tex_off", "new_dims", "src_off")]


class GstexSelectPair(ctypes.Structure):
    """gstex_select_pair (added within ABI 19): one (src, dst) texel tensor of gstex_select_texels."""
    _fields_ = [("src", c_void_p), ("dst", c_void_p)]


class GstexSelectTexelsArgs(ctypes.Structure):
    """gstex_select_texels_args (added within ABI 19): the jagged gather."""
    _fields_ = [("n_new", c_int32), ("channels", c_int32), ("n_tensors", c_int32), ("n_texels_new", c_int64),
                ("n_texels", c_int64), ("new_dims", c_void_p), ("src_off", c_void_p),
                ("tensors", GstexSelectPair * SELECT_MAX_TENSORS)]


TSDF_MAX_VIEWS = 8  # GSTEX_TSDF_MAX_VIEWS
NN_MAX_CELLS = 1 << 26  # GSTEX_NN_MAX_CELLS
NN_MAX_AXIS_CELLS = 4096  # GSTEX_NN_MAX_AXIS_CELLS
NN_MAX_K = 8  # GSTEX_NN_MAX_K
SAMPLE_MAX_N = 256  # GSTEX_SAMPLE_MAX_N
MESH_TABLE_WORDS = 102  # GSTEX_MESH_TABLE_WORDS
DENSITY_KEEP, DENSITY_CLONE, DENSITY_SPLIT, DENSITY_PRUNE = 0, 1, 2, 3  # GSTEX_DENSITY_*
DENSITY_ROLE_COPY, DENSITY_ROLE_MOMENT, DENSITY_ROLE_MEANS, DENSITY_ROLE_LOG_SCALES = 0, 1, 2, 3  # GSTEX_DENSITY_ROLE_*
DENSITY_MAX_TENSORS = 24  # GSTEX_DENSITY_MAX_TENSORS
GT_F32, GT_U8 = 0, 1  # GSTEX_GT_*
MASK_F32, MASK_BOOL = 0, 1  # GSTEX_MASK_*
ADAM_ZERO_GRAD = 1  # GSTEX_ADAM_ZERO_GRAD
ADAM_GRID_SHIFT = 8  # GSTEX_ADAM_GRID_SHIFT
BIN_CAPPED = 1  # GSTEX_BIN_CAPPED
BIN_COUNT_ZEROED = 2  # GSTEX_BIN_COUNT_ZEROED
BWD_GENERIC, BWD_TRAIN = 0, 1  # GSTEX_BWD_*: what gstex_raster_bwd_variant returns
_P = c_void_p
_CAM = POINTER(GstexCamera)

# name -> (restype, argtypes); must mirror include/gstex_hip.h
SIGNATURES = {
    "gstex_last_error": (c_char_p, []),
    "gstex_abi_version": (c_int32, []),
    "gstex_project_points": (c_int32, [c_int32, _P, _CAM, _P, _P, _P]),
    "gstex_project_points_bwd": (c_int32, [c_int32, _P, _CAM, _P, _P, _P, _P]),
    "gstex_aabb_2d": (c_int32, [c_int32, _P, _P, c_float, _P, _CAM, _P, _P, _P]),
    "gstex_aabb_2d_bwd": (c_int32, [c_int32, _P, _P, c_float, _P, _CAM, _P, _P, _P, _P, _P]),
    "gstex_num_tiles_hit": (c_int32, [c_int32, _P, _P, c_int32, c_int32, c_int32, _P, _P]),
    "gstex_preprocess": (c_int32, [c_int32, _P, _P, c_float, _P, _CAM, _P, _P, _P, _P, _P]),
    "gstex_scan_workspace_size": (c_size_t, [c_int32]),
    "gstex_scan_offsets": (c_int32, [c_int32, _P, _P, _P, c_size_t, POINTER(GstexPairGuard), _P]),
    "gstex_bin_workspace_size": (c_size_t, [c_int32, c_int64, c_int32]),
    "gstex_bin_sort": (
        c_int32,
        [c_int32, c_int64, _P, _P, _P, _P, c_int32, c_int32, c_int32, _P, _P, _P, _P, c_int32, _P, c_size_t, _P],
    ),
    "gstex_tile_order": (c_int32, [c_int32, _P, _P, _P]),
    "gstex_host_words_alloc": (c_int32, [c_int32, POINTER(c_void_p), POINTER(c_void_p)]),
    "gstex_host_words_free": (c_int32, [c_void_p]),
    "gstex_event_create": (c_int32, [c_int32, POINTER(c_void_p)]),
    "gstex_event_record": (c_int32, [c_void_p, c_void_p]),
    "gstex_event_elapsed": (c_int32, [c_void_p, c_void_p, POINTER(ctypes.c_float)]),
    "gstex_stream_wait_event": (c_int32, [c_void_p, c_void_p]),
    "gstex_event_destroy": (c_int32, [c_void_p]),
    "gstex_raster_setup": (
        c_int32,
        [c_int32, _P, _P, c_float, _P, _P, _P, _P, _P, _P, _P, _P, _P, _CAM, _P, _P, _P],
    ),
    "gstex_raster_fwd": (c_int32, [POINTER(GstexRasterFwdArgs), _P]),
    "gstex_raster_aux_bytes": (c_size_t, [c_int64, c_int32, c_int32]),
    "gstex_unit_order": (c_int32, [c_int32, _P, _P, _P, _P]),
    "gstex_unit_order_scratch_words": (c_size_t, []),
    "gstex_raster_bwd": (c_int32, [POINTER(GstexRasterBwdArgs), _P]),
    "gstex_raster_bwd_variant": (c_int32, [POINTER(GstexRasterBwdArgs)]),
    "gstex_raster_setup_bwd": (c_int32, [POINTER(GstexRasterSetupBwdArgs), _P]),
    "gstex_raster_viewmat_bwd_workspace": (c_size_t, [c_int32]),
    "gstex_raster_viewmat_bwd": (c_int32, [POINTER(GstexRasterViewmatBwdArgs), _P]),
    "gstex_sh_dirs_bwd": (c_int32, [c_int32, c_int32, c_int32, c_int32, _P, _P, _P, _P, _P]),
    "gstex_sh_fwd": (c_int32, [c_int32, c_int32, c_int32, _P, _P, _P, _P]),
    "gstex_sh_bwd": (c_int32, [c_int32, c_int32, c_int32, _P, _P, _P, _P]),
    "gstex_texture_sample": (c_int32, [c_int64, c_int32, _P, _P, c_int64, _P, _P, _P]),
    "gstex_texture_sample_bwd": (c_int32, [c_int64, c_int32, _P, c_int64, _P, _P, _P, _P]),
    "gstex_activate_fwd": (c_int32, [c_int32, _P, _P, _P, _P, _P, c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gstex_activate_bwd": (c_int32, [c_int32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gstex_sh_rest_fwd": (c_int32, [c_int32, c_int32, c_int32, _P, _P, _P, _P]),
    "gstex_sh_rest_bwd": (c_int32, [c_int32, c_int32, c_int32, _P, _P, _P, _P]),
    "gstex_texture_edit": (c_int32, [_CAM, c_int32, _P, _P, _P, _P, _P, _P, _P, _P, c_int64, _P, _P]),
    "gstex_paint_scatter": (c_int32, [POINTER(GstexPaintScatterArgs), _P]),
    "gstex_paint_blend": (c_int32, [POINTER(GstexPaintBlendArgs), _P]),
    "gstex_loss_workspace_size": (c_size_t, [c_int32, c_int32]),
    "gstex_loss_fwd": (c_int32, [c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, POINTER(c_float), c_float, _P, _P,
                                 _P, c_size_t, _P]),
    "gstex_loss_bwd": (c_int32, [c_int32, c_int32, c_int32, _P, _P, _P, _P, _P, POINTER(c_float), c_float, _P, _P,
                                 _P, _P, _P, c_size_t, _P]),
    "gstex_loss_target_workspace_size": (c_size_t, [c_int32, c_int32]),
    "gstex_loss_target_fwd": (c_int32, [c_int32, c_int32, c_int32, _P, _P, _P, _P, POINTER(GstexLossTarget),
                                        POINTER(c_float), c_float, _P, _P, _P, _P, c_size_t, _P]),
    "gstex_loss_target_bwd": (c_int32, [c_int32, c_int32, c_int32, _P, _P, _P, _P, POINTER(GstexLossTarget),
                                        POINTER(c_float), c_float, _P, _P, _P, _P, _P, c_size_t, _P]),
    "gstex_eval_metrics_workspace_size": (c_size_t, [c_int32, c_int32]),
    "gstex_eval_metrics": (c_int32, [c_int32, c_int32, c_int32, _P, _P, _P, _P, POINTER(GstexLossTarget),
                                     POINTER(c_float), _P, _P, _P, _P, _P, c_size_t, _P]),
    "gstex_adam_step": (c_int32, [c_int32, POINTER(GstexAdamTensor), c_double, c_double, c_double, c_int32, c_float,
                                  _P, _P]),
    "gstex_train_prologue": (c_int32, [POINTER(GstexTrainPrologueArgs), _P]),
    "gstex_train_prologue_scan_bytes": (c_size_t, [c_int32]),
    "gstex_train_epilogue": (c_int32, [POINTER(GstexTrainEpilogueArgs), _P]),
    "gstex_density_accum": (c_int32, [c_int32, _P, _P, _CAM, _P, _P, _P, _P, _P, _P, _P]),
    "gstex_density_plan": (c_int32, [POINTER(GstexDensityPlanArgs), _P]),
    "gstex_density_apply": (c_int32, [POINTER(GstexDensityApplyArgs), _P]),
    "gstex_tsdf_integrate": (c_int32, [POINTER(GstexTsdfIntegrateArgs), _P]),
    "gstex_mesh_extract_mark": (c_int32, [POINTER(GstexMeshExtractArgs), _P]),
    "gstex_mesh_extract_emit": (c_int32, [POINTER(GstexMeshExtractArgs), _P]),
    "gstex_nn_grid_count": (c_int32, [POINTER(GstexNnGrid), c_int64, _P, _P, _P]),
    "gstex_nn_grid_place": (c_int32, [POINTER(GstexNnGrid), c_int64, _P, _P, _P, _P, _P]),
    "gstex_nn_query": (c_int32, [POINTER(GstexNnQueryArgs), _P]),
    "gstex_mesh_sample_mark": (c_int32, [POINTER(GstexMeshSampleArgs), _P]),
    "gstex_mesh_sample_emit": (c_int32, [POINTER(GstexMeshSampleArgs), _P]),
    "gstex_cluster_shapes": (c_int32, [c_int64, _P, _P, c_int32, _P, _P, _P]),
    "gstex_cluster_degree": (c_int32, [POINTER(GstexClusterArgs), _P]),
    "gstex_cluster_link": (c_int32, [POINTER(GstexClusterArgs), _P]),
    "gstex_cluster_roots": (c_int32, [c_int64, c_int32, _P, _P, _P, _P]),
    "gstex_cluster_assign": (c_int32, [POINTER(GstexClusterArgs), _P]),
    "gstex_cluster_pair_w2": (c_int32, [c_int64, _P, _P, c_int32, _P, c_int64, _P, _P, _P, _P, _P]),
    "gstex_select_plan": (c_int32, [POINTER(GstexSelectPlanArgs), _P]),
    "gstex_select_dims": (c_int32, [POINTER(GstexSelectDimsArgs), _P]),
    "gstex_select_texels": (c_int32, [POINTER(GstexSelectTexelsArgs), _P]),
}

_lib = None
_lock = threading.Lock()


class GstexError(RuntimeError):
    pass


def load(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load (once) and return the C-ABI library; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(path):
                raise GstexError(
                    f"{path} is missing: build it with `make -C gstex_amd/csrc` "
                    "(or `python -c 'import __graft_entry__ as g; g.build()'`). "
                    "gstex_amd has no CPU fallback."
                )
            lib = ctypes.CDLL(path)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            _lib = lib
    return _lib


def last_error() -> str:
    msg = load().gstex_last_error()
    return msg.decode() if msg else ""


def call(name: str, *args) -> None:
    """Call a status-returning entry point; raise GstexError with the library's message."""
    rc = getattr(load(), name)(*args)
    if rc != 0:
        raise GstexError(f"{name} failed (status {rc}): {last_error()}")


def ptr(t) -> int | None:
    """Device pointer of a tensor (None for None / empty)."""
    if t is None:
        return None
    if t.numel() == 0:
        return None
    return t.data_ptr()


def stream_of(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


class _Event:
    __slots__ = ("_h",)
    KIND = 0

    def __init__(self):
        h = c_void_p()
        call("gstex_event_create", self.KIND, ctypes.byref(h))
        self._h = h.value

    def record(self, device=None, stream: int | None = None) -> None:
        """Record on `stream` (a HIP stream handle), default the current stream of `device`."""
        call("gstex_event_record", self._h, stream if stream is not None else torch.cuda.current_stream(device).cuda_stream)

    @property
    def handle(self) -> int:
        return self._h

    def __del__(self):
        try:
            if self._h:
                load().gstex_event_destroy(self._h)
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


class TimingEvent(_Event):
    """A HIP event for timing only (gstex_event_create(GSTEX_EVENT_TIMING), ABI 14: no system-scope fence when
    recorded, so a pair around a kernel does not write back and invalidate the caches between launches);
    elapsed_time(end) in ms once both have completed."""

    __slots__ = ()
    KIND = 0

    def elapsed_time(self, end: "TimingEvent") -> float:
        ms = c_float()
        call("gstex_event_elapsed", self._h, end._h, ctypes.byref(ms))
        return float(ms.value)


class OrderEvent(_Event):
    """A HIP event for ordering one stream after another on the same device (GSTEX_EVENT_ORDER: no timing, a
    device-scope release instead of the default event's system-scope one); wait(stream) = hipStreamWaitEvent."""

    __slots__ = ()
    KIND = 1

    def wait(self, device=None, stream: int | None = None) -> None:
        call("gstex_stream_wait_event",
             stream if stream is not None else torch.cuda.current_stream(device).cuda_stream, self._h)


def make_camera(viewmat, c2w, fx, fy, cx, cy, H, W, block) -> GstexCamera:
    """viewmat: device fp32 (3,4) contiguous; c2w: device fp32 (4,4) contiguous or None."""
    return GstexCamera(
        ptr(viewmat), ptr(c2w) if c2w is not None else None,
        float(fx), float(fy), float(cx), float(cy), int(H), int(W), int(block),
    )
