"""ctypes binding of libdexnerf_hip.so (C ABI declared in include/dexnerf_hip.h).

No torch types cross the boundary: tensors are passed as raw device pointers (`tensor.data_ptr()`) plus
sizes, and work is enqueued on PyTorch's current HIP stream.  The library is REQUIRED for any device
tensor: there is no eager/CPU fallback - `lib()` raises if the shared object is missing.
"""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DEXNERF_HIP_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libdexnerf_hip.so"))

PREC_F32 = 0
PREC_BF16 = 1
PREC_F16 = 2
PACK_CORE, PACK_G48, PACK_ALL = 1, 2, 3   # dn_mlp_pack_parts: the streams of a packed buffer
PREC_BF16_S8 = 3   # training entry points: bf16 arithmetic, 8-bit saved activations / gradients (experimental)

EXPORTS = (
    "dn_abi_version", "dn_last_error", "dn_ray_bundle", "dn_coarse_depths", "dn_positional_encoding",
    "dn_mlp_packed_bytes", "dn_mlp_pack", "dn_run_network", "dn_mlp_forward_encoded", "dn_volume_render",
    "dn_volume_render_backward", "dn_sample_pdf", "dn_fine_depths", "dn_render_workspace_bytes", "dn_render_rays",
    "dn_mlp_train_sizes", "dn_mlp_backward_packed_bytes", "dn_mlp_pack_backward", "dn_run_network_train",
    "dn_mlp_backward_data", "dn_mlp_unpack", "dn_mlp_weight_grad", "dn_mlp_weight_grad_all",
    "dn_select_rays", "dn_select_rays_indirect", "dn_ndc_rays", "dn_dex_error_sweep", "dn_depth_error_image",
    "dn_render_train_workspace_bytes", "dn_render_rays_train", "dn_render_rays_backward",
    "dn_set_s8_grad_scale", "dn_mlp_pack_parts", "dn_fp16_range_guard", "dn_select_rays_draw", "dn_mse2_loss", "dn_rng_fill", "dn_mlp_pack_train_pair",
    "dn_adam_step", "dn_pack_ray_rows", "dn_mlp_weight_grad_pair",
    "dn_mlp_weight_grad_scratch_bytes", "dn_mlp_weight_grad_all_ws", "dn_mlp_weight_grad_pair_ws", "dn_render_rays_backward_ws",
    "dn_select_rays_draw_ndc",
    "dn_mlp_input_grad_packed_bytes", "dn_mlp_pack_input_grad", "dn_mlp_backward_input_workspace_bytes", "dn_mlp_backward_input",
    "dn_mlp_density_desc", "dn_mlp_density_packed_bytes", "dn_mlp_pack_density", "dn_composite_density", "dn_density_resample",
    "dn_render_depth_workspace_bytes", "dn_render_rays_depth",
    "dn_volume_render_backward_geom", "dn_coarse_depths_backward", "dn_fine_depths_backward",
    "dn_select_rays_indirect_ndc", "dn_camera_grad_scratch_bytes", "dn_camera_grad",
    "dn_select_rays_views", "dn_select_rays_draw_views", "dn_camera_grad_views_scratch_bytes", "dn_camera_grad_views",
    "dn_pose_records", "dn_pose_records_backward", "dn_render_rays_train_geom", "dn_render_backward_geom_workspace_bytes",
    "dn_render_rays_backward_geom",
    "dn_render_loss",
    "dn_camera_records", "dn_camera_records_scratch_bytes", "dn_camera_records_backward",
)

# include/dexnerf_hip_ext.h: the entry points added after ABI version 2 (the table above and DN_ABI_VERSION stay as they are)
EXT_EXPORTS = ("dn_distortion_loss", "dn_render_reg_workspace_bytes", "dn_render_rays_backward_reg")

# include/dexnerf_hip_anneal.h: the coarse-to-fine positional encoding (nerf.EncodingAnneal)
ANNEAL_EXPORTS = ("dn_encoding_anneal_amplitudes", "dn_encoding_anneal_scale_weights", "dn_encoding_anneal_scale_grads",
                  "dn_encoding_anneal_scale_weights_pair", "dn_encoding_anneal_scale_grads_pair")

# include/dexnerf_hip_exposure.h: the loss head with a per-view exposure correction (refine_exposure= on the fused steps)
EXPOSURE_EXPORTS = ("dn_render_loss_exposure",)

# include/dexnerf_hip_normals.h: density-gradient surface normals composited beside the Dex depths (nerf.render_dex_normals)
NORMALS_EXPORTS = ("dn_composite_normals", "dn_render_normals_workspace_bytes", "dn_render_rays_normals")

# include/dexnerf_hip_quantile.h: opacity-quantile (median) depth maps beside the Dex depths (nerf.render_dex_depth(quantiles=...))
QUANTILE_EXPORTS = ("dn_composite_density_quantiles", "dn_render_rays_depth_quantiles")
MAX_QUANTILES = 64   # DN_MAX_QUANTILES

# include/dexnerf_hip_mesh.h: the Dex threshold surface of a sampled density field as a triangle mesh (nerf.extract_dex_mesh)
MESH_EXPORTS = ("dn_isosurface_workspace_bytes", "dn_isosurface_count", "dn_isosurface_emit")
ISO_SCAN_BLOCK = 1024               # DN_ISO_SCAN_BLOCK: elements per workgroup at each of the three scan levels
ISO_MAX_GRID_VERTICES = 1 << 28     # DN_ISO_MAX_GRID_VERTICES

# include/dexnerf_hip_occupancy.h: an occupancy bit grid and the compaction of ray samples against it (nerf.OccupancyGrid,
# nerf.render_dex_depth(occupancy=...))
OCCUPANCY_EXPORTS = ("dn_occupancy_words", "dn_occupancy_build", "dn_occupancy_compact_workspace_bytes", "dn_occupancy_compact_count",
                     "dn_occupancy_compact_emit", "dn_occupancy_gather")
OCC_MAX_AXIS_CELLS = 1 << 24        # DN_OCC_MAX_AXIS_CELLS
OCC_MAX_CELLS = 1 << 30             # DN_OCC_MAX_CELLS
OCC_MAX_DILATE = 8                  # DN_OCC_MAX_DILATE
OCC_MAX_SAMPLES = 1 << 30           # DN_OCC_MAX_SAMPLES
OCC_MAX_SAMPLES_PER_RAY = 2048      # DN_OCC_MAX_SAMPLES_PER_RAY
OCC_FILL = -3.4028234663852886e+38  # DN_OCC_FILL: -FLT_MAX

# include/dexnerf_hip_cull.h: the emit with view directions and the gather of whole rows - the compaction for the culled colour and
# normal renders (nerf.run_one_iter_of_nerf(occupancy=...), nerf.render_dex_normals(occupancy=...))
CULL_EXPORTS = ("dn_occupancy_compact_emit_dirs", "dn_occupancy_gather_rows")
CULL_MAX_WIDTH = 4                  # DN_CULL_MAX_WIDTH

# include/dexnerf_hip_refine.h: sub-sample Dex depths - the first crossing bracketed by the compositing pass and bisected on the density
# network (nerf.render_dex_depth(refine_steps=...))
REFINE_EXPORTS = ("dn_composite_density_brackets", "dn_dex_bisect", "dn_dex_refine_finish", "dn_render_depth_refined_workspace_bytes",
                  "dn_render_rays_depth_refined")
MAX_REFINE_STEPS = 24               # DN_MAX_REFINE_STEPS

# include/dexnerf_hip_span.h: a ray's near / far tightened to the occupied span of an occupancy grid (nerf.OccupancyGrid.ray_spans,
# nerf.render_dex_depth(ray_span=...))
SPAN_EXPORTS = ("dn_occupancy_ray_spans",)

# include/dexnerf_hip_layers.h: Dex depth layers - every entry into and exit from {sigma > m} along a ray (nerf.render_dex_layers)
LAYERS_EXPORTS = ("dn_composite_density_layers", "dn_dex_layers_finish", "dn_render_depth_layers_workspace_bytes",
                  "dn_render_rays_depth_layers")
MAX_LAYERS = 8                      # DN_MAX_LAYERS
MAX_LAYER_RECORDS = 2048            # DN_MAX_LAYER_RECORDS

# include/dexnerf_hip_live.h: an occupancy grid refreshed on the device while the networks train (nerf.LiveOccupancyGrid,
# nerf.FusedTrainStep(ray_span=...))
LIVE_EXPORTS = ("dn_occupancy_cell_points", "dn_occupancy_ema_workspace_bytes", "dn_occupancy_ema_update")
RNG_STREAM_CELL = 6                 # kRngStreamCell (csrc/dn_rng.h)


class MlpDesc(ctypes.Structure):
    """dn_mlp_desc (mirrors FlexibleNeRFModel.__init__, reference nerf/models.py:186-196)."""
    _fields_ = [(n, c_int32) for n in (
        "num_layers", "hidden_size", "skip_connect_every", "num_encoding_fn_xyz", "num_encoding_fn_dir",
        "include_input_xyz", "include_input_dir", "use_viewdirs", "log_sampling_xyz", "log_sampling_dir")]


_lib = None


def _declare(lib):
    fp, vp = c_void_p, c_void_p  # device pointers travel as integers
    lib.dn_abi_version.restype = c_int
    lib.dn_last_error.restype = c_char_p
    lib.dn_ray_bundle.argtypes = [c_int, c_int, POINTER(c_float), POINTER(c_float), c_float, c_float, c_float, fp, fp, vp]
    lib.dn_coarse_depths.argtypes = [fp, c_int, c_int64, c_int, c_int, fp, fp, vp]
    lib.dn_positional_encoding.argtypes = [fp, c_int64, c_int, c_int, c_int, c_int, fp, vp]
    lib.dn_mlp_packed_bytes.argtypes = [POINTER(MlpDesc), c_int]
    lib.dn_mlp_packed_bytes.restype = c_size_t
    lib.dn_mlp_pack.argtypes = [POINTER(MlpDesc), c_int, POINTER(c_void_p), POINTER(c_void_p), vp, vp]
    lib.dn_mlp_pack_parts.argtypes = [POINTER(MlpDesc), c_int, POINTER(c_void_p), POINTER(c_void_p), vp, c_int, vp]
    lib.dn_run_network.argtypes = [POINTER(MlpDesc), c_int, vp, fp, fp, fp, c_int, fp, c_int64, c_int, fp, vp]
    lib.dn_mlp_forward_encoded.argtypes = [POINTER(MlpDesc), c_int, vp, fp, c_int64, fp, vp]
    lib.dn_volume_render.argtypes = [fp, fp, fp, c_int, fp, c_float, c_int, POINTER(c_float), c_int, c_int64, c_int,
                                     fp, fp, fp, fp, fp, fp, vp]
    lib.dn_volume_render_backward.argtypes = [fp, fp, fp, c_int, fp, c_float, c_int, c_int64, c_int, fp, fp, fp, fp,
                                              fp, fp, vp]
    lib.dn_sample_pdf.argtypes = [fp, fp, fp, c_int64, c_int, c_int, fp, fp, vp]
    lib.dn_fine_depths.argtypes = [fp, fp, fp, c_int64, c_int, c_int, fp, fp, vp]
    lib.dn_render_workspace_bytes.argtypes = [c_int64, c_int, c_int]
    lib.dn_render_workspace_bytes.restype = c_size_t
    lib.dn_render_rays.argtypes = [POINTER(MlpDesc), vp, POINTER(MlpDesc), vp, c_int, fp, c_int, c_int64, c_int, c_int,
                                   c_int, c_float, c_int, POINTER(c_float), c_int, fp, fp, fp, fp, fp, fp, fp, fp, fp,
                                   fp, fp, vp, vp]
    lib.dn_mlp_train_sizes.argtypes = [POINTER(MlpDesc), c_int, c_int64, POINTER(c_size_t), POINTER(c_size_t),
                                       POINTER(c_size_t)]
    lib.dn_mlp_backward_packed_bytes.argtypes = [POINTER(MlpDesc), c_int]
    lib.dn_mlp_backward_packed_bytes.restype = c_size_t
    lib.dn_mlp_pack_backward.argtypes = [POINTER(MlpDesc), c_int, POINTER(c_void_p), vp, vp]
    lib.dn_run_network_train.argtypes = [POINTER(MlpDesc), c_int, vp, fp, fp, fp, c_int, fp, c_int64, c_int, fp, vp, vp, vp]
    lib.dn_mlp_backward_data.argtypes = [POINTER(MlpDesc), c_int, vp, fp, vp, c_int64, vp, vp]
    lib.dn_mlp_unpack.argtypes = [POINTER(MlpDesc), c_int, c_int, vp, c_int64, c_int, c_int, c_int, fp, c_int, c_int, vp]
    lib.dn_mlp_weight_grad.argtypes = [POINTER(MlpDesc), c_int, vp, vp, c_int64, c_int, c_int, c_int, c_int, c_int, fp, c_int,
                                       fp, vp]
    lib.dn_select_rays.argtypes = [c_int, c_int, POINTER(c_float), POINTER(c_float), c_float, c_float, c_float, c_float, c_float,
                                   vp, c_int64, fp, c_int, fp, fp, vp]
    lib.dn_select_rays_indirect.argtypes = [c_int, c_int, fp, vp, c_float, c_float, vp, c_int64, fp, c_int, fp, fp, vp]
    lib.dn_ndc_rays.argtypes = [c_int, c_int, ctypes.c_double, ctypes.c_double, fp, fp, c_int64, fp, fp, vp]
    lib.dn_dex_error_sweep.argtypes = [fp, fp, c_int, c_int64, vp, c_float, c_float, vp, vp]
    lib.dn_depth_error_image.argtypes = [fp, fp, vp, c_int, c_int, c_float, fp, vp]
    lib.dn_mlp_weight_grad_all.argtypes = [POINTER(MlpDesc), c_int, vp, vp, c_int64, POINTER(c_void_p), POINTER(c_void_p), vp]
    lib.dn_mlp_weight_grad_pair.argtypes = [POINTER(MlpDesc), c_int, vp, vp, c_int64, POINTER(c_void_p), POINTER(c_void_p), vp, vp, c_int64,
                                            POINTER(c_void_p), POINTER(c_void_p), vp]
    lib.dn_mlp_weight_grad_scratch_bytes.argtypes = [POINTER(MlpDesc), c_int]
    lib.dn_mlp_weight_grad_scratch_bytes.restype = c_size_t
    lib.dn_mlp_weight_grad_all_ws.argtypes = [POINTER(MlpDesc), c_int, vp, vp, c_int64, POINTER(c_void_p), POINTER(c_void_p), vp, c_size_t, vp]
    lib.dn_mlp_weight_grad_pair_ws.argtypes = [POINTER(MlpDesc), c_int, vp, vp, c_int64, POINTER(c_void_p), POINTER(c_void_p), vp, vp, c_int64,
                                               POINTER(c_void_p), POINTER(c_void_p), vp, c_size_t, vp]
    lib.dn_set_s8_grad_scale.argtypes = [c_float]
    lib.dn_fp16_range_guard.argtypes = [POINTER(MlpDesc)]
    lib.dn_render_train_workspace_bytes.argtypes = [c_int64, c_int, c_int]
    lib.dn_render_train_workspace_bytes.restype = c_size_t
    lib.dn_render_rays_train.argtypes = [POINTER(MlpDesc), vp, POINTER(MlpDesc), vp, c_int, fp, c_int, c_int64, c_int, c_int,
                                         c_int, c_float, c_int, POINTER(c_float), c_int, fp, fp, fp, fp, fp, fp, fp, fp, fp,
                                         fp, fp, vp, vp, vp, vp, vp, vp, c_int, vp]
    lib.dn_render_rays_backward.argtypes = [POINTER(MlpDesc), vp, POINTER(MlpDesc), vp, c_int, fp, c_int, c_int64, c_int, c_int,
                                            c_float, c_int, fp, fp, fp, fp, fp, fp, fp, fp, vp, vp, vp, vp, vp, vp, vp,
                                            POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p), c_int, vp, vp]
    lib.dn_render_rays_backward_ws.argtypes = [POINTER(MlpDesc), vp, POINTER(MlpDesc), vp, c_int, fp, c_int, c_int64, c_int, c_int,
                                               c_float, c_int, fp, fp, fp, fp, fp, fp, fp, fp, vp, vp, vp, vp, vp, vp, vp,
                                               POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p), c_int, vp, vp, c_size_t, vp]
    lib.dn_select_rays_draw.argtypes = [c_int, c_int, fp, vp, c_int, c_float, c_float, vp, c_int64, fp, c_int, fp, fp, vp, vp]
    lib.dn_select_rays_draw_ndc.argtypes = [c_int, c_int, fp, vp, c_int, c_float, c_float, vp, c_int64, fp, c_int, fp, fp, vp,
                                            ctypes.c_double, ctypes.c_double, vp]
    lib.dn_mse2_loss.argtypes = [fp, fp, fp, c_int64, c_int, fp, fp, fp, vp, vp]
    lib.dn_render_loss.argtypes = [fp, fp, fp, fp, fp, fp, vp, vp, vp, c_int64, c_int64, c_int, c_float, c_float, c_float, c_float, c_float, c_float,
                                   fp, fp, fp, fp, fp, vp, vp]
    lib.dn_rng_fill.argtypes = [vp, ctypes.c_uint32, c_int64, c_int, fp, vp]
    lib.dn_pack_ray_rows.argtypes = [fp, fp, fp, c_float, c_float, c_int64, fp, vp]
    dbl = ctypes.c_double
    lib.dn_adam_step.argtypes = [fp, fp, fp, fp, c_int64, fp, fp, dbl, dbl, dbl, dbl, dbl, c_int, vp]
    lib.dn_mlp_pack_train_pair.argtypes = [POINTER(MlpDesc), POINTER(c_void_p), POINTER(c_void_p), vp, vp, POINTER(c_void_p), POINTER(c_void_p),
                                           vp, vp, vp]
    lib.dn_mlp_input_grad_packed_bytes.argtypes = [POINTER(MlpDesc), c_int]
    lib.dn_mlp_input_grad_packed_bytes.restype = c_size_t
    lib.dn_mlp_pack_input_grad.argtypes = [POINTER(MlpDesc), c_int, POINTER(c_void_p), vp, vp]
    lib.dn_mlp_backward_input_workspace_bytes.argtypes = [POINTER(MlpDesc), c_int64, c_int]
    lib.dn_mlp_backward_input_workspace_bytes.restype = c_size_t
    lib.dn_mlp_backward_input.argtypes = [POINTER(MlpDesc), c_int, vp, vp, fp, fp, fp, c_int, fp, c_int64, c_int, fp, fp, fp, fp, vp,
                                          c_size_t, vp]
    lib.dn_mlp_density_desc.argtypes = [POINTER(MlpDesc), POINTER(MlpDesc)]
    lib.dn_mlp_density_packed_bytes.argtypes = [POINTER(MlpDesc), c_int]
    lib.dn_mlp_density_packed_bytes.restype = c_size_t
    lib.dn_mlp_pack_density.argtypes = [POINTER(MlpDesc), c_int, POINTER(c_void_p), POINTER(c_void_p), vp, vp]
    lib.dn_composite_density.argtypes = [fp, fp, fp, c_int, fp, c_float, fp, c_int, c_int64, c_int, fp, fp, fp, vp]
    lib.dn_density_resample.argtypes = [fp, fp, fp, c_int, fp, c_float, fp, c_int64, c_int, c_int, fp, fp, fp, vp]
    lib.dn_render_depth_workspace_bytes.argtypes = [c_int64, c_int, c_int]
    lib.dn_render_depth_workspace_bytes.restype = c_size_t
    lib.dn_render_rays_depth.argtypes = [POINTER(MlpDesc), vp, POINTER(MlpDesc), vp, c_int, fp, c_int, c_int64, c_int, c_int, c_int,
                                         c_float, fp, c_int, fp, fp, fp, fp, fp, fp, fp, fp, fp, vp, vp]
    lib.dn_volume_render_backward_geom.argtypes = [fp, fp, fp, c_int, fp, c_float, c_int, c_int64, c_int, fp, fp, fp, fp, fp, fp, fp, fp, vp]
    lib.dn_coarse_depths_backward.argtypes = [fp, c_int, c_int64, c_int, c_int, fp, fp, fp, vp]
    lib.dn_fine_depths_backward.argtypes = [fp, fp, fp, c_int64, c_int, c_int, fp, vp]
    lib.dn_select_rays_indirect_ndc.argtypes = [c_int, c_int, fp, vp, c_float, c_float, vp, c_int64, fp, c_int, fp, fp, dbl, dbl, vp]
    lib.dn_camera_grad_scratch_bytes.argtypes = [c_int64]
    lib.dn_camera_grad_scratch_bytes.restype = c_size_t
    lib.dn_camera_grad.argtypes = [c_int, c_int, fp, vp, c_int64, fp, c_int, fp, c_int, fp, c_int, dbl, dbl, vp, c_size_t, fp, vp]
    lib.dn_select_rays_views.argtypes = [c_int, c_int, fp, c_int, vp, c_float, c_float, vp, c_int64, fp, c_int, fp, fp, dbl, dbl, vp]
    lib.dn_select_rays_draw_views.argtypes = [c_int, c_int, fp, c_int, c_float, c_float, vp, c_int64, fp, c_int, fp, fp, vp, vp, dbl, dbl, vp]
    lib.dn_camera_grad_views_scratch_bytes.argtypes = [c_int64, c_int]
    lib.dn_camera_grad_views_scratch_bytes.restype = c_size_t
    lib.dn_camera_grad_views.argtypes = [c_int, c_int, fp, c_int, vp, vp, c_int64, fp, c_int, fp, c_int, fp, c_int, dbl, dbl, vp, c_size_t, fp, vp]
    lib.dn_pose_records.argtypes = [fp, fp, fp, c_int, dbl, c_int, fp, fp, vp]
    lib.dn_pose_records_backward.argtypes = [fp, fp, fp, c_int, fp, fp, vp]
    lib.dn_camera_records.argtypes = [fp, fp, c_int, dbl, fp, fp, c_int, dbl, c_int, fp, fp, vp]
    lib.dn_camera_records_scratch_bytes.argtypes = [c_int]
    lib.dn_camera_records_scratch_bytes.restype = c_size_t
    lib.dn_camera_records_backward.argtypes = [fp, fp, fp, c_int, dbl, fp, fp, c_int, vp, c_int, fp, fp, fp, fp, vp, c_size_t, vp]
    lib.dn_render_rays_train_geom.argtypes = lib.dn_render_rays_train.argtypes[:-1] + [fp, vp]
    lib.dn_render_backward_geom_workspace_bytes.argtypes = [POINTER(MlpDesc), POINTER(MlpDesc), c_int64, c_int, c_int, c_int]
    lib.dn_render_backward_geom_workspace_bytes.restype = c_size_t
    lib.dn_render_rays_backward_geom.argtypes = [POINTER(MlpDesc), vp, vp, POINTER(MlpDesc), vp, vp, c_int, fp, c_int, c_int64, c_int, c_int,
                                                 c_int, c_int, c_float, c_int, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, vp, vp, vp, vp, vp, vp, vp,
                                                 POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p), vp, vp, c_size_t,
                                                 vp, c_size_t, fp, vp]
    for name in EXPORTS:
        if name not in ("dn_render_backward_geom_workspace_bytes", "dn_last_error", "dn_mlp_density_packed_bytes", "dn_render_depth_workspace_bytes", "dn_mlp_packed_bytes", "dn_render_workspace_bytes",
                        "dn_mlp_backward_packed_bytes", "dn_render_train_workspace_bytes",
                        "dn_mlp_input_grad_packed_bytes", "dn_mlp_backward_input_workspace_bytes", "dn_camera_grad_scratch_bytes",
                        "dn_camera_grad_views_scratch_bytes"):
            getattr(lib, name).restype = c_int
    # the extension header
    lib.dn_distortion_loss.argtypes = [fp, fp, fp, c_int, c_int64, c_int, c_float, fp, fp, c_int, vp, fp, vp]
    lib.dn_distortion_loss.restype = c_int
    lib.dn_render_reg_workspace_bytes.argtypes = [c_int64, c_int, c_int]
    lib.dn_render_reg_workspace_bytes.restype = c_size_t
    lib.dn_render_rays_backward_reg.argtypes = lib.dn_render_rays_backward_ws.argtypes[:-1] + [c_float, c_float, vp, c_size_t, fp, vp]
    lib.dn_render_rays_backward_reg.restype = c_int
    # the encoding-anneal header
    lib.dn_encoding_anneal_amplitudes.argtypes = [vp, c_int64, dbl, dbl, c_int, c_int, c_int, fp, vp]
    lib.dn_encoding_anneal_scale_weights.argtypes = [POINTER(MlpDesc), POINTER(c_void_p), fp, POINTER(c_void_p), vp]
    lib.dn_encoding_anneal_scale_grads.argtypes = [POINTER(MlpDesc), fp, POINTER(c_void_p), vp]
    pv = POINTER(c_void_p)
    lib.dn_encoding_anneal_scale_weights_pair.argtypes = [POINTER(MlpDesc), pv, pv, POINTER(MlpDesc), pv, pv, fp, vp]
    lib.dn_encoding_anneal_scale_grads_pair.argtypes = [POINTER(MlpDesc), pv, POINTER(MlpDesc), pv, fp, vp]
    for name in ANNEAL_EXPORTS:
        getattr(lib, name).restype = c_int
    # the exposure header: dn_render_loss's arguments, then eps, P, n_views, exposure_scale, view_mask ahead of the outputs, g_eps behind them
    lib.dn_render_loss_exposure.argtypes = lib.dn_render_loss.argtypes[:18] + [fp, c_int, c_int, c_float, vp, fp, fp, fp, fp, fp, fp, vp, vp]
    lib.dn_render_loss_exposure.restype = c_int
    # the normals header
    lib.dn_composite_normals.argtypes = [fp, fp, fp, c_int, fp, c_float, fp, fp, c_int, c_int64, c_int, fp, fp, fp, fp, fp, vp]
    lib.dn_composite_normals.restype = c_int
    lib.dn_render_normals_workspace_bytes.argtypes = [POINTER(MlpDesc), POINTER(MlpDesc), c_int, c_int64, c_int, c_int]
    lib.dn_render_normals_workspace_bytes.restype = c_size_t
    lib.dn_render_rays_normals.argtypes = [POINTER(MlpDesc), vp, POINTER(MlpDesc), vp, vp, vp, c_int, fp, c_int, c_int64, c_int, c_int, c_int,
                                           c_float, fp, c_int, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, vp, c_size_t, vp]
    lib.dn_render_rays_normals.restype = c_int
    # the quantile header: dn_composite_density's / dn_render_rays_depth's arguments with d_quantiles, n_quant, interp (and qdepth)
    lib.dn_composite_density_quantiles.argtypes = [fp, fp, fp, c_int, fp, c_float, fp, c_int, fp, c_int, c_int, c_int64, c_int, fp, fp, fp, fp, vp]
    lib.dn_composite_density_quantiles.restype = c_int
    lib.dn_render_rays_depth_quantiles.argtypes = lib.dn_render_rays_depth.argtypes[:-2] + [fp, c_int, c_int, fp, vp, vp]
    lib.dn_render_rays_depth_quantiles.restype = c_int
    # the mesh header
    lib.dn_isosurface_workspace_bytes.argtypes = [c_int, c_int, c_int]
    lib.dn_isosurface_workspace_bytes.restype = c_size_t
    lib.dn_isosurface_count.argtypes = [fp, c_int, fp, fp, fp, c_int, c_int, c_int, c_float, vp, vp, vp]
    lib.dn_isosurface_count.restype = c_int
    lib.dn_isosurface_emit.argtypes = [fp, c_int, fp, fp, fp, c_int, c_int, c_int, c_float, vp, c_int64, c_int64, fp, vp, vp]
    lib.dn_isosurface_emit.restype = c_int
    # the occupancy header
    lib.dn_occupancy_words.argtypes = [c_int, c_int, c_int]
    lib.dn_occupancy_words.restype = c_int64
    lib.dn_occupancy_build.argtypes = [fp, c_int, c_int, c_int, c_int, c_float, c_int, c_int, vp, vp, vp]
    lib.dn_occupancy_build.restype = c_int
    lib.dn_occupancy_compact_workspace_bytes.argtypes = [c_int64, c_int]
    lib.dn_occupancy_compact_workspace_bytes.restype = c_size_t
    lib.dn_occupancy_compact_count.argtypes = [fp, c_int, fp, c_int64, c_int, vp, c_int, c_int, c_int] + [c_float] * 9 + [vp, vp, vp, vp]
    lib.dn_occupancy_compact_count.restype = c_int
    lib.dn_occupancy_compact_emit.argtypes = [fp, c_int, fp, c_int64, c_int, vp, c_int64, fp, vp]
    lib.dn_occupancy_compact_emit.restype = c_int
    lib.dn_occupancy_gather.argtypes = [vp, fp, c_int64, c_int64, fp, vp, vp, vp]
    lib.dn_occupancy_gather.restype = c_int
    # the cull header
    lib.dn_occupancy_compact_emit_dirs.argtypes = [fp, c_int, fp, c_int64, c_int, vp, c_int64, fp, fp, vp]
    lib.dn_occupancy_compact_emit_dirs.restype = c_int
    lib.dn_occupancy_gather_rows.argtypes = [vp, fp, c_int, c_int64, c_int64, c_int] + [c_float] * 4 + [fp, c_int, vp, vp, vp]
    lib.dn_occupancy_gather_rows.restype = c_int
    # the refine header
    lib.dn_composite_density_brackets.argtypes = [fp, fp, fp, c_int, fp, c_int, c_int64, c_int, fp, fp, fp, fp, fp, vp]
    lib.dn_composite_density_brackets.restype = c_int
    lib.dn_dex_bisect.argtypes = [fp, fp, fp, c_int, c_int64, fp, vp]
    lib.dn_dex_bisect.restype = c_int
    lib.dn_dex_refine_finish.argtypes = [fp, fp, c_int, c_int64, fp, fp, vp]
    lib.dn_dex_refine_finish.restype = c_int
    lib.dn_render_depth_refined_workspace_bytes.argtypes = [c_int64, c_int, c_int, c_int]
    lib.dn_render_depth_refined_workspace_bytes.restype = c_size_t
    lib.dn_render_rays_depth_refined.argtypes = lib.dn_render_rays_depth.argtypes[:-2] + [c_int, fp, fp, vp, vp]
    lib.dn_render_rays_depth_refined.restype = c_int
    # the span header
    lib.dn_occupancy_ray_spans.argtypes = [fp, c_int, c_int64, vp, c_int, c_int, c_int] + [c_float] * 10 + [c_int, fp, vp, vp]
    lib.dn_occupancy_ray_spans.restype = c_int
    # the layers header
    lib.dn_composite_density_layers.argtypes = [fp, fp, fp, c_int, fp, c_int, c_int, c_int64, c_int, fp, fp, fp, fp, fp, vp, vp]
    lib.dn_composite_density_layers.restype = c_int
    lib.dn_dex_layers_finish.argtypes = [fp, fp, c_int, c_int, c_int, c_int64, fp, fp, vp]
    lib.dn_dex_layers_finish.restype = c_int
    lib.dn_render_depth_layers_workspace_bytes.argtypes = [c_int64, c_int, c_int, c_int, c_int]
    lib.dn_render_depth_layers_workspace_bytes.restype = c_size_t
    lib.dn_render_rays_depth_layers.argtypes = lib.dn_render_rays_depth.argtypes[:-2] + [c_int, c_int, fp, vp, fp, vp, vp]
    lib.dn_render_rays_depth_layers.restype = c_int
    # the live-grid header
    lib.dn_occupancy_cell_points.argtypes = [c_int, c_int, c_int] + [c_float] * 6 + [c_int64, c_int64, vp, fp, vp]
    lib.dn_occupancy_cell_points.restype = c_int
    lib.dn_occupancy_ema_workspace_bytes.argtypes = [c_int, c_int, c_int, c_int]
    lib.dn_occupancy_ema_workspace_bytes.restype = c_size_t
    lib.dn_occupancy_ema_update.argtypes = [fp, c_int, fp, c_int, c_int, c_int, c_int, c_float, c_float, c_int, c_int, fp, vp, vp, vp, vp]
    lib.dn_occupancy_ema_update.restype = c_int


def lib():
    """The loaded library; raises RuntimeError (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"libdexnerf_hip.so not found at {LIB_PATH}: build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (or `make -C dex-nerf_amd/csrc`).  The HIP path has no fallback.")
        handle = ctypes.CDLL(LIB_PATH)
        _declare(handle)
        if handle.dn_abi_version() != 2:
            raise RuntimeError("libdexnerf_hip.so ABI version mismatch")
        _lib = handle
    return _lib


def available():
    return os.path.exists(LIB_PATH)


def check(rc, what=""):
    if rc != 0:
        msg = lib().dn_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what or 'dexnerf_hip'} failed (code {rc}): {msg}")


def ptr(t):
    """Device pointer of a contiguous fp32 tensor (None -> NULL)."""
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "HIP entry points need contiguous device tensors"
    return c_void_p(t.data_ptr())


def stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def host_floats(values):
    arr = (c_float * max(len(values), 1))(*[float(v) for v in values])
    return arr


def f32c(t):
    """Contiguous fp32 view/copy of a device tensor."""
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()
