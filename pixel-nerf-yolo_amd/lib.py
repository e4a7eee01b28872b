"""
ctypes binding of libpnyolo.so (C ABI: include/pnyolo.h).

The library is built in-tree (``make -C pixel-nerf-yolo_amd/csrc``, driven by
``__graft_entry__.build()``) and loaded from this directory.  There is no CPU fallback: if the
shared object is missing or no MI355X is visible, calls raise.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# PNYOLO_LIB selects a diagnostic build (tools/stamp_build.sh); the product is libpnyolo.so
LIB_PATH = os.environ.get("PNYOLO_LIB") or os.path.join(_HERE, "libpnyolo.so")
CSRC = os.path.join(_HERE, "csrc")

c_float_p = C.POINTER(C.c_float)
c_i64_p = C.POINTER(C.c_int64)
c_int_p = C.POINTER(C.c_int)


class ModelDesc(C.Structure):
    _fields_ = [
        ("d_latent", C.c_int32), ("d_hidden", C.c_int32), ("d_out", C.c_int32), ("n_blocks", C.c_int32),
        ("combine_layer", C.c_int32), ("num_freqs", C.c_int32), ("freq_factor", C.c_float),
        ("yolo", C.c_int32), ("has_fine", C.c_int32), ("device", C.c_int32), ("enc_use_first_pool", C.c_int32),
    ]


class RenderOpts(C.Structure):
    _fields_ = [
        ("n_coarse", C.c_int32), ("n_fine", C.c_int32), ("n_fine_depth", C.c_int32), ("depth_std", C.c_float),
        ("white_bkgd", C.c_int32), ("lindisp", C.c_int32),
        ("u_coarse_dev", C.c_void_p), ("u_fine_dev", C.c_void_p), ("u_fine2_dev", C.c_void_p),
        ("g_depth_dev", C.c_void_p), ("seed", C.c_uint64),
        ("sigma_noise_coarse_dev", C.c_void_p), ("sigma_noise_fine_dev", C.c_void_p),
    ]


class RenderOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "rgb_coarse", "depth_coarse", "weights_coarse", "rgb_fine", "depth_fine", "weights_fine",
        "z_coarse", "z_fine", "sample_coarse", "sample_fine")]


class RenderSaved(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("z_coarse", "sample_coarse", "z_fine", "sample_fine", "depth_coarse")]


class RenderGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("rgb_coarse", "depth_coarse", "weights_coarse", "rgb_fine", "depth_fine",
                                          "weights_fine")]


class AdamHyper(C.Structure):
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("weight_decay", C.c_double), ("step", C.c_int64)]


class TrainBatchDesc(C.Structure):
    _fields_ = [("n_objs", C.c_int32), ("n_views", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("n_rays", C.c_int32), ("z_near", C.c_float), ("z_far", C.c_float), ("focal_rows", C.c_int32),
                ("focal_cols", C.c_int32), ("c_rows", C.c_int32), ("seed", C.c_uint64), ("draw_offset", C.c_uint64)]


class TrainBatchDraws(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("pix_inds_dev", "image_ids_dev", "u_x_dev", "u_y_dev")]


class YoloBatchDesc(C.Structure):
    _fields_ = [("n_views_all", C.c_int32), ("n_views", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("n_scales", C.c_int32), ("cell_sizes", C.c_int32 * 4), ("n_anchors", C.c_int32), ("z_near", C.c_float),
                ("z_far", C.c_float)]


class RgbLossDesc(C.Structure):
    _fields_ = [("use_l1_coarse", C.c_int32), ("use_l1_fine", C.c_int32), ("lambda_coarse", C.c_float), ("lambda_fine", C.c_float)]


class YoloLossDesc(C.Structure):
    _fields_ = [("num_anchors", C.c_int32), ("num_classes", C.c_int32), ("box_loss", C.c_float), ("object_loss", C.c_float),
                ("no_object_loss", C.c_float), ("class_loss", C.c_float)]


class YoloBatchesDesc(C.Structure):
    _fields_ = [("n_scales", C.c_int32), ("batch_rows", C.c_int32), ("rows", C.c_int64 * 4)]


class ViewMetricsDesc(C.Structure):
    _fields_ = [("n_views", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("gt_layout", C.c_int32),
                ("win_size", C.c_int32)]


class LpipsDesc(C.Structure):
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("pred_kind", C.c_int32), ("gt_kind", C.c_int32),
                ("clamp", C.c_int32), ("batch_size", C.c_int32)]


class ColorJitterDesc(C.Structure):
    _fields_ = [("n_objs", C.c_int32), ("n_views", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("in_format", C.c_int32)]


class IngestDesc(C.Structure):
    _fields_ = [("n_views", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32),
                ("out_height", C.c_int32), ("out_width", C.c_int32), ("resize", C.c_int32), ("white_mask", C.c_int32)]


class YoloTargetsDesc(C.Structure):
    _fields_ = [("n_views", C.c_int32), ("max_boxes", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("n_scales", C.c_int32), ("cell_sizes", C.c_int32 * 4), ("n_anchors", C.c_int32), ("ignore_iou_thresh", C.c_float)]


class DetectViewsDesc(C.Structure):
    _fields_ = [("form", C.c_int32), ("n_views", C.c_int32), ("n_scales", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("cell_sizes", C.c_int32 * 4), ("n_anchors", C.c_int32), ("n_pred_rows", C.c_int32), ("n_target_rows", C.c_int32),
                ("max_kept", C.c_int32), ("nms_iou", C.c_double), ("nms_threshold", C.c_double), ("match_iou", C.c_double)]


# name -> (restype, argtypes); every symbol include/pnyolo.h declares
SIGNATURES = {
    "pny_version": (C.c_int, []),
    "pny_last_error": (C.c_char_p, []),
    "pny_model_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(ModelDesc)]),
    "pny_model_destroy": (None, [C.c_void_p]),
    "pny_model_load_weights": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, c_i64_p, C.c_int]),
    "pny_model_finalize": (C.c_int, [C.c_void_p]),
    "pny_model_use_fine": (C.c_int, [C.c_void_p, C.c_int]),
    "pny_model_bind_param": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p]),
    "pny_model_refresh": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pny_scene_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p]),
    "pny_scene_destroy": (None, [C.c_void_p]),
    "pny_scene_set_groups": (C.c_int, [C.c_void_p, C.c_int]),
    "pny_scene_set_cameras": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                        C.c_int, C.c_int]),
    "pny_scene_set_latent": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "pny_latent_levels": (C.c_int, [C.POINTER(C.c_void_p), c_int_p, c_int_p, c_int_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pny_latent_levels_backward": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), c_int_p, c_int_p, c_int_p, C.c_int, C.c_int, C.c_void_p]),
    "pny_scene_set_latent_levels": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), c_int_p, c_int_p, c_int_p, C.c_int, C.c_int,
                                              C.c_void_p]),
    "pny_scene_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "pny_scenes_encode": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "pny_scene_get_latent": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pny_scene_latent_shape": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_int)] * 4),
    "pny_gen_rays": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, c_float_p, c_float_p, C.c_float, C.c_float,
                               C.c_int, C.c_void_p, C.c_void_p]),
    "pny_gen_rays_range": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, c_float_p, c_float_p, C.c_float, C.c_float,
                                     C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "pny_sample_train_batch": (C.c_int, [C.POINTER(TrainBatchDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.POINTER(TrainBatchDraws), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pny_yolo_train_batch": (C.c_int, [C.POINTER(YoloBatchDesc), C.c_void_p, c_i64_p, c_float_p, c_float_p, C.POINTER(C.c_void_p),
                                       C.c_void_p, C.c_void_p, c_i64_p, C.c_void_p]),
    "pny_query": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "pny_render": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(RenderOpts), C.POINTER(RenderOut),
                             C.c_void_p]),
    "pny_yolo_render": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    "pny_sample_coarse": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p,
                                    C.c_void_p]),
    "pny_composite": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "pny_sample_fine": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                                  C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                  C.c_void_p, C.c_void_p]),
    "pny_yolo_aggregate": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pny_cells_to_bboxes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                      C.c_void_p]),
    "pny_nms": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                          C.c_void_p]),
    "pny_tp_fp_fn": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double,
                               C.c_void_p, C.c_void_p]),
    "pny_detect_views": (C.c_int, [C.POINTER(DetectViewsDesc), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), c_float_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "pny_detect_sweep": (C.c_int, [C.POINTER(DetectViewsDesc), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), c_float_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_double), C.c_int32,
                                   C.POINTER(C.c_double), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pny_scene_set_projection": (C.c_int, [C.c_void_p, C.c_int]),
    "pny_scene_set_precision": (C.c_int, [C.c_void_p, C.c_int]),
    "pny_scene_bind_latent_grad": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pny_scene_last_precision": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "pny_scene_last_backward_precision": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "pny_model_set_deterministic": (C.c_int, [C.c_void_p, C.c_int]),
    "pny_scene_last_latent_grad_mode": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "pny_model_range_status": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint), C.c_int]),
    "pny_trunk_train_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p]),
    "pny_trunk_train_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "pny_trunk_unit": (C.c_int, [C.c_int] + [C.POINTER(C.c_int)] * 5),
    "pny_trunk_conv": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 3 + [C.c_int, C.c_void_p,
                                 C.POINTER(C.c_int), C.c_void_p]),
    "pny_trunk_conv_dw": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int), c_i64_p,
                                    C.c_void_p]),
    "pny_trunk_bn_forward": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pny_trunk_bn_backward": (C.c_int, [C.c_void_p] * 6 + [C.c_int64, C.c_int, C.c_int] + [C.c_void_p] * 5),
    "pny_trunk_maxpool": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pny_trunk_maxpool_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pny_trunk_upsample": (C.c_int, [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_void_p]),
    "pny_trunk_upsample_backward": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_void_p]),
    "pny_scene_project": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pny_scene_projection": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int), C.c_void_p]),
    "pny_scene_last_mlp_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                           C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "pny_scene_enable_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "pny_scene_last_backward_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pny_yolo_render_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p,
                                           C.c_void_p, C.c_int, C.c_void_p]),
    "pny_model_defer_weight_grads": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int64]),
    "pny_scene_stash_next_render": (C.c_int, [C.c_void_p, C.c_int]),
    "pny_model_flush_weight_grads": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "pny_model_last_flush_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pny_model_last_flush_precision": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "pny_model_bind_grad": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p]),
    "pny_query_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "pny_composite_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pny_render_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(RenderOpts), C.POINTER(RenderSaved),
                                      C.POINTER(RenderGrads), C.c_int, C.c_void_p]),
    "pny_scene_last_depth_sel": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "pny_locate_depth_samples": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                                           C.c_float, C.c_void_p, C.c_void_p]),
    "pny_depth_grad_gather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "pny_yolo_aggregate_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pny_optim_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "pny_optim_destroy": (None, [C.c_void_p]),
    "pny_optim_add_tensor": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "pny_optim_adam_step": (C.c_int, [C.c_void_p, C.POINTER(AdamHyper), C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_void_p,
                                      C.c_void_p]),
    "pny_rgb_loss": (C.c_int, [C.POINTER(RgbLossDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p]),
    "pny_yolo_loss": (C.c_int, [C.POINTER(YoloLossDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p]),
    "pny_yolo_loss_batches": (C.c_int, [C.POINTER(YoloLossDesc), C.POINTER(YoloBatchesDesc), C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pny_yolo_loss_batches_count": (C.c_int, [C.POINTER(YoloBatchesDesc)]),
    "pny_finite_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "pny_finite_destroy": (None, [C.c_void_p]),
    "pny_finite_add_tensor": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int]),
    "pny_finite_check": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pny_finite_check_tensors": (C.c_int, [C.POINTER(C.c_void_p), c_i64_p, C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.c_void_p]),
    "pny_finite_reset": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "pny_view_metrics": (C.c_int, [C.POINTER(ViewMetricsDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pny_lpips_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "pny_lpips_destroy": (None, [C.c_void_p]),
    "pny_lpips_load_weights": (C.c_int, [C.c_void_p, C.c_char_p, c_float_p, c_i64_p, C.c_int]),
    "pny_lpips_finalize": (C.c_int, [C.c_void_p, C.c_void_p]),
    "pny_lpips_workspace_bytes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "pny_lpips_forward": (C.c_int, [C.c_void_p, C.POINTER(LpipsDesc), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "pny_lpips_prepare": (C.c_int, [C.POINTER(LpipsDesc), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "pny_lpips_maxpool2": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pny_lpips_distance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pny_lpips_conv": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int),
                                 C.c_void_p]),
    "pny_color_jitter": (C.c_int, [C.POINTER(ColorJitterDesc), C.c_void_p, c_float_p, C.c_void_p, C.c_void_p]),
    "pny_ingest_views": (C.c_int, [C.POINTER(IngestDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pny_yolo_build_targets": (C.c_int, [C.POINTER(YoloTargetsDesc), C.c_void_p, C.c_void_p, c_float_p, C.POINTER(C.c_void_p),
                                         C.c_void_p]),
    "pny_resident_train_batch": (C.c_int, [C.POINTER(TrainBatchDesc), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                           C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.POINTER(TrainBatchDraws), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pny_ingest_views_indexed": (C.c_int, [C.POINTER(IngestDesc), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "pny_grid_points": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int64, C.c_int64, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    "pny_mc_workspace_bytes": (C.c_int, [C.POINTER(C.c_int32), c_i64_p]),
    "pny_mc_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pny_mc_emit": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_float, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                              C.c_void_p]),
    "pny_occupancy_words": (C.c_int, [C.POINTER(C.c_int32), c_i64_p]),
    "pny_occupancy_build": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_float, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "pny_occupancy_classify_workspace_bytes": (C.c_int, [C.c_int64, c_i64_p]),
    "pny_occupancy_classify": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                         C.c_void_p]),
    "pny_scene_set_occupancy": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                          C.c_int, C.c_void_p]),
    "pny_scene_last_cull": (C.c_int, [C.c_void_p, c_i64_p, c_i64_p]),
    "pny_scene_set_termination": (C.c_int, [C.c_void_p, C.c_float, C.c_int]),
    "pny_scene_last_segments": (C.c_int, [C.c_void_p, C.c_int, c_i64_p, c_i64_p, C.c_int, C.POINTER(C.c_int)]),
    "pny_termination_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "pny_occupancy_classify_segment": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
}

_lib = None
ABI_VERSION = 11
OK, ERR_ARG, ERR_STATE, ERR_HIP, ERR_NOGPU, ERR_RANGE = 0, -1, -2, -3, -4, -5   # pny_status
PROJECTION = {"off": 0, "on": 1, "auto": 2}
# f16: opt-in single-plane mode for no-grad launches, f16_train: the same for training too; both outside the 1e-4 parity bar
PRECISION = {"f32": 0, "f16x2": 1, "auto": 2, "f16": 3, "f16_train": 5}
LAST_PRECISION = {0: "f32", 1: "f16x2", 2: "f16"}   # pny_scene_last_precision, pny_scene_last_backward_precision
PROJECTION_ROUTE_TILED = {1: "f32", 2: "f16x2"}     # pny_scene_projection: PNY_PROJECTION_ROUTE_TILED_*; >= 111: the 1x1 convolution


RANGE_BITS = {1: "activation", 2: "gradient", 4: "weight"}   # include/pnyolo.h PNY_RANGE_*
YOLO_BATCH_MAX_VIEWS, YOLO_BATCH_MAX_SCALES = 16, 4           # PNY_YOLO_BATCH_MAX_*
FINITE_NAN, FINITE_INF, FINITE_MAX_IMMEDIATE = 1, 2, 8        # PNY_FINITE_*
GT_LAYOUT = {"nhwc01": 0, "nchw_pm1": 1}                      # PNY_GT_NHWC_01, PNY_GT_NCHW_PM1
GT_FLAT, METRICS_WIN = 2, 7                                   # PNY_GT_FLAT (util.psnr's form); the SSIM window of this build
# pny_lpips_desc::pred_kind / gt_kind (PNY_LPIPS_*), the smallest image side, the channels of the 13 convolutions and 5 taps
LPIPS_KIND = {"nhwc01": 0, "nchw_pm1": 1, "u8": 2, "nchw01": 3}
LPIPS_MIN_SIZE = 16
LPIPS_CIN = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512)
LPIPS_COUT = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
LPIPS_TAP_CH = (64, 128, 256, 512, 512)
VGG16_FEATURES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)   # torchvision vgg16().features: indices of the convolutions
VGG16_SLICE = (1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5)               # the lpips package's slice of each
IMG_F32_NCHW_PM1, IMG_U8_NHWC, JITTER_MAX_OBJS = 0, 1, 64     # PNY_IMG_*, PNY_JITTER_MAX_OBJS
RESIZE = {"none": 0, "bilinear_u8": 1, "area": 2}             # PNY_RESIZE_*
YOLO_TARGETS_MAX_ANCHORS = 64                                 # PNY_YOLO_TARGETS_MAX_ANCHORS
# pny_detect_views: candidates of one list of one view (PNY_DETECT_MAX_CANDIDATES: 53 bytes of LDS each), its input forms, the
# columns of a view's record and its status bits (PNY_DETECT_*)
DETECT_MAX_CANDIDATES, DETECT_MAX_ANCHORS = 2048, 4
DETECT_CELLS, DETECT_BOXES = 0, 1
DETECT_RECORD = ("tp", "fp", "fn", "kept_targets", "kept_preds", "targets_above", "preds_above", "status")
DETECT_TARGETS_OVERFLOW, DETECT_PREDS_OVERFLOW, DETECT_BAD_SEGMENT = 1, 2, 4
# pny_detect_sweep: the most NMS IoUs, confidence cuts and match IoUs of one sweep (the header states them in its comment), and
# the columns of its three outputs
DETECT_SWEEP_MAX_NMS_IOUS, DETECT_SWEEP_MAX_CUTS, DETECT_SWEEP_MAX_MATCH_IOUS = 8, 32, 8
DETECT_SWEEP_COUNTS = ("tp", "fp", "fn")
DETECT_SWEEP_LISTS = ("kept_targets", "kept_preds", "status")
DETECT_SWEEP_TOTALS = ("tp", "fp", "fn", "refused")
MC_SCAN_TILE, MC_MAX_POINTS = 1024, (2 ** 31 - 1) // 3        # csrc/pny_recon.h: points per scan tile; 3 X Y Z < 2^31
MAX_LATENT_LEVELS = 8                                         # PNY_MAX_LATENT_LEVELS
# bits of the `accumulate` argument of the backward calls and of pny_model_flush_weight_grads (include/pnyolo.h)
ACC_ADD, ACC_IMMEDIATE, ACC_FINE_ONLY, ACC_COARSE_ONLY = 1, 2, 4, 8    # PNY_ACC_*
FLUSH_COARSE_ONLY, FLUSH_FINE_ONLY = 16, 32                            # PNY_FLUSH_*


class PnyError(RuntimeError):
    pass


class PnyRangeError(PnyError):
    """An f16 (F16X2 / F16) launch met a value outside the f16 range (include/pnyolo.h pny_model_range_status)."""


def build(verbose=False):
    """Compile libpnyolo.so for gfx950 (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j4"]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
    if res.returncode != 0:
        raise PnyError("building libpnyolo.so failed (see output above)")
    return LIB_PATH


def load():
    """dlopen libpnyolo.so and type every entry point.  Raises if the library was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PnyError(
            "libpnyolo.so not found at %s: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback for the HIP path)" % LIB_PATH)
    # torch ships its own libamdhip64; it must be loaded FIRST so that libpnyolo.so binds to the
    # same HIP runtime instance -- streams and device pointers are shared across the boundary.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.pny_version() != ABI_VERSION:
        raise PnyError("libpnyolo.so ABI version mismatch")
    _lib = lib
    return lib


def check(rc):
    if rc == ERR_RANGE:
        raise PnyRangeError("libpnyolo: %s (status %d)" % (load().pny_last_error().decode("utf-8", "replace"), rc))
    if rc != 0:
        raise PnyError("libpnyolo: %s (status %d)" % (load().pny_last_error().decode("utf-8", "replace"), rc))


def _get_int(fn, handle):
    """The value of a one-integer getter ``int fn(handle, int* out)``."""
    v = C.c_int(0)
    check(fn(handle, C.byref(v)))
    return int(v.value)


def ptr(t):
    """Raw device / host pointer of a contiguous fp32 torch tensor (or None)."""
    if t is None:
        return None
    import torch
    assert t.dtype == torch.float32 and t.is_contiguous(), "libpnyolo takes contiguous fp32 tensors"
    return C.c_void_p(t.data_ptr())


def stream_of(device):
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
