"""
Scoring rendered views against the ground truth on the library's kernel (csrc/metrics.hip): the last step of the reference's
eval scripts (eval/eval.py:288-345, eval/calc_metrics.py:189-191), which bring every render to the host, clamp it, truncate
it to bytes for the PNG and call skimage's ``compare_ssim(multichannel=True, data_range=1)`` and ``compare_psnr(data_range=1)``
per view.  Here the renders stay on the device, one launch scores all views of an object, and nothing waits for the device:

  compare_views(rgb, gt, ...) -> ViewMetrics(psnr, ssim, rgb8)   (NV,) float64, (NV,) float64, (NV, H, W, 3) uint8 | None
  psnr(pred, target)          -> 0-dim float64                    the reference's util.psnr (src/util/util.py:502-509)

The prediction is clamped to [0, 1] in fp32; a NaN prediction makes both metrics of its view NaN and writes byte 0.  SSIM is
skimage's definition for win_size 7 (uniform window, sample covariance, K1 = 0.01, K2 = 0.03), sums in fp64; identical images
give PSNR +inf.  Results are bit-identical from run to run.  fp32 tensors on an MI355X only; there is no CPU path and no
fallback.
"""
import collections
import ctypes as C

import torch

from . import lib as _lib
from .lib import ViewMetricsDesc, check, stream_of

ViewMetrics = collections.namedtuple("ViewMetrics", ("psnr", "ssim", "rgb8"))


def _f32(t, what):
    """An fp32 tensor, or an error that names the argument.  (Type and shape are refused before the device is looked at.)"""
    if not isinstance(t, torch.Tensor):
        raise TypeError("pixel_nerf_yolo_amd.metrics: %s must be a tensor, got %s" % (what, type(t).__name__))
    if t.dtype != torch.float32:
        raise _lib.PnyError("pixel_nerf_yolo_amd.metrics: %s must be fp32, got %s" % (what, t.dtype))
    return t.detach()


def _dev(t, what, device=None):
    """The tensor, contiguous, on an MI355X (made contiguous if it is not), or an error that names the argument."""
    if t.device.type != "cuda":
        raise _lib.PnyError("pixel_nerf_yolo_amd.metrics: %s is on %s; the metrics run on an MI355X only (there is no CPU path)"
                            % (what, t.device))
    if device is not None and t.device != device:
        raise _lib.PnyError("pixel_nerf_yolo_amd.metrics: %s is on %s, the prediction on %s" % (what, t.device, device))
    return t.contiguous()


def _launch(desc, rgb, gt, out, rgb8):
    dev = rgb.device
    with torch.cuda.device(dev):
        check(_lib.load().pny_view_metrics(C.byref(desc), C.c_void_p(rgb.data_ptr()), C.c_void_p(gt.data_ptr()),
                                           None if out is None else C.c_void_p(out.data_ptr()),
                                           None if rgb8 is None else C.c_void_p(rgb8.data_ptr()), stream_of(dev)))


def compare_views(rgb, gt, gt_layout="nhwc01", want_uint8=True, H=None, W=None, want_metrics=True):
    """
    :param rgb (NV, H, W, 3) renders, or (NV * H * W, 3) as the renderer returns them, with H and W given
    :param gt  "nhwc01": (NV, H, W, 3) in [0, 1], taken as given (calc_metrics.py);
               "nchw_pm1": (NV, 3, H, W) in [-1, 1], the dataset's ``images`` (eval.py:315 forms images * 0.5 + 0.5)
    :param want_uint8 also return ``(clamp(rgb, 0, 1) * 255).astype(uint8)`` (eval.py:288-291), the PNG writer's input
    :param want_metrics False: convert only (psnr and ssim are None)
    :return ViewMetrics(psnr (NV,) float64, ssim (NV,) float64, rgb8 (NV, H, W, 3) uint8 or None), all on rgb's device
    """
    if gt_layout not in _lib.GT_LAYOUT:
        raise ValueError("pixel_nerf_yolo_amd.metrics.compare_views: gt_layout must be one of %s, got %r"
                         % (sorted(_lib.GT_LAYOUT), gt_layout))
    if not want_uint8 and not want_metrics:
        raise ValueError("pixel_nerf_yolo_amd.metrics.compare_views: neither the metrics nor the 8-bit image is asked for")
    rgb, gt = _f32(rgb, "rgb"), _f32(gt, "gt")
    if rgb.dim() == 2 and H is not None and W is not None:
        if rgb.shape[1] != 3 or rgb.shape[0] == 0 or rgb.shape[0] % (H * W):
            raise ValueError("pixel_nerf_yolo_amd.metrics.compare_views: rgb %s is not (NV * %d * %d, 3)" % (tuple(rgb.shape), H, W))
        rgb = rgb.reshape(-1, H, W, 3)
    if rgb.dim() != 4 or rgb.shape[3] != 3 or rgb.shape[0] == 0:
        raise ValueError("pixel_nerf_yolo_amd.metrics.compare_views: rgb must be (NV, H, W, 3), or (NV * H * W, 3) with H and W "
                         "given; got %s" % (tuple(rgb.shape),))
    NV, H, W = (int(v) for v in rgb.shape[:3])
    want = (NV, H, W, 3) if gt_layout == "nhwc01" else (NV, 3, H, W)
    if tuple(gt.shape) != want:
        raise ValueError("pixel_nerf_yolo_amd.metrics.compare_views: gt has shape %s, gt_layout %r of rgb %s needs %s"
                         % (tuple(gt.shape), gt_layout, tuple(rgb.shape), want))
    if H < _lib.METRICS_WIN or W < _lib.METRICS_WIN:
        raise ValueError("pixel_nerf_yolo_amd.metrics.compare_views: H and W must be at least the SSIM window, %d; got %d x %d"
                         % (_lib.METRICS_WIN, H, W))
    rgb = _dev(rgb, "rgb")
    gt = _dev(gt, "gt", rgb.device)
    out = torch.empty(NV, 2, device=rgb.device, dtype=torch.float64) if want_metrics else None
    rgb8 = torch.empty(NV, H, W, 3, device=rgb.device, dtype=torch.uint8) if want_uint8 else None
    desc = ViewMetricsDesc(n_views=NV, height=H, width=W, gt_layout=_lib.GT_LAYOUT[gt_layout], win_size=_lib.METRICS_WIN)
    _launch(desc, rgb, gt, out, rgb8)
    return ViewMetrics(None if out is None else out[:, 0], None if out is None else out[:, 1], rgb8)


def psnr(pred, target):
    """The reference's util.psnr (src/util/util.py:502-509), ``-10 * log10(mean((pred - target) ** 2))`` over all elements, no
    clamp, on device tensors: one view of the same kernel with the SSIM part off.  Difference, squares and mean in fp64.
    :return 0-dim float64 device tensor (the reference returns a Python float; ``float(...)`` is the one host wait)"""
    pred, target = _f32(pred, "pred"), _f32(target, "target")
    if pred.shape != target.shape:
        raise ValueError("pixel_nerf_yolo_amd.metrics.psnr: target has shape %s, pred %s (no broadcasting)"
                         % (tuple(target.shape), tuple(pred.shape)))
    if pred.numel() == 0:
        raise ValueError("pixel_nerf_yolo_amd.metrics.psnr: pred is empty")
    if pred.numel() >= 2 ** 31:
        raise ValueError("pixel_nerf_yolo_amd.metrics.psnr: 2^31 elements or more")
    pred = _dev(pred, "pred")
    target = _dev(target, "target", pred.device)
    out = torch.empty(1, 2, device=pred.device, dtype=torch.float64)
    desc = ViewMetricsDesc(n_views=1, height=1, width=pred.numel(), gt_layout=_lib.GT_FLAT, win_size=_lib.METRICS_WIN)
    _launch(desc, pred, target, out, None)
    return out[0, 0]
