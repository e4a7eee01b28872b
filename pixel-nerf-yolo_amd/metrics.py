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

The third number of the eval tail, LPIPS on VGG-16 (calc_metrics.py:186-246), runs on the device too (csrc/lpips.hip):

  LPIPS(net="vgg")(in0, in1, normalize=False) -> (N, 1, 1, 1) fp32    the lpips package's call
  lpips_views(model, rgb, gt, ...)            -> (NV,) float64         in compare_views' shapes, plus uint8 images
"""
import collections
import ctypes as C
import re

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


# ------------------------------------------------------------------------------------------------------------ LPIPS
LPIPS_SHIFT, LPIPS_SCALE = (-.030, -.088, -.188), (.458, .448, .450)    # the scaling layer, compiled into the library


def lpips_tensor_names():
    """The library's names of the 31 tensors: conv{i}.weight, conv{i}.bias (execution order), lin{k}.weight."""
    return (["conv%d.%s" % (i, p) for i in range(13) for p in ("weight", "bias")] + ["lin%d.weight" % k for k in range(5)])


def _lpips_shape(name):
    family, i = re.fullmatch(r"(conv|lin)(\d+)\.(?:weight|bias)", name).groups()
    i = int(i)
    if family == "lin":
        return (_lib.LPIPS_TAP_CH[i],)
    return (_lib.LPIPS_COUT[i], _lib.LPIPS_CIN[i], 3, 3) if name.endswith("weight") else (_lib.LPIPS_COUT[i],)


def _lpips_host(t, name, key):
    """A weight tensor as contiguous fp32 on the host in the library's shape, or an error that names the key it came from."""
    t = torch.as_tensor(t).detach().to("cpu", torch.float32)
    want = _lpips_shape(name)
    if name.startswith("lin"):
        if t.numel() != want[0]:
            raise ValueError("pixel_nerf_yolo_amd.metrics.LPIPS: %r has shape %s, needs %d elements" % (key, tuple(t.shape), want[0]))
        t = t.reshape(want)
    elif tuple(t.shape) != want:
        raise ValueError("pixel_nerf_yolo_amd.metrics.LPIPS: %r has shape %s, needs %s" % (key, tuple(t.shape), want))
    return t.contiguous()


class LPIPS:
    """
    LPIPS v0.1 on VGG-16 (``lpips.LPIPS(net="vgg")`` in eval mode, ``spatial=False``) on the library's kernels
    (csrc/lpips.hip; the 13 convolutions on the trunk's exact-fp32 MFMA kernel).  No gradients: inputs are detached.  No
    trained weights ship with this project: load the package's state dict, torchvision's VGG-16 plus the five linear layers,
    or tensors (``synth.vgg16_lpips_state`` gives seeded stand-ins).  Any other ``net`` raises NotImplementedError.

    The accepted key names are written down from the public ``lpips`` and ``torchvision`` packages, neither of which is
    available where this library is built and tested: they could not be checked against the packages themselves.
    """

    def __init__(self, net="vgg"):
        if net != "vgg":
            raise NotImplementedError("pixel_nerf_yolo_amd.metrics.LPIPS: net=%r is not implemented, only net='vgg'" % (net,))
        self.net = net
        self.tensors = {}          # library name -> fp32 host tensor
        self._handle = None        # pny_lpips*, created with the first finalize
        self._device = None        # where the weights were finalized
        self._work = None          # the workspace of lpips_views, kept

    def __del__(self):
        if getattr(self, "_handle", None) is not None:
            try:
                _lib.load().pny_lpips_destroy(self._handle)
            except Exception:
                pass
            self._handle = None

    # -------------------------------------------------------------------------------------------- weights
    def _set(self, tensors):
        missing = [n for n in lpips_tensor_names() if n not in tensors]
        if missing:
            raise KeyError("pixel_nerf_yolo_amd.metrics.LPIPS: missing %s" % ", ".join(repr(tensors.source[n]) for n in missing))
        self.tensors = {n: tensors[n] for n in lpips_tensor_names()}
        self._device = None        # finalize again on the next call
        return self

    def load_tensors(self, convs, lins):
        """:param convs 13 (weight (cout, cin, 3, 3), bias (cout)) pairs in execution order; :param lins 5 weights of C elements"""
        if len(convs) != 13 or len(lins) != 5:
            raise ValueError("pixel_nerf_yolo_amd.metrics.LPIPS.load_tensors: convs must hold 13 (weight, bias) pairs and lins 5 "
                             "weights, got %d and %d" % (len(convs), len(lins)))
        t = _Named()
        for i, (w, b) in enumerate(convs):
            t.put("conv%d.weight" % i, w, "convs[%d][0]" % i)
            t.put("conv%d.bias" % i, b, "convs[%d][1]" % i)
        for k, w in enumerate(lins):
            t.put("lin%d.weight" % k, w, "lins[%d]" % k)
        return self._set(t)

    def load_state_dict(self, sd):
        """
        Either the ``lpips`` package's own state dict (``net.slice1.0.weight``, ``net.slice1.2.*``, ``net.slice2.{5,7}.*``,
        ``net.slice3.{10,12,14}.*``, ``net.slice4.{17,19,21}.*``, ``net.slice5.{24,26,28}.*``, ``lin{k}.model.1.weight``; the
        ``lins.{k}.model.1.weight`` duplicates are accepted, the scaling layer's buffers are checked against the compiled-in
        constants and otherwise ignored), or torchvision's ``features.{i}.weight / .bias`` together with
        ``lin{k}.model.1.weight``.  A missing or mis-shaped key is named in the error.
        """
        package = any(k.startswith("net.slice") for k in sd)
        t = _Named()
        for i, (f, s) in enumerate(zip(_lib.VGG16_FEATURES, _lib.VGG16_SLICE)):
            for p in ("weight", "bias"):
                key = ("net.slice%d.%d.%s" % (s, f, p)) if package else ("features.%d.%s" % (f, p))
                t.source["conv%d.%s" % (i, p)] = key
                if key in sd:
                    t.put("conv%d.%s" % (i, p), sd[key], key)
        for k in range(5):
            key = "lin%d.model.1.weight" % k
            if key not in sd and ("lins.%d.model.1.weight" % k) in sd:
                key = "lins.%d.model.1.weight" % k
            t.source["lin%d.weight" % k] = key
            if key in sd:
                t.put("lin%d.weight" % k, sd[key], key)
        for key, want in (("scaling_layer.shift", LPIPS_SHIFT), ("scaling_layer.scale", LPIPS_SCALE)):
            if key in sd:
                got = torch.as_tensor(sd[key]).detach().to("cpu", torch.float32).reshape(-1)
                if got.numel() != 3 or not torch.equal(got, torch.tensor(want, dtype=torch.float32)):
                    raise ValueError("pixel_nerf_yolo_amd.metrics.LPIPS: %r is %s, the library has %s compiled in"
                                     % (key, got.tolist(), list(want)))
        return self._set(t)

    def _ready(self, device):
        """The handle with its weights on `device` (uploaded and packed on first use, and again after new weights)."""
        if not self.tensors:
            raise _lib.PnyError("pixel_nerf_yolo_amd.metrics.LPIPS: no weights loaded (load_state_dict / load_tensors)")
        if self._device == device:
            return self._handle
        L = _lib.load()
        with torch.cuda.device(device):
            if self._handle is None:
                h = C.c_void_p()
                check(L.pny_lpips_create(C.byref(h)))
                self._handle = h
            for name, t in self.tensors.items():
                shape = (C.c_int64 * t.dim())(*t.shape)
                check(L.pny_lpips_load_weights(self._handle, name.encode(), C.cast(C.c_void_p(t.data_ptr()), _lib.c_float_p), shape,
                                               t.dim()))
            check(L.pny_lpips_finalize(self._handle, stream_of(device)))
        self._device, self._work = device, None
        return self._handle

    def _workspace(self, device, batch, H, W):
        """One workspace per model, allocated on the first call and kept: it only grows (a call that needs more bytes than it
        has, or runs on another device, replaces it; smaller shapes reuse it)."""
        need = lpips_workspace_bytes(batch, H, W)
        if self._work is None or self._work.device != device or self._work.numel() < need:
            self._work = None
            self._work = torch.empty(need, device=device, dtype=torch.uint8)
        return self._work

    # -------------------------------------------------------------------------------------------- the package's call
    def __call__(self, in0, in1, normalize=False):
        """
        :param in0, in1 (N, 3, H, W) fp32 in [-1, 1], or in [0, 1] with ``normalize=True`` (then 2 x - 1 is taken first)
        :return (N, 1, 1, 1) fp32 on the inputs' device
        """
        who = "pixel_nerf_yolo_amd.metrics.LPIPS.__call__"
        in0, in1 = _f32(in0, "in0"), _f32(in1, "in1")
        if in0.dim() != 4 or in0.shape[1] != 3 or in0.shape[0] == 0:
            raise ValueError("%s: in0 must be (N, 3, H, W), got %s" % (who, tuple(in0.shape)))
        if in1.shape != in0.shape:
            raise ValueError("%s: in1 has shape %s, in0 %s (no broadcasting)" % (who, tuple(in1.shape), tuple(in0.shape)))
        N, _, H, W = (int(v) for v in in0.shape)
        _check_size(who, H, W)
        in0 = _dev(in0, "in0")
        in1 = _dev(in1, "in1", in0.device)
        kind = "nchw01" if normalize else "nchw_pm1"
        return _lpips_run(self, in0, in1, kind, kind, N, H, W, 32, False).to(torch.float32).reshape(N, 1, 1, 1)


class _Named(dict):
    """library name -> host tensor, with the caller's own name of each for the errors"""

    def __init__(self):
        super().__init__()
        self.source = {n: n for n in lpips_tensor_names()}

    def put(self, name, t, key):
        self.source[name] = key
        self[name] = _lpips_host(t, name, key)


def lpips_workspace_bytes(n_pairs, H, W):
    """pny_lpips_workspace_bytes: the device bytes a batch of n_pairs pairs of H x W needs (runs on the host alone)."""
    b = C.c_size_t(0)
    check(_lib.load().pny_lpips_workspace_bytes(int(n_pairs), int(H), int(W), C.byref(b)))
    return int(b.value)


def _check_size(who, H, W):
    if H < _lib.LPIPS_MIN_SIZE or W < _lib.LPIPS_MIN_SIZE:
        raise ValueError("%s: H and W must be at least %d (relu5_3 would be empty); got %d x %d" % (who, _lib.LPIPS_MIN_SIZE, H, W))


def _lpips_run(model, pred, gt, pred_kind, gt_kind, NV, H, W, batch_size, clamp):
    dev = pred.device
    handle = model._ready(dev)
    batch = min(int(batch_size), NV)
    work = model._workspace(dev, batch, H, W)
    out = torch.empty(NV, device=dev, dtype=torch.float64)
    desc = _lib.LpipsDesc(height=H, width=W, pred_kind=_lib.LPIPS_KIND[pred_kind], gt_kind=_lib.LPIPS_KIND[gt_kind],
                          clamp=1 if clamp else 0, batch_size=batch)
    L = _lib.load()
    with torch.cuda.device(dev):
        st = stream_of(dev)
        for i0 in range(0, NV, batch):
            n = min(batch, NV - i0)
            check(L.pny_lpips_forward(handle, C.byref(desc), C.c_void_p(pred[i0:i0 + n].data_ptr()), C.c_void_p(gt[i0:i0 + n].data_ptr()),
                                      n, C.c_void_p(work.data_ptr()), C.c_void_p(out[i0:].data_ptr()), st))
    return out


def _img(t, what):
    """An fp32 or uint8 image tensor, or an error that names the argument."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("pixel_nerf_yolo_amd.metrics: %s must be a tensor, got %s" % (what, type(t).__name__))
    if t.dtype not in (torch.float32, torch.uint8):
        raise _lib.PnyError("pixel_nerf_yolo_amd.metrics: %s must be fp32 or uint8, got %s" % (what, t.dtype))
    return t.detach()


def lpips_views(model, rgb, gt, gt_layout="nhwc01", H=None, W=None, batch_size=32, clamp=False):
    """
    LPIPS of every rendered view against its ground truth (calc_metrics.py:186-246), in the shapes of ``compare_views``.
    :param model an ``LPIPS`` with weights loaded
    :param rgb (NV, H, W, 3) renders in [0, 1], fp32 or uint8 (``compare_views``' rgb8), or fp32 (NV * H * W, 3) with H and W given
    :param gt  fp32 "nhwc01": (NV, H, W, 3) in [0, 1]; fp32 "nchw_pm1": (NV, 3, H, W) in [-1, 1]; uint8: (NV, H, W, 3) bytes
               whatever gt_layout says
    :param batch_size views per pass of the network (calc_metrics.py's --lpips_batch_size); it sizes the one workspace, which is
               allocated on the first call and kept on the model.  A view's value has the same bits at every batch size.
    :param clamp clamp an fp32 rgb to [0, 1] first (the lpips package does not)
    :return (NV,) float64 on rgb's device; nothing waits for the device
    """
    who = "pixel_nerf_yolo_amd.metrics.lpips_views"
    if not isinstance(model, LPIPS):
        raise TypeError("%s: model must be a metrics.LPIPS, got %s" % (who, type(model).__name__))
    if gt_layout not in _lib.GT_LAYOUT:
        raise ValueError("%s: gt_layout must be one of %s, got %r" % (who, sorted(_lib.GT_LAYOUT), gt_layout))
    if int(batch_size) < 1:
        raise ValueError("%s: batch_size must be at least 1, got %r" % (who, batch_size))
    rgb, gt = _img(rgb, "rgb"), _img(gt, "gt")
    if rgb.dim() == 2 and H is not None and W is not None:
        if rgb.shape[1] != 3 or rgb.shape[0] == 0 or rgb.shape[0] % (H * W):
            raise ValueError("%s: rgb %s is not (NV * %d * %d, 3)" % (who, tuple(rgb.shape), H, W))
        rgb = rgb.reshape(-1, H, W, 3)
    if rgb.dim() != 4 or rgb.shape[3] != 3 or rgb.shape[0] == 0:
        raise ValueError("%s: rgb must be (NV, H, W, 3), or (NV * H * W, 3) with H and W given; got %s" % (who, tuple(rgb.shape)))
    NV, H, W = (int(v) for v in rgb.shape[:3])
    gt_kind = "u8" if gt.dtype == torch.uint8 else gt_layout
    want = (NV, 3, H, W) if gt_kind == "nchw_pm1" else (NV, H, W, 3)
    if tuple(gt.shape) != want:
        raise ValueError("%s: gt has shape %s, %s of rgb %s needs %s"
                         % (who, tuple(gt.shape), "uint8" if gt_kind == "u8" else "gt_layout %r" % gt_layout, tuple(rgb.shape), want))
    _check_size(who, H, W)
    rgb = _dev(rgb, "rgb")
    gt = _dev(gt, "gt", rgb.device)
    return _lpips_run(model, rgb, gt, "u8" if rgb.dtype == torch.uint8 else "nhwc01", gt_kind, NV, H, W, batch_size, clamp)
