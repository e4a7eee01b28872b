"""
The training-time colour jitter on the library's kernel (csrc/augment.hip): what ``data.ColorJitterDataset`` (reference
src/data/data_util.py:13-55) does to every item on the host -- one (hue, saturation, brightness, contrast) draw per object,
applied to all of its views as four passes per view -- as ONE launch for all objects and views of a batch, on the current
stream, with nothing waiting for the device:

  color_jitter(images, factors, out=None) -> (SB, NV, 3, H, W) or (NV, 3, H, W) fp32 in [-1, 1]

The factors are drawn on the host exactly as before (``data.ColorJitterDataset(defer=True)`` puts them into
``data["jitter"]``).  The arithmetic is this project's ``data.adjust_*`` in fp32 with the contrast mean summed in fp64; the
same input gives the same bits on every run, for an image alone as for the same image inside a batch.  Device tensors on an
MI355X only; there is no CPU path and no fallback (the host path is ``data.ColorJitterDataset`` itself).

``ingest_views`` (csrc/ingest.hip) is the step before it: decoded ``uint8`` views to the normalised fp32 NCHW tensor, with the
resize of ``data.YOLODataset`` (``data.resize_bilinear_u8``) or of ``data.SRNDataset`` (area) and SRN's white-background mask and
bounding boxes, in one launch (two with the mask):

  ingest_views(images_u8, size=None, scale=None, resize=None, white_mask=False, jitter=None, out=None)
      -> images (..., 3, OH, OW), or (images, masks (..., 1, OH, OW), bbox (..., 4)) with white_mask
"""
import ctypes as C

import numpy as np
import torch

from . import lib as _lib
from .lib import ColorJitterDesc, check, stream_of

_WHO = "pixel_nerf_yolo_amd.augment.color_jitter: "


def _factors(factors, sb):
    """(SB, 4) contiguous fp32 numpy array of host factors, or an error that names the argument."""
    if isinstance(factors, torch.Tensor):
        if factors.device.type != "cpu":
            raise _lib.PnyError(_WHO + "factors is on %s; the factors are host values (they travel in the kernel arguments)"
                                % factors.device)
        factors = factors.detach().numpy()
    f = np.ascontiguousarray(np.asarray(factors, dtype=np.float32))
    if f.shape == (4,) and sb == 1:
        f = f.reshape(1, 4)
    if f.shape != (sb, 4):
        raise ValueError(_WHO + "factors has shape %s; %d object%s need%s (%d, 4) {hue, saturation, brightness, contrast}%s"
                         % (tuple(f.shape), sb, "" if sb == 1 else "s", "s" if sb == 1 else "", sb, " or (4,)" if sb == 1 else ""))
    return f


def color_jitter(images, factors, out=None):
    """
    :param images  device tensor: (NV, 3, H, W) or (SB, NV, 3, H, W) fp32 in [-1, 1] (the datasets' ``images``), or
                   (NV, H, W, 3) or (SB, NV, H, W, 3) uint8 (decoded images as ``data.imread`` returns them)
    :param factors host tensor, array or list, (SB, 4) -- (4,) for one object -- {hue, saturation, brightness, contrast} per
                   object: |hue| <= 0.5, the others finite and >= 0
    :param out     fp32 (..., 3, H, W) device tensor to write, contiguous; ``out=images`` jitters fp32 images in place
    :return the jittered images, fp32 (..., 3, H, W) in [-1, 1] (``out`` if given)
    """
    if not isinstance(images, torch.Tensor):
        raise TypeError(_WHO + "images must be a tensor, got %s" % type(images).__name__)
    if images.dtype not in (torch.float32, torch.uint8):
        raise _lib.PnyError(_WHO + "images must be fp32 (NCHW in [-1, 1]) or uint8 (NHWC), got %s" % images.dtype)
    is_bytes = images.dtype == torch.uint8
    if images.dim() not in (4, 5) or images.shape[-1 if is_bytes else -3] != 3 or images.numel() == 0:
        raise ValueError(_WHO + "images must be %s, got %s %s"
                         % ("(NV, H, W, 3) or (SB, NV, H, W, 3) for uint8" if is_bytes else "(NV, 3, H, W) or (SB, NV, 3, H, W) for fp32",
                            tuple(images.shape), images.dtype))
    sb = int(images.shape[0]) if images.dim() == 5 else 1
    nv = int(images.shape[-4])
    h, w = (int(v) for v in (images.shape[-3:-1] if is_bytes else images.shape[-2:]))
    f = _factors(factors, sb)
    if images.device.type != "cuda":
        raise _lib.PnyError(_WHO + "images is on %s; the jitter runs on an MI355X only (the host path is data.ColorJitterDataset)"
                            % images.device)
    want = tuple(images.shape[:-3]) + (3, h, w)
    if out is None:
        out = torch.empty(want, device=images.device, dtype=torch.float32)
    else:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != want:
            raise ValueError(_WHO + "out must be an fp32 tensor of shape %s, got %s"
                             % (want, "%s %s" % (tuple(out.shape), out.dtype) if isinstance(out, torch.Tensor) else type(out).__name__))
        if out.device != images.device:
            raise _lib.PnyError(_WHO + "out is on %s, images on %s" % (out.device, images.device))
        if not out.is_contiguous():
            raise ValueError(_WHO + "out must be contiguous")
    src = images.detach()
    if not src.is_contiguous():
        src = src.contiguous()
    fn = _lib.load().pny_color_jitter
    per_obj_in, per_obj_out = nv * h * w * 3 * src.element_size(), nv * h * w * 3 * 4
    with torch.cuda.device(images.device):
        st = stream_of(images.device)
        for o in range(0, sb, _lib.JITTER_MAX_OBJS):
            n = min(_lib.JITTER_MAX_OBJS, sb - o)
            desc = ColorJitterDesc(n_objs=n, n_views=nv, height=h, width=w,
                                   in_format=_lib.IMG_U8_NHWC if is_bytes else _lib.IMG_F32_NCHW_PM1)
            check(fn(C.byref(desc), C.c_void_p(src.data_ptr() + o * per_obj_in), f[o:o + n].ctypes.data_as(_lib.c_float_p),
                     C.c_void_p(out.data_ptr() + o * per_obj_out), st))
    return out


_WHO_IN = "pixel_nerf_yolo_amd.augment.ingest_views: "


def _two(v, name, kind):
    try:
        a, b = (kind(x) for x in v)
    except (TypeError, ValueError):
        raise ValueError(_WHO_IN + "%s must be a pair, got %r" % (name, v))
    return a, b


def ingest_views(images_u8, size=None, scale=None, resize=None, white_mask=False, jitter=None, out=None):
    """
    :param images_u8  device tensor (NV, H, W, C) or (SB, NV, H, W, C) uint8, C = 3 or 4 (alpha is ignored): decoded views as
                      ``data.imread`` returns them.  Views are independent: SB folds into NV
    :param scale      (fx, fy): bilinear resize to round(H fy) x round(W fx), ``data.resize_bilinear_u8`` (the ``yolo`` dataset)
    :param size       (OH, OW), with ``resize`` "area" (``F.interpolate(mode="area")``, the ``srn`` dataset) or "bilinear_u8"
    :param resize     None (no resize; "bilinear_u8" when ``scale`` is given), "none", "bilinear_u8" or "area"
    :param white_mask also SRN's mask (1 where no byte of the pixel is 255) and its boxes [cmin, rmin, cmax, rmax], scaled like
                      the dataset's; a view with an empty mask gets [W, H, -1, -1] (the host path raises there; nothing waits
                      for the device here, so test ``bbox[..., 2] < 0``)
    :param jitter     factors for ``color_jitter``, applied in place behind the ingest as a second launch
    :param out        fp32 (..., 3, OH, OW) device tensor to write, contiguous
    :return images fp32 (..., 3, OH, OW) in [-1, 1]; with white_mask (images, masks (..., 1, OH, OW), bbox (..., 4))
    """
    if not isinstance(images_u8, torch.Tensor):
        raise TypeError(_WHO_IN + "images_u8 must be a tensor, got %s" % type(images_u8).__name__)
    if images_u8.dtype != torch.uint8:
        raise _lib.PnyError(_WHO_IN + "images_u8 must be uint8 (NHWC, as decoded), got %s" % images_u8.dtype)
    if images_u8.dim() not in (4, 5) or images_u8.shape[-1] not in (3, 4) or images_u8.numel() == 0:
        raise ValueError(_WHO_IN + "images_u8 must be (NV, H, W, C) or (SB, NV, H, W, C) with C = 3 or 4, got %s"
                         % (tuple(images_u8.shape),))
    lead = tuple(images_u8.shape[:-3])
    h, w, ch = (int(v) for v in images_u8.shape[-3:])
    if resize is not None and resize not in _lib.RESIZE:
        raise ValueError(_WHO_IN + "resize must be None, 'none', 'bilinear_u8' or 'area', got %r" % (resize,))
    if scale is not None and size is not None:
        raise ValueError(_WHO_IN + "scale and size are both given; scale=(fx, fy) or size=(OH, OW)")
    if scale is not None:
        if resize not in (None, "bilinear_u8"):
            raise ValueError(_WHO_IN + "scale goes with resize='bilinear_u8' (cv2's output-size rule), got resize=%r" % (resize,))
        fx, fy = _two(scale, "scale", float)
        oh, ow, mode = int(round(h * fy)), int(round(w * fx)), "bilinear_u8"
        if oh < 1 or ow < 1:
            raise ValueError(_WHO_IN + "scale %r gives an empty %d x %d output" % (tuple(scale), oh, ow))
    elif size is not None:
        if resize not in ("area", "bilinear_u8"):
            raise ValueError(_WHO_IN + "size needs resize='area' or resize='bilinear_u8', got resize=%r" % (resize,))
        oh, ow = _two(size, "size", int)
        mode = resize
        if oh < 1 or ow < 1:
            raise ValueError(_WHO_IN + "size must be positive, got %r" % (tuple(size),))
    else:
        if resize not in (None, "none"):
            raise ValueError(_WHO_IN + "resize=%r needs size=(OH, OW)%s" % (resize, " or scale=(fx, fy)" if resize == "bilinear_u8" else ""))
        oh, ow, mode = h, w, "none"
    if white_mask and mode == "bilinear_u8":
        raise ValueError(_WHO_IN + "white_mask goes with resize='area' or no resize (no dataset resizes a mask bilinearly)")
    if images_u8.device.type != "cuda":
        raise _lib.PnyError(_WHO_IN + "images_u8 is on %s; the ingest runs on an MI355X only (the host path is data.py's datasets)"
                            % images_u8.device)
    want = lead + (3, oh, ow)
    if out is None:
        out = torch.empty(want, device=images_u8.device, dtype=torch.float32)
    else:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != want:
            raise ValueError(_WHO_IN + "out must be an fp32 tensor of shape %s, got %s"
                             % (want, "%s %s" % (tuple(out.shape), out.dtype) if isinstance(out, torch.Tensor) else type(out).__name__))
        if out.device != images_u8.device:
            raise _lib.PnyError(_WHO_IN + "out is on %s, images_u8 on %s" % (out.device, images_u8.device))
        if not out.is_contiguous():
            raise ValueError(_WHO_IN + "out must be contiguous")
    src = images_u8.detach()
    if not src.is_contiguous():
        src = src.contiguous()
    nv = src.numel() // (h * w * ch)
    masks = bbox = None
    if white_mask:
        masks = torch.empty(lead + (1, oh, ow), device=src.device, dtype=torch.float32)
        bbox = torch.empty(lead + (4,), device=src.device, dtype=torch.float32)
    desc = _lib.IngestDesc(n_views=nv, height=h, width=w, channels=ch, out_height=oh, out_width=ow, resize=_lib.RESIZE[mode],
                           white_mask=int(bool(white_mask)))
    with torch.cuda.device(src.device):
        check(_lib.load().pny_ingest_views(C.byref(desc), C.c_void_p(src.data_ptr()), C.c_void_p(out.data_ptr()),
                                           None if masks is None else C.c_void_p(masks.data_ptr()),
                                           None if bbox is None else C.c_void_p(bbox.data_ptr()), stream_of(src.device)))
    if jitter is not None:
        color_jitter(out, jitter, out=out)
    return (out, masks, bbox) if white_mask else out
