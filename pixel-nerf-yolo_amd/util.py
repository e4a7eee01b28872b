"""
Ray generation and the YOLO detection tail with the reference's signatures (src/util/util.py:240-278 ``gen_rays``,
:808-876 ``gen_rays_yolo``), executed by libpnyolo's gen_rays kernel.  Output lives on a CUDA
device (that of ``poses``, or the current one when ``poses`` is a CPU tensor as at the reference's call sites).
``sample_train_batch`` is the trainer's ray batch and ground truth in one launch (no counterpart function in the reference:
it replaces the per-object loop of train/trainlib/PixelNerfTrainer.py:76-123).
"""
import ctypes as C

import torch

from . import lib as _lib
from .lib import check, ptr, stream_of


def _pair(v, name):
    t = torch.as_tensor(v, dtype=torch.float32).detach().cpu().reshape(-1)
    if t.numel() == 1:
        t = t.repeat(2)
    assert t.numel() == 2, "%s must be a scalar or (x, y)" % name
    return (C.c_float * 2)(float(t[0]), float(t[1]))


def _device_of(poses, device):
    """Device the rays are generated on: `device` if given, the device of `poses` if that is a GPU, else the
    current CUDA device -- the reference's call sites pass CPU poses and move the result afterwards
    (eval/eval.py:258 `.to(device=device)`, a no-op then).  No GPU at all is an error: there is no CPU path."""
    if device is not None:
        dev = torch.device(device)
    elif poses.device.type == "cuda":
        dev = poses.device
    elif torch.cuda.is_available():
        dev = torch.device("cuda", torch.cuda.current_device())
    else:
        dev = poses.device
    if dev.type != "cuda":
        raise RuntimeError("libpnyolo needs a cuda device: there is no CPU path")
    return dev


def gen_rays(poses, width, height, focal, z_near, z_far, c=None, ndc=False, device=None):
    """
    :param poses (B, 4, 4) camera-to-world
    :return (B, H, W, 8) [origin(3), unit direction(3), near, far]
    """
    if ndc:
        raise NotImplementedError("ndc=True calls an undefined ndc_rays in the reference (util.py:262): dead branch")
    dev = _device_of(poses, device)
    B = poses.shape[0]
    out = torch.empty(B, height, width, 8, device=dev, dtype=torch.float32)
    f = _pair(focal, "focal")
    cc = _pair([width * 0.5, height * 0.5] if c is None else c, "c")
    p = poses.detach().to("cpu", torch.float32).contiguous()
    check(_lib.load().pny_gen_rays(ptr(p), B, int(width), int(height), f, cc, float(z_near), float(z_far), 0,
                                   ptr(out), stream_of(dev)))
    return out


def gen_rays_range(poses, width, height, focal, z_near, z_far, first_ray, n_rays, c=None, yolo=False, device=None):
    """Rays [first_ray, first_ray + n_rays) of the flattened (B, H, W) pixel grid of ``gen_rays`` (or
    ``gen_rays_yolo`` with yolo=True) -> (n_rays, 8), bit-identical to the corresponding rows of the full call.
    Not part of the reference's interface: it is how a rank of a ray-sharded render (dist.render_frame_sharded)
    produces its own slice of a frame on its own device."""
    dev = _device_of(poses, device)
    B = poses.shape[0]
    out = torch.empty(int(n_rays), 8, device=dev, dtype=torch.float32)
    f = _pair(focal, "focal")
    cc = _pair([width * 0.5, height * 0.5] if c is None else c, "c")
    p = poses.detach().to("cpu", torch.float32).contiguous()
    check(_lib.load().pny_gen_rays_range(ptr(p), B, int(width), int(height), f, cc, float(z_near), float(z_far),
                                         int(bool(yolo)), int(first_ray), int(n_rays), ptr(out), stream_of(dev)))
    return out


def gen_rays_yolo(poses, width, height, focal, c, z_near, z_far, device=None):
    """
    :param poses (B, 4, 4) world-to-camera extrinsics;  focal (2), c (2)
    :return (B, H, W, 8) [origin(3), direction(3) (not normalised), near, far]
    """
    dev = _device_of(poses, device)
    B = poses.shape[0]
    out = torch.empty(B, height, width, 8, device=dev, dtype=torch.float32)
    p = poses.detach().to("cpu", torch.float32).contiguous()
    check(_lib.load().pny_gen_rays(ptr(p), B, int(width), int(height), _pair(focal, "focal"), _pair(c, "c"),
                                   float(z_near), float(z_far), 1, ptr(out), stream_of(dev)))
    return out


# ------------------------------------------------------------------ training batch
def _dev_f32(t, dev):
    """fp32, contiguous, on dev: in place when it already is, else an asynchronous copy (no wait on the host)."""
    return torch.as_tensor(t).detach().to(dev, torch.float32, non_blocking=True).contiguous()


def _dev_i64(t, dev):
    return torch.as_tensor(t).detach().to(dev, torch.int64, non_blocking=True).contiguous()


def sample_train_batch(images, poses, focal, z_near, z_far, ray_batch_size, c=None, bboxes=None, seed=None, draws=None,
                       draw_offset=0):
    """
    The rays of one training step and their ground truth for all SB objects, in one kernel launch: what the reference's
    PixelNerfTrainer.calc_losses:76-123 prepares per object (gen_rays of every view, an NHWC copy of the images, CPU pixel
    indices, two gathers) for the ray_batch_size pixels per object it keeps.  Nothing of size NV * H * W is written and the
    host waits for nothing: GPU inputs are used in place, CPU ``poses`` / ``focal`` / ``c`` / ``bboxes`` are copied over
    asynchronously.

    :param images (SB, NV, 3, H, W) in [-1, 1];  poses (SB, NV, 4, 4) camera-to-world
    :param focal scalar, (SB,) one per object, (1, 2) or (SB, 2);  c None (image centre), (2,), (1, 2) or (SB, 2)
    :param bboxes None: uniform over all pixels of all views (PixelNerfTrainer.py:112); (SB, NV, 4) `cmin rmin cmax rmax`:
           util.bbox_sample (src/util/util.py:222-237)
    :param seed 64-bit Philox seed of the draws; None takes one per call from torch's default (CPU) generator, so
           torch.manual_seed governs a run.  Ray r of object s uses draw index draw_offset + s * ray_batch_size + r.
    :param draws replay instead: {"pix_inds": (SB, B) int64} (uniform) or {"image_ids": (SB, B) int64, "u_x", "u_y":
           (SB, B) float32} (bbox) -- the values torch.randint / torch.rand gave the reference
    :return rays (SB, B, 8), rgb_gt (SB, B, 3) = images * 0.5 + 0.5 at the pixels, pix (SB, B, 3) int32 [view, y, x]
    """
    dev = _device_of(images, None)
    SB, NV, ch, H, W = images.shape
    assert ch == 3 and tuple(poses.shape) == (SB, NV, 4, 4), "images (SB, NV, 3, H, W), poses (SB, NV, 4, 4)"
    B = int(ray_batch_size)
    img, p = _dev_f32(images, dev), _dev_f32(poses, dev)
    f = _dev_f32(focal, dev)
    if f.dim() <= 1:
        assert f.numel() in (1, SB), "focal: a scalar, (SB,), (1, 2) or (SB, 2)"
        f = f.reshape(-1, 1)
    assert f.dim() == 2 and f.shape[0] in (1, SB) and f.shape[1] in (1, 2), "focal: a scalar, (SB,), (1, 2) or (SB, 2)"
    cc = None
    if c is not None:
        cc = _dev_f32(c, dev).reshape(-1, 2)
        assert cc.shape[0] in (1, SB), "c: (2,), (1, 2) or (SB, 2)"
    bb = None
    if bboxes is not None:
        bb = _dev_f32(bboxes, dev)
        assert tuple(bb.shape) == (SB, NV, 4), "bboxes (SB, NV, 4)"
    desc = _lib.TrainBatchDesc(n_objs=SB, n_views=NV, height=H, width=W, n_rays=B, z_near=float(z_near), z_far=float(z_far),
                               focal_rows=f.shape[0], focal_cols=f.shape[1], c_rows=1 if cc is None else cc.shape[0],
                               seed=0, draw_offset=int(draw_offset))
    dr, keep = None, []
    if draws is not None:
        assert seed is None, "draws replay the pixel choice: a seed has no effect"
        names = ("image_ids", "u_x", "u_y") if bb is not None else ("pix_inds",)
        assert set(draws) == set(names), "draws must hold exactly %s" % (names,)
        keep = [(_dev_f32 if n.startswith("u_") else _dev_i64)(draws[n], dev) for n in names]
        assert all(tuple(t.shape) == (SB, B) for t in keep), "draws are (SB, ray_batch_size)"
        dr = _lib.TrainBatchDraws(**{n + "_dev": t.data_ptr() for n, t in zip(names, keep)})
    elif seed is None:
        hi, lo = torch.randint(0, 2 ** 32, (2,), dtype=torch.int64).tolist()   # the CPU generator: nothing to wait for
        desc.seed = (hi << 32) | lo
    else:
        desc.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    rays = torch.empty(SB, B, 8, device=dev, dtype=torch.float32)
    rgb_gt = torch.empty(SB, B, 3, device=dev, dtype=torch.float32)
    pix = torch.empty(SB, B, 3, device=dev, dtype=torch.int32)
    check(_lib.load().pny_sample_train_batch(C.byref(desc), ptr(img), ptr(p), ptr(f), ptr(cc), ptr(bb),
                                             None if dr is None else C.byref(dr), ptr(rays), ptr(rgb_gt),
                                             C.c_void_p(pix.data_ptr()), stream_of(dev)))
    return rays, rgb_gt, pix


# ------------------------------------------------------------------ YOLO detection tail
def _boxes_to_dev(bboxes, dev):
    t = torch.as_tensor(bboxes, dtype=torch.float32).reshape(-1, 6)
    return t.to(dev).contiguous()


def convert_cells_to_bboxes(predictions, anchors, h, w, is_predictions=True, as_tensor=False):
    """reference src/util/util.py:633-689.  predictions (B, h, w, A, 7 | 6) on a cuda device.
    Returns the reference's nested list (B x (A*h*w) x 6: [class, score, x, y, w, h]) or, with
    as_tensor=True, a (B, A*h*w, 6) device tensor (no host round trip)."""
    dev = _device_of(predictions, None)   # the reference's call site hands over CPU tensors (YoloTrainer.py:279-289)
    L = _lib.load()
    p = predictions.detach().to(dev, torch.float32).contiguous()
    B, A = p.shape[0], p.shape[3]
    assert p.shape[1] == h and p.shape[2] == w and p.shape[4] == (7 if is_predictions else 6)
    anc = torch.as_tensor(anchors, dtype=torch.float32).detach().cpu().reshape(-1, 2).contiguous()
    assert anc.shape[0] == A
    out = torch.empty(B, h * w * A, 6, device=dev, dtype=torch.float32)
    for b in range(B):
        check(L.pny_cells_to_bboxes(ptr(p[b]), ptr(anc), h, w, A, int(bool(is_predictions)), ptr(out[b]),
                                    stream_of(dev)))
    return out if as_tensor else out.cpu().tolist()


def nms(bboxes, iou_threshold, threshold, device=None, as_tensor=False):
    """reference src/util/util.py:691-722 -> (kept boxes, highest confidence, boxes above threshold).
    bboxes: list of [class, score, x, y, w, h] or an (n, 6) tensor."""
    dev = torch.device(device) if device is not None else (bboxes.device if torch.is_tensor(bboxes) else torch.device("cuda"))
    b = _boxes_to_dev(bboxes, dev)
    n = b.shape[0]
    if n == 0:
        raise ValueError("max() arg is an empty sequence")  # what the reference raises on an empty list
    L = _lib.load()
    kept = torch.empty(n, 6, device=b.device, dtype=torch.float32)
    meta = torch.zeros(2, device=b.device, dtype=torch.int32)
    hc = torch.empty(1, device=b.device, dtype=torch.float32)
    check(L.pny_nms(ptr(b), n, float(iou_threshold), float(threshold), ptr(kept), C.c_void_p(meta.data_ptr()), ptr(hc),
                    stream_of(b.device)))
    m = meta.cpu()
    kept = kept[: int(m[0])]
    return (kept if as_tensor else kept.cpu().tolist()), float(hc.item()), int(m[1])


def calculate_tp_fp_fn(target_bboxes, prediction_bboxes, nms_iou, nms_t, match_iou, print_hc=False, device=None):
    """reference src/util/util.py:765-802 -> (tp, fp, fn)."""
    dev = torch.device(device) if device is not None else (
        prediction_bboxes.device if torch.is_tensor(prediction_bboxes) else torch.device("cuda"))
    t, p = _boxes_to_dev(target_bboxes, dev), _boxes_to_dev(prediction_bboxes, dev)
    if t.shape[0] == 0 or p.shape[0] == 0:
        raise ValueError("max() arg is an empty sequence")  # nms() of the reference on an empty list
    out = torch.zeros(3, device=t.device, dtype=torch.int32)
    check(_lib.load().pny_tp_fp_fn(ptr(t), t.shape[0], ptr(p), p.shape[0], float(nms_iou), float(nms_t),
                                   float(match_iou), C.c_void_p(out.data_ptr()), stream_of(t.device)))
    tp, fp, fn = (int(v) for v in out.cpu())
    return tp, fp, fn


def calculate_precision_recall_f1(tp, fp, fn):
    """reference src/util/util.py:798-803 (host arithmetic on three integers)."""
    precision = tp / (tp + fp) if tp + fp > 0 else 0
    recall = tp / (tp + fn) if tp + fn > 0 else 0
    f1 = 2 * (precision * recall) / (precision + recall) if precision + recall > 0 else 0
    return precision, recall, f1
