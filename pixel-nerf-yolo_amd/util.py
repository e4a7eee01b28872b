"""
Ray generation and the YOLO detection tail with the reference's signatures (src/util/util.py:240-278 ``gen_rays``,
:808-876 ``gen_rays_yolo``), executed by libpnyolo's gen_rays kernel.  Output lives on a CUDA
device (that of ``poses``, or the current one when ``poses`` is a CPU tensor as at the reference's call sites).
``sample_train_batch`` is the trainer's ray batch and ground truth in one launch (no counterpart function in the reference:
it replaces the per-object loop of train/trainlib/PixelNerfTrainer.py:76-123).  ``yolo_train_batch`` /
``stage_yolo_targets`` (``build_yolo_targets``: the grids built on the device from the label rows) and ``FiniteMonitor`` are the same for the YOLO trainer: the batch of train/trainlib/YoloTrainer.py:93-129
in one launch, and its NaN / Inf tests (:163-194) without a host wait.  ``score_detections`` / ``DetectionMeter`` score all views of
a YOLO metric pass (YoloTrainer.py:338-354) in one launch per source-view set and one read per pass.  ``psnr`` is the reference's util.psnr (:502-509) on
device tensors (metrics.py).
"""
import ctypes as C

import torch

from . import lib as _lib
from .lib import check, ptr, stream_of
from .metrics import psnr  # noqa: F401  (the reference's util.psnr)


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


# ------------------------------------------------------------------ YOLO training batch
def stage_yolo_targets(all_bboxes, device):
    """
    The dataset's target grids on the device, one tensor per scale: ``all_bboxes`` is data["bboxes"] as the reference's
    trainer receives it -- an NV-long list of num_scales-long tuples of (1, Hs, Ws, A, 6) tensors -- and the result a
    num_scales-long list of (NV, Hs, Ws, A, 6) fp32 tensors on ``device``, what YoloTrainer.py:97-101 builds per scale.  One
    stack on the host and ONE copy per scale instead of NV * num_scales copies.
    """
    dev = torch.device(device)
    out = []
    for s in range(len(all_bboxes[0])):
        grid = torch.stack([torch.as_tensor(view[s]) for view in all_bboxes]).squeeze(1)
        out.append(grid.to(dev, torch.float32, non_blocking=True).contiguous())
    return out


def build_yolo_targets(labels, n_labels, height, width, cell_sizes, anchors, ignore_iou_thresh, device):
    """
    The target grids of all views of an item, built on the device in one launch (include/pnyolo.h pny_yolo_build_targets): what
    ``data.YOLODataset._get_all_bboxes`` computes per view in Python and ``stage_yolo_targets`` stacks and copies.

    :param labels (NV, MAXB, 5) host float64 {cx, cy, w, h, cls}, normalised to the image; n_labels (NV,) rows used per view
    :param height, width the resized image the grids refer to; cell_sizes one per scale
    :param anchors (num_scales * A, 2) or (num_scales, A, 2) {w, h}; ignore_iou_thresh as ``yolo.ignore_iou_thresh``
    :return num_scales-long list of (NV, height // cell, width // cell, A, 6) fp32 device tensors: ``stage_yolo_targets``' result
    Raises ValueError naming the view and row of a label with cx or cy outside [0, 1) or a non-finite or non-positive w or h
    (the reference's IndexError); checked on the host, so nothing waits for the device.
    """
    import numpy as np
    who = "pixel_nerf_yolo_amd.util.build_yolo_targets: "
    dev = torch.device(device)
    lab = np.ascontiguousarray(np.asarray(labels.numpy() if isinstance(labels, torch.Tensor) else labels, dtype=np.float64))
    if lab.ndim != 3 or lab.shape[2] != 5 or lab.shape[0] < 1:
        raise ValueError(who + "labels must be (NV, MAXB, 5) {cx, cy, w, h, cls}, got %s" % (tuple(lab.shape),))
    nv, maxb = int(lab.shape[0]), int(lab.shape[1])
    cnt = np.asarray(n_labels.numpy() if isinstance(n_labels, torch.Tensor) else n_labels)
    if cnt.shape != (nv,) or not np.issubdtype(cnt.dtype, np.integer) or (cnt < 0).any() or (cnt > maxb).any():
        raise ValueError(who + "n_labels must be (%d,) integers in 0 .. %d, got %s %s" % (nv, maxb, tuple(cnt.shape), cnt.tolist()
                                                                                         if cnt.size <= 64 else cnt.dtype))
    cnt = np.ascontiguousarray(cnt.astype(np.int32))
    cells = [int(v) for v in cell_sizes]
    anc = np.ascontiguousarray(np.asarray(anchors.numpy() if isinstance(anchors, torch.Tensor) else anchors, dtype=np.float32))
    if not 1 <= len(cells) <= _lib.YOLO_BATCH_MAX_SCALES:
        raise ValueError(who + "cell_sizes must hold 1 .. %d scales, got %d" % (_lib.YOLO_BATCH_MAX_SCALES, len(cells)))
    anc = anc.reshape(-1, 2) if anc.ndim == 3 and anc.shape[0] == len(cells) and anc.shape[2] == 2 else anc
    if anc.ndim != 2 or anc.shape[1] != 2 or anc.shape[0] == 0 or anc.shape[0] % len(cells) or anc.shape[0] > _lib.YOLO_TARGETS_MAX_ANCHORS:
        raise ValueError(who + "anchors must be (num_scales * A, 2) with %d scale%s and at most %d rows, got %s"
                         % (len(cells), "" if len(cells) == 1 else "s", _lib.YOLO_TARGETS_MAX_ANCHORS, tuple(anc.shape)))
    A = anc.shape[0] // len(cells)
    used = np.arange(maxb)[None, :] < cnt[:, None]
    cx, cy, bw, bh = lab[..., 0], lab[..., 1], lab[..., 2], lab[..., 3]
    with np.errstate(invalid="ignore"):
        bad = used & ~((cx >= 0) & (cx < 1) & (cy >= 0) & (cy < 1) & np.isfinite(bw) & (bw > 0) & np.isfinite(bh) & (bh > 0)
                       & np.isfinite(lab[..., 4]))
    if bad.any():
        v, r = (int(i) for i in np.argwhere(bad)[0])
        raise ValueError(who + "labels[%d, %d] = %s (view %d, row %d): cx and cy must lie in [0, 1), w and h be finite and positive"
                         % (v, r, lab[v, r].tolist(), v, r))
    if dev.type != "cuda":
        raise _lib.PnyError(who + "device is %s; the targets are built on an MI355X only (the host path is "
                            "data.YOLODataset._get_all_bboxes)" % dev)
    if maxb == 0:                                              # no label in any view: one unused row
        lab, maxb = np.zeros((nv, 1, 5)), 1
    boxes = torch.from_numpy(lab).to(dev, non_blocking=True)
    counts = torch.from_numpy(cnt).to(dev, non_blocking=True)
    height, width = int(height), int(width)
    grids = [torch.empty(nv, height // max(c, 1), width // max(c, 1), A, 6, device=dev, dtype=torch.float32) for c in cells]
    desc = _lib.YoloTargetsDesc(n_views=nv, max_boxes=maxb, height=height, width=width, n_scales=len(cells),
                                cell_sizes=(C.c_int32 * 4)(*cells), n_anchors=A, ignore_iou_thresh=float(ignore_iou_thresh))
    with torch.cuda.device(dev):
        check(_lib.load().pny_yolo_build_targets(C.byref(desc), C.c_void_p(boxes.data_ptr()), C.c_void_p(counts.data_ptr()),
                                                 anc.ctypes.data_as(_lib.c_float_p),
                                                 (C.c_void_p * len(grids))(*[g.data_ptr() for g in grids]), stream_of(dev)))
    return grids


def yolo_train_batch(poses, view_ids, focal, c, targets, height, width, cell_sizes, z_near, z_far, device=None, flat=False):
    """
    The rays and target cells of one YOLO training step for one object, over all scales and selected views, in one kernel
    launch: what the reference's YoloTrainer.calc_losses:93-129 prepares per scale (gen_rays_yolo at the scale's grid size,
    the grids indexed by image_ord, both flattened).

    :param poses (NV, 4, 4) world-to-camera extrinsics of all views of the object, on the CPU as the dataset gives them
    :param view_ids (NS,) the object's row of image_ord: 1 .. 16 view indices, any order, repeats allowed
    :param focal (2), c (2) full-resolution intrinsics; a scale uses focal / cell and c / cell
    :param targets num_scales device tensors (NV, H // cell, W // cell, A, 6): stage_yolo_targets
    :return (rays_per_scale, targets_per_scale): lists of views (NS * Hs * Ws, 8) and (NS * Hs * Ws, A, 6) into two flat
            buffers, rows ordered (position in view_ids, y, x).  torch.split(rays_per_scale[s].unsqueeze(0), ray_batch_size,
            dim=1) gives the trainer's mini-batches.
            flat=True: (rays (N, 8), targets (N, A, 6), rows_per_scale) instead -- the two flat buffers themselves and the
            row count of each scale, as loss.YoloLoss.forward_batches takes them (one render, one loss, one backward per step).
    """
    dev = _device_of(targets[0], device)
    cells = [int(v) for v in cell_sizes]
    ids = torch.as_tensor(view_ids, dtype=torch.int64).detach().cpu().reshape(-1).contiguous()
    assert 1 <= len(cells) <= _lib.YOLO_BATCH_MAX_SCALES and len(targets) == len(cells), "one target grid per scale, 1 .. 4 scales"
    NV, NS, A = poses.shape[0], ids.numel(), targets[0].shape[3]
    grids = []
    for t, cell in zip(targets, cells):
        assert t.device == dev and t.dtype == torch.float32 and t.is_contiguous(), "targets: contiguous fp32 on the device"
        assert 1 <= cell <= min(height, width) and tuple(t.shape) == (NV, height // cell, width // cell, A, 6), \
            "a target grid is (NV, H // cell, W // cell, A, 6)"
        grids.append(t.data_ptr())
    off = [0]
    for cell in cells:
        off.append(off[-1] + NS * (height // cell) * (width // cell))
    desc = _lib.YoloBatchDesc(n_views_all=NV, n_views=NS, height=int(height), width=int(width), n_scales=len(cells),
                              cell_sizes=(C.c_int32 * 4)(*cells), n_anchors=A, z_near=float(z_near), z_far=float(z_far))
    p = poses.detach().to("cpu", torch.float32).contiguous()
    rays = torch.empty(off[-1], 8, device=dev, dtype=torch.float32)
    tout = torch.empty(off[-1], A, 6, device=dev, dtype=torch.float32)
    got = (C.c_int64 * (len(cells) + 1))()
    with torch.cuda.device(dev):
        check(_lib.load().pny_yolo_train_batch(C.byref(desc), ptr(p), C.cast(ids.data_ptr(), _lib.c_i64_p), _pair(focal, "focal"),
                                               _pair(c, "c"), (C.c_void_p * len(grids))(*grids), ptr(rays), ptr(tout), got,
                                               stream_of(dev)))
    assert list(got) == off
    if flat:
        return rays, tout, [b - a for a, b in zip(off, off[1:])]
    return [rays[a:b] for a, b in zip(off, off[1:])], [tout[a:b] for a, b in zip(off, off[1:])]


class FiniteMonitor:
    """
    The NaN / Inf tests of a training step without a host wait (include/pnyolo.h pny_finite_*): every ``check`` is one kernel
    launch that ORs what it finds into two int32 words per group on the device, and ``report`` is the step's single read.
    Replaces the reference's `if torch.isnan(x).any()` / `torch.isinf(x).any()` tests (YoloTrainer.py:163-194).

        mon = FiniteMonitor(("render", "targets", "grads"), device)
        mon.watch("grads", list(net.parameters()), names, grads=True)
        ... per mini-batch:  mon.check("render", render); mon.check("targets", bboxes_gt); loss.backward(); mon.check("grads")
        ... per step:        bad = mon.report(); mon.reset()

    Tensors are contiguous fp32 on the monitor's device.  A group is either watched or checked with tensors given in the
    call, not both: `first` is a row of the registered table for the one and a position in the call for the other.
    """

    def __init__(self, groups, device):
        self.groups = list(groups)
        assert len(set(self.groups)) == len(self.groups) and self.groups, "group names must be distinct"
        self.device = _device_of(torch.empty(0), device)
        if self.device.index is None:                      # "cuda": the current device, by its index (tensors carry one)
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.flags = torch.empty(len(self.groups), 2, device=self.device, dtype=torch.int32)   # [bits, first] per group
        self._watched = {}     # group -> dict(tensors, names, grads, ptrs, first)
        self._names = {}       # table index -> name (this handle)
        self._h = None
        self._new_handle()
        self.reset()

    def _new_handle(self):
        L = _lib.load()
        if self._h is not None:
            L.pny_finite_destroy(self._h)
        self._h = C.c_void_p()
        check(L.pny_finite_create(C.byref(self._h), self.device.index))
        self._names, self._rows = {}, 0
        for w in self._watched.values():
            w["ptrs"] = None

    def close(self):
        if self._h is not None:
            _lib.load().pny_finite_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _buffers(self, w):
        ts = [(t.grad if w["grads"] else t) for t in w["tensors"]]
        for t in ts:
            assert t is None or (t.device == self.device and t.dtype == torch.float32 and t.is_contiguous()), \
                "FiniteMonitor takes contiguous fp32 tensors on its device"
        return ts

    def watch(self, group, tensors, names=None, grads=False):
        """Registers the buffers `check(group)` scans.  grads=True: the buffer of each tensor is its `.grad` at the time of
        the check (None: nothing to scan).  names: what `report` calls them (default: their position)."""
        tensors = list(tensors)
        names = [str(n) for n in names] if names is not None else ["%s[%d]" % (group, i) for i in range(len(tensors))]
        assert len(names) == len(tensors)
        self._watched[group] = dict(tensors=tensors, names=names, grads=bool(grads), ptrs=None, first=0)

    def _register(self, group, w, bufs, ptrs):
        L = _lib.load()
        g = self.groups.index(group)
        w["first"] = self._rows
        for t, name in zip(bufs, w["names"]):
            i = L.pny_finite_add_tensor(self._h, None if t is None else C.c_void_p(t.data_ptr()), 0 if t is None else t.numel(), g)
            if i < 0:
                check(i)
            self._names[i] = name
            self._rows = i + 1
        w["ptrs"] = ptrs

    def check(self, group, *tensors):
        """check(group, t0, t1, ...): scans up to 8 tensors now.  check(group): scans the watched buffers of the group, which
        are registered again first when one of them has moved (a new .grad after zero_grad(set_to_none=True))."""
        L = _lib.load()
        g = self.groups.index(group)
        with torch.cuda.device(self.device):
            if tensors:
                assert group not in self._watched, "group %r is watched: check it without tensors" % (group,)
                assert len(tensors) <= _lib.FINITE_MAX_IMMEDIATE, "at most 8 tensors per immediate check: watch() larger sets"
                n = len(tensors)
                for t in tensors:
                    assert t.device == self.device and t.dtype == torch.float32 and t.is_contiguous(), \
                        "FiniteMonitor takes contiguous fp32 tensors on its device"
                check(L.pny_finite_check_tensors((C.c_void_p * n)(*[t.data_ptr() for t in tensors]),
                                                 (C.c_int64 * n)(*[t.numel() for t in tensors]), (C.c_int32 * n)(*([g] * n)), n,
                                                 C.c_void_p(self.flags.data_ptr()), stream_of(self.device)))
                return
            w = self._watched[group]
            bufs = self._buffers(w)
            ptrs = [(0, 0) if t is None else (t.data_ptr(), t.numel()) for t in bufs]
            if ptrs != w["ptrs"]:
                self._register(group, w, bufs, ptrs)
            check(L.pny_finite_check(self._h, w["first"], len(bufs), C.c_void_p(self.flags.data_ptr()), stream_of(self.device)))

    def reset(self):
        """Clears the flags (one launch).  Also the moment a table that re-registration has grown is started afresh: no flag
        word refers to an old row then."""
        live = sum(len(w["tensors"]) for w in self._watched.values())
        if self._rows > 4 * live + 64:
            self._new_handle()
        with torch.cuda.device(self.device):
            check(_lib.load().pny_finite_reset(C.c_void_p(self.flags.data_ptr()), len(self.groups), stream_of(self.device)))

    def report(self):
        """The step's one device-to-host read -> {group: (has_nan, has_inf, name of the first tensor hit or None)}.  For a
        watched group the name is the watched tensor's; for immediate checks it is `group[i]`, i the position in the call."""
        words = self.flags.cpu().tolist()
        out = {}
        for group, (bits, first) in zip(self.groups, words):
            name = None
            if bits:
                name = self._names.get(first) if group in self._watched else "%s[%d]" % (group, first)
            out[group] = (bool(bits & _lib.FINITE_NAN), bool(bits & _lib.FINITE_INF), name)
        return out


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


# ------------------------------------------------------------------ YOLO metric pass: all views in one launch
class DetectionScores:
    """What ``score_detections`` leaves on the device; nothing here has been read by the host.

    per_view (V, 8) int32, columns ``lib.DETECT_RECORD``: tp, fp, fn, kept targets, kept predictions, targets and predictions
    above the confidence threshold, status (0, or ``lib.DETECT_*`` bits: the view was refused and counts as 0).
    highest_conf (V, 2): the highest score of all target / prediction boxes of the view.
    totals (4,) int64: tp, fp, fn, refused views -- the tensor the call added to.
    kept_targets, kept_preds: None, or (V, max_kept, 6) survivors in the reference's output order (want_boxes=True); the
    counts are in per_view, rows past a view's count are not written."""

    def __init__(self, per_view, highest_conf, totals, kept_targets=None, kept_preds=None):
        self.per_view, self.highest_conf, self.totals = per_view, highest_conf, totals
        self.kept_targets, self.kept_preds = kept_targets, kept_preds


def _detect_fail(msg, exc=ValueError, who="score_detections"):
    raise exc("pixel_nerf_yolo_amd.util.%s: %s" % (who, msg))


def _detect_tensor(t, name, dev, who="score_detections"):
    """A float32 tensor on the GPU, contiguous (a copy on the device if it was not)."""
    if not torch.is_tensor(t):
        _detect_fail("%s must be a torch tensor, got %s" % (name, type(t).__name__), TypeError, who=who)
    if t.dtype != torch.float32:
        _detect_fail("%s must be float32, got %s" % (name, t.dtype), TypeError, who=who)
    if t.device.type != "cuda":
        _detect_fail("%s is on %s; the scorer runs on an MI355X only (the host path is calculate_tp_fp_fn per view)"
                     % (name, t.device), _lib.PnyError, who=who)
    if dev is not None and t.device != dev:
        _detect_fail("%s is on %s, the other inputs on %s" % (name, t.device, dev), who=who)
    return t.detach().contiguous()


def _detect_offsets(off, name, n_rows, n_views, who="score_detections"):
    """(V + 1) int32 offsets.  A host tensor / list is checked here (starts at 0, ascends, ends inside the rows) and copied over;
    a device tensor is used in place and checked by the kernel (a bad segment is a refused view)."""
    if torch.is_tensor(off) and off.device.type == "cuda":
        if off.dtype != torch.int32 or off.dim() != 1:
            _detect_fail("%s on the device must be a 1-d int32 tensor, got %s %s" % (name, off.dtype, tuple(off.shape)), TypeError, who=who)
        if n_views is not None and off.numel() != n_views + 1:
            _detect_fail("%s must hold n_views + 1 = %d entries, got %d" % (name, n_views + 1, off.numel()), who=who)
        return off.contiguous(), None
    o = torch.as_tensor(off)
    if o.dim() != 1 or o.numel() < 2 or o.dtype.is_floating_point or o.dtype == torch.bool:
        _detect_fail("%s must be a 1-d integer sequence of V + 1 entries, got %s %s" % (name, o.dtype, tuple(o.shape)), who=who)
    if n_views is not None and o.numel() != n_views + 1:
        _detect_fail("%s must hold n_views + 1 = %d entries, got %d" % (name, n_views + 1, o.numel()), who=who)
    v = o.to(torch.int64).tolist()
    if v[0] != 0:
        _detect_fail("%s must start at 0, got %d" % (name, v[0]), who=who)
    if any(b < a for a, b in zip(v, v[1:])):
        _detect_fail("%s must ascend, got %s" % (name, v if len(v) <= 20 else v[:20] + ["..."]), who=who)
    if v[-1] > n_rows:
        _detect_fail("%s ends at %d, past the %d rows" % (name, v[-1], n_rows), who=who)
    return o.to(torch.int32), max(b - a for a, b in zip(v, v[1:]))


def _detect_inputs(who, preds, targets, anchors, height, width, cell_sizes, n_views, boxes):
    """The inputs of ``score_detections`` and ``sweep_detections``, validated once: -> (desc with the form, the view count and the
    geometry or row counts, the device, the eight input arguments of pny_detect_views / pny_detect_sweep, the boxes of the longest
    list, what must stay alive until the launch is enqueued)."""
    dev = None
    keep = []
    desc = _lib.DetectViewsDesc()
    p_ptrs = t_ptrs = anc_ptr = None
    rows = [None, None]
    offs = [None, None]
    if boxes is not None:
        if preds is not None or targets is not None:
            _detect_fail("give either preds / targets (cells) or boxes=, not both", who=who)
        if len(boxes) != 4:
            _detect_fail("boxes must be (pred_rows, pred_offsets, target_rows, target_offsets)", who=who)
        longest = 0
        checked = []
        for i, name in ((0, "pred"), (2, "target")):
            r = boxes[i]
            if not torch.is_tensor(r) or r.dim() != 2 or r.shape[1] != 6:
                _detect_fail("%s_rows must be a (n, 6) tensor, got %s" % (name, tuple(r.shape) if torch.is_tensor(r) else type(r).__name__), who=who)
            o, seg = _detect_offsets(boxes[i + 1], name + "_offsets", r.shape[0], n_views, who=who)
            if n_views is None:
                n_views = o.numel() - 1
            elif o.numel() != n_views + 1:
                _detect_fail("%s_offsets must hold n_views + 1 = %d entries, got %d" % (name, n_views + 1, o.numel()), who=who)
            longest = max(longest, r.shape[0] if seg is None else seg)
            checked.append((r, o, name))
        for k, (r, o, name) in enumerate(checked):
            rows[k] = _detect_tensor(r, name + "_rows", dev, who=who)
            dev = rows[k].device
            offs[k] = o if o.device == dev else o.to(dev, non_blocking=True)
        desc.form, desc.n_views = _lib.DETECT_BOXES, int(n_views)
        desc.n_pred_rows, desc.n_target_rows = rows[0].shape[0], rows[1].shape[0]
    else:
        if preds is None or targets is None:
            _detect_fail("preds and targets (one tensor per scale), or boxes=, are required", who=who)
        preds, targets = list(preds), list(targets)
        cells = [int(v) for v in cell_sizes]
        if not 1 <= len(cells) <= _lib.YOLO_BATCH_MAX_SCALES:
            _detect_fail("cell_sizes must hold 1 .. %d scales, got %d" % (_lib.YOLO_BATCH_MAX_SCALES, len(cells)), who=who)
        if len(preds) != len(cells) or len(targets) != len(cells):
            _detect_fail("one prediction and one target tensor per scale: %d scales, %d preds, %d targets" % (len(cells), len(preds), len(targets)), who=who)
        anc = torch.as_tensor(anchors, dtype=torch.float32).detach().cpu()
        if anc.dim() == 3 and anc.shape[0] == len(cells) and anc.shape[2] == 2:
            anc = anc.reshape(-1, 2)
        if anc.dim() != 2 or anc.shape[1] != 2 or anc.shape[0] == 0 or anc.shape[0] % len(cells):
            _detect_fail("anchors must be (num_scales * A, 2) with %d scale%s, got %s" % (len(cells), "" if len(cells) == 1 else "s", tuple(anc.shape)), who=who)
        A = anc.shape[0] // len(cells)
        if A > _lib.DETECT_MAX_ANCHORS:
            _detect_fail("at most %d anchors per scale, got %d" % (_lib.DETECT_MAX_ANCHORS, A), who=who)
        anc = anc.contiguous()
        height, width = int(height), int(width)
        if n_views is None or int(n_views) < 1:
            _detect_fail("n_views (the views in the lists) must be given and positive, got %r" % (n_views,), who=who)
        n_views = int(n_views)
        longest = 0
        for s, cell in enumerate(cells):
            if not 1 <= cell <= min(height, width):
                _detect_fail("cell_sizes[%d] = %d must be 1 .. min(height, width)" % (s, cell), who=who)
            per = (height // cell) * (width // cell)
            longest += per * A
            for t, name, cols in ((preds[s], "preds", 7), (targets[s], "targets", 6)):
                if not torch.is_tensor(t) or t.dim() != 3:
                    _detect_fail("%s[%d] must be a (n_views * Hs * Ws, A, %d) tensor, got %s"
                                 % (name, s, cols, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__), who=who)
                if tuple(t.shape) != (n_views * per, A, cols):
                    _detect_fail("%s[%d] must be (n_views * Hs * Ws, A, %d) = %s, got %s" % (name, s, cols, (n_views * per, A, cols), tuple(t.shape)), who=who)
        for s in range(len(cells)):
            preds[s] = _detect_tensor(preds[s], "preds[%d]" % s, dev, who=who)
            dev = preds[s].device
            targets[s] = _detect_tensor(targets[s], "targets[%d]" % s, dev, who=who)
        desc.form, desc.n_views, desc.n_scales, desc.height, desc.width = _lib.DETECT_CELLS, n_views, len(cells), height, width
        desc.cell_sizes, desc.n_anchors = (C.c_int32 * 4)(*cells), A
        p_ptrs = (C.c_void_p * len(cells))(*[t.data_ptr() for t in preds])
        t_ptrs = (C.c_void_p * len(cells))(*[t.data_ptr() for t in targets])
        anc_ptr = C.cast(anc.data_ptr(), _lib.c_float_p)
        keep = [preds, targets, anc]
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    return desc, dev, (p_ptrs, t_ptrs, anc_ptr, vp(rows[0]), vp(offs[0]), vp(rows[1]), vp(offs[1])), longest, [keep, rows, offs]


def score_detections(preds, targets, anchors, height, width, cell_sizes, nms_iou, nms_t, match_iou, n_views=None, totals=None,
                     want_boxes=False, boxes=None):
    """
    The detection counts of all views of a YOLO metric step in ONE launch (include/pnyolo.h pny_detect_views): what the
    reference's YoloTrainer.metric_step (train/trainlib/YoloTrainer.py:338-354) does per destination view --
    convert_cells_to_bboxes per scale, .tolist(), calculate_tp_fp_fn -- with equal counts, for every view at once and without a
    host read.  The call returns as soon as the kernel is enqueued.

    :param preds num_scales tensors (n_views * Hs * Ws, A, 7), the renders of ``YoloRenderer`` on the rays of
           ``yolo_train_batch``; targets num_scales tensors (n_views * Hs * Ws, A, 6), its target cells.  fp32, on the GPU;
           non-contiguous ones are copied there.  A view's list is its cells of every scale in turn, (y, x, anchor) within one.
    :param anchors (num_scales * A, 2) or (num_scales, A, 2), A <= 4; height, width the image; cell_sizes one per scale (<= 4)
    :param nms_iou, nms_t, match_iou as ``calculate_tp_fp_fn`` takes them
    :param n_views views in the lists (required for cells; for boxes implied by the offsets)
    :param totals a (4,) int64 device tensor [tp, fp, fn, refused views] to ADD to (``DetectionMeter`` owns one); None: a fresh one
    :param want_boxes also the kept boxes of both lists per view
    :param boxes instead of preds / targets (pass None for both and for anchors / height / width / cell_sizes):
           (pred_rows, pred_offsets, target_rows, target_offsets) -- decoded rows (n, 6) [class, score, x, y, w, h] on the GPU and
           V + 1 offsets each, on the host (checked here) or int32 on the device (checked by the kernel)
    :return DetectionScores of device tensors

    At most ``lib.DETECT_MAX_CANDIDATES`` (2048) boxes of one list of one view may pass the confidence and size filters; a view
    above that is refused, not truncated: its status is non-zero and it counts in totals[3] alone.
    """
    desc, dev, inputs, longest, keep = _detect_inputs("score_detections", preds, targets, anchors, height, width, cell_sizes, n_views, boxes)
    desc.nms_iou, desc.nms_threshold, desc.match_iou = float(nms_iou), float(nms_t), float(match_iou)
    if totals is None:
        totals = torch.zeros(4, device=dev, dtype=torch.int64)
    elif not (torch.is_tensor(totals) and totals.dtype == torch.int64 and tuple(totals.shape) == (4,) and totals.device == dev
              and totals.is_contiguous()):
        _detect_fail("totals must be a contiguous (4,) int64 tensor on %s" % dev)
    V = desc.n_views
    per_view = torch.empty(V, len(_lib.DETECT_RECORD), device=dev, dtype=torch.int32)
    hc = torch.empty(V, 2, device=dev, dtype=torch.float32)
    kt = kp = None
    if want_boxes:
        desc.max_kept = max(1, min(int(longest), _lib.DETECT_MAX_CANDIDATES))
        kt = torch.zeros(V, desc.max_kept, 6, device=dev, dtype=torch.float32)
        kp = torch.zeros(V, desc.max_kept, 6, device=dev, dtype=torch.float32)
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    with torch.cuda.device(dev):
        check(_lib.load().pny_detect_views(C.byref(desc), *inputs, vp(per_view), vp(hc), vp(totals), vp(kt), vp(kp), stream_of(dev)))
    del keep
    return DetectionScores(per_view, hc, totals, kt, kp)


class DetectionMeter:
    """
    The running tp / fp / fn of a YOLO metric pass (the three sums of YoloTrainer.metric_step, train/trainlib/YoloTrainer.py:349-351,
    over the whole test loader): ``update`` is ``score_detections`` adding into the meter's own four device words -- one launch, no
    read -- and ``report`` is the pass's ONE device-to-host read.

        meter = DetectionMeter(device)
        for batch in test_loader:  meter.update(renders, target_cells, anchors, H, W, cell_sizes, nms_iou, nms_t, match_iou, n_views=NS)
        precision, recall, f1 = meter.report(prf=True);  meter.reset()
    """

    def __init__(self, device):
        self.device = _device_of(torch.empty(0), device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.totals = torch.zeros(4, device=self.device, dtype=torch.int64)

    def update(self, *args, **kwargs):
        """``score_detections(...)`` into this meter's totals -> its DetectionScores (per-view records, still on the device)."""
        assert "totals" not in kwargs, "the meter adds into its own totals"
        return score_detections(*args, totals=self.totals, **kwargs)

    def reset(self):
        self.totals.zero_()

    def report(self, prf=False):
        """(tp, fp, fn), or with prf=True (precision, recall, f1) by ``calculate_precision_recall_f1``.  Raises PnyError when
        views were refused (more than ``lib.DETECT_MAX_CANDIDATES`` candidates, or a bad segment): the sums would miss them."""
        tp, fp, fn, failed = (int(v) for v in self.totals.cpu().tolist())
        if failed:
            raise _lib.PnyError("pixel_nerf_yolo_amd.util.DetectionMeter.report: %d view%s refused since the last reset (more than %d "
                                "candidates in one list of a view, or a bad segment): tp, fp, fn would miss them; the per-view "
                                "status of every update names them" % (failed, " was" if failed == 1 else "s were",
                                                                       _lib.DETECT_MAX_CANDIDATES))
        return calculate_precision_recall_f1(tp, fp, fn) if prf else (tp, fp, fn)


# ------------------------------------------------------------------ YOLO metric pass: its three thresholds swept in one launch
class DetectionSweep:
    """What ``sweep_detections`` leaves on the device; nothing here has been read by the host.  With V views and
    I = len(nms_ious), T = len(nms_ts), M = len(match_ious), in C order:

    counts (V, I, T, M, 3) int32: tp, fp, fn of the view at setting (nms_ious[i], nms_ts[t], match_ious[m]);
    lists (V, I, T, 3) int32: kept targets, kept predictions, status (0, or ``lib.DETECT_*`` bits: refused at that cut, counts 0);
    totals (I, T, M, 4) int64: tp, fp, fn, refused views -- the tensor the call added to;
    nms_ious, nms_ts, match_ious: the three tuples as given."""

    def __init__(self, counts, lists, totals, nms_ious, nms_ts, match_ious):
        self.counts, self.lists, self.totals = counts, lists, totals
        self.nms_ious, self.nms_ts, self.match_ious = nms_ious, nms_ts, match_ious


def _sweep_thresholds(who, nms_ious, nms_ts, match_ious):
    """The three threshold arguments as tuples of floats, order and duplicates kept; ValueError naming the argument for an empty
    or too long list or a value that is not finite.  Touches no tensor and no library: it runs first."""
    out = []
    for name, values, most in (("nms_ious", nms_ious, _lib.DETECT_SWEEP_MAX_NMS_IOUS), ("nms_ts", nms_ts, _lib.DETECT_SWEEP_MAX_CUTS),
                               ("match_ious", match_ious, _lib.DETECT_SWEEP_MAX_MATCH_IOUS)):
        if isinstance(values, (int, float)):
            values = (values,)
        try:
            values = tuple(float(v) for v in values)
        except (TypeError, ValueError):
            _detect_fail("%s must be a float or a sequence of floats, got %r" % (name, values), who=who)
        if not 1 <= len(values) <= most:
            _detect_fail("%s must hold 1 .. %d values, got %d" % (name, most, len(values)), who=who)
        for k, v in enumerate(values):
            if v != v or v in (float("inf"), float("-inf")):
                _detect_fail("%s[%d] = %r must be finite" % (name, k, v), who=who)
        out.append(values)
    return tuple(out)


def sweep_detections(preds, targets, anchors, height, width, cell_sizes, nms_ious, nms_ts, match_ious, n_views=None, totals=None,
                     boxes=None, _who="sweep_detections"):
    """
    The detection counts of all views of a YOLO metric step at EVERY setting of a grid of thresholds, in ONE launch
    (include/pnyolo.h pny_detect_sweep): setting (i, t, m) holds the integers ``score_detections`` gives at
    (nms_ious[i], nms_ts[t], match_ious[m]), on a render that is made once.  The reference scores one setting per pass
    (eval/eval_yolo.py) and asks for the next on stdin (eval/gen_images_yolo.py:110-117), with an encode and a render each time.
    The call returns as soon as the kernel is enqueued and reads nothing.

    :param preds, targets, anchors, height, width, cell_sizes, n_views, boxes as ``score_detections`` takes them
    :param nms_ious (util.nms iou_threshold), nms_ts (util.nms threshold, the confidence cut), match_ious: each a float or a
           sequence of floats: at most ``lib.DETECT_SWEEP_MAX_NMS_IOUS`` (8), ``lib.DETECT_SWEEP_MAX_CUTS`` (32) and
           ``lib.DETECT_SWEEP_MAX_MATCH_IOUS`` (8), all finite; order and duplicates are kept.  Checked before anything else.
    :param totals a contiguous (I, T, M, 4) int64 device tensor to ADD to (``DetectionSweepMeter`` owns one); None: a fresh one
    :return DetectionSweep of device tensors

    A view with more than ``lib.DETECT_MAX_CANDIDATES`` boxes of one list past the filters at a cut is refused at that cut, not
    truncated: its status there is non-zero, its counts are 0 and it counts in totals[i, t, :, 3] alone.  Kept boxes are not part
    of a sweep: ``score_detections(..., want_boxes=True)`` at the chosen setting gives them.
    """
    nms_ious, nms_ts, match_ious = _sweep_thresholds(_who, nms_ious, nms_ts, match_ious)
    desc, dev, inputs, _, keep = _detect_inputs(_who, preds, targets, anchors, height, width, cell_sizes, n_views, boxes)
    shape = (len(nms_ious), len(nms_ts), len(match_ious))
    if totals is None:
        totals = torch.zeros(*shape, 4, device=dev, dtype=torch.int64)
    elif not (torch.is_tensor(totals) and totals.dtype == torch.int64 and tuple(totals.shape) == shape + (4,) and totals.device == dev
              and totals.is_contiguous()):
        _detect_fail("totals must be a contiguous %s int64 tensor on %s" % (shape + (4,), dev), who=_who)
    V = desc.n_views
    counts = torch.empty(V, *shape, 3, device=dev, dtype=torch.int32)
    lists = torch.empty(V, shape[0], shape[1], 3, device=dev, dtype=torch.int32)
    arr = lambda v: (C.c_double * len(v))(*v)   # noqa: E731
    vp = lambda t: C.c_void_p(t.data_ptr())     # noqa: E731
    with torch.cuda.device(dev):
        check(_lib.load().pny_detect_sweep(C.byref(desc), *inputs, arr(nms_ious), shape[0], arr(nms_ts), shape[1], arr(match_ious), shape[2],
                                           vp(counts), vp(lists), vp(totals), stream_of(dev)))
    del keep
    return DetectionSweep(counts, lists, totals, nms_ious, nms_ts, match_ious)


class DetectionSweepReport:
    """A sweep's totals on the host (``DetectionSweepMeter.report``), every array (I, T, M) over nms_ious x nms_ts x match_ious:

    tp, fp, fn, refused: numpy int64;
    precision, recall, f1: float64 by ``calculate_precision_recall_f1`` on the setting's three integers, NaN where views were
    refused at the setting (its sums miss them)."""

    def __init__(self, totals, nms_ious, nms_ts, match_ious):
        import numpy as np
        self.nms_ious, self.nms_ts, self.match_ious = tuple(nms_ious), tuple(nms_ts), tuple(match_ious)
        shape = (len(self.nms_ious), len(self.nms_ts), len(self.match_ious))
        totals = np.ascontiguousarray(totals, dtype=np.int64)
        if totals.shape != shape + (4,):
            raise ValueError("pixel_nerf_yolo_amd.util.DetectionSweepReport: totals must be %s, got %s" % (shape + (4,), totals.shape))
        self.tp, self.fp, self.fn, self.refused = (totals[..., k].copy() for k in range(4))
        self.precision, self.recall, self.f1 = (np.full(shape, np.nan, np.float64) for _ in range(3))
        for idx in np.ndindex(*shape):
            if not self.refused[idx]:
                self.precision[idx], self.recall[idx], self.f1[idx] = calculate_precision_recall_f1(
                    int(self.tp[idx]), int(self.fp[idx]), int(self.fn[idx]))

    def best(self):
        """(nms_iou, nms_t, match_iou, precision, recall, f1) of the highest F1 among the settings without refused views; the
        first such setting in C order on a tie.  PnyError when every setting has refused views."""
        import numpy as np
        ok = self.refused == 0
        if not ok.any():
            raise _lib.PnyError("pixel_nerf_yolo_amd.util.DetectionSweepReport.best: all %d settings have refused views (%d refusals "
                                "of a view at a setting in all: more than %d candidates in one list of a view, or a bad segment)"
                                % (ok.size, int(self.refused.sum()), _lib.DETECT_MAX_CANDIDATES))
        i, t, m = np.unravel_index(int(np.argmax(np.where(ok, self.f1, -np.inf))), ok.shape)    # argmax: the first maximum
        return (self.nms_ious[i], self.nms_ts[t], self.match_ious[m], float(self.precision[i, t, m]), float(self.recall[i, t, m]),
                float(self.f1[i, t, m]))


class DetectionSweepMeter:
    """
    The running tp / fp / fn of a YOLO metric pass at every setting of a grid of thresholds: ``update`` is ``sweep_detections``
    adding into the meter's own (I, T, M, 4) device words -- one launch, no read -- and ``report`` is the pass's ONE
    device-to-host read: the precision / recall / F1 table from which the operating point is picked.

        meter = DetectionSweepMeter(device, nms_ious=(0.45, 0.6, 0.75), nms_ts=[0.05 * k for k in range(1, 17)], match_ious=(0.2, 0.5))
        for batch in test_loader:  meter.update(renders, target_cells, anchors, H, W, cell_sizes, n_views=NS)
        table = meter.report();  nms_iou, nms_t, match_iou, precision, recall, f1 = table.best();  meter.reset()
    """

    def __init__(self, device, nms_ious, nms_ts, match_ious):
        self.nms_ious, self.nms_ts, self.match_ious = _sweep_thresholds("DetectionSweepMeter", nms_ious, nms_ts, match_ious)
        self.device = _device_of(torch.empty(0), device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.totals = torch.zeros(len(self.nms_ious), len(self.nms_ts), len(self.match_ious), 4, device=self.device, dtype=torch.int64)

    def update(self, preds, targets, anchors, height, width, cell_sizes, n_views=None, boxes=None):
        """``sweep_detections(...)`` at the meter's thresholds into its totals -> its DetectionSweep (still on the device)."""
        return sweep_detections(preds, targets, anchors, height, width, cell_sizes, self.nms_ious, self.nms_ts, self.match_ious,
                                n_views=n_views, totals=self.totals, boxes=boxes, _who="DetectionSweepMeter.update")

    def reset(self):
        self.totals.zero_()

    def report(self):
        """The DetectionSweepReport of everything added since the last reset."""
        return DetectionSweepReport(self.totals.cpu().numpy(), self.nms_ious, self.nms_ts, self.match_ious)
