"""
The training losses of the reference's ``model/loss.py`` (src/model/loss.py) on the library's kernels (csrc/loss.hip): each
``forward`` is ONE launch that computes the terms and the gradient with respect to the predictions, with no device -> host
wait; ``backward`` multiplies the saved gradient by ``grad_output`` (one ATen mul).  Same names and constructors as the
reference's module, so its trainers bind with ``from pixel_nerf_yolo_amd import loss`` in place of ``from model import loss``
(INTEGRATION.md):

  get_rgb_loss(conf, coarse, using_bg, reduction)  MSE or L1 criterion, ``forward(outputs, targets)`` -> 0-dim loss
  NerfLoss                                         PixelNerfTrainer.py:147-154 whole: both passes, the lambdas and the sum
  YoloLoss                                         loss.py:107-179; unlike loss.py:145,147 it leaves ``pred`` and ``target`` untouched
  YoloLoss.forward_batches                         the losses of ALL mini-batches of a YoloTrainer step (YoloTrainer.py:149-208) in
                                                   one launch, each normalised by its own counts, with the gradient of their sum

What the shipped configs disable or never reach is refused by name (``AlphaLossNV2``, ``get_alpha_loss``,
``RGBWithUncertainty``, ``RGBWithBackground``, ``use_uncertainty``, a reduction other than "mean").  fp32 tensors on an
MI355X only; there is no CPU path and no fallback.
"""
import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from . import lib as _lib
from .lib import RgbLossDesc, YoloBatchesDesc, YoloLossDesc, check, stream_of


def _unsupported(name, why):
    raise NotImplementedError("pixel_nerf_yolo_amd.loss.%s is not implemented (%s)" % (name, why))


class AlphaLossNV2(torch.nn.Module):
    def __init__(self, *args, **kwargs):
        _unsupported("AlphaLossNV2", "the shipped configs set lambda_alpha = 0 and the reference's trainers never call it")


def get_alpha_loss(conf):
    _unsupported("get_alpha_loss", "the shipped configs set lambda_alpha = 0 and the reference's trainers never call it")


class RGBWithUncertainty(torch.nn.Module):
    def __init__(self, *args, **kwargs):
        _unsupported("RGBWithUncertainty", "loss.*.use_uncertainty is off in every shipped config")


class RGBWithBackground(torch.nn.Module):
    def __init__(self, *args, **kwargs):
        _unsupported("RGBWithBackground", "the reference's get_rgb_loss never returns it")


def _dev_f32(t, what, device=None):
    """A contiguous fp32 tensor on an MI355X (made contiguous if it is not), or an error that names the argument."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("pixel_nerf_yolo_amd.loss: %s must be a tensor, got %s" % (what, type(t).__name__))
    if t.device.type != "cuda":
        raise _lib.PnyError("pixel_nerf_yolo_amd.loss: %s is on %s; the losses run on an MI355X only (there is no CPU path)"
                            % (what, t.device))
    if device is not None and t.device != device:
        raise _lib.PnyError("pixel_nerf_yolo_amd.loss: %s is on %s, the predictions on %s" % (what, t.device, device))
    if t.dtype != torch.float32:
        raise _lib.PnyError("pixel_nerf_yolo_amd.loss: %s must be fp32, got %s" % (what, t.dtype))
    return t.contiguous()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class _RgbLossFn(torch.autograd.Function):
    """(coarse, fine | None, gt) -> (terms (3,) {rc, rf, t}, t as a 0-dim view of it); only t carries a gradient."""

    @staticmethod
    def forward(ctx, coarse, fine, gt, desc, owner, grad_on):
        coarse = _dev_f32(coarse, "the coarse prediction")
        dev = coarse.device
        gt = _dev_f32(gt, "the ground truth", dev)
        if fine is not None:
            fine = _dev_f32(fine, "the fine prediction", dev)
        for t, what in ((gt, "the ground truth"), (fine, "the fine prediction")):
            if t is not None and t.shape != coarse.shape:
                raise ValueError("pixel_nerf_yolo_amd.loss: %s has shape %s, the coarse prediction %s (no broadcasting)"
                                 % (what, tuple(t.shape), tuple(coarse.shape)))
        # (grad_on: grad mode at the module's call; inside forward it is always off and needs_input_grad ignores no_grad)
        need_c, need_f = grad_on and ctx.needs_input_grad[0], grad_on and fine is not None and ctx.needs_input_grad[1]
        terms = torch.empty(3, device=dev, dtype=torch.float32)
        d_c = torch.empty_like(coarse) if need_c else None
        d_f = torch.empty_like(fine) if need_f else None
        with torch.cuda.device(dev):
            check(_lib.load().pny_rgb_loss(C.byref(desc), _p(coarse), _p(fine), _p(gt), coarse.numel(), _p(terms), _p(d_c), _p(d_f),
                                           stream_of(dev)))
        ctx.save_for_backward(d_c, d_f)
        ctx.set_materialize_grads(False)
        owner.saved_grads = (d_c, d_f)
        ctx.mark_non_differentiable(terms)
        return terms, terms[2]

    @staticmethod
    @once_differentiable
    def backward(ctx, _g_terms, g):
        d_c, d_f = ctx.saved_tensors
        if g is None:
            return (None,) * 6
        return (None if d_c is None else d_c * g, None if d_f is None else d_f * g, None, None, None, None)


class _RgbLoss(torch.nn.Module):
    """``torch.nn.MSELoss()`` / ``torch.nn.L1Loss()`` as the reference's get_rgb_loss returns them: one pass of pny_rgb_loss."""

    def __init__(self, use_l1):
        super().__init__()
        self.use_l1 = bool(use_l1)
        self.saved_grads = (None, None)   # the gradient buffers the last forward wrote (None: none was asked for)

    def forward(self, outputs, targets):
        desc = RgbLossDesc(use_l1_coarse=int(self.use_l1), use_l1_fine=0, lambda_coarse=1.0, lambda_fine=0.0)
        return _RgbLossFn.apply(outputs, None, targets, desc, self, torch.is_grad_enabled())[1]

    def extra_repr(self):
        return "use_l1=%s" % self.use_l1


def get_rgb_loss(conf, coarse=True, using_bg=False, reduction="mean"):
    """model/loss.py:92-104."""
    if conf.get_bool("use_uncertainty", False) and not coarse:
        _unsupported("get_rgb_loss(use_uncertainty=True)", "RGBWithUncertainty: off in every shipped config")
    if reduction != "mean":
        _unsupported("get_rgb_loss(reduction=%r)" % (reduction,), "the reference's trainers use the default, \"mean\"")
    return _RgbLoss(conf.get_bool("use_l1"))


class NerfLoss(torch.nn.Module):
    """PixelNerfTrainer.calc_losses:147-154 in one launch: ``forward(coarse_rgb, fine_rgb | None, rgb_gt)`` ->
    ``(loss, terms)``, terms the (3,) device tensor {rc, rf, t} of the trainer's loss_dict (one ``terms.tolist()`` replaces its
    three ``.item()``), loss = t as a 0-dim view of it.  Only ``loss`` carries a gradient."""

    def __init__(self, rgb_conf, rgb_fine_conf, lambda_coarse=1.0, lambda_fine=1.0):
        super().__init__()
        for c, coarse in ((rgb_conf, True), (rgb_fine_conf, False)):
            if c.get_bool("use_uncertainty", False) and not coarse:
                _unsupported("NerfLoss(use_uncertainty=True)", "RGBWithUncertainty: off in every shipped config")
        self.use_l1_coarse, self.use_l1_fine = bool(rgb_conf.get_bool("use_l1")), bool(rgb_fine_conf.get_bool("use_l1"))
        self.lambda_coarse, self.lambda_fine = float(lambda_coarse), float(lambda_fine)
        self.saved_grads = (None, None)

    @classmethod
    def from_conf(cls, conf):
        """conf["loss"] (trainlib/PixelNerfTrainer.py:27-38)."""
        fine = conf["rgb_fine"] if "rgb_fine" in conf else conf["rgb"]
        return cls(conf["rgb"], fine, conf.get_float("lambda_coarse"), conf.get_float("lambda_fine"))

    def forward(self, coarse_rgb, fine_rgb, rgb_gt):
        desc = RgbLossDesc(use_l1_coarse=int(self.use_l1_coarse), use_l1_fine=int(self.use_l1_fine),
                           lambda_coarse=self.lambda_coarse, lambda_fine=self.lambda_fine)
        terms, loss = _RgbLossFn.apply(coarse_rgb, fine_rgb, rgb_gt, desc, self, torch.is_grad_enabled())
        return loss, terms


class _YoloLossFn(torch.autograd.Function):
    """(pred, target, anchors) -> (terms (5,), total, box, object, no_object, class as 0-dim views); total carries the gradient."""

    @staticmethod
    def forward(ctx, pred, target, anchors, desc, owner, grad_on):
        A = desc.num_anchors
        pred = _dev_f32(pred, "pred")
        dev = pred.device
        target = _dev_f32(target, "target", dev)
        anchors = _dev_f32(anchors, "anchors", dev)
        if pred.dim() < 2 or pred.shape[-2] != A or pred.shape[-1] < 6:
            raise ValueError("pixel_nerf_yolo_amd.loss.YoloLoss: pred must be (..., %d, 5 + C) with C >= 1, got %s" % (A, tuple(pred.shape)))
        if tuple(target.shape) != tuple(pred.shape[:-1]) + (6,):
            raise ValueError("pixel_nerf_yolo_amd.loss.YoloLoss: target must be %s, got %s"
                             % (tuple(pred.shape[:-1]) + (6,), tuple(target.shape)))
        if anchors.numel() != 2 * A:
            raise ValueError("pixel_nerf_yolo_amd.loss.YoloLoss: anchors must hold %d (w, h) pairs, got %s" % (A, tuple(anchors.shape)))
        desc.num_classes = pred.shape[-1] - 5
        cells = pred.numel() // (A * pred.shape[-1])
        if cells < 1:
            raise ValueError("pixel_nerf_yolo_amd.loss.YoloLoss: pred is empty")
        terms = torch.empty(5, device=dev, dtype=torch.float32)
        counts = torch.empty(2, device=dev, dtype=torch.int32)
        d_pred = torch.empty_like(pred) if grad_on and ctx.needs_input_grad[0] else None
        with torch.cuda.device(dev):
            check(_lib.load().pny_yolo_loss(C.byref(desc), _p(pred), _p(target), _p(anchors), cells, _p(terms), _p(counts),
                                            _p(d_pred), stream_of(dev)))
        ctx.save_for_backward(d_pred)
        ctx.set_materialize_grads(False)
        owner.counts, owner.saved_grad = counts, d_pred
        views = terms.unbind(0)
        ctx.mark_non_differentiable(terms, *views[1:])
        return (terms,) + tuple(views)

    @staticmethod
    @once_differentiable
    def backward(ctx, _g_terms, g, *_others):
        (d_pred,) = ctx.saved_tensors
        return (None if d_pred is None or g is None else d_pred * g, None, None, None, None, None)


class _YoloLossBatchesFn(torch.autograd.Function):
    """(pred, target, anchors (S, A, 2)) -> (step (6,), step[0] as a 0-dim view); only step[0], the sum of the mini-batches'
    totals, carries a gradient."""

    @staticmethod
    def forward(ctx, pred, target, anchors, desc, batches, owner, grad_on):
        who = "pixel_nerf_yolo_amd.loss.YoloLoss.forward_batches: "
        A, S = desc.num_anchors, batches.n_scales
        pred = _dev_f32(pred, "pred")
        dev = pred.device
        target = _dev_f32(target, "target", dev)
        anchors = _dev_f32(anchors, "anchors", dev)
        ctx.pred_shape = pred.shape
        if pred.dim() == 4 and pred.shape[0] == 1:
            pred = pred[0]
        if pred.dim() != 3 or pred.shape[1] != A or pred.shape[2] < 6:
            raise ValueError(who + "pred must be (N, %d, 5 + C) or (1, N, %d, 5 + C) with C >= 1, got %s" % (A, A, tuple(pred.shape)))
        N = pred.shape[0]
        if tuple(target.shape) not in ((N, A, 6), (1, N, A, 6)):
            raise ValueError(who + "target must be %s, got %s" % ((N, A, 6), tuple(target.shape)))
        if tuple(anchors.shape) != (S, A, 2):
            raise ValueError(who + "anchors must be (%d, %d, 2), one (A, 2) per entry of rows_per_scale, got %s"
                             % (S, A, tuple(anchors.shape)))
        if sum(batches.rows[:S]) != N:
            raise ValueError(who + "rows_per_scale %s add up to %d rows, pred has %d" % (list(batches.rows[:S]), sum(batches.rows[:S]), N))
        desc.num_classes = pred.shape[2] - 5
        L = _lib.load()
        M = L.pny_yolo_loss_batches_count(C.byref(batches))
        if M < 0:
            check(M)
        step = torch.empty(6, device=dev, dtype=torch.float32)
        terms = torch.empty(M, 5, device=dev, dtype=torch.float32)
        counts = torch.empty(M, 2, device=dev, dtype=torch.int32)
        d_pred = torch.empty_like(pred) if grad_on and ctx.needs_input_grad[0] else None
        with torch.cuda.device(dev):
            check(L.pny_yolo_loss_batches(C.byref(desc), C.byref(batches), _p(pred), _p(target), _p(anchors), _p(terms), _p(counts),
                                          _p(step), _p(d_pred), stream_of(dev)))
        ctx.save_for_backward(d_pred)
        ctx.set_materialize_grads(False)
        owner.batch_terms, owner.batch_counts, owner.saved_grad = terms, counts, d_pred
        ctx.mark_non_differentiable(step)
        return step, step[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, _g_step, g):
        (d_pred,) = ctx.saved_tensors
        return (None if d_pred is None or g is None else (d_pred * g).reshape(ctx.pred_shape), None, None, None, None, None, None)


class YoloLoss(torch.nn.Module):
    """model/loss.py:107-179: ``forward(pred, target, anchors)`` -> (total, box_loss, object_loss, no_object_loss, class_loss),
    0-dim views of one device tensor (``.terms``); ``.counts`` is the (2,) int32 device tensor {n_obj, n_noobj} of the last
    call.  ``total`` carries the gradient w.r.t. ``pred``; the four unweighted terms are reporting values.  ``pred`` and
    ``target`` are left untouched (the reference overwrites pred[..., 1:3] and target[..., 3:5], loss.py:145,147)."""

    def __init__(self, num_anchors_per_scale, box_loss, object_loss, no_object_loss, class_loss):
        super().__init__()
        self.num_anchors_per_scale = int(num_anchors_per_scale)
        self.box_loss, self.object_loss = float(box_loss), float(object_loss)
        self.no_object_loss, self.class_loss = float(no_object_loss), float(class_loss)
        self.terms = self.counts = self.saved_grad = self.batch_terms = self.batch_counts = None

    def forward(self, pred, target, anchors):
        desc = YoloLossDesc(num_anchors=self.num_anchors_per_scale, num_classes=0, box_loss=self.box_loss,
                            object_loss=self.object_loss, no_object_loss=self.no_object_loss, class_loss=self.class_loss)
        out = _YoloLossFn.apply(pred, target, anchors, desc, self, torch.is_grad_enabled())
        self.terms = out[0]
        return out[1:]

    def forward_batches(self, pred, target, anchors, rows_per_scale, ray_batch_size):
        """The losses of ALL mini-batches of a training step in one launch, normalised per mini-batch as the trainer's loop
        normalises them (train/trainlib/YoloTrainer.py:149-208; include/pnyolo.h pny_yolo_loss_batches).

        :param pred (N, A, 5 + C) or (1, N, A, 5 + C): the render of all rows of all scales, flat (util.yolo_train_batch(flat=True))
        :param target (N, A, 6) or (1, N, A, 6)
        :param anchors (S, A, 2) device tensor, or a list of S device tensors (A, 2)
        :param rows_per_scale S row counts that add up to N; scale s is cut into ceil(rows / ray_batch_size) mini-batches
        :return (loss_sum, step_terms): step_terms (6,) on the device = {sum of the mini-batches' totals, then the trainer's
                loss_dict: t, box_loss, object_loss, no_object_loss, class_loss (sums divided by the number of mini-batches)};
                loss_sum = step_terms[0] as a 0-dim view, the only value with a gradient: loss_sum.backward() gives what the
                loop's loss.backward(retain_graph=True) calls accumulate.  ``.batch_terms`` (M, 5) and ``.batch_counts``
                (M, 2) are the mini-batches' own values, on the device."""
        if isinstance(anchors, (list, tuple)):
            anchors = torch.stack([_dev_f32(a, "anchors[%d]" % i) for i, a in enumerate(anchors)])
        rows = [int(r) for r in rows_per_scale]
        if not 1 <= len(rows) <= 4:
            raise ValueError("pixel_nerf_yolo_amd.loss.YoloLoss.forward_batches: rows_per_scale must hold 1 .. 4 row counts, got %d" % len(rows))
        desc = YoloLossDesc(num_anchors=self.num_anchors_per_scale, num_classes=0, box_loss=self.box_loss,
                            object_loss=self.object_loss, no_object_loss=self.no_object_loss, class_loss=self.class_loss)
        batches = YoloBatchesDesc(n_scales=len(rows), batch_rows=int(ray_batch_size), rows=(C.c_int64 * 4)(*rows))
        step, loss_sum = _YoloLossBatchesFn.apply(pred, target, anchors, desc, batches, self, torch.is_grad_enabled())
        return loss_sum, step

    @classmethod
    def from_conf(cls, conf, num_anchors_per_scale):
        return cls(num_anchors_per_scale, conf["yolo.weights.box_loss"], conf["yolo.weights.object_loss"],
                   conf["yolo.weights.no_object_loss"], conf["yolo.weights.class_loss"])
