"""
fp64 restatement of the two training losses in plain torch, written from what the reference computes; nothing is modified
in place and torch.autograd supplies the gradients.  Checked against the reference's own recorded results
(tests/golden/losses.npz) by test_cpu_loss.py, and used as the yardstick of the kernels' shape sweep (test_gpu_loss.py).

  rgb_terms   train/trainlib/PixelNerfTrainer.py:147-154 with the criteria of src/model/loss.py:92-104
  yolo_terms  src/model/loss.py:121-163 with util.iou, src/util/util.py:582-608
"""
import torch

F64 = torch.float64


def _elem(x, g, use_l1):
    return (x - g).abs() if use_l1 else (x - g) ** 2


def rgb_terms(coarse, fine, gt, use_l1_coarse=False, use_l1_fine=False, lambda_coarse=1.0, lambda_fine=1.0, dtype=F64):
    """-> (3,) {rc, rf, t}: rc = lambda_coarse * mean(e(coarse, gt)), rf likewise (0 without a fine pass), t = rc + rf.
    dtype: the arithmetic (fp64, the yardstick; tools/loss_sweep.py times the same ATen sequence in fp32 on the GPU)."""
    rc = lambda_coarse * _elem(coarse.to(dtype), gt.to(dtype), use_l1_coarse).mean()
    rf = lambda_fine * _elem(fine.to(dtype), gt.to(dtype), use_l1_fine).mean() if fine is not None \
        else torch.zeros((), dtype=dtype, device=coarse.device)
    return torch.stack([rc, rf, rc + rf])


def rgb_with_grads(coarse, fine, gt, **kw):
    """-> (terms (3,), d t / d coarse, d t / d fine or None), fp64, on the CPU."""
    c = coarse.detach().cpu().to(F64).requires_grad_()
    f = None if fine is None else fine.detach().cpu().to(F64).requires_grad_()
    terms = rgb_terms(c, f, gt.detach().cpu().to(F64), **kw)
    terms[2].backward()
    return terms.detach(), c.grad, None if f is None else f.grad


def iou(b1, b2):
    """util.py:582-608: boxes [x, y, w, h]; corners from centre -+ size / 2, clamped intersection, abs of the areas, + 1e-6."""
    a_x1, a_y1, a_x2, a_y2 = b1[:, 0] - b1[:, 2] / 2, b1[:, 1] - b1[:, 3] / 2, b1[:, 0] + b1[:, 2] / 2, b1[:, 1] + b1[:, 3] / 2
    b_x1, b_y1, b_x2, b_y2 = b2[:, 0] - b2[:, 2] / 2, b2[:, 1] - b2[:, 3] / 2, b2[:, 0] + b2[:, 2] / 2, b2[:, 1] + b2[:, 3] / 2
    inter = (torch.minimum(a_x2, b_x2) - torch.maximum(a_x1, b_x1)).clamp(min=0) * \
            (torch.minimum(a_y2, b_y2) - torch.maximum(a_y1, b_y1)).clamp(min=0)
    area_a, area_b = ((a_x2 - a_x1) * (a_y2 - a_y1)).abs(), ((b_x2 - b_x1) * (b_y2 - b_y1)).abs()
    return inter / (area_a + area_b - inter + 1e-6)


def yolo_terms(pred, target, anchors, weights, dtype=F64):
    """pred (..., A, 5 + C), target (..., A, 6), anchors (A, 2), weights (box, object, no_object, class) ->
    ((5,) {total, box, object, no_object, class}, n_obj, n_noobj).  The class index must be inside [0, C).  dtype as in
    rgb_terms.  Like the reference it gathers by boolean masks and reads the two counts on the host."""
    A, row = pred.shape[-2], pred.shape[-1]
    p, t = pred.to(dtype).reshape(-1, A, row), target.to(dtype).reshape(-1, A, 6)
    anc = anchors.to(dtype).reshape(1, A, 2).expand(p.shape[0], A, 2)
    obj, noobj = t[..., 0] == 1, t[..., 0] == 0
    n_obj, n_noobj = int(obj.sum()), int(noobj.sum())
    zero = torch.zeros((), dtype=dtype, device=p.device)
    # loss.py:128-130, BCELoss against 0 with ATen's clamp of the logarithm at -100
    no_object = (-(torch.log1p(-p[..., 0][noobj]).clamp(min=-100.0))).mean() if n_noobj else zero * float("nan")
    if n_obj:
        po, to, ao = p[obj], t[obj], anc[obj]
        sxy = torch.sigmoid(po[:, 1:3])
        boxes = torch.cat([sxy, torch.exp(po[:, 3:5]) * ao], dim=-1)                       # loss.py:135-137
        ious = iou(boxes, to[:, 1:5]).detach()                                              # :139
        object_ = ((po[:, 0] - ious * to[:, 0]) ** 2).mean()                                # :141-142
        box_t = torch.cat([to[:, 1:3], torch.log(1e-6 + to[:, 3:5] / ao)], dim=-1)          # :147
        box = ((torch.cat([sxy, po[:, 3:5]], dim=-1) - box_t) ** 2).mean()                  # :145, 149-150 (over 4 n_obj)
        cls = to[:, 5].long()
        class_ = (torch.logsumexp(po[:, 5:], dim=-1) - po[:, 5:].gather(1, cls[:, None])[:, 0]).mean()   # :153-154
    else:
        box = object_ = class_ = zero
    w_box, w_obj, w_noobj, w_cls = (float(w) for w in weights)
    total = w_box * box + w_obj * object_ + w_noobj * no_object + w_cls * class_            # :157-163
    return torch.stack([total, box, object_, no_object, class_]), n_obj, n_noobj


def yolo_with_grads(pred, target, anchors, weights):
    """-> (terms (5,), d total / d pred, n_obj, n_noobj), fp64, on the CPU."""
    p = pred.detach().cpu().to(F64).requires_grad_()
    terms, n_obj, n_noobj = yolo_terms(p, target.detach().cpu(), anchors.detach().cpu(), weights)
    if terms[0].requires_grad:
        terms[0].backward()
    grad = p.grad if p.grad is not None else torch.zeros_like(p)
    return terms.detach(), grad, n_obj, n_noobj
