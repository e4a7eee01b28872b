#!/usr/bin/env python3
"""
tests/golden/losses.npz: what the REFERENCE's own loss modules (src/model/loss.py) return, and the gradients autograd gives
for them, on seeded inputs, captured on CPU.

Imports the reference the way tools/make_golden.py does (its stubs for the absent third-party modules, the suite's CPU
arithmetic settings) and runs
  YoloLoss.forward (loss.py:121-163) on clones -- it overwrites pred[..., 1:3] and target[..., 3:5] -- with pred a non-leaf
      copy of the recorded tensor, as the renderer's output is in the trainer (train/trainlib/YoloTrainer.py:181-186), and
      total.backward();
  get_rgb_loss's modules (loss.py:92-104) through the trainer's lines (train/trainlib/PixelNerfTrainer.py:147-154) with
      lambda_coarse = 0.7, lambda_fine = 1.3, and loss.backward().

YOLO cases (pred (1, cells, A, 5 + C), target (1, cells, A, 6), weights of conf/exp/yolo.conf: 1, 20, 1, 1):
  y128     (1, 128, 3, 7)   about 5 % object cells, 10 % ignored (-1)
  y37      (1, 37, 3, 7)    a ragged tail
  ynoobj   (1, 40, 3, 7)    no object cell at all
  ya1c1    (1, 48, 1, 6)    A = 1, C = 1
  ya3c5    (1, 48, 3, 10)   A = 3, C = 5
p_obj in [1e-3, 1 - 1e-3], w, h logits in [-2, 2], target sizes in [0.02, 0.9]: the magnitudes of conf/exp/yolo.conf.
RGB cases: mse_mse (4, 128, 3); l1_mse (2, 50, 3) L1 coarse with MSE fine; coarse_only (2, 50, 3) MSE without a fine pass.
Without a fine pass the trainer's loss is the UNSCALED coarse criterion (lambda_coarse then only enters loss_dict["rc"], :148);
coarse_only is therefore captured with lambda_coarse = 1, the shipped value, where rc = t as in pny_rgb_loss.

Per YOLO case: pred, target, anchors, weights, terms (total, box, object, no_object, class), d_pred.  Per RGB case: coarse,
fine, gt, use_l1 (2,), lambdas (2,), raw (the criteria's own values), terms (rc, rf, t), d_coarse, d_fine.
Fixed zip timestamps: a second run gives the same bytes.

Usage:  python tools/make_loss_golden.py     (build container only: needs the reference checkout)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (sets the suite's CPU arithmetic before torch is imported)
from make_train_batch_golden import write_npz  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pixel_nerf_yolo_amd.conf import Conf  # noqa: E402

YOLO_WEIGHTS = (1.0, 20.0, 1.0, 1.0)    # box, object, no_object, class (conf/exp/yolo.conf:42-47)
YOLO_CASES = {   # name: (cells, A, C, fraction of object cells, fraction ignored, seed)
    "y128": (128, 3, 2, 0.05, 0.10, 301),
    "y37": (37, 3, 2, 0.10, 0.10, 302),
    "ynoobj": (40, 3, 2, 0.0, 0.10, 303),
    "ya1c1": (48, 1, 1, 0.15, 0.10, 304),
    "ya3c5": (48, 3, 5, 0.10, 0.10, 305),
}
RGB_CASES = {    # name: (shape, use_l1 coarse, use_l1 fine, has fine, seed)
    "mse_mse": ((4, 128, 3), False, False, True, 401),
    "l1_mse": ((2, 50, 3), True, False, True, 402),
    "coarse_only": ((2, 50, 3), False, False, False, 403),
}
LAMBDAS = (0.7, 1.3)


def yolo_inputs(cells, A, C, f_obj, f_ign, seed):
    rs = np.random.RandomState(seed)
    pred = np.empty((1, cells, A, 5 + C), dtype=np.float32)
    pred[..., 0] = rs.uniform(1e-3, 1.0 - 1e-3, size=(1, cells, A))
    pred[..., 1:3] = rs.randn(1, cells, A, 2)
    pred[..., 3:5] = rs.uniform(-2.0, 2.0, size=(1, cells, A, 2))
    pred[..., 5:] = rs.randn(1, cells, A, C)
    target = np.empty((1, cells, A, 6), dtype=np.float32)
    u = rs.rand(1, cells, A)
    obj = np.where(u < f_obj, 1.0, np.where(u < f_obj + f_ign, -1.0, 0.0))
    if f_obj > 0 and not (obj == 1.0).any():
        obj[0, cells // 2, 0] = 1.0
    target[..., 0] = obj
    target[..., 1:3] = rs.uniform(0.0, 1.0, size=(1, cells, A, 2))
    target[..., 3:5] = rs.uniform(0.02, 0.9, size=(1, cells, A, 2))
    target[..., 5] = rs.randint(0, C, size=(1, cells, A))
    anchors = rs.uniform(0.1, 0.6, size=(A, 2)).astype(np.float32)
    return torch.from_numpy(pred), torch.from_numpy(target), torch.from_numpy(anchors)


def capture_yolo(ref_loss, name, d):
    cells, A, C, f_obj, f_ign, seed = YOLO_CASES[name]
    pred, target, anchors = yolo_inputs(cells, A, C, f_obj, f_ign, seed)
    crit = ref_loss.YoloLoss(A, *YOLO_WEIGHTS)
    leaf = pred.clone().requires_grad_()
    out = crit(leaf.clone(), target.clone(), anchors.clone())
    out[0].backward()
    terms = np.array([float(t) for t in out], dtype=np.float32)
    d[name + "_pred"], d[name + "_target"], d[name + "_anchors"] = mg.np_(pred), mg.np_(target), mg.np_(anchors)
    d[name + "_weights"] = np.array(YOLO_WEIGHTS, dtype=np.float32)
    d[name + "_terms"], d[name + "_d_pred"] = terms, mg.np_(leaf.grad)
    n_obj = int((target[..., 0] == 1).sum())
    print("captured", name, tuple(pred.shape), "n_obj", n_obj, "n_noobj", int((target[..., 0] == 0).sum()), "terms", terms)
    assert (n_obj == 0) == (f_obj == 0)


def capture_rgb(ref_loss, name, d):
    shape, l1_c, l1_f, has_fine, seed = RGB_CASES[name]
    rs = np.random.RandomState(seed)
    coarse, fine, gt = (torch.from_numpy(rs.uniform(0.0, 1.0, size=shape).astype(np.float32)) for _ in range(3))
    crit_c = ref_loss.get_rgb_loss(Conf({"use_l1": l1_c}), True)
    crit_f = ref_loss.get_rgb_loss(Conf({"use_l1": l1_f}), False)
    lam_c, lam_f = LAMBDAS if has_fine else (1.0, LAMBDAS[1])
    c, f = coarse.clone().requires_grad_(), fine.clone().requires_grad_()
    # PixelNerfTrainer.calc_losses:147-157
    rgb_loss = crit_c(c, gt)
    raw = [rgb_loss.item(), 0.0]
    terms = [rgb_loss.item() * lam_c, 0.0, 0.0]
    if has_fine:
        fine_loss = crit_f(f, gt)
        rgb_loss = rgb_loss * lam_c + fine_loss * lam_f
        raw[1] = fine_loss.item()
        terms[1] = fine_loss.item() * lam_f
    rgb_loss.backward()
    terms[2] = rgb_loss.item()
    d[name + "_coarse"], d[name + "_gt"] = mg.np_(coarse), mg.np_(gt)
    d[name + "_use_l1"] = np.array([l1_c, l1_f], dtype=np.int32)
    d[name + "_lambdas"] = np.array([lam_c, lam_f], dtype=np.float32)
    d[name + "_raw"], d[name + "_terms"] = np.array(raw, dtype=np.float32), np.array(terms, dtype=np.float32)
    d[name + "_d_coarse"] = mg.np_(c.grad)
    if has_fine:
        d[name + "_fine"], d[name + "_d_fine"] = mg.np_(fine), mg.np_(f.grad)
    print("captured", name, shape, "raw", raw, "terms", terms)


def main():
    mg.install_shims()
    from model import loss as ref_loss

    d = {}
    for name in YOLO_CASES:
        capture_yolo(ref_loss, name, d)
    for name in RGB_CASES:
        capture_rgb(ref_loss, name, d)
    path = os.path.join(mg.OUT, "losses.npz")
    write_npz(path, d)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
