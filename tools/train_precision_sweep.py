"""Speed and gradient error of the training step under the matrix precisions `f32`, `auto` and `f16_train` (MI355X).

The step is bench.py's --mode train step (C2 model, SB = 4 objects x 3 source views of 128x128 encoded by the frozen trunk,
128 rays per object, 64 + 32 (16) samples, MSE(coarse) + MSE(fine), Adam lr 1e-4; the module constants are imported from
bench.py, the batch shape is the one train_main sets).  Every precision starts from the same weights and sees the same
pixels.  One JSON line per precision:

  ms_per_step_median        median wall time of a step over --steps timed steps (after --warmup)
  kernel_ms                 MLP kernel time per step by stage (HIP events, summed over the concurrent scenes):
                            forward (incl. the stashing training forward), recompute (0 while the stash fits), chain (the
                            dX chain), weight_grads (immediate weight-gradient GEMMs with the latent-gradient and depth
                            kernels stamped beside them, plus the deferred flush).  The latent gradient has no column of
                            its own: the library stamps it with the GEMMs, and this frozen-trunk step has none.
  loss_curve                the loss of every step (warm-up and timed)
  grad_err_vs_f32           the first step's gradients against `f32`'s: max |g - g_f32| / max |g_f32| per MLP tensor
                            (max and median over the tensors, and the worst tensor)

Usage: python tools/train_precision_sweep.py [--steps 20] [--warmup 4] [--precisions f32,auto,f16_train]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (workload constants only; bench.py is not run)

SB, H, W, RB, KC, KF, KFD = 4, 128, 128, 128, 64, 32, 16   # bench.py train_main's batch


def run(prec, steps, warmup, dev):
    import numpy as np
    import torch

    from pixel_nerf_yolo_amd import conf as pconf, synth
    from pixel_nerf_yolo_amd.model import make_model
    from pixel_nerf_yolo_amd.render import NeRFRenderer
    from pixel_nerf_yolo_amd.util import gen_rays

    net = make_model(pconf.default_mv()["model"], stop_encoder_grad=True)
    sd = {}
    sd.update({"mlp_coarse." + k: v for k, v in synth.mlp_state(71).items()})
    sd.update({"mlp_fine." + k: v for k, v in synth.mlp_state(72).items()})
    sd.update(synth.resnet34_state(74, residual_gain=0.25))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    net = net.to(dev).train()
    if prec != "auto":
        net.set_matrix_precision(prec)
    net.encoder.eval()
    for p_ in net.encoder.parameters():
        p_.requires_grad_(False)
    ren = NeRFRenderer(n_coarse=KC, n_fine=KF, n_fine_depth=KFD, depth_std=0.01, white_bkgd=True).train()
    par = ren.bind_parallel(net, None).train()
    opt = torch.optim.Adam([p_ for p_ in net.parameters() if p_.requires_grad], lr=1e-4)
    rs = np.random.RandomState(5)
    images = torch.from_numpy(np.stack([synth.images(80 + i, bench.NS, H, W) for i in range(SB)])).to(dev)
    poses = torch.from_numpy(np.stack([synth.scene_cameras(bench.NS, radius=1.3 + 0.02 * i)[0] for i in range(SB)]))
    focal = torch.full((SB,), bench.FOCAL128)
    tgt = torch.from_numpy(np.stack([synth.pose_spherical(120.0 + 10 * i, -20.0, 1.3) for i in range(SB)]))
    all_rays = gen_rays(tgt, W, H, torch.tensor(bench.FOCAL128), bench.Z_NEAR, bench.Z_FAR, device=dev).reshape(SB, -1, 8)
    gt_all = torch.from_numpy(rs.uniform(0, 1, size=(SB, H * W, 3)).astype(np.float32)).to(dev)
    first_grads = None

    def step(i):
        nonlocal first_grads
        pix = torch.from_numpy(np.random.RandomState(1000 + i).randint(0, H * W, size=(SB, RB))).to(dev)
        rays = torch.gather(all_rays, 1, pix[..., None].expand(-1, -1, 8))
        gt = torch.gather(gt_all, 1, pix[..., None].expand(-1, -1, 3))
        ren.base_seed = 77 + i   # the same sampling jitter for every precision
        net.encode(images, poses, focal)
        out = par(rays, want_weights=True)
        loss = torch.nn.functional.mse_loss(out["coarse"]["rgb"], gt) + torch.nn.functional.mse_loss(out["fine"]["rgb"], gt)
        opt.zero_grad()
        loss.backward()
        if first_grads is None:
            first_grads = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None and k.startswith("mlp_")}
        opt.step()
        return loss

    net.enable_kernel_timing(True)
    curve = []
    for i in range(warmup):
        curve.append(step(i).detach())
    torch.cuda.synchronize(dev)
    k_ms = [0.0] * 4
    step_ms = []
    t_prev = time.perf_counter()
    for i in range(steps):
        curve.append(step(warmup + i).detach())
        f = net.last_mlp_stats(full=True)
        b = net.last_backward_stats()
        k_ms[0] += f["kernel_ms"]
        for j in range(3):
            k_ms[1 + j] += b["kernel_ms"][j]
        k_ms[3] += net.last_flush_stats()[1]
        t_now = time.perf_counter()
        step_ms.append((t_now - t_prev) * 1e3)
        t_prev = t_now
    torch.cuda.synchronize(dev)
    net.enable_kernel_timing(False)
    res = {"precision": prec, "steps": steps, "warmup": warmup, "ms_per_step_median": statistics.median(step_ms),
           "kernel_ms": dict(zip(("forward", "recompute", "chain", "weight_grads"), [m / steps for m in k_ms])),
           "loss_curve": [float(v) for v in curve], "last_backward_precision": net.last_backward_precision()}
    return res, first_grads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--precisions", default="f32,auto,f16_train")
    args = ap.parse_args()
    import torch
    import pnyolo_pkg
    pnyolo_pkg.load()
    dev = torch.device("cuda", 0)
    ref = None
    for prec in args.precisions.split(","):
        res, g = run(prec, args.steps, args.warmup, dev)
        if prec == "f32":
            ref = g
        if ref is not None:
            errs = {k: float((g[k] - ref[k]).abs().max()) / max(float(ref[k].abs().max()), 1e-30) for k in ref}
            worst = max(errs, key=errs.get)
            res["grad_err_vs_f32"] = {"max": errs[worst], "median": statistics.median(errs.values()), "worst_tensor": worst}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
