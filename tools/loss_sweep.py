#!/usr/bin/env python3
"""
Time per forward + backward call and kernel launches per call of the two training losses, fused (pixel_nerf_yolo_amd.loss,
one launch each) against the ATen sequence of tests/loss_ref.py in fp32 on the GPU (the reference's operations: boolean-mask
gathers, host reads of the two counts, sigmoid / exp / cat / IoU / BCE / MSE / cross entropy and their autograd graph).

Shapes: YOLO (1, 128, 3, 7), one training mini-batch of 128 rays x 3 anchors; NeRF (4, 128, 3), one step's rays.
Timing: HIP events around 200 calls after 20 warm-up calls, median of 5 repeats.  Launches: torch.profiler, one call.
Prints one JSON line.  Needs an MI355X.

Usage:  python tools/loss_sweep.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pnyolo_pkg  # noqa: E402

pnyolo_pkg.load()

import numpy as np  # noqa: E402
import torch  # noqa: E402

import loss_ref  # noqa: E402
from pixel_nerf_yolo_amd import conf as pconf  # noqa: E402
from pixel_nerf_yolo_amd import loss as ploss  # noqa: E402

WARMUP, CALLS, REPEATS = 20, 200, 5
WEIGHTS = (1.0, 20.0, 1.0, 1.0)


def time_us(fn):
    """Median over REPEATS of the HIP-event time of CALLS calls, per call, in microseconds."""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        b.synchronize()
        per_call.append(a.elapsed_time(b) * 1000.0 / CALLS)
    return float(np.median(per_call)), [round(v, 2) for v in per_call]


def launches(fn):
    """Device kernels and device copies of one call (torch.profiler)."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    kernels = copies = 0
    for e in prof.events():
        if str(e.device_type).endswith("CUDA"):
            if e.name.lower().startswith(("memcpy", "memset")):
                copies += 1
            else:
                kernels += 1
    return kernels, copies


def main():
    assert torch.cuda.is_available(), "tools/loss_sweep.py needs an MI355X"
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(1)
    cells, A, Cn = 128, 3, 2
    pred = np.empty((1, cells, A, 5 + Cn), dtype=np.float32)
    pred[..., 0] = rs.uniform(1e-3, 1 - 1e-3, size=(1, cells, A))
    pred[..., 1:3] = rs.randn(1, cells, A, 2)
    pred[..., 3:5] = rs.uniform(-2, 2, size=(1, cells, A, 2))
    pred[..., 5:] = rs.randn(1, cells, A, Cn)
    target = np.empty((1, cells, A, 6), dtype=np.float32)
    u = rs.rand(1, cells, A)
    target[..., 0] = np.where(u < 0.05, 1.0, np.where(u < 0.15, -1.0, 0.0))
    target[..., 1:3] = rs.uniform(0, 1, size=(1, cells, A, 2))
    target[..., 3:5] = rs.uniform(0.02, 0.9, size=(1, cells, A, 2))
    target[..., 5] = rs.randint(0, Cn, size=(1, cells, A))
    pred, target = torch.from_numpy(pred).to(dev), torch.from_numpy(target).to(dev)
    anchors = torch.from_numpy(rs.uniform(0.1, 0.6, size=(A, 2)).astype(np.float32)).to(dev)
    coarse, fine, gt = (torch.from_numpy(rs.uniform(0, 1, size=(4, 128, 3)).astype(np.float32)).to(dev) for _ in range(3))

    yolo = ploss.YoloLoss(A, *WEIGHTS)
    nerf = ploss.NerfLoss(pconf.Conf({"use_l1": False}), pconf.Conf({"use_l1": False}), 1.0, 1.0)
    p = pred.clone().requires_grad_()
    c, f = coarse.clone().requires_grad_(), fine.clone().requires_grad_()

    def yolo_fused():
        p.grad = None
        yolo(p, target, anchors)[0].backward()

    def yolo_aten():
        p.grad = None
        loss_ref.yolo_terms(p, target, anchors, WEIGHTS, dtype=torch.float32)[0][0].backward()

    def nerf_fused():
        c.grad = f.grad = None
        nerf(c, f, gt)[0].backward()

    def nerf_aten():
        c.grad = f.grad = None
        loss_ref.rgb_terms(c, f, gt, dtype=torch.float32)[2].backward()

    out = {"tool": "loss_sweep", "device": torch.cuda.get_device_name(0), "calls": CALLS, "warmup": WARMUP, "repeats": REPEATS,
           "yolo_shape": [1, cells, A, 5 + Cn], "nerf_shape": [4, 128, 3]}
    for name, fn in (("yolo_fused", yolo_fused), ("yolo_aten", yolo_aten), ("nerf_fused", nerf_fused), ("nerf_aten", nerf_aten)):
        med, runs = time_us(fn)
        k, m = launches(fn)
        out[name] = {"us_per_call": round(med, 2), "repeats_us": runs, "kernel_launches": k, "device_copies": m}
    out["yolo_speedup"] = round(out["yolo_aten"]["us_per_call"] / out["yolo_fused"]["us_per_call"], 2)
    out["nerf_speedup"] = round(out["nerf_aten"]["us_per_call"] / out["nerf_fused"]["us_per_call"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
