#!/usr/bin/env python3
"""
Time per metrics.compare_views call (one launch: clamped bytes, PSNR and SSIM of every view, left on the device) and kernel
launches per call, against the reference's sequence on the same box: the device -> host copy of the render (eval/eval.py:278
`rgb[0].cpu()`) plus the clamp, the byte conversion and the per-view metrics on one thread as eval.py:288-345 runs them -- here
the fp64 restatement of tests/metrics_ref.py (scipy's uniform_filter, the routine skimage calls), since skimage is not installed.

Shapes: NV in {1, 47, 251} views of 128 x 128 and one view of 400 x 400.
Timing: fused, HIP events around 100 calls after 10 warm-up calls, median of 5 repeats; reference, wall clock of whole passes
(copy, then metrics), median of 3.  Launches: torch.profiler, one call.  Prints one JSON line (profiles/view_metrics_sweep.json
is one run of it).  Needs an MI355X.

Usage:  python tools/view_metrics_sweep.py
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pnyolo_pkg  # noqa: E402

pnyolo_pkg.load()

import numpy as np  # noqa: E402
import torch  # noqa: E402

import metrics_ref as mr  # noqa: E402
from pixel_nerf_yolo_amd import metrics as pmetrics  # noqa: E402

WARMUP, CALLS, REPEATS, REF_REPEATS = 10, 100, 5, 3
SHAPES = ((1, 128, 128), (47, 128, 128), (251, 128, 128), (1, 400, 400))


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
    assert torch.cuda.is_available(), "tools/view_metrics_sweep.py needs an MI355X"
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    out = {"tool": "view_metrics_sweep", "device": torch.cuda.get_device_name(0), "calls": CALLS, "warmup": WARMUP,
           "repeats": REPEATS, "reference_repeats": REF_REPEATS, "reference": "tests/metrics_ref.py (fp64, scipy uniform_filter), 1 thread",
           "shapes": []}
    rs = np.random.RandomState(1)
    for nv, h, w in SHAPES:
        gt = rs.uniform(0, 1, size=(nv, h, w, 3)).astype(np.float32)
        rgb = (gt + np.float32(0.05) * rs.standard_normal(gt.shape).astype(np.float32)).astype(np.float32)
        rgb_d, gt_d = torch.from_numpy(rgb).to(dev), torch.from_numpy(gt).to(dev)

        def fused():
            return pmetrics.compare_views(rgb_d, gt_d)

        med, runs = time_us(fused)
        k, m = launches(fused)
        ref_ms, copy_ms = [], []
        for _ in range(REF_REPEATS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = rgb_d.cpu().numpy()
            t1 = time.perf_counter()
            mr.to_bytes(host)
            mr.view_metrics(host, gt)
            t2 = time.perf_counter()
            copy_ms.append((t1 - t0) * 1e3)
            ref_ms.append((t2 - t0) * 1e3)
        res = fused()
        _, p_ref, s_ref = mr.view_metrics(rgb, gt)
        out["shapes"].append({
            "views": nv, "height": h, "width": w, "fused_us_per_call": round(med, 2), "fused_repeats_us": runs,
            "kernel_launches": k, "device_copies": m, "reference_ms_per_pass": round(float(np.median(ref_ms)), 3),
            "reference_copy_ms": round(float(np.median(copy_ms)), 3),
            "max_psnr_err_db": float(np.abs(res.psnr.cpu().numpy() - p_ref).max()),
            "max_ssim_err": float(np.abs(res.ssim.cpu().numpy() - s_ref).max())})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
