#!/usr/bin/env python3
"""
Time per metrics.lpips_views call (LPIPS on VGG-16 of every view, left on the device) and kernel launches per call, against the
same definition run in fp32 through ATen on the same GPU: tests/lpips_ref.py on device tensors (torch.nn.functional.conv2d,
max_pool2d and elementwise kernels), walked in the same batches of 32 pairs as calc_metrics.py's --lpips_batch_size.  Seeded
stand-in weights (synth.vgg16_lpips_state): the time does not depend on the values.

Shapes: NV in {47, 251} views of 128 x 128 and one view of 400 x 400 (those of tools/view_metrics_sweep.py).
Timing: both sides are warmed up at the shape, then HIP events around windows of at least 3 calls and about half a second,
median of REPEATS windows per side, the two sides alternating.  Launches: torch.profiler, one call.  Also records the largest difference between the two
sides' values.  Prints one JSON line (profiles/lpips_sweep.json is one run of it).  Needs an MI355X.

Usage:  python tools/lpips_sweep.py
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

import lpips_ref as lr  # noqa: E402
from pixel_nerf_yolo_amd import metrics as pmetrics  # noqa: E402
from pixel_nerf_yolo_amd import synth  # noqa: E402

WARMUP, MIN_CALLS, WINDOW_MS, REPEATS, BATCH = 2, 3, 500.0, 3, 32
SHAPES = ((47, 128, 128), (251, 128, 128), (1, 400, 400))


def window_ms(fn, calls):
    """HIP-event time of `calls` calls, per call, in milliseconds."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def time_pair(f, g):
    """Both sides warmed up, then REPEATS windows of each, alternating; a window is at least MIN_CALLS calls and about
    WINDOW_MS long.  -> (median f, median g, f's windows, g's windows, calls per window of f and of g), milliseconds per call."""
    calls = []
    for fn in (f, g):
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        calls.append(max(MIN_CALLS, int(np.ceil(WINDOW_MS / max(window_ms(fn, 1), 1e-3)))))
    tf, tg = [], []
    for _ in range(REPEATS):
        tf.append(window_ms(f, calls[0]))
        tg.append(window_ms(g, calls[1]))
    return float(np.median(tf)), float(np.median(tg)), [round(v, 3) for v in tf], [round(v, 3) for v in tg], calls


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
    assert torch.cuda.is_available(), "tools/lpips_sweep.py needs an MI355X"
    dev = torch.device("cuda:0")
    state = synth.vgg16_lpips_state(4711)
    model = pmetrics.LPIPS().load_state_dict(state)
    convs, lins = lr.weights_of(state)
    convs_d, lins_d = [(w.to(dev), b.to(dev)) for w, b in convs], [w.to(dev) for w in lins]
    out = {"tool": "lpips_sweep", "device": torch.cuda.get_device_name(0), "min_calls": MIN_CALLS, "window_ms": WINDOW_MS, "warmup": WARMUP, "repeats": REPEATS,
           "batch_size": BATCH, "reference": "tests/lpips_ref.py in fp32 on the GPU (ATen conv2d / max_pool2d), batches of 32 pairs",
           "shapes": []}
    rs = np.random.RandomState(1)
    for nv, h, w in SHAPES:
        gt = torch.from_numpy(rs.uniform(0, 1, size=(nv, h, w, 3)).astype(np.float32))
        rgb = (gt + torch.from_numpy(rs.standard_normal((nv, h, w, 3)).astype(np.float32)) * 0.05).clamp(0, 1).to(dev)
        gt = gt.to(dev)

        def fused():
            return pmetrics.lpips_views(model, rgb, gt, batch_size=BATCH)

        def aten():
            vals = []
            with torch.no_grad():
                for i0 in range(0, nv, BATCH):
                    x0 = lr.pm1_from_01(rgb[i0:i0 + BATCH]).permute(0, 3, 1, 2)
                    x1 = lr.pm1_from_01(gt[i0:i0 + BATCH]).permute(0, 3, 1, 2)
                    vals.append(lr.lpips(x0, x1, convs_d, lins_d, dtype=torch.float32)[0])
            return torch.cat(vals)

        diff = float((fused().cpu() - aten().cpu().double()).abs().max())
        value = float(fused().mean())
        t_f, t_a, reps_f, reps_a, calls = time_pair(fused, aten)
        k_f, c_f = launches(fused)
        k_a, c_a = launches(aten)
        out["shapes"].append({"views": nv, "height": h, "width": w, "calls_per_window": calls, "mean_value": value, "max_abs_diff_to_aten_fp32": diff,
                              "lpips_views_ms": round(t_f, 3), "lpips_views_ms_repeats": reps_f, "lpips_views_kernels": k_f,
                              "lpips_views_copies": c_f, "aten_fp32_ms": round(t_a, 3), "aten_fp32_ms_repeats": reps_a,
                              "aten_fp32_kernels": k_a, "aten_fp32_copies": c_a, "aten_over_lpips_views": round(t_a / t_f, 3)})
        del rgb, gt
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
