#!/usr/bin/env python3
"""
Time per augment.color_jitter call (one launch: saturation, hue, contrast and brightness of every view of every object) against
two yardsticks taken in the same run:
  * the host path as it stands without the kernel: data.ColorJitterDataset.apply_color_jitter on one item (all views of one
    object) on ONE CPU thread (for the byte format the float conversion of data.image_to_tensor_balanced is timed beside it);
  * ``out.copy_(inp)`` of the same device tensors: what moving the bytes alone costs.

Shapes (SB x NV x H x W): 1 x 49 x 300 x 400 as floats and as bytes (a YOLO / DTU item), 4 x 49 x 300 x 400, 4 x 50 x 128 x 128
and 1 x 1 x 400 x 400 as floats.  One workgroup owns one image, so the last shape runs on one CU.
Timing: a pair of device events around every one of CALLS calls after WARMUP; min, median and max over the calls.
Errors: the kernel's and the host chain's worst absolute difference from the fp64 restatement of tests/augment_ref.py, in output
units [-1, 1], over the objects named in "error_objects" (all of them where the batch is small).
Prints one JSON line (profiles/color_jitter_sweep.json is one run of it).  Needs an MI355X.

Usage:  python tools/color_jitter_sweep.py
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

import augment_ref as ar  # noqa: E402
from pixel_nerf_yolo_amd import augment as paug  # noqa: E402
from pixel_nerf_yolo_amd import data as pdata  # noqa: E402

WARMUP, CALLS = 10, 100
SHAPES = ((1, 49, 300, 400, "float"), (1, 49, 300, 400, "bytes"), (4, 49, 300, 400, "float"), (4, 50, 128, 128, "float"),
          (1, 1, 400, 400, "float"))
ERROR_PIXELS = 8e6        # batches above this many pixels have their first and last object checked, not all


def event_times_us(fn):
    """Device-event time of each of CALLS calls after WARMUP, in microseconds."""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    t = np.array([a.elapsed_time(b) * 1000.0 for a, b in pairs])
    return {"min": round(float(t.min()), 2), "median": round(float(np.median(t)), 2), "max": round(float(t.max()), 2)}


class _Item:
    z_near = z_far = base_path = image_to_tensor = None


def host_item(images_np, fmt, seed):
    """One item through the host path on one thread: (jittered float32 (NV, 3, H, W), the fp64 factors it drew, seconds for the
    jitter, seconds for the byte -> float conversion or None)."""
    convert_s = None
    if fmt == "bytes":
        t0 = time.perf_counter()
        x = torch.stack([pdata.image_to_tensor_balanced(im) for im in images_np])
        convert_s = time.perf_counter() - t0
    else:
        x = torch.from_numpy(images_np.copy())
    ds = pdata.ColorJitterDataset(_Item())
    np.random.seed(seed)
    factors = np.array(ds.draw_factors())
    np.random.seed(seed)
    t0 = time.perf_counter()
    out = ds.apply_color_jitter(x)
    return out.numpy(), factors, time.perf_counter() - t0, convert_s


def worst_error(got, images_np, factors):
    """max |got - restatement| over the views of one object, one view at a time (the restatement is fp64)."""
    return max(float(np.abs(got[v:v + 1].astype(np.float64) - ar.jitter(images_np[v:v + 1], factors)).max()) for v in range(len(got)))


def main():
    assert torch.cuda.is_available(), "tools/color_jitter_sweep.py needs an MI355X"
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    out = {"tool": "color_jitter_sweep", "device": torch.cuda.get_device_name(0), "calls": CALLS, "warmup": WARMUP,
           "host": "data.ColorJitterDataset.apply_color_jitter, torch fp32, 1 thread, one item (object)",
           "error_units": "output, [-1, 1]", "shapes": []}
    rs = np.random.RandomState(1)
    for sb, nv, h, w, fmt in SHAPES:
        if fmt == "bytes":
            images = rs.randint(0, 256, size=(sb, nv, h, w, 3)).astype(np.uint8)
        else:
            images = rs.uniform(-1, 1, size=(sb, nv, 3, h, w)).astype(np.float32)
        host_out, f0, host_s, convert_s = host_item(images[0], fmt, 100 + nv)
        factors = np.stack([f0] + [np.array([rs.uniform(-0.1, 0.1)] + list(rs.uniform(0.9, 1.1, 3))) for _ in range(sb - 1)])
        f32 = factors.astype(np.float32)
        inp = torch.from_numpy(images).to(dev)
        res = torch.empty(sb, nv, 3, h, w, device=dev)
        copy_src = inp if fmt == "float" else inp.permute(0, 1, 4, 2, 3)
        t_kernel = event_times_us(lambda: paug.color_jitter(inp, f32, out=res))
        t_copy = event_times_us(lambda: res.copy_(copy_src))
        paug.color_jitter(inp, f32, out=res)
        got = res.cpu().numpy()
        objs = list(range(sb)) if sb * nv * h * w <= ERROR_PIXELS else sorted({0, sb - 1})
        row = {"objects": sb, "views": nv, "height": h, "width": w, "format": fmt,
               "kernel_us": t_kernel, "copy_us": t_copy, "kernel_over_copy": round(t_kernel["median"] / t_copy["median"], 2),
               "copy": "out.copy_(inp)" if fmt == "float" else "out.copy_(inp NHWC -> NCHW), uint8 -> fp32",
               "host_ms_per_item": round(host_s * 1e3, 2), "host_ms_per_batch": round(host_s * 1e3 * sb, 2),
               "host_over_kernel": round(host_s * 1e6 * sb / t_kernel["median"], 1),
               "error_objects": objs,
               "kernel_max_err": max(worst_error(got[o], images[o], f32[o]) for o in objs),
               "host_max_err": worst_error(host_out, images[0], factors[0])}
        if convert_s is not None:
            row["host_convert_ms_per_item"] = round(convert_s * 1e3, 2)
        out["shapes"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
