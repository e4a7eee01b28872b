#!/usr/bin/env python3
"""
Time per augment.ingest_views and util.build_yolo_targets call against yardsticks taken in the same run:
  * the host chain of data.py as it stands without the kernels, on ONE CPU thread: per view resize_bilinear_u8 +
    image_to_tensor_balanced (YOLODataset), or mask, box, image_to_tensor_balanced and F.interpolate(mode="area") of images and
    masks (SRNDataset); for the targets YOLODataset._get_all_bboxes per view + util.stage_yolo_targets;
  * a plain device copy of the same input bytes (``dst.copy_(src)``, uint8): what moving the input alone costs.

Shapes: 49 views 1080 x 1920 -> 512 x 960 by image_scale (0.5, 0.47407) (a YOLO item); 4 x 50 SRN views 128 -> 64 with mask and
box (two launches); 49 views x 8 boxes of targets at 512 x 960, cell 32, 3 anchors (one launch).
Timing: a pair of device events around every one of CALLS calls after WARMUP; min, median and max over the calls.  The target
call includes its two host-to-device copies.  The host chain is timed once.
Prints one JSON line (profiles/ingest_sweep.json is one run of it).  Needs an MI355X.

Usage:  python tools/ingest_sweep.py
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

import ingest_ref as ir  # noqa: E402
from pixel_nerf_yolo_amd import augment as paug  # noqa: E402
from pixel_nerf_yolo_amd import util as putil  # noqa: E402

WARMUP, CALLS = 5, 50
SCALE = (0.5, 0.47407)


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


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


def row(name, t_kernel, t_copy, host_s, **more):
    r = {"case": name, "kernel_us": t_kernel, "host_ms": round(host_s * 1e3, 2), "host_over_kernel": round(host_s * 1e6 / t_kernel["median"], 1)}
    if t_copy is not None:
        r.update(copy_us=t_copy, kernel_over_copy=round(t_kernel["median"] / t_copy["median"], 2))
    r.update(more)
    return r


def main():
    assert torch.cuda.is_available(), "tools/ingest_sweep.py needs an MI355X"
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    out = {"tool": "ingest_sweep", "device": torch.cuda.get_device_name(0), "calls": CALLS, "warmup": WARMUP,
           "host": "data.py's chain after decoding, torch fp32, 1 thread", "copy": "dst.copy_(src) of the input bytes", "cases": []}
    rs = np.random.RandomState(1)

    # a YOLO item
    u8 = rs.randint(0, 256, size=(49, 1080, 1920, 3)).astype(np.uint8)
    (host, _), host_s = timed(lambda: ir.host_bilinear(u8, *SCALE))
    src = torch.from_numpy(u8).to(dev)
    dst, res = torch.empty_like(src), torch.empty(49, 3, 512, 960, device=dev)
    t_kernel = event_times_us(lambda: paug.ingest_views(src, scale=SCALE, out=res))
    t_copy = event_times_us(lambda: dst.copy_(src))
    got = res.cpu()
    out["cases"].append(row("yolo 49 x 1080 x 1920 -> 512 x 960 bilinear", t_kernel, t_copy, host_s, launches=1,
                            bytes_differing_from_host=int((got != host).sum()), bytes_total=got.numel(),
                            max_abs_diff_from_host=float((got - host).abs().max())))
    del src, dst, res, u8, host, got

    # an SRN batch
    u8 = rs.randint(0, 255, size=(4, 50, 128, 128, 3)).astype(np.uint8)
    u8[:, :, :20] = 255
    u8[:, :, :, 100:] = 255
    (h_img, h_mask, h_box), host_s = timed(lambda: [torch.stack(t) for t in zip(*[ir.host_srn(o, (64, 64)) for o in u8])])
    src = torch.from_numpy(u8).to(dev)
    dst = torch.empty_like(src)
    t_kernel = event_times_us(lambda: paug.ingest_views(src, size=(64, 64), resize="area", white_mask=True))
    t_copy = event_times_us(lambda: dst.copy_(src))
    img, mask, box = (t.cpu() for t in paug.ingest_views(src, size=(64, 64), resize="area", white_mask=True))
    out["cases"].append(row("srn 4 x 50 x 128 x 128 -> 64 x 64 area, mask and box", t_kernel, t_copy, host_s, launches=2,
                            image_max_abs_diff_from_host=float((img - h_img).abs().max()),
                            mask_max_abs_diff_from_host=float((mask - h_mask).abs().max()), boxes_equal_host=bool(torch.equal(box, h_box))))

    # the targets of a YOLO item
    anchors = ir.YOLO_ANCHORS[:3]
    views = [[[float(rs.uniform(0, 1)), float(rs.uniform(0, 1)), float(rs.uniform(0.03, 0.6)), float(rs.uniform(0.03, 0.6)), float(k % 3)]
              for k in range(8)] for _ in range(49)]
    lab, cnt = ir.pack_labels(views)
    host, host_s = timed(lambda: putil.stage_yolo_targets(ir.host_targets(views, 512, 960, [32], anchors, 3, ir.YOLO_IGNORE_IOU), dev))
    torch.cuda.synchronize()
    t_kernel = event_times_us(lambda: putil.build_yolo_targets(lab, cnt, 512, 960, [32], anchors, ir.YOLO_IGNORE_IOU, dev))
    got = putil.build_yolo_targets(lab, cnt, 512, 960, [32], anchors, ir.YOLO_IGNORE_IOU, dev)
    out["cases"].append(row("targets 49 views x 8 boxes, 512 x 960, cell 32, 3 anchors", t_kernel, None, host_s, launches=1,
                            equal_host=bool(torch.equal(got[0], host[0])) if ir.distinct_ious(views, anchors) else None))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
