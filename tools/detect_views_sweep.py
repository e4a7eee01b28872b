#!/usr/bin/env python3
"""
The tail of a YOLO metric pass at the real geometry (960 x 512 images, cells of 32 / 64 / 128: 30 x 16, 15 x 8 and 7 x 4 cells
of 3 anchors), 1 and 3 scales, 3 / 9 / 16 views, two ways on the same rendered cells and target cells:

  batched   util.DetectionMeter.update: pny_detect_views, ONE launch for all views, nothing read (the pass reads once, in
            report(), which is not in the timed window: it is once per pass, not per update);
  per_view  what the tree did before: util.convert_cells_to_bboxes(as_tensor=True) per scale and list (one launch per image),
            a concatenation per list, and util.calculate_tp_fp_fn per view (an allocation, three launches and a blocking read of
            three integers each), the reads included.

Timing: wall clock around CALLS calls ending in a device synchronise, after WARMUP calls, median of REPEATS, the two ways
alternating within a repeat.  Launches and copies: torch.profiler on one call.  The counts of the two ways are compared (they
must be equal) before anything is timed.  Writes one JSON object to --out (default profiles/detect_views_sweep.json) and prints
it.  Needs an MI355X.

Usage:  python tools/detect_views_sweep.py [--out PATH]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pnyolo_pkg  # noqa: E402

pnyolo_pkg.load()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pixel_nerf_yolo_amd import util as putil  # noqa: E402

WARMUP, CALLS, REPEATS = 5, 20, 5
H, W, A = 512, 960, 3
SCALES = {1: (32,), 3: (32, 64, 128)}
VIEWS = (3, 9, 16)
NMS_IOU, MATCH_IOU = 0.5, 0.2
ANCHORS = np.array([[3.6, 4.1], [5.4, 6.9], [8.8, 9.5], [1.8, 2.0], [2.7, 3.4], [4.4, 4.7], [0.9, 1.0], [1.3, 1.7], [2.2, 2.4]], np.float32)


def scene(n_views, cells, seed):
    """Rendered cells and target cells per scale, (V * Hs * Ws, A, 7 | 6): about one target in twenty cells, predictions whose
    objectness follows the targets with noise, so that both lists survive the threshold in realistic numbers."""
    rs = np.random.RandomState(seed)
    preds, targets = [], []
    for c in cells:
        n = n_views * (H // c) * (W // c)
        t = np.zeros((n, A, 6), np.float32)
        obj = rs.rand(n, A) < 0.05
        t[..., 0] = obj
        t[..., 1:3] = rs.rand(n, A, 2)
        t[..., 3:5] = rs.uniform(0.5, 3.0, size=(n, A, 2))
        t[..., 5] = rs.randint(0, 2, size=(n, A))
        p = rs.randn(n, A, 7).astype(np.float32) * 0.3
        p[..., 0] = np.where(obj, 0.8, 0.1) + 0.25 * rs.randn(n, A)
        p[..., 1:3] += (t[..., 1:3] - 0.5) * 4
        preds.append(p.astype(np.float32))
        targets.append(t)
    return preds, targets


def timed(fn):
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / CALLS


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
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detect_views_sweep.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/detect_views_sweep.py needs an MI355X"
    dev = torch.device("cuda:0")
    out = {"tool": "detect_views_sweep", "device": torch.cuda.get_device_name(0), "image": [H, W], "anchors_per_scale": A,
           "calls": CALLS, "warmup": WARMUP, "repeats": REPEATS, "nms_iou": NMS_IOU, "match_iou": MATCH_IOU,
           "per_view": "convert_cells_to_bboxes per scale + calculate_tp_fp_fn per view, reads included", "shapes": []}
    for n_scales, cells in sorted(SCALES.items()):
        anchors = torch.from_numpy(ANCHORS[:n_scales * A].copy())
        for V in VIEWS:
            preds, targets = scene(V, cells, seed=100 * n_scales + V)
            nms_t = 0.45
            p = [torch.from_numpy(a).to(dev) for a in preds]
            t = [torch.from_numpy(a).to(dev) for a in targets]
            meter = putil.DetectionMeter(dev)
            last = {}

            def batched():
                last["scores"] = meter.update(p, t, anchors, H, W, list(cells), NMS_IOU, nms_t, MATCH_IOU, n_views=V)

            def per_view():
                lists = []
                for arrs, is_pred in ((t, False), (p, True)):
                    per_scale = [putil.convert_cells_to_bboxes(a.reshape(V, H // c, W // c, A, -1), anchors[s * A:(s + 1) * A], H // c, W // c,
                                                               is_pred, as_tensor=True) for s, (a, c) in enumerate(zip(arrs, cells))]
                    lists.append(torch.cat(per_scale, dim=1) if len(per_scale) > 1 else per_scale[0])
                tot = [0, 0, 0]
                for v in range(V):
                    for i, n in enumerate(putil.calculate_tp_fp_fn(lists[0][v], lists[1][v], NMS_IOU, nms_t, MATCH_IOU)):
                        tot[i] += n
                last["per_view"] = tot

            meter.reset()
            batched()
            per_view()
            rec = last["scores"].per_view.cpu().numpy()
            got = meter.report()
            assert list(got) == last["per_view"], (got, last["per_view"])
            kb, cb = launches(batched)
            kp, cp = launches(per_view)
            for _ in range(WARMUP):
                batched()
                per_view()
            torch.cuda.synchronize()
            tb, tp = [], []
            for _ in range(REPEATS):
                tb.append(timed(batched))
                tp.append(timed(per_view))
            shape = {"scales": n_scales, "views": V, "boxes_per_view": int(sum((H // c) * (W // c) * A for c in cells)),
                     "tp_fp_fn": list(got), "kept_targets_per_view": round(float(rec[:, 3].mean()), 1),
                     "kept_predictions_per_view": round(float(rec[:, 4].mean()), 1),
                     "batched_us_per_update": round(float(np.median(tb)), 1), "batched_repeats_us": [round(v, 1) for v in tb],
                     "batched_kernel_launches": kb, "batched_device_copies": cb,
                     "per_view_us_per_step": round(float(np.median(tp)), 1), "per_view_repeats_us": [round(v, 1) for v in tp],
                     "per_view_kernel_launches": kp, "per_view_device_copies": cp,
                     "ratio": round(float(np.median(tp) / np.median(tb)), 1)}
            out["shapes"].append(shape)
            print(json.dumps(shape), flush=True)
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
