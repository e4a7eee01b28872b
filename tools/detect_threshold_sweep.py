#!/usr/bin/env python3
"""
The thresholds of a YOLO metric pass swept at the real geometry (960 x 512 images, 3 anchors; one scale of 30 x 16 cells = 1440
boxes per view, three scales = 1884), 3 and 9 views, I x T x M = 1 x 8 x 1 and 4 x 8 x 4 settings (NMS IoUs x confidence cuts x
match IoUs), two ways on the same rendered cells and target cells (the scenes of tools/detect_views_sweep.py):

  sweep       util.DetectionSweepMeter.update: pny_detect_sweep, ONE launch of V * I * T workgroups, nothing read;
  sequential  util.DetectionMeter.update once per setting: I * T * M launches of pny_detect_views (V workgroups each), nothing
              read.  That kernel is the parent commit's: the yardstick.

Timing: wall clock around CALLS passes ending in a device synchronise, after WARMUP passes, median of REPEATS, the two ways
alternating within a repeat.  A last section times the sweep alone at 128, 256, 288 and 512 workgroups (the device has 256
compute units and a workgroup's LDS map leaves room for one per unit).  Launches and copies: torch.profiler on one pass of each,
outside the timed windows.  Before anything is timed the two ways' counts are compared, setting by setting and view by view
(they must be equal).  Writes one JSON object to --out (default profiles/detect_threshold_sweep.json) and prints it.  Needs an
MI355X.

Usage:  python tools/detect_threshold_sweep.py [--out PATH]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from detect_views_sweep import ANCHORS, SCALES, A, H, W, launches, scene  # noqa: E402  (loads the package too)
from pixel_nerf_yolo_amd import util as putil  # noqa: E402

WARMUP, REPEATS = 3, 5
SWEEP_CALLS = 20
VIEWS = (3, 9)
STEP_VIEWS = (4, 8, 9, 16)          # 128, 256, 288 and 512 workgroups of a 4 x 8 grid
CUTS = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8)
SWEEPS = {"1x8x1": ((0.75,), CUTS, (0.2,)), "4x8x4": ((0.45, 0.55, 0.65, 0.75), CUTS, (0.2, 0.3, 0.4, 0.5))}


def timed(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detect_threshold_sweep.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/detect_threshold_sweep.py needs an MI355X"
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out = {"tool": "detect_threshold_sweep", "device": torch.cuda.get_device_name(0), "compute_units": cus, "image": [H, W],
           "anchors_per_scale": A, "sweep_calls": SWEEP_CALLS, "warmup": WARMUP, "repeats": REPEATS, "cuts": list(CUTS),
           "sequential": "DetectionMeter.update (pny_detect_views) once per setting, nothing read", "shapes": []}
    for n_scales, cells in sorted(SCALES.items()):
        anchors = torch.from_numpy(ANCHORS[:n_scales * A].copy())
        for V in VIEWS:
            preds, targets = scene(V, cells, seed=100 * n_scales + V)
            p = [torch.from_numpy(a).to(dev) for a in preds]
            t = [torch.from_numpy(a).to(dev) for a in targets]
            inputs = (p, t, anchors, H, W, list(cells))
            for name, (nms_ious, nms_ts, match_ious) in SWEEPS.items():
                n_settings = len(nms_ious) * len(nms_ts) * len(match_ious)
                seq_calls = max(2, SWEEP_CALLS * 8 // n_settings)          # windows of comparable length
                sweep_meter = putil.DetectionSweepMeter(dev, nms_ious, nms_ts, match_ious)
                meter = putil.DetectionMeter(dev)
                last = {}

                def sweep():
                    last["sweep"] = sweep_meter.update(*inputs, n_views=V)

                def sequential():
                    last["records"] = [[[meter.update(*inputs, iou, cut, match, n_views=V).per_view for match in match_ious]
                                        for cut in nms_ts] for iou in nms_ious]

                sweep()
                sequential()
                counts = last["sweep"].counts.cpu().numpy()
                lists = last["sweep"].lists.cpu().numpy()
                for i in range(len(nms_ious)):
                    for k in range(len(nms_ts)):
                        for m in range(len(match_ious)):
                            rec = last["records"][i][k][m].cpu().numpy()
                            assert np.array_equal(rec[:, :3], counts[:, i, k, m]) and np.array_equal(rec[:, [3, 4, 7]], lists[:, i, k]), (name, i, k, m)
                table = sweep_meter.report()
                ks, cs = launches(sweep)
                kq, cq = launches(sequential)
                for _ in range(WARMUP):
                    sweep()
                    sequential()
                torch.cuda.synchronize()
                ts, tq = [], []
                for _ in range(REPEATS):
                    ts.append(timed(sweep, SWEEP_CALLS))
                    tq.append(timed(sequential, seq_calls))
                best = table.best()
                shape = {"scales": n_scales, "views": V, "boxes_per_view": int(sum((H // c) * (W // c) * A for c in cells)),
                         "sweep": name, "settings": n_settings, "workgroups": V * len(nms_ious) * len(nms_ts),
                         "rounds_of_workgroups": -(-V * len(nms_ious) * len(nms_ts) // cus),
                         "kept_predictions_per_view_by_cut": [round(float(x), 1) for x in lists[:, -1, :, 1].mean(0)],
                         "best_setting": [best[0], best[1], best[2]], "best_f1": round(best[5], 4),
                         "sweep_us_per_update": round(float(np.median(ts)), 1), "sweep_repeats_us": [round(v, 1) for v in ts],
                         "sweep_kernel_launches": ks, "sweep_device_copies": cs,
                         "sequential_calls_per_window": seq_calls,
                         "sequential_us_per_pass": round(float(np.median(tq)), 1), "sequential_repeats_us": [round(v, 1) for v in tq],
                         "sequential_kernel_launches": kq, "sequential_device_copies": cq,
                         "ratio": round(float(np.median(tq) / np.median(ts)), 2)}
                out["shapes"].append(shape)
                print(json.dumps(shape), flush=True)
    # the grid against the compute units: three scales, 4 x 8 x 1 settings (32 workgroups per view), the sweep alone
    nms_ious, nms_ts, match_ious = SWEEPS["4x8x4"][0], CUTS, (0.2,)
    cells = SCALES[3]
    anchors = torch.from_numpy(ANCHORS[:3 * A].copy())
    out["grid_steps"] = []
    for V in STEP_VIEWS:
        preds, targets = scene(V, cells, seed=300 + V)
        p = [torch.from_numpy(a).to(dev) for a in preds]
        t = [torch.from_numpy(a).to(dev) for a in targets]
        sweep_meter = putil.DetectionSweepMeter(dev, nms_ious, nms_ts, match_ious)
        sweep = lambda: sweep_meter.update(p, t, anchors, H, W, list(cells), n_views=V)      # noqa: E731
        for _ in range(WARMUP):
            sweep()
        torch.cuda.synchronize()
        ts = [timed(sweep, SWEEP_CALLS) for _ in range(REPEATS)]
        step = {"views": V, "workgroups": V * 32, "rounds_of_workgroups": -(-V * 32 // cus),
                "sweep_us_per_update": round(float(np.median(ts)), 1), "sweep_repeats_us": [round(v, 1) for v in ts]}
        out["grid_steps"].append(step)
        print(json.dumps(step), flush=True)
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
