#!/usr/bin/env python3
"""The front end of a training step -- rays and ground truth of the sampled pixels -- two ways:

  reference_style: the reference's call-site sequence (train/trainlib/PixelNerfTrainer.py:84-123) on this package's API as it
                   was before util.sample_train_batch: per object gen_rays of every view, images * 0.5 + 0.5 and its NHWC
                   copy, CPU torch.randint / bbox_sample, the two gathers, torch.stack;
  sample_train_batch: one call, one kernel launch (seeded draws).

Shapes: SRN (4 objects x 50 views of 128 x 128) and DTU (4 x 49 views of 300 x 400), 128 rays per object, uniform and bbox
sampling.  Images and poses are on the device before the clock starts, as in the trainer (:61-64); focal stays on the CPU
as data["focal"] does.  Per leg, after warm-up, each call on its own with the device idle at the start:
  * wall_ms: host clock from the call to a device synchronise behind it (host work included);
  * device_ms: HIP events around the call (first kernel's start to last kernel's end, gaps included);
  * issue_ms: host clock until the call returns, without the synchronise.
Median (p25, p75) over --calls calls.  Prints one JSON line per leg and writes them to profiles/train_batch_sweep.json.

usage: python tools/train_batch_sweep.py [--calls 30] [--warmup 5] [--out profiles/train_batch_sweep.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"srn": (4, 50, 128, 128, 131.25), "dtu": (4, 49, 300, 400, 350.0)}   # SB, NV, H, W, focal
RAYS = 128
Z_NEAR, Z_FAR = 0.8, 1.8


def bbox_sample(bboxes, num_pix):
    """The reference's util.bbox_sample (src/util/util.py:222-237) restated: CPU draws, boxes (NV, 4) on the CPU."""
    import torch
    image_ids = torch.randint(0, bboxes.shape[0], (num_pix,))
    pb = bboxes[image_ids]
    x = (torch.rand(num_pix) * (pb[:, 2] + 1 - pb[:, 0]) + pb[:, 0]).long()
    y = (torch.rand(num_pix) * (pb[:, 3] + 1 - pb[:, 1]) + pb[:, 1]).long()
    return torch.stack((image_ids, y, x), dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_batch_sweep.json"))
    args = ap.parse_args()
    assert args.calls >= 20, "median of at least 20 calls"

    import numpy as np
    import torch

    import pnyolo_pkg
    pnyolo_pkg.load()
    from pixel_nerf_yolo_amd import synth
    from pixel_nerf_yolo_amd.util import gen_rays, sample_train_batch

    dev = torch.device("cuda", 0)
    rows = []
    for shape, (SB, NV, H, W, focal_v) in SHAPES.items():
        rs = np.random.RandomState(11)
        images = torch.from_numpy(rs.uniform(-1, 1, size=(SB, NV, 3, H, W)).astype(np.float32)).to(dev)
        poses = torch.from_numpy(np.stack([np.stack([synth.pose_spherical(360.0 * v / NV, -20.0, 1.3 + 0.1 * s)
                                                     for v in range(NV)]) for s in range(SB)])).to(dev)
        focal = torch.full((SB,), focal_v)                                       # data["focal"] (SB,), CPU
        lo = np.stack([rs.randint(0, W // 2, size=(SB, NV)), rs.randint(0, H // 2, size=(SB, NV))], -1)
        hi = lo + np.stack([rs.randint(1, W // 2, size=(SB, NV)), rs.randint(1, H // 2, size=(SB, NV))], -1)
        bboxes = torch.from_numpy(np.concatenate([lo, hi], -1).astype(np.float32))   # data["bbox"] (SB, NV, 4), CPU

        def reference_style(use_bbox):
            all_rgb_gt, all_rays = [], []
            for obj in range(SB):
                images_0to1 = images[obj] * 0.5 + 0.5
                cam_rays = gen_rays(poses[obj], W, H, focal[obj], Z_NEAR, Z_FAR, c=None)
                rgb_gt_all = images_0to1.permute(0, 2, 3, 1).contiguous().reshape(-1, 3)
                if use_bbox:
                    pix = bbox_sample(bboxes[obj], RAYS)
                    pix_inds = pix[..., 0] * H * W + pix[..., 1] * W + pix[..., 2]
                else:
                    pix_inds = torch.randint(0, NV * H * W, (RAYS,))
                all_rgb_gt.append(rgb_gt_all[pix_inds])
                all_rays.append(cam_rays.view(-1, 8)[pix_inds].to(device=dev))
            return torch.stack(all_rays), torch.stack(all_rgb_gt)

        def sampler(use_bbox):
            rays, rgb_gt, _ = sample_train_batch(images, poses, focal, Z_NEAR, Z_FAR, RAYS, bboxes=bboxes if use_bbox else None)
            return rays, rgb_gt

        for mode in ("uniform", "bbox"):
            for name, fn in (("reference_style", reference_style), ("sample_train_batch", sampler)):
                wall, devt, issue = [], [], []
                torch.cuda.reset_peak_memory_stats(dev)
                for it in range(args.warmup + args.calls):
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    e0.record()
                    out = fn(mode == "bbox")
                    e1.record()
                    t1 = time.perf_counter()
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    if it >= args.warmup:
                        wall.append((t2 - t0) * 1e3)
                        issue.append((t1 - t0) * 1e3)
                        devt.append(e0.elapsed_time(e1))
                    del out

                def q(v):
                    return [round(float(np.percentile(v, p)), 4) for p in (50, 25, 75)]
                row = dict(shape=shape, SB=SB, NV=NV, H=H, W=W, rays_per_object=RAYS, mode=mode, leg=name, calls=args.calls,
                           wall_ms=q(wall), device_ms=q(devt), issue_ms=q(issue),
                           peak_alloc_mb=round(torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1))
                rows.append(row)
                print(json.dumps(row), flush=True)
        del images
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(dict(device=torch.cuda.get_device_name(0), note="median, p25, p75 per entry", rows=rows), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
