#!/usr/bin/env python3
"""The optimizer stage of bench.py's training step, three ways: torch.optim.Adam as bench.py has it (ATen's multi-tensor
path), torch.optim.Adam(fused=True), and pixel_nerf_yolo_amd.optim.Adam(model=net) (one launch per group with the weight
refresh chained).  The step: SB = 4 objects x 3 views of 128 x 128, 128 rays per object, 64 + 32 (16
depth) samples, MSE(coarse) + MSE(fine), backward, optimizer; trunk frozen (60 MLP tensors) and trunk trained (+ ~110).

Per leg, after warm-up:
  * median_ms (p25, p75): whole steps timed one by one, device synchronised at each end;
  * tail_ms: with the device idle after backward(), wall clock of optimizer.step() + net._sync() up to a device synchronise --
    everything between the end of backward() and the point where the next step's first render kernel can start
    (optimizer, parameter-version check, weight refresh, Python);
  * tail_issue_ms: the same calls without the synchronise (host time to enqueue them);
  * optimizer_span_ms: device time from an event in front of optimizer.step() to one behind it, device idle at the start
    (the optimizer's kernels and the gaps between them; for this package's class it includes the chained refresh).
Prints one JSON line per leg and writes them to profiles/optimizer_sweep.json.

usage: python tools/optimizer_sweep.py [--steps 40] [--warmup 6] [--probe 20] [--out profiles/optimizer_sweep.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPTIMIZERS = ("torch", "torch_fused", "pnyolo")


def leg(train_encoder, which, steps, warmup, probe):
    import numpy as np
    import torch

    from pixel_nerf_yolo_amd import conf as pconf, synth
    from pixel_nerf_yolo_amd.model import make_model
    from pixel_nerf_yolo_amd.optim import Adam
    from pixel_nerf_yolo_amd.render import NeRFRenderer
    from pixel_nerf_yolo_amd.util import gen_rays

    dev = torch.device("cuda", 0)
    SB, NS, H, W, RB, KC, KF, KFD = 4, 3, 128, 128, 128, 64, 32, 16
    focal = 131.25                 # bench.py FOCAL128
    net = make_model(pconf.default_mv()["model"], stop_encoder_grad=not train_encoder)
    sd = {}
    sd.update({"mlp_coarse." + k: v for k, v in synth.mlp_state(71).items()})
    sd.update({"mlp_fine." + k: v for k, v in synth.mlp_state(72).items()})
    sd.update(synth.resnet34_state(74, residual_gain=0.25))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    net = net.to(dev).train()
    if not train_encoder:
        net.encoder.eval()
        for p in net.encoder.parameters():
            p.requires_grad_(False)
    ren = NeRFRenderer(n_coarse=KC, n_fine=KF, n_fine_depth=KFD, depth_std=0.01, white_bkgd=True).train()
    params = [p for p in net.parameters() if p.requires_grad]
    if which == "torch":
        opt = torch.optim.Adam(params, lr=1e-4)
    elif which == "torch_fused":
        opt = torch.optim.Adam(params, lr=1e-4, fused=True)
    else:
        opt = Adam(params, lr=1e-4, model=net)
    rs = np.random.RandomState(5)
    images = torch.from_numpy(np.stack([synth.images(80 + i, NS, H, W) for i in range(SB)])).to(dev)
    poses = torch.from_numpy(np.stack([synth.scene_cameras(NS, radius=1.3 + 0.02 * i)[0] for i in range(SB)]))
    fl = torch.full((SB,), focal)
    tgt = torch.from_numpy(np.stack([synth.pose_spherical(120.0 + 10 * i, -20.0, 1.3) for i in range(SB)]))
    all_rays = gen_rays(tgt, W, H, torch.tensor(focal), 0.8, 1.8, device=dev).reshape(SB, -1, 8)
    gt_all = torch.from_numpy(rs.uniform(0, 1, size=(SB, H * W, 3)).astype(np.float32)).to(dev)

    def backward(i):
        pix = torch.from_numpy(np.random.RandomState(1000 + i).randint(0, H * W, size=(SB, RB))).to(dev)
        rays = torch.gather(all_rays, 1, pix[..., None].expand(-1, -1, 8))
        gt = torch.gather(gt_all, 1, pix[..., None].expand(-1, -1, 3))
        net.encode(images, poses, fl)
        out = ren(net, rays, want_weights=True)
        loss = torch.nn.functional.mse_loss(out["coarse"]["rgb"], gt) + torch.nn.functional.mse_loss(out["fine"]["rgb"], gt)
        opt.zero_grad()
        loss.backward()

    for i in range(warmup):
        backward(i)
        opt.step()
    torch.cuda.synchronize()
    ms = []
    for i in range(steps):
        t0 = time.perf_counter()
        backward(100 + i)
        opt.step()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    tail, issue, span = [], [], []
    for i in range(3 * probe):
        backward(500 + i)
        torch.cuda.synchronize()
        kind = i % 3
        if kind == 0:       # synchronised wall clock of the step's tail
            t0 = time.perf_counter()
            opt.step()
            net._sync()
            torch.cuda.synchronize()
            tail.append(1e3 * (time.perf_counter() - t0))
        elif kind == 1:     # host time to enqueue it
            t0 = time.perf_counter()
            opt.step()
            net._sync()
            issue.append(1e3 * (time.perf_counter() - t0))
        else:               # device span of the optimizer alone
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            opt.step()
            e1.record()
            torch.cuda.synchronize()
            span.append(e0.elapsed_time(e1))
    torch.cuda.synchronize()
    q = np.percentile(ms, [25, 50, 75])
    return dict(trunk="trained" if train_encoder else "frozen", optimizer=which, tensors=len(params),
                parameters=int(sum(p.numel() for p in params)), steps=steps,
                median_ms=round(float(q[1]), 3), p25_ms=round(float(q[0]), 3), p75_ms=round(float(q[2]), 3),
                tail_ms=round(float(np.median(tail)), 4), tail_issue_ms=round(float(np.median(issue)), 4),
                optimizer_span_ms=round(float(np.median(span)), 4), range_status=net.range_status())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--probe", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimizer_sweep.json"))
    args = ap.parse_args()
    import pnyolo_pkg
    pnyolo_pkg.load()
    rows = []
    for train_encoder in (False, True):
        for which in OPTIMIZERS:
            rows.append(leg(train_encoder, which, args.steps, args.warmup, args.probe))
            print(json.dumps(rows[-1]), flush=True)
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
