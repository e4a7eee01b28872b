#!/usr/bin/env python3
"""Step time of the deterministic latent gradient (PixelNeRFNet.set_deterministic) against the
float-atomic default, on bench.py's training step: SB = 4 objects x 3 views of 128 x 128, 128 rays per object, 64 + 32
(16 depth) samples, MSE(coarse) + MSE(fine), backward, Adam.  Two graphs: the trunk trained (the reference's default: the
latent gradient feeds the trunk's backward) and the trunk frozen (--freeze_enc: no latent gradient, so the mode has nothing
to do).  Each leg: warm-up steps, then `--steps` steps timed one by one (device synchronised at each end); prints one JSON
line per leg with the median and the quartiles in ms.

usage: python tools/deterministic_sweep.py [--steps 40] [--warmup 6]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def leg(train_encoder, deterministic, steps, warmup):
    import numpy as np
    import torch

    from pixel_nerf_yolo_amd import conf as pconf, synth
    from pixel_nerf_yolo_amd.model import make_model
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
    net.set_deterministic(deterministic)
    ren = NeRFRenderer(n_coarse=KC, n_fine=KF, n_fine_depth=KFD, depth_std=0.01, white_bkgd=True).train()
    opt = torch.optim.Adam([p for p in net.parameters() if p.requires_grad], lr=1e-4)
    rs = np.random.RandomState(5)
    images = torch.from_numpy(np.stack([synth.images(80 + i, NS, H, W) for i in range(SB)])).to(dev)
    poses = torch.from_numpy(np.stack([synth.scene_cameras(NS, radius=1.3 + 0.02 * i)[0] for i in range(SB)]))
    fl = torch.full((SB,), focal)
    tgt = torch.from_numpy(np.stack([synth.pose_spherical(120.0 + 10 * i, -20.0, 1.3) for i in range(SB)]))
    all_rays = gen_rays(tgt, W, H, torch.tensor(focal), 0.8, 1.8, device=dev).reshape(SB, -1, 8)
    gt_all = torch.from_numpy(rs.uniform(0, 1, size=(SB, H * W, 3)).astype(np.float32)).to(dev)

    def step(i):
        pix = torch.from_numpy(np.random.RandomState(1000 + i).randint(0, H * W, size=(SB, RB))).to(dev)
        rays = torch.gather(all_rays, 1, pix[..., None].expand(-1, -1, 8))
        gt = torch.gather(gt_all, 1, pix[..., None].expand(-1, -1, 3))
        net.encode(images, poses, fl)
        out = ren(net, rays, want_weights=True)
        loss = torch.nn.functional.mse_loss(out["coarse"]["rgb"], gt) + torch.nn.functional.mse_loss(out["fine"]["rgb"], gt)
        opt.zero_grad()
        loss.backward()
        opt.step()

    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    ms = []
    for i in range(steps):
        t0 = time.perf_counter()
        step(100 + i)
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    took = net.last_latent_grad_deterministic() if train_encoder else None
    q = np.percentile(ms, [25, 50, 75])
    return dict(trunk="trained" if train_encoder else "frozen", deterministic=deterministic, took_deterministic_path=took,
                steps=steps, median_ms=round(float(q[1]), 3), p25_ms=round(float(q[0]), 3), p75_ms=round(float(q[2]), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=6)
    args = ap.parse_args()
    import pnyolo_pkg
    pnyolo_pkg.load()
    for train_encoder in (True, False):
        for det in (False, True):
            print(json.dumps(leg(train_encoder, det, args.steps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
