"""Speed and error of the matrix precisions on bench.py's C2 and C3 frames (MI355X).

For each workload the frame of `bench.py` (same seeds, cameras and inputs; the constants are imported from it) is rendered
under `f32`, `f16x2` and `f16` (include/pnyolo.h pny_scene_set_precision), and one JSON line is printed per workload:

  ms_per_frame, rays_per_s    median over --steps frames (encode + projection + render, as bench.py's C3 leg times it)
  mlp_kernel_ms               MLP kernel time of the frame (pny_scene_last_mlp_stats with pny_scene_enable_timing)
  f16_pipe_frac               issued f16 MFMA FLOP / mlp_kernel_ms / 2516.8 TF/s (f16x2 issues 3 MFMAs per product, f16 one;
                              f32 runs on the fp32 pipe: null)
  max_abs_rgb, max_abs_depth, psnr_db   the fine pass against the `f32` render of the same frame (same sample draws)

Usage: python tools/precision_sweep.py [--steps 5] [--workloads c2,c3]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (workload constants only; bench.py is not run)

PRECISIONS = ("f32", "f16x2", "f16")
MFMA_PER_PRODUCT = {"f32": None, "f16x2": 3, "f16": 1}


def build_frame(wl, dev):
    import torch
    from pixel_nerf_yolo_amd import conf as pconf, synth
    from pixel_nerf_yolo_amd.model import make_model
    from pixel_nerf_yolo_amd.render import NeRFRenderer
    from pixel_nerf_yolo_amd.util import gen_rays_range

    side, d_latent, lat_side, kc, kf, kfd, _, _ = bench.WORKLOADS[wl]
    mconf = pconf.default_mv()
    if d_latent != 512:
        mconf.d["model"]["encoder"]["backbone"] = "custom"
    net = make_model(mconf["model"]).eval()
    sd = {}
    sd.update({"mlp_coarse." + k: v for k, v in synth.mlp_state(71, d_latent=d_latent).items()})
    sd.update({"mlp_fine." + k: v for k, v in synth.mlp_state(72, d_latent=d_latent).items()})
    if wl == "c2":
        sd.update(synth.resnet34_state(74, residual_gain=0.25))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    net = net.to(dev)
    src, _ = synth.scene_cameras(bench.NS)
    images = torch.from_numpy(synth.images(75, bench.NS, side, side)).to(dev) if wl == "c2" else \
        torch.zeros(bench.NS, 3, side, side, device=dev)
    focal, c = torch.tensor(bench.FOCAL128 * side / 128.0), torch.tensor([[side * 0.5, side * 0.5]])
    poses = torch.from_numpy(src)[None]
    lat = None if wl == "c2" else torch.from_numpy(synth.latent(76, bench.NS, d_latent, lat_side, lat_side)).to(dev)
    rays = gen_rays_range(torch.from_numpy(synth.pose_spherical(120.0, -20.0, 1.3))[None], side, side, focal, bench.Z_NEAR,
                          bench.Z_FAR, 0, side * side, c=c[0], device=dev).reshape(1, -1, 8)
    ren = NeRFRenderer(n_coarse=kc, n_fine=kf, n_fine_depth=kfd, depth_std=0.01, white_bkgd=True).eval()

    def frame():
        net.encode(images[None], poses, focal, c=c, latent=lat)
        ren.base_seed, ren._calls = 1234, 0          # the same sample draws in every frame and precision
        with torch.no_grad():
            out = ren(net, rays)
        return out["fine"]["rgb"][0], out["fine"]["depth"][0]

    return net, frame, side * side


def sweep(wl, steps, dev):
    import torch
    net, frame, n_rays = build_frame(wl, dev)
    res, ref = {}, None
    for prec in PRECISIONS:
        net.set_matrix_precision(prec)
        frame()
        torch.cuda.synchronize()
        ms, kms, flops = [], [], 0.0
        net.enable_kernel_timing(True)
        for _ in range(steps):
            t0 = time.perf_counter()
            rgb, depth = frame()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
            st = net.last_mlp_stats(full=True)
            kms.append(st["kernel_ms"])
            flops = st["flops"]
        net.enable_kernel_timing(False)
        kernel = net.last_launch_precision()
        ms_med, k_med = statistics.median(ms), statistics.median(kms)
        r = {"kernel": kernel, "ms_per_frame": round(ms_med, 3), "rays_per_s": round(n_rays / (ms_med * 1e-3)),
             "mlp_kernel_ms": round(k_med, 3), "f16_pipe_frac": None}
        if MFMA_PER_PRODUCT[prec] and k_med > 0:
            r["f16_pipe_frac"] = round(flops * MFMA_PER_PRODUCT[prec] / (k_med * 1e-3) / 1e12 / bench.PEAK_F16_MFMA_TFLOPS, 4)
        if ref is None:
            ref = (rgb.clone(), depth.clone())
        mse = float(((rgb - ref[0]) ** 2).mean())
        r["max_abs_rgb"] = float((rgb - ref[0]).abs().max())
        r["max_abs_depth"] = float((depth - ref[1]).abs().max())
        r["psnr_db"] = None if mse == 0.0 else round(10.0 * math.log10(1.0 / mse), 2)
        res[prec] = r
    line = {"workload": wl, "rays": n_rays, "steps": steps, "precisions": res}
    if res["f16"]["mlp_kernel_ms"] > 0:
        line["f16_speedup_over_f16x2_mlp_kernel"] = round(res["f16x2"]["mlp_kernel_ms"] / res["f16"]["mlp_kernel_ms"], 3)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--workloads", default="c2,c3")
    args = ap.parse_args()
    import torch
    import pnyolo_pkg
    pnyolo_pkg.load()
    assert torch.cuda.is_available(), "precision_sweep.py needs an MI355X"
    dev = torch.device("cuda", 0)
    for wl in args.workloads.split(","):
        print(json.dumps(sweep(wl, args.steps, dev)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
