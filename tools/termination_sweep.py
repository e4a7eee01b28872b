#!/usr/bin/env python3
"""
What early ray termination (net.set_termination; csrc/termination.hip, csrc/pny_termination.h) costs and saves on the C2 frame
of bench.py: 128 x 128 rays, 3 source views, ResNet-34 encoder, 64 coarse + 32 fine (16 depth) samples, white background.
  * the default render (mode off): the yardstick.  `--default-only` prints just this leg; it uses nothing this mode added, so
    the same file runs on the parent commit's tree and the two can be compared within their own spread;
  * t_min so small that nothing terminates (1e-30), at S = 2, 4, 8: the pure price of S host waits and S smaller MLP launches
    per pass;
  * SYNTHETIC opacity.  The seeded weights are not opaque (a ray ends at a transmittance of about 0.7 - 0.85), so the sigma row
    of lin_out (weight row 3 and its bias) of both MLPs is scaled by a gain g, bisected until about 75 %, 50 % and 25 % of the
    coarse samples are kept at t_min = 1e-2 and S = 4 (the floor at S = 4 is 25 %: segment 0 is always evaluated, so the last
    target is met only as closely as the gain's upper bound allows; the achieved fraction is reported).  Each opacity at
    S = 2, 4, 8: the frame's ms, the kept fraction per pass and per segment, the ms of the MLP kernels (the library's event
    pairs), what is left (classify, gather, expand, update, composite, sampling and the idle time of the host waits), and the
    PSNR against the SAME weights rendered without termination;
  * one case with a ball-shaped occupancy grid attached as well (the radius bisected to keep about half the coarse samples).
How much a TRAINED scene keeps is not measured here: there is no trained checkpoint in the tree.
Timing: a pair of device events around every one of CALLS frames after WARMUP; min, median and max over the calls; the same
Philox seed for every frame.  Prints one JSON line (profiles/termination_sweep.json is one run of it).  Needs an MI355X.

Usage:  python tools/termination_sweep.py [--default-only]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pnyolo_pkg  # noqa: E402

pnyolo_pkg.load()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pixel_nerf_yolo_amd import conf as pconf  # noqa: E402
from pixel_nerf_yolo_amd import synth  # noqa: E402
from pixel_nerf_yolo_amd.model import make_model  # noqa: E402
from pixel_nerf_yolo_amd.render import NeRFRenderer  # noqa: E402
from pixel_nerf_yolo_amd.util import gen_rays  # noqa: E402

WARMUP, CALLS = 3, 20
NS, SIDE, KC, KF, KFD = 3, 128, 64, 32, 16
FOCAL128, Z_NEAR, Z_FAR = 131.25, 0.8, 1.8
BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
RESO = (128, 128, 128)
T_MIN, T_NEVER = 1e-2, 1e-30
SEGMENTS = (2, 4, 8)
GAIN_MAX = 1e3


def spread(t):
    t = np.asarray(t)
    return {"min": round(float(t.min()), 4), "median": round(float(np.median(t)), 4), "max": round(float(t.max()), 4)}


def event_times_ms(fn, calls=CALLS, warmup=WARMUP):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    return spread([a.elapsed_time(b) for a, b in pairs])


def c2_scene(dev):
    """bench.py's C2 scene: the same seeds, cameras and images."""
    net = make_model(pconf.default_mv()["model"]).eval()
    sd = {}
    sd.update({"mlp_coarse." + k: v for k, v in synth.mlp_state(71, d_latent=512).items()})
    sd.update({"mlp_fine." + k: v for k, v in synth.mlp_state(72, d_latent=512).items()})
    sd.update(synth.resnet34_state(74, residual_gain=0.25))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    net = net.to(dev)
    src, tgt = synth.scene_cameras(NS)
    images = torch.from_numpy(synth.images(75, NS, SIDE, SIDE)).to(dev)
    focal, c = torch.tensor(FOCAL128), torch.tensor([[SIDE * 0.5, SIDE * 0.5]])
    net.encode(images[None], torch.from_numpy(src)[None], focal, c=c)
    net.project_latent()
    rays = gen_rays(torch.from_numpy(tgt)[None].to(dev), SIDE, SIDE, focal, Z_NEAR, Z_FAR, c=c[0]).reshape(1, -1, 8).contiguous()
    ren = NeRFRenderer(n_coarse=KC, n_fine=KF, n_fine_depth=KFD, depth_std=0.01, white_bkgd=True).eval()
    return net, ren, rays


def frame(net, ren, rays):
    ren._calls = 0            # the same Philox seed for every frame
    with torch.no_grad():
        return ren(net, rays)


def frame_row(net, ren, rays):
    ms = event_times_ms(lambda: frame(net, ren, rays))
    return {"frame_ms": ms, "rays_per_s": round(rays.shape[1] / (ms["median"] * 1e-3))}


def psnr(a, b):
    return round(float(-10.0 * torch.log10(torch.mean((a - b) ** 2).clamp_min(1e-20))), 2)


class Opacity:
    """The sigma row of lin_out of both MLPs times a gain, in place (the library follows in-place changes of the weights)."""

    def __init__(self, net):
        self.net = net
        self.rows = [(m.lin_out, m.lin_out.weight[3].detach().clone(), m.lin_out.bias[3].detach().clone())
                     for m in (net.mlp_coarse, net.mlp_fine)]

    def set(self, gain):
        with torch.no_grad():
            for lin, w, b in self.rows:
                lin.weight[3].copy_(w * gain)
                lin.bias[3].copy_(b * gain)


def mlp_kernel_ms(net, ren, rays):
    net.enable_kernel_timing(True)
    frame(net, ren, rays)
    torch.cuda.synchronize()
    ms = net.last_mlp_stats(full=True)["kernel_ms"]
    net.enable_kernel_timing(False)
    return ms


def terminated_row(net, ren, rays, t_min, segments, plain_ms, plain_rgb):
    net.set_termination(t_min, segments)
    row = {"t_min": t_min, "segments": segments}
    row.update(frame_row(net, ren, rays))
    rgb = frame(net, ren, rays)["fine"]["rgb"]
    cull, segs = net.last_cull(), net.last_termination()
    n = rays.shape[1]
    row["kept_fraction"] = {p: round(cull[p][0] / cull[p][1], 4) for p in cull}
    row["segments_issued"] = {p: len(segs[p]) for p in segs}
    row["alive_fraction_per_segment"] = {p: [round(a / n, 4) for a, _ in segs[p]] for p in segs}
    row["kept_per_segment"] = {p: [k for _, k in segs[p]] for p in segs}
    row["psnr_db_vs_unterminated"] = psnr(rgb, plain_rgb)
    mlp_ms = mlp_kernel_ms(net, ren, rays)
    row["stage_ms"] = {"mlp_kernels": round(mlp_ms, 4), "rest_of_frame": round(row["frame_ms"]["median"] - mlp_ms, 4)}
    row["speedup_vs_unterminated"] = round(plain_ms / row["frame_ms"]["median"], 3)
    net.set_termination(None)
    return row


def gain_keeping(net, ren, rays, opacity, fraction):
    """The gain (log-bisected in 1 .. GAIN_MAX) at which about `fraction` of the coarse samples are kept at T_MIN and S = 4."""
    lo, hi = 0.0, float(np.log(GAIN_MAX))
    net.set_termination(T_MIN, 4)
    for _ in range(14):
        mid = 0.5 * (lo + hi)
        opacity.set(float(np.exp(mid)))
        frame(net, ren, rays)
        kept, total = net.last_cull()["coarse"]
        lo, hi = (mid, hi) if kept / total > fraction else (lo, mid)
    net.set_termination(None)
    return float(np.exp(0.5 * (lo + hi)))


def ball_grid(radius, dev):
    from pixel_nerf_yolo_amd import recon as precon
    ax = torch.linspace(-1.0, 1.0, RESO[0], device=dev)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    sigma = ((x * x + y * y + z * z) <= radius * radius).float().contiguous()
    return precon.occupancy_grid(None, BOX[0], BOX[1], sigma_thresh=0.5, dilate=0, outside_empty=True, sigma=sigma)


def radius_keeping(net, ren, rays, fraction, dev):
    lo, hi = 0.0, 1.8
    for _ in range(12):
        mid = 0.5 * (lo + hi)
        net.set_occupancy(ball_grid(mid, dev))
        frame(net, ren, rays)
        kept, total = net.last_cull()["coarse"]
        lo, hi = (mid, hi) if kept / total < fraction else (lo, mid)
    net.set_occupancy(None)
    return 0.5 * (lo + hi)


def main():
    assert torch.cuda.is_available(), "tools/termination_sweep.py needs an MI355X"
    dev = torch.device("cuda:0")
    net, ren, rays = c2_scene(dev)
    out = {"tool": "termination_sweep", "device": torch.cuda.get_device_name(0), "calls": CALLS, "warmup": WARMUP,
           "frame": "C2: %d x %d rays, %d views, %d + %d (%d depth) samples" % (SIDE, SIDE, NS, KC, KF, KFD)}
    out["default"] = frame_row(net, ren, rays)
    if "--default-only" in sys.argv:
        print(json.dumps(out))
        return
    base = out["default"]["frame_ms"]["median"]
    plain = frame(net, ren, rays)["fine"]["rgb"].clone()
    out["default_mlp_kernels_ms"] = round(mlp_kernel_ms(net, ren, rays), 4)
    out["nothing_terminates"] = [terminated_row(net, ren, rays, T_NEVER, s, base, plain) for s in SEGMENTS]
    opacity = Opacity(net)
    out["opacity"] = {"note": "SYNTHETIC: the sigma row of lin_out of both MLPs times a gain; the seeded weights are not opaque, and "
                              "how much a trained scene keeps is not measured", "cases": []}
    for fraction in (0.75, 0.5, 0.25):
        g = gain_keeping(net, ren, rays, opacity, fraction)
        opacity.set(g)
        case = {"target_coarse_fraction_at_S4": fraction, "sigma_gain": round(g, 3), "unterminated": frame_row(net, ren, rays)}
        opaque_ms = case["unterminated"]["frame_ms"]["median"]
        opaque_rgb = frame(net, ren, rays)["fine"]["rgb"].clone()
        case["terminated"] = [terminated_row(net, ren, rays, T_MIN, s, opaque_ms, opaque_rgb) for s in SEGMENTS]
        if fraction == 0.5:     # ... and with a grid attached as well
            r = radius_keeping(net, ren, rays, 0.5, dev)
            grid = ball_grid(r, dev)
            net.set_occupancy(grid)
            grid_row = frame_row(net, ren, rays)
            grid_rgb = frame(net, ren, rays)["fine"]["rgb"].clone()
            cull = net.last_cull()
            grid_row["kept_fraction"] = {p: round(cull[p][0] / cull[p][1], 4) for p in cull}
            both = terminated_row(net, ren, rays, T_MIN, 4, grid_row["frame_ms"]["median"], grid_rgb)
            net.set_occupancy(None)
            case["with_ball_grid"] = {"radius": round(r, 4), "grid_only": grid_row, "grid_and_termination": both}
        out["opacity"]["cases"].append(case)
    opacity.set(1.0)
    again = frame(net, ren, rays)["fine"]["rgb"]
    out["default_after"] = frame_row(net, ren, rays)
    out["default_bit_identical_after_switching_off"] = bool(torch.equal(again, plain))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
