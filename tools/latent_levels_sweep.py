#!/usr/bin/env python3
"""
Time per PixelNeRFNet.encode(latent=[m0, m1, m2]) call and per backward from the channel-last latent gradient to the maps'
gradients, against yardsticks taken in the same run on the same inputs:
  * the ATen sequence the list path replaces: F.interpolate(bilinear, align_corners=True) per level, torch.cat,
    encode(latent=tensor) (which transposes to channel-last); backwards, the channel-last gradient made NCHW
    (permute + contiguous, what PixelNeRFNet.latent_grad's result() does for a tensor latent) and autograd through cat and the interpolations;
  * a plain device copy of the latent's bytes (``dst.copy_(src)``): what moving the result alone costs.
The two stage entries alone (pny_latent_levels, pny_latent_levels_backward: one launch each) are timed beside them.

Shapes: 3 views x (256, 512, 1024) channels at (64 x 64, 32 x 32, 16 x 16) and at (64 x 120, 32 x 60, 16 x 30), the real
data's geometry; d_latent = 1792.
Timing: a pair of device events around every one of CALLS calls after WARMUP; min, median and max over the calls.
Prints one JSON line (profiles/latent_levels_sweep.json is one run of it).  Needs an MI355X.

Usage:  python tools/latent_levels_sweep.py
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pnyolo_pkg  # noqa: E402

pnyolo_pkg.load()

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402

from pixel_nerf_yolo_amd import conf as pconf  # noqa: E402
from pixel_nerf_yolo_amd import lib as plib  # noqa: E402
from pixel_nerf_yolo_amd import synth  # noqa: E402
from pixel_nerf_yolo_amd.lib import check, ptr, stream_of  # noqa: E402
from pixel_nerf_yolo_amd.model import make_model  # noqa: E402

WARMUP, CALLS = 5, 50
NS, CHANNELS = 3, (256, 512, 1024)
SHAPES = {"64x64": ((64, 64), (32, 32), (16, 16)), "64x120": ((64, 120), (32, 60), (16, 30))}


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


def aten_latent(maps):
    size0 = tuple(maps[0].shape[-2:])
    return torch.cat([Fn.interpolate(m, size0, mode="bilinear", align_corners=True) for m in maps], dim=1)


def main():
    assert torch.cuda.is_available(), "tools/latent_levels_sweep.py needs an MI355X"
    dev = torch.device("cuda:0")
    L = plib.load()
    c = pconf.default_mv()
    c.d["model"]["encoder"]["backbone"] = "custom"            # d_latent = 1792, the latent is supplied
    net = make_model(c["model"], stop_encoder_grad=True).to(dev).train()
    poses, _ = synth.scene_cameras(NS)
    poses, focal = torch.from_numpy(poses)[None], torch.tensor(115.2)
    out = {"tool": "latent_levels_sweep", "device": torch.cuda.get_device_name(0), "calls": CALLS, "warmup": WARMUP, "views": NS,
           "channels": list(CHANNELS), "aten": "F.interpolate per level, torch.cat, encode(latent=tensor); backward: permute + "
           "contiguous of the channel-last gradient, autograd through cat and interpolate",
           "copy": "dst.copy_(src) of the latent's bytes", "cases": []}
    rs = np.random.RandomState(1)
    for name, sizes in SHAPES.items():
        (h0, w0), ltot = sizes[0], sum(CHANNELS)
        images = torch.zeros(1, NS, 3, 2 * h0, 2 * w0)
        maps = [torch.from_numpy(rs.randn(NS, ch, h, w).astype(np.float32)).to(dev).requires_grad_() for ch, (h, w) in zip(CHANNELS, sizes)]
        g = torch.from_numpy(rs.randn(NS, h0, w0, ltot).astype(np.float32)).to(dev)       # channel-last, as latent_grad's buffer
        src = torch.empty(NS, h0, w0, ltot, device=dev)
        dst = torch.empty_like(src)

        # per call
        t_this = event_times_us(lambda: net.encode(images, poses, focal, latent=maps))
        lat_this = net.latent(0)
        t_aten = event_times_us(lambda: net.encode(images, poses, focal, latent=aten_latent(maps)))
        lat_aten = net.latent(0)
        t_copy = event_times_us(lambda: dst.copy_(src))
        # the stage entries alone
        n = len(maps)
        arr = [(C.c_int * n)(*v) for v in (CHANNELS, [s[0] for s in sizes], [s[1] for s in sizes])]
        detached = [m.detach() for m in maps]
        ptrs = (C.c_void_p * n)(*[m.data_ptr() for m in detached])
        t_stage = event_times_us(lambda: check(L.pny_latent_levels(ptrs, *arr, n, NS, ptr(src), stream_of(dev))))
        d_maps = [torch.empty_like(m) for m in detached]
        d_ptrs = (C.c_void_p * n)(*[m.data_ptr() for m in d_maps])
        t_stage_bwd = event_times_us(lambda: check(L.pny_latent_levels_backward(ptr(g), d_ptrs, *arr, n, NS, stream_of(dev))))

        # per backward, from the channel-last gradient to the maps' gradients
        net.encode(images, poses, focal, latent=maps)
        token = net.differentiable_latent()
        assert token is not None
        t_bwd_this = event_times_us(lambda: torch.autograd.grad(token, maps, g, retain_graph=True))
        g_this = torch.autograd.grad(token, maps, g, retain_graph=True)
        lat = aten_latent(maps)
        t_bwd_aten = event_times_us(lambda: torch.autograd.grad(lat, maps, g.permute(0, 3, 1, 2).contiguous(), retain_graph=True))
        g_aten = torch.autograd.grad(lat, maps, g.permute(0, 3, 1, 2).contiguous(), retain_graph=True)

        def rel(a, b):
            return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)
        out["cases"].append({
            "case": "%d x %s at %s" % (NS, CHANNELS, sizes), "latent_bytes": src.numel() * 4,
            "encode_list_us": t_this, "encode_aten_us": t_aten, "copy_us": t_copy, "assemble_kernel_us": t_stage,
            "encode_aten_over_list": round(t_aten["median"] / t_this["median"], 2),
            "assemble_kernel_over_copy": round(t_stage["median"] / t_copy["median"], 2),
            "backward_list_us": t_bwd_this, "backward_aten_us": t_bwd_aten, "adjoint_kernel_us": t_stage_bwd,
            "backward_aten_over_list": round(t_bwd_aten["median"] / t_bwd_this["median"], 2),
            "latent_max_diff_over_max": rel(lat_this, lat_aten),
            "gradient_max_diff_over_max": max(rel(a, b) for a, b in zip(g_this, g_aten))})
        del maps, g, src, dst, lat, token, g_this, g_aten, lat_this, lat_aten, d_maps, detached
    print(json.dumps(out))


if __name__ == "__main__":
    main()
