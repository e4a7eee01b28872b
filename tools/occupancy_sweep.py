#!/usr/bin/env python3
"""
What an occupancy grid (net.set_occupancy; csrc/occupancy.hip) costs and saves on the C2 frame of bench.py: 128 x 128 rays,
3 source views, ResNet-34 encoder, 64 coarse + 32 fine (16 depth) samples, white background, seeded weights.
  * the default render (no grid attached): the yardstick.  `--default-only` prints just this leg; it uses nothing this mode
    added, so the same file runs on the parent commit's tree and the two can be compared within their own spread;
  * an all-occupied grid: the pure overhead of classify, gather, expand and the two host waits;
  * ball-shaped synthetic grids (sigma 1 inside a ball about the origin, outside_empty) whose radius is bisected until about
    50 %, 25 % and 10 % of the COARSE samples are kept: the kept fraction of each pass, the frame's ms and rays/s, the ms of the
    classification of each pass (the stage entry on the frame's own depths), of the MLP kernels (the library's event pairs) and
    what is left (gather, expand, composite, sampling and the idle time of the two host waits);
  * the one-off cost of recon.occupancy_grid at 128^3 (two sigma_grid passes and the build) and the break-even number of frames;
  * PSNR of culled against unculled frames for grids learnt from this model at a few thresholds.  The weights are SEEDED, not
    trained: there is no object and no free space in their sigma, so these lines say what the mode does to a frame when the
    grid cuts into sigma, and little about a trained model's free space.
Timing: a pair of device events around every one of CALLS frames after WARMUP; min, median and max over the calls; the same
Philox seed for every frame.  Prints one JSON line (profiles/occupancy_sweep.json is one run of it).  Needs an MI355X.

Usage:  python tools/occupancy_sweep.py [--default-only]
"""
import ctypes as C
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

from pixel_nerf_yolo_amd import conf as pconf  # noqa: E402
from pixel_nerf_yolo_amd import lib as plib  # noqa: E402
from pixel_nerf_yolo_amd import recon as precon  # noqa: E402
from pixel_nerf_yolo_amd import synth  # noqa: E402
from pixel_nerf_yolo_amd.model import make_model  # noqa: E402
from pixel_nerf_yolo_amd.render import NeRFRenderer  # noqa: E402
from pixel_nerf_yolo_amd.util import gen_rays  # noqa: E402

WARMUP, CALLS = 3, 20
NS, SIDE, KC, KF, KFD = 3, 128, 64, 32, 16
FOCAL128, Z_NEAR, Z_FAR = 131.25, 0.8, 1.8
BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
RESO = (128, 128, 128)


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


def classify_ms(grid, rays, z):
    """The stage entry on the frame's own depths of one pass."""
    L, dev = plib.load(), rays.device
    n, k = z.shape
    need = C.c_int64(0)
    plib.check(L.pny_occupancy_classify_workspace_bytes(n * k, C.byref(need)))
    ws = torch.empty(need.value, device=dev, dtype=torch.uint8)
    slot = torch.empty(n, k, device=dev, dtype=torch.int32)
    kept = torch.empty(1, device=dev, dtype=torch.int64)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    args = (p(grid.bits), (C.c_int32 * 3)(*grid.dims), (C.c_double * 3)(*grid.c1), (C.c_double * 3)(*grid.c2), int(grid.outside_empty),
            p(rays), p(z), n, k, p(slot), p(kept), p(ws), need.value, plib.stream_of(dev))
    return event_times_ms(lambda: plib.check(L.pny_occupancy_classify(*args)))


def culled_row(net, ren, rays, grid, default_ms, with_stages=True):
    net.set_occupancy(grid)
    row = frame_row(net, ren, rays)
    cull = net.last_cull()
    row["kept_fraction"] = {p: round(cull[p][0] / cull[p][1], 4) for p in cull}
    row["kept"] = {p: list(cull[p]) for p in cull}
    row["speedup_vs_default"] = round(default_ms / row["frame_ms"]["median"], 3)
    if with_stages:
        n = rays.shape[1]
        dbg = {"z_coarse": torch.empty(1, n, KC, device=rays.device), "z_fine": torch.empty(1, n, KC + KF, device=rays.device)}
        ren._debug_out = dbg
        net.enable_kernel_timing(True)
        frame(net, ren, rays)
        torch.cuda.synchronize()
        mlp_ms = net.last_mlp_stats(full=True)["kernel_ms"]
        net.enable_kernel_timing(False)
        ren._debug_out = None
        cms = {"coarse": classify_ms(grid, rays[0], dbg["z_coarse"][0]), "fine": classify_ms(grid, rays[0], dbg["z_fine"][0])}
        row["stage_ms"] = {"classify": cms, "mlp_kernels": round(mlp_ms, 4),
                           "rest_of_frame": round(row["frame_ms"]["median"] - mlp_ms - cms["coarse"]["median"] - cms["fine"]["median"], 4)}
    net.set_occupancy(None)
    return row


def ball_sigma(radius, dev):
    ax = torch.linspace(-1.0, 1.0, RESO[0], device=dev)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    return ((x * x + y * y + z * z) <= radius * radius).float().contiguous()


def ball_grid(radius, dev):
    return precon.occupancy_grid(None, BOX[0], BOX[1], sigma_thresh=0.5, dilate=0, outside_empty=True, sigma=ball_sigma(radius, dev))


def radius_keeping(net, ren, rays, fraction, dev):
    lo, hi = 0.0, 1.8
    for _ in range(14):
        mid = 0.5 * (lo + hi)
        net.set_occupancy(ball_grid(mid, dev))
        frame(net, ren, rays)
        kept, total = net.last_cull()["coarse"]
        lo, hi = (mid, hi) if kept / total < fraction else (lo, mid)
    net.set_occupancy(None)
    return 0.5 * (lo + hi)


def main():
    assert torch.cuda.is_available(), "tools/occupancy_sweep.py needs an MI355X"
    dev = torch.device("cuda:0")
    net, ren, rays = c2_scene(dev)
    out = {"tool": "occupancy_sweep", "device": torch.cuda.get_device_name(0), "calls": CALLS, "warmup": WARMUP,
           "frame": "C2: %d x %d rays, %d views, %d + %d (%d depth) samples" % (SIDE, SIDE, NS, KC, KF, KFD)}
    out["default"] = frame_row(net, ren, rays)
    if "--default-only" in sys.argv:
        print(json.dumps(out))
        return
    base = out["default"]["frame_ms"]["median"]
    plain = frame(net, ren, rays)["fine"]["rgb"].clone()
    out["all_occupied"] = culled_row(net, ren, rays, precon.occupancy_grid(
        None, BOX[0], BOX[1], sigma_thresh=0.5, dilate=0, outside_empty=False, sigma=torch.ones(RESO, device=dev)), base)
    out["balls"] = []
    for fraction in (0.5, 0.25, 0.1):
        r = radius_keeping(net, ren, rays, fraction, dev)
        row = {"target_coarse_fraction": fraction, "radius": round(r, 4)}
        row.update(culled_row(net, ren, rays, ball_grid(r, dev), base))
        out["balls"].append(row)
    # the one-off cost: two sigma_grid passes and the build, host clock around the whole call, synchronised
    vol = precon.sigma_grid(net, BOX[0], BOX[1], RESO, coarse=True)
    vol_f = precon.sigma_grid(net, BOX[0], BOX[1], RESO, coarse=False)
    both = torch.maximum(vol, vol_f)
    t = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        precon.occupancy_grid(net, BOX[0], BOX[1], RESO, sigma_thresh=float(both.median()), dilate=1)
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    build = {d: event_times_ms(lambda d=d: precon.occupancy_grid(None, BOX[0], BOX[1], sigma_thresh=0.5, dilate=d, sigma=(vol, vol_f)))
             for d in (0, 1, 4)}
    out["one_off"] = {"occupancy_grid_128_ms_host_clock": spread(t), "build_only_ms_by_dilate_with_python": build,
                      "bits_bytes": 4 * precon.occupancy_words(RESO)}
    for row in out["balls"]:
        saved = base - row["frame_ms"]["median"]
        row["break_even_frames"] = round(float(np.median(t)) / saved, 1) if saved > 0 else None
    out["learnt"] = {"note": "seeded weights, not a trained model: these say little about a trained model's free space", "cases": []}
    for q in (0.5, 0.75, 0.9):
        thresh = float(torch.quantile(both.reshape(-1)[:: 8], q))
        grid = precon.occupancy_grid(None, BOX[0], BOX[1], sigma_thresh=thresh, dilate=1, sigma=(vol, vol_f))
        row = {"sigma_quantile": q, "sigma_thresh": round(thresh, 5), "occupied_fraction": round(grid.n_occupied / grid.n_cells, 4)}
        row.update(culled_row(net, ren, rays, grid, base, with_stages=False))
        net.set_occupancy(grid)
        row["psnr_db_vs_unculled"] = psnr(frame(net, ren, rays)["fine"]["rgb"], plain)
        net.set_occupancy(None)
        out["learnt"]["cases"].append(row)
    again = frame(net, ren, rays)["fine"]["rgb"]
    out["default_after"] = frame_row(net, ren, rays)
    out["default_bit_identical_after_clearing"] = bool(torch.equal(again, plain))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
