#!/usr/bin/env python3
"""
Device time of the mesh extraction (pixel_nerf_yolo_amd.recon) against yardsticks taken in the same run:
  * recon.sigma_grid at 128^3 on the C1 model (one 64 x 64 source view, ResNet-34 encoder, coarse MLP), default
    slabs of 100 000 points: grid points, the network and the copy of the sigma channel, nothing on the host;
  * pny_mc_count + pny_mc_emit (recon.extract_mesh without its allocations: workspace and outputs are reused) at 128^3 and 256^3,
    on a ball and, at 128^3, on that model's volume at its median sigma; the launch count of each call;
  * for scale, the device-to-host copy of the same volume, which any host marching cubes pays first, and the numpy restatement
    (tests/recon_ref.py) of the same extraction on ONE CPU thread.
Timing: a pair of device events around every one of CALLS calls after WARMUP; min, median and max over the calls.  The count and
emit halves are also timed apart; the read of the two counts between them is not in either (it is in "extract_mesh_ms", a host
clock around the whole Python call, allocations included).  The restatement is timed once, and every device mesh is compared
with it.
Prints one JSON line (profiles/recon_sweep.json is one run of it).  Needs an MI355X.

Usage:  python tools/recon_sweep.py
"""
import ctypes as C
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

import recon_ref as rr  # noqa: E402
from helpers import load_mlp  # noqa: E402
from pixel_nerf_yolo_amd import conf as pconf  # noqa: E402
from pixel_nerf_yolo_amd import lib as plib  # noqa: E402
from pixel_nerf_yolo_amd import recon as precon  # noqa: E402
from pixel_nerf_yolo_amd import synth  # noqa: E402
from pixel_nerf_yolo_amd.model import make_model  # noqa: E402

WARMUP, CALLS = 3, 20


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
    t = np.array([a.elapsed_time(b) for a, b in pairs])
    return {"min": round(float(t.min()), 4), "median": round(float(np.median(t)), 4), "max": round(float(t.max()), 4)}


def host_ms(fn, calls=5):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(t)), 3)


def c1_net(dev):
    net = make_model(pconf.default_mv()["model"]).eval()
    load_mlp(net.mlp_coarse, 11, 512, 4)
    load_mlp(net.mlp_fine, 12, 512, 4)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.resnet34_state(14).items()}, strict=False)
    net = net.to(dev)
    src, _ = synth.scene_cameras(1)
    net.encode(torch.from_numpy(synth.images(15, 1, 64, 64))[None], torch.from_numpy(src)[None], torch.tensor(65.6),
               c=torch.tensor([[32.0, 32.0]]))
    return net


def mesh_case(name, vol, iso, with_restatement=True):
    """One volume: the two entry points on reused buffers, the Python call, the copy to the host, the restatement."""
    L, dev = plib.load(), vol.device
    dims = [int(v) for v in vol.shape]
    d = (C.c_int32 * 3)(*dims)
    ws = torch.empty(precon.workspace_bytes(dims), device=dev, dtype=torch.uint8)
    counts = torch.empty(2, device=dev, dtype=torch.int32)
    st = plib.stream_of(dev)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def count():
        plib.check(L.pny_mc_count(p(vol), d, iso, p(ws), p(counts), st))

    count()
    nv, nt = (int(v) for v in counts.cpu())
    verts, tris = torch.empty(nv, 3, device=dev), torch.empty(nt, 3, device=dev, dtype=torch.int32)

    def emit():
        plib.check(L.pny_mc_emit(p(vol), d, iso, p(ws), nv, nt, p(verts), p(tris), st))

    def both():
        count()
        emit()

    n = dims[0] * dims[1] * dims[2]
    n1 = -(-n // plib.MC_SCAN_TILE)
    row = {"case": name, "dims": dims, "iso": iso, "vertices": nv, "triangles": nt,
           "launches": {"count": 2 if n1 <= plib.MC_SCAN_TILE else 4, "emit": (nv > 0) + (nt > 0)},
           "count_ms": event_times_ms(count), "emit_ms": event_times_ms(emit), "count_plus_emit_ms": event_times_ms(both),
           "extract_mesh_ms_host_clock": host_ms(lambda: precon.extract_mesh(vol, iso)),
           "workspace_bytes": ws.numel()}
    pinned = torch.empty(vol.shape, dtype=torch.float32, pin_memory=True)
    row["copy_to_host_ms"] = event_times_ms(lambda: pinned.copy_(vol, non_blocking=True))
    if with_restatement:
        host = vol.cpu().numpy()
        t0 = time.perf_counter()
        rv, rt = rr.extract_mesh(host, iso)
        row["restatement_1_thread_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        row["equal_restatement"] = bool(rv.tobytes() == verts.cpu().numpy().tobytes() and rt.tobytes() == tris.cpu().numpy().tobytes())
    return row


def main():
    assert torch.cuda.is_available(), "tools/recon_sweep.py needs an MI355X"
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    out = {"tool": "recon_sweep", "device": torch.cuda.get_device_name(0), "calls": CALLS, "warmup": WARMUP, "cases": []}
    net = c1_net(dev)
    reso = [128, 128, 128]
    vol = precon.sigma_grid(net, reso=reso)
    out["sigma_grid"] = {"model": "C1: 1 view 64 x 64, ResNet-34, coarse MLP", "reso": reso, "eval_batch_size": 100000,
                         "launches_grid_points": -(-128 ** 3 // 100000),
                         "ms": event_times_ms(lambda: precon.sigma_grid(net, reso=reso), calls=5, warmup=1),
                         "sigma_min": float(vol.min()), "sigma_max": float(vol.max())}
    iso = float(vol.median())
    while bool((vol == iso).any()):
        iso = float(np.nextafter(np.float32(iso), np.float32(np.inf))) + 1e-4 * abs(iso)
        iso = float(np.float32(iso))
    out["cases"].append(mesh_case("C1 model volume 128^3 at its median sigma", vol, iso))
    for n in (128, 256):
        f = rr.ball_field((n, n, n), centre=np.array([0.07, -0.03, 0.05]), radius=0.6)
        out["cases"].append(mesh_case("ball %d^3" % n, torch.from_numpy(f).to(dev), float(rr.avoid_iso(f, 0.0131))))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
