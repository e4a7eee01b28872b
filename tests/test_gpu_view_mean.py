"""
The view-mean order of the no-grad f16 MLP kernels (-m gpu; csrc/mlp_h2.hip): the last per-view block's fc_1
runs once per sample, on the mean over views of relu(net + b_fc0), instead of once per view --
    mean_v(h_v + fc_1(R_v)) = mean_v(h_v) + fc_1(mean_v R_v).

Every case is a no-grad query under PNYOLO_PROJECTION=on, on each of the three routes that run this source: the split kernel
on 64-sample tiles (PNYOLO_H2_SPLIT=0), on 32-sample tiles (=1), and the single-plane f16 kernel.  The two split routes run
the view-mean order; the single-plane kernel shares the source, slabs and scratch but keeps the per-view order (mlp_h2.hip
header comment), and is held to the same properties.  References: the oracle in float64.  Bars: those of the routes' own
parity tests (TOL of test_gpu_parity.py, QUERY_TOL of test_gpu_f16.py); nothing new.  Latent 16 x 16, L = 512.
"""
import numpy as np
import pytest
import torch

import pnyolo_oracle as orc
from helpers import DEV, dt, maxabs, scene_pair
from pixel_nerf_yolo_amd import synth
from test_gpu_f16 import QUERY_TOL
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

F64 = torch.float64
H = W = 32
LAT_HW = (16, 16)
L, D_OUT, HID, D_IN = 512, 4, 512, 42
# (name, scene precision, PNYOLO_H2_SPLIT, reported kernel precision, bar, runs the view-mean order)
ROUTES = (("h2", "f16x2", "0", "f16x2", TOL, True), ("h2s", "f16x2", "1", "f16x2", TOL, True), ("h1", "f16", None, "f16", QUERY_TOL, False))
SHAPES = ((5, 3), (2, 1), (3, 2), (6, 5))     # (n_blocks, combine_layer): (2, 1) last per-view block = block 0; (6, 5) the LDS bias-table limit
VIEWS = (1, 2, 3, 4)
N_POINTS = (70, 200)                          # ragged last tile on 64- and on 32-sample tiles; 200 = several tiles


def points(n=max(N_POINTS)):
    rs = np.random.RandomState(4242)
    xyz = rs.uniform(-0.3, 0.3, size=(n, 3)).astype(np.float32)
    vd = rs.standard_normal((n, 3)).astype(np.float32)
    vd /= np.linalg.norm(vd, axis=1, keepdims=True)
    return xyz, vd


def build(monkeypatch, ns, nb, cl, seed=6100):
    monkeypatch.setenv("PNYOLO_PROJECTION", "on")
    monkeypatch.setenv("PNYOLO_MLP_PRECISION", "f16x2")
    monkeypatch.delenv("PNYOLO_GRID", raising=False)
    net, sc = scene_pair(ns, H, W, L, D_OUT, nb, cl, seed, lat_hw=LAT_HW, dtype=F64)
    return net.eval(), sc


def run(net, monkeypatch, route, xyz, vd):
    """One no-grad coarse query on `route`; asserts that the route ran."""
    name, prec, split, reported = route[:4]
    net.set_matrix_precision(prec)
    if split is None:
        monkeypatch.delenv("PNYOLO_H2_SPLIT", raising=False)
    else:
        monkeypatch.setenv("PNYOLO_H2_SPLIT", split)
    with torch.no_grad():
        out = net(dt(xyz)[None], coarse=True, viewdirs=dt(vd)[None])[0].clone()
    torch.cuda.synchronize()
    assert net.last_launch_precision() == reported, name
    st = net.last_mlp_stats(full=True)
    assert st["projected"] and st["launches"] == 1
    return out


_REF = {}


def reference(sc, key, xyz, vd):
    if key not in _REF:
        with torch.no_grad():
            _REF[key] = orc.query(sc, xyz, vd, coarse=True).to(F64)
    return _REF[key]


@pytest.mark.parametrize("ns", VIEWS)
@pytest.mark.parametrize("nb,cl", SHAPES)
def test_shape_sweep_against_fp64(monkeypatch, nb, cl, ns):
    net, sc = build(monkeypatch, ns, nb, cl)
    xyz, vd = points()
    ref = reference(sc, (nb, cl, ns), xyz, vd)
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 1e-2
    for route in ROUTES:
        for n in N_POINTS:
            out = run(net, monkeypatch, route, xyz[:n], vd[:n])
            err = float((out.cpu().to(F64) - ref[:n]).abs().max())
            print("view-mean (%d, %d) NS=%d n=%d %s: max |err| vs float64 %.3e (bar %.1e)" % (nb, cl, ns, n, route[0], err, route[4]))
            assert err < route[4], (route[0], n, err)


@pytest.mark.parametrize("nb,cl,ns", [(5, 3, 3), (2, 1, 2)])
def test_several_tiles_per_workgroup(monkeypatch, nb, cl, ns):
    """PNYOLO_GRID=1: one workgroup walks every tile, so both slabs are reused tile after tile; bit-equal to the uncapped launch."""
    net, _ = build(monkeypatch, ns, nb, cl)
    xyz, vd = points(200)
    for route in ROUTES:
        monkeypatch.delenv("PNYOLO_GRID", raising=False)
        free = run(net, monkeypatch, route, xyz, vd)
        monkeypatch.setenv("PNYOLO_GRID", "1")
        capped = run(net, monkeypatch, route, xyz, vd)
        assert torch.equal(free, capped), route[0]


@pytest.mark.parametrize("nb,cl", [(5, 3), (2, 1)])
def test_copies_of_one_view_equal_the_single_view(monkeypatch, nb, cl):
    """NS = 2 and NS = 4 views that are copies of one camera and one latent: the running sums are 2 x and 4 x one view's values
    (x + x, 2x + x rounded, and fl(3x) + x = 4x again: the rounding error of 3x is at most half an ulp of 4x, ties to the even
    mantissa of x) and the scaling is by 1/2 and 1/4 -- all exact --, so every route returns the NS = 1 scene's bits."""
    seed = 6300
    net, _ = build(monkeypatch, 1, nb, cl, seed)
    xyz, vd = points(200)
    one = {r[0]: run(net, monkeypatch, r, xyz, vd) for r in ROUTES}
    poses, _ = synth.scene_cameras(1)
    lat = torch.from_numpy(synth.latent(seed + 3, 1, L, *LAT_HW))
    for k in (2, 4):
        net.encode(torch.zeros(1, k, 3, H, W), torch.from_numpy(poses).repeat(k, 1, 1)[None], torch.tensor(0.9 * W),
                   c=torch.tensor([[W * 0.5, H * 0.5]]), latent=lat.repeat(k, 1, 1, 1))
        for r in ROUTES:
            out = run(net, monkeypatch, r, xyz, vd)
            assert torch.equal(out, one[r[0]]), (r[0], k, maxabs(out, one[r[0]]))


@pytest.mark.parametrize("nb,cl", [(2, 1), (5, 3)])
def test_shapes_identical_and_deterministic(monkeypatch, nb, cl):
    net, _ = build(monkeypatch, 3, nb, cl)
    xyz, vd = points(200)
    outs = {}
    for route in ROUTES:
        a = run(net, monkeypatch, route, xyz, vd)
        b = run(net, monkeypatch, route, xyz, vd)
        assert torch.equal(a, b), route[0]
        outs[route[0]] = a
    assert torch.equal(outs["h2"], outs["h2s"])
    assert not torch.equal(outs["h2"], outs["h1"])


def flops_per_point(ns, nb, cl, view_mean):
    """Executed GEMM FLOPs (2 per MAC, unpadded) of a projected forward: per view lin_in and the per-view blocks' fc_0 / fc_1,
    then the post-mean blocks and lin_out; in the view-mean order NS - 1 of the last per-view fc_1 GEMMs do not run."""
    nvb = min(cl, nb)
    per_view = D_IN * HID + 2 * nvb * HID * HID
    post = 2 * (nb - nvb) * HID * HID + HID * D_OUT
    return 2 * (ns * per_view + post) - (2 * (ns - 1) * HID * HID if view_mean else 0)


def test_flop_accounting(monkeypatch):
    assert flops_per_point(3, 5, 3, True) == 10618880 and flops_per_point(3, 5, 3, False) == 11667456
    xyz, vd = points(200)
    n = xyz.shape[0]
    net, _ = build(monkeypatch, 3, 5, 3)
    for route in ROUTES:
        run(net, monkeypatch, route, xyz, vd)
        assert net.last_mlp_stats(full=True)["flops"] == flops_per_point(3, 5, 3, route[5]) * n, route[0]
    net.set_matrix_precision("f32")               # an F32-pinned scene: the fp32 kernel, the per-view order
    with torch.no_grad():
        net(dt(xyz)[None], coarse=True, viewdirs=dt(vd)[None])
    assert net.last_launch_precision() == "f32"
    st = net.last_mlp_stats(full=True)
    assert st["projected"] and st["flops"] == flops_per_point(3, 5, 3, False) * n
    net1, _ = build(monkeypatch, 1, 5, 3)
    for route in ROUTES:
        run(net1, monkeypatch, route, xyz, vd)
        assert net1.last_mlp_stats(full=True)["flops"] == flops_per_point(1, 5, 3, False) * n, route[0]
