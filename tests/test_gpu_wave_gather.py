"""
The wave-owned block entry of the no-grad f16 MLP kernels (-m gpu; csrc/mlp_h2.hip h2wave_entry): a wave gathers
the projected channels of its own 64 (or 128) feature rows for every sample of the tile, 32 features x 32 samples at a time,
stages them in its own plane bytes and adds them to the accumulators there.  What can go wrong is a mapping: sample <-> lane
and pass, feature quad <-> lane, the staging column swizzle, the tap record a lane re-reads, the prefetched first piece.

Every case is a no-grad projected query on each of the three routes that run this source (test_gpu_view_mean.py ROUTES: the
split kernel on 64- and on 32-sample tiles, the single-plane f16 kernel), against the oracle in float64 at the routes' own bars
(TOL of test_gpu_parity.py, QUERY_TOL of test_gpu_f16.py); nothing new.  The latent maps are random per pixel and channel, and
every output depends on all 512 channels of h through lin_out, so a permuted sample, quad or tile is an O(1) error.
Image 32 x 32, L = 512.
"""
import numpy as np
import pytest
import torch

import pnyolo_oracle as orc
from helpers import scene_pair
from test_gpu_view_mean import ROUTES, run

pytestmark = pytest.mark.gpu

F64 = torch.float64
H = W = 32
L, D_OUT = 512, 4
SQUARE, NARROW = (16, 16), (16, 8)            # latent (rows, columns); NARROW: a row / column mix-up in the tap record shows
# ragged last tiles on 64- and on 32-sample tiles; pass groups of 8 samples partly (1, 7, 9, 33, 65, 70) or wholly clamped
N_POINTS = (1, 7, 8, 9, 31, 33, 64, 65, 70, 200)
# (n_blocks, combine_layer): (2, 1) block 0's entry only (fetched before lin_in; no piece is fetched underneath a GEMM);
# the others fetch the next block's first piece underneath fc_1, and the last per-view block has no successor
SHAPES = ((2, 1), (5, 3), (3, 2), (6, 5))
VIEWS = (1, 2, 3, 4)
N = max(N_POINTS)


def build(monkeypatch, ns, nb, cl, lat_hw=SQUARE, seed=7300):
    monkeypatch.setenv("PNYOLO_PROJECTION", "on")
    monkeypatch.setenv("PNYOLO_MLP_PRECISION", "f16x2")
    monkeypatch.delenv("PNYOLO_GRID", raising=False)
    net, sc = scene_pair(ns, H, W, L, D_OUT, nb, cl, seed, lat_hw=lat_hw, dtype=F64)
    return net.eval(), sc


def points(n=N, spread=0.3):
    rs = np.random.RandomState(4343)
    xyz = rs.uniform(-spread, spread, size=(n, 3)).astype(np.float32)
    vd = rs.standard_normal((n, 3)).astype(np.float32)
    vd /= np.linalg.norm(vd, axis=1, keepdims=True)
    return xyz, vd


_REF = {}


def reference(sc, key, xyz, vd):
    if key not in _REF:
        with torch.no_grad():
            _REF[key] = orc.query(sc, xyz, vd, coarse=True).to(F64)
    return _REF[key]


def check(net, sc, monkeypatch, key, xyz, vd, counts):
    ref = reference(sc, key, xyz, vd)
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 1e-2
    for route in ROUTES:
        for n in counts:
            out = run(net, monkeypatch, route, xyz[:n], vd[:n])
            err = float((out.cpu().to(F64) - ref[:n]).abs().max())
            print("wave gather %s n=%d %s: max |err| vs float64 %.3e (bar %.1e)" % (key, n, route[0], err, route[4]))
            assert err < route[4], (route[0], n, err)


def test_sample_lane_mapping_at_the_edges(monkeypatch):
    net, sc = build(monkeypatch, 3, 5, 3)
    xyz, vd = points()
    check(net, sc, monkeypatch, ("edges", 5, 3, 3), xyz, vd, N_POINTS)


@pytest.mark.parametrize("ns", VIEWS)
@pytest.mark.parametrize("nb,cl", SHAPES)
def test_every_feature_row_of_every_wave(monkeypatch, nb, cl, ns):
    net, sc = build(monkeypatch, ns, nb, cl)
    xyz, vd = points()
    check(net, sc, monkeypatch, ("rows", nb, cl, ns), xyz, vd, (N,))


# ---- taps ---------------------------------------------------------------------------------------------------------------
def cameras(sc):
    w2c = sc.w2c.to(F64)
    return w2c[:, :, :3], w2c[:, :, 3], sc.focal.to(F64).expand(sc.ns, 2), sc.c.to(F64).expand(sc.ns, 2)


def project(sc, xyz, lat_hw):
    """Latent-pixel coordinates (ix, iy), each (views, points), in float64: the oracle's projection (query, index_latent)."""
    R, t, foc, cc = cameras(sc)
    xc = torch.matmul(R[:, None], torch.from_numpy(xyz).to(F64)[None, :, :, None])[..., 0] + t[:, None]
    uv = -xc[:, :, :2] / xc[:, :, 2:] * foc[:, None] + cc[:, None]
    return uv[..., 0] * lat_hw[1] / W, uv[..., 1] * lat_hw[0] / H


def unproject(sc, v, ix, iy, lat_hw):
    """The world point that view v sees at latent pixel (ix, iy), at the camera depth of the world origin."""
    R, t, foc, cc = cameras(sc)
    zc = t[v, 2]
    u, w = ix * W / lat_hw[1], iy * H / lat_hw[0]
    xc = torch.stack((-(u - cc[v, 0]) / foc[v, 0] * zc, -(w - cc[v, 1]) / foc[v, 1] * zc, zc))
    return (R[v].t() @ (xc - t[v])).numpy().astype(np.float32)


def tap_points(sc, lat_hw):
    hl, wl = lat_hw
    xyz, vd = points()
    xyz[8:16] = xyz[8]                                    # 8 consecutive samples of one load on one pixel: identical lines
    xyz[19:27] = xyz[19]                                  # ... and across two loads
    ns = sc.ns
    xyz[32] = unproject(sc, 0, wl - 1.0, 3.3, lat_hw)           # exactly onto the last column
    xyz[33] = unproject(sc, 0, 2.7, hl - 1.0, lat_hw)           # ... the last row
    xyz[34] = unproject(sc, 1 % ns, wl - 1.0, hl - 1.0, lat_hw)   # ... the last pixel
    xyz[35] = unproject(sc, 2 % ns, 0.0, 0.0, lat_hw)           # ... the first
    for i in range(8):                                          # outside one view's map on each side
        xyz[40 + i] = unproject(sc, i % ns, -2.5, 1.0 + 1.7 * i, lat_hw)
        xyz[48 + i] = unproject(sc, i % ns, wl + 1.5, 1.0 + 1.7 * i, lat_hw)
        xyz[56 + i] = unproject(sc, i % ns, 0.4 + 0.9 * i, hl + 0.5, lat_hw)
        xyz[64 + i] = unproject(sc, i % ns, 0.4 + 0.9 * i, -1.5, lat_hw)
    return xyz, vd


def tap_census(sc, xyz, lat_hw):
    hl, wl = lat_hw
    ix, iy = project(sc, xyz, lat_hw)
    inside = (ix >= 0) & (ix <= wl - 1) & (iy >= 0) & (iy <= hl - 1)
    wholly_out = (ix <= -1) | (ix >= wl) | (iy <= -1) | (iy >= hl)
    return dict(mixed=int((inside.any(0) & wholly_out.any(0)).sum()), last_col=int(((ix - (wl - 1)).abs() < 1e-4).sum()),
                last_row=int(((iy - (hl - 1)).abs() < 1e-4).sum()))


def test_taps_outside_on_the_edge_and_on_one_pixel(monkeypatch):
    net, sc = build(monkeypatch, 3, 5, 3, lat_hw=NARROW)
    xyz, vd = tap_points(sc, NARROW)
    census = tap_census(sc, xyz, NARROW)
    print("wave gather taps:", census)
    assert census["mixed"] >= 8 and census["last_col"] >= 2 and census["last_row"] >= 2, census
    check(net, sc, monkeypatch, ("taps", 5, 3, 3), xyz, vd, (N,))


# ---- properties without a bar ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,cl,ns", [(5, 3, 3), (2, 1, 2)])
def test_shapes_agree_runs_repeat_and_batches_do_not_matter(monkeypatch, nb, cl, ns):
    net, sc = build(monkeypatch, ns, nb, cl, lat_hw=NARROW)
    xyz, vd = tap_points(sc, NARROW)
    outs = {}
    for route in ROUTES:
        a = run(net, monkeypatch, route, xyz, vd)
        b = run(net, monkeypatch, route, xyz, vd)
        assert torch.equal(a, b), route[0]
        for i in (0, 12, 33, 45, 63, 64, 199):           # a point queried alone = the same point inside the batch
            alone = run(net, monkeypatch, route, xyz[i:i + 1], vd[i:i + 1])
            assert torch.equal(alone[0], a[i]), (route[0], i)
        outs[route[0]] = a
    assert torch.equal(outs["h2"], outs["h2s"])
