"""
The sample geometry at its edges on every no-grad route (-m gpu): world -> camera, the perspective divide with the mode's sign,
grid_sample coordinates, tap validity, behind-camera culling (csrc/mlp_core.h camera_point / pixel_coords / pixel_taps).

The scene is test_gpu_dispatch.tiny_net's (2 views, 32 x 32 images, a 4 x 4 latent, 2 blocks, combine_layer 1, L = 256); the 128
query points fill a box wide enough that, per view, a point has all four bilinear taps inside the latent map, one to three of
them, or none (test_gpu_dispatch.query's +-0.3 box keeps all four inside for every point).  The reference is the oracle in
float64 on the same weights and latent.  Points with a pixel coordinate within 1e-3 of an integer in [-1, Wl] are dropped:
fp32 and fp64 may floor differently there, and the output is discontinuous at an out-of-range tap's border.
"""
import numpy as np
import pytest
import torch

import pnyolo_oracle as orc
from helpers import DEV, scene_pair
from pixel_nerf_yolo_amd import synth
from test_gpu_dispatch import H, HL, W, WL, reported, tiny_net
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

F64 = torch.float64
SEED, L, NS, NB, CL = 5100, 256, 2, 2, 1      # tiny_net's defaults, spelled out for the oracle side
N, BOX, NEAR_INT = 128, 0.8, 1e-3
MAX_DROPPED = N * 5 // 100                    # at most 5 % of the points
MIN_CLASS = 16
# single-plane f16 (PNY_PRECISION_F16): relative to max(1, max |ref|) like TOL; twice the one measurement on the MI355X
# (test_gpu_f16.py's convention for its single-plane bars), taken on the build before the geometry moved into shared helpers
F16_TOL = 1.1e-3                              # measured 5.48e-4


def points(box=BOX):
    rs = np.random.RandomState(77)
    xyz = rs.uniform(-box, box, (N, 3)).astype(np.float32)
    vd = rs.standard_normal((N, 3)).astype(np.float32)
    return xyz, vd / np.linalg.norm(vd, axis=1, keepdims=True)


def pixel_coords(sc, xyz):
    """(ix, iy, z) per view, each (ns, n), in float64: oracle.query's projection and encoder.py:97-98's unnormalisation."""
    w2c = sc.w2c.to(F64)
    xc = torch.matmul(w2c[:, None, :, :3], torch.from_numpy(xyz).to(F64)[None, :, :, None])[..., 0] + w2c[:, None, :, 3]
    uv = (xc[..., :2] if sc.yolo else -xc[..., :2]) / xc[..., 2:]
    uv = uv * sc.focal.to(F64).expand(sc.ns, 2)[:, None] + sc.c.to(F64).expand(sc.ns, 2)[:, None]
    ls = torch.tensor([WL, HL], dtype=F64)
    g = uv * (ls / (ls - 1) * 2.0 / torch.tensor([W, H], dtype=F64)) - 1.0
    return ((g[..., 0] + 1) / 2 * (WL - 1)).numpy(), ((g[..., 1] + 1) / 2 * (HL - 1)).numpy(), xc[..., 2].numpy()


def select(sc, xyz):
    """keep (n,) bool, and per point whether SOME view sees it with 4 / 1..3 / 0 valid taps, and whether some view has z >= 0."""
    ix, iy, z = pixel_coords(sc, xyz)
    near = np.zeros(ix.shape, bool)
    for k in range(-1, WL + 1):
        near |= (np.abs(ix - k) < NEAR_INT) | (np.abs(iy - k) < NEAR_INT)
    x0, y0 = np.floor(ix), np.floor(iy)
    nvalid = sum(((x >= 0) & (x <= WL - 1) & (y >= 0) & (y <= HL - 1)).astype(int)
                 for x, y in ((x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1)))
    cls = dict(full=(nvalid == 4).any(0), partial=((nvalid >= 1) & (nvalid <= 3)).any(0), none=(nvalid == 0).any(0),
               behind=(z >= 0).any(0))
    return ~near.any(0), cls


def check_selection(keep, cls, classes):
    counts = {k: int((cls[k] & keep).sum()) for k in cls}
    print("dropped %d of %d; points by class (some view): %s" % (int((~keep).sum()), keep.size, counts))
    assert int((~keep).sum()) <= MAX_DROPPED
    for k in classes:
        assert counts[k] >= MIN_CLASS, (k, counts)


def rel_err(out, ref, keep):
    assert out.shape == ref.shape and bool(torch.isfinite(out).all())
    err = (out.double().cpu() - ref).abs()[torch.from_numpy(keep)]
    return float(err.max()) / max(1.0, float(ref.abs().max()))


@pytest.fixture(scope="module")
def nerf_ref():
    """(xyz, vd, keep, float64 reference (n, 4)) of tiny_net's scene, computed once."""
    mc = synth.mlp_state(SEED, d_latent=L, n_blocks=NB, combine_layer=CL)
    poses, _ = synth.scene_cameras(NS)
    sc = orc.Scene(mc, None, synth.latent(SEED + 7, NS, L, HL, WL), poses, torch.tensor(0.9 * W), None, W, H,
                   n_blocks=NB, combine_layer=CL, dtype=F64)
    xyz, vd = points()
    keep, cls = select(sc, xyz)
    check_selection(keep, cls, ("full", "partial", "none"))
    with torch.no_grad():
        ref = orc.query(sc, torch.from_numpy(xyz), torch.from_numpy(vd), coarse=True)
    assert ref.dtype == F64
    return xyz, vd, keep, ref


# route: (precision, projection, PNYOLO_H2_SPLIT, reported (kernel, projected), bar)
ROUTES = {
    "f32_direct": ("f32", "off", None, ("f32", False), TOL),
    "f32_projected": ("f32", "on", None, ("f32", True), TOL),
    "f16x2_tile64": ("f16x2", "on", "0", ("f16x2", True), TOL),
    "f16x2_tile32": ("f16x2", "on", "1", ("f16x2", True), TOL),
    "f16": ("f16", "on", None, ("f16", True), F16_TOL),
}


def run(net, xyz, vd):
    with torch.no_grad():
        out = net(torch.from_numpy(xyz)[None].to(DEV), coarse=True, viewdirs=torch.from_numpy(vd)[None].to(DEV))
    torch.cuda.synchronize()
    return out[0]


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_nerf_tap_edges(route, nerf_ref, monkeypatch):
    prec, proj, split, want, tol = ROUTES[route]
    xyz, vd, keep, ref = nerf_ref
    if split is not None:
        monkeypatch.setenv("PNYOLO_H2_SPLIT", split)
    net, _ = tiny_net(L, NS, NB, CL, prec=prec, proj=proj, seed=SEED)
    out = run(net, xyz, vd)
    assert reported(net) == want
    err = rel_err(out, ref, keep)
    print("%s: max |err| / max(1, max |ref|) = %.3e (bar %.1e)" % (route, err, tol))
    assert err < tol


# YOLO mode keeps the latent at z < 0 only (models.py:224,254-264).  scene_pair's two extrinsics conventions put the whole box
# in front of (yolo_flip=False: z < 0, taps at work) or behind (yolo_flip=True: z >= 0, every latent zeroed) both cameras.
# Its cameras stand at radius 4 with a focal length of 40 / 44 pixels: the +-0.8 box projects inside the map for all but 11
# points, so the box is twice as wide here (the same draws scaled; |z| stays above 2) -- 68 / 74 / 27 points with four, some
# and no valid taps in some view.
YOLO_L, YOLO_DOUT, YOLO_BOX = 1792, 21, 1.6
YOLO_ROUTES = {"f32_direct": ("f32", "off", ("f32", False)), "f16x2": ("f16x2", "on", ("f16x2", True))}


@pytest.fixture(scope="module", params=[False, True], ids=["z_negative", "z_positive"])
def yolo_case(request):
    flip = request.param
    net, sc = scene_pair(NS, H, W, YOLO_L, YOLO_DOUT, NB, CL, 5200, yolo=True, lat_hw=(HL, WL), dtype=F64, yolo_flip=flip)
    net = net.eval()
    xyz, vd = points(YOLO_BOX)
    keep, cls = select(sc, xyz)
    check_selection(keep, cls, ("full", "partial", "none") + (("behind",) if flip else ()))
    if not flip:
        assert not (cls["behind"] & keep).any()
    with torch.no_grad():
        ref = orc.query(sc, torch.from_numpy(xyz), torch.from_numpy(vd), coarse=True).detach()
    return net, xyz, vd, keep, ref


@pytest.mark.parametrize("route", sorted(YOLO_ROUTES))
def test_yolo_tap_edges_and_cull(route, yolo_case):
    prec, proj, want = YOLO_ROUTES[route]
    net, xyz, vd, keep, ref = yolo_case
    net.set_matrix_precision(prec)
    net.set_latent_projection(proj)
    out = run(net, xyz, vd)
    assert reported(net) == want
    err = rel_err(out, ref, keep)
    print("yolo %s: max |err| / max(1, max |ref|) = %.3e (bar %.1e)" % (route, err, TOL))
    assert err < TOL
