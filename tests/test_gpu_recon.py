"""
The mesh extraction on the MI355X (pixel_nerf_yolo_amd.recon, csrc/recon.hip) against its numpy restatement (tests/recon_ref.py,
itself held to closed forms by tests/test_cpu_recon.py):

  * grid points written in slabs: coordinates bit-equal to util.gen_grid's, directions within 2 ulp of the fp32 restatement (one
    correctly rounded square root and one division each; the observed maximum is printed), the origin's direction exactly 0;
  * meshes -- counts, int32 triangles, fp32 vertices -- bit-equal to the restatement's: the analytic fields, all 256 one-cell
    volumes, thin and random volumes, a NaN sample, empty meshes, and a ball in (80, 128, 128): 1 310 720 points are more than
    SCAN_TILE * SCAN_TILE = 1024 * 1024, so the tile sums are themselves scanned in two levels (the deepest the library has:
    3 X Y Z < 2^31 leaves at most 683 tiles of sums);
  * identical bits from run to run, also after another shape used the same workspace;
  * end to end: a synthetic model's sigma volume bit-equal to net.forward on the same slabs, and marching_cubes() equal to
    extract_mesh() of that volume scaled as the reference scales.
"""
import warnings

import numpy as np
import pytest
import torch

import recon_ref as rr
from helpers import DEV, load_mlp
from pixel_nerf_yolo_amd import conf as pconf
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd import recon as precon
from pixel_nerf_yolo_amd import synth
from pixel_nerf_yolo_amd.model import make_model

pytestmark = pytest.mark.gpu

SCAN_TILE = 1024        # csrc/pny_recon.h MC_SCAN_TILE: points (and tile sums) one workgroup scans


def on_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_mesh(field, iso, what="", workspace=None):
    """The device mesh of `field` against the restatement's, bit for bit; returns the restated (vertices, triangles)."""
    iso = rr.avoid_iso(field, iso)
    v, t = precon.extract_mesh(on_dev(field), float(iso), workspace=workspace)
    rv, rt = rr.extract_mesh(field, iso)
    assert v.dtype == torch.float32 and t.dtype == torch.int32 and v.device.type == "cuda" and t.device.type == "cuda"
    assert tuple(v.shape) == rv.shape and tuple(t.shape) == rt.shape, (what, tuple(v.shape), rv.shape, tuple(t.shape), rt.shape)
    hv, ht = v.cpu().numpy(), t.cpu().numpy()
    assert same_bits(ht, rt), what
    if not same_bits(hv, rv):
        ulp = np.abs(hv.view(np.int32).astype(np.int64) - rv.view(np.int32).astype(np.int64)).max()
        raise AssertionError("%s: vertices differ from the restatement by up to %d ulp" % (what, ulp))
    return rv, rt


# --------------------------------------------------------------------------- grid points
def test_grid_points_in_slabs_against_gen_grid():
    c1, c2, reso = (-1, -0.5, 0.25), (1, 2, 0.75), (5, 4, 3)
    xyz, dirs = [], []
    for i0 in range(0, 60, 7):                       # 7 does not divide 60
        a, b = precon.grid_points(c1, c2, reso, i0, min(i0 + 7, 60), device=DEV)
        xyz.append(a.cpu().numpy()), dirs.append(b.cpu().numpy())
    xyz, dirs = np.concatenate(xyz), np.concatenate(dirs)
    grid = rr.gen_grid(c1, c2, reso)
    assert same_bits(xyz, grid)
    ref = rr.view_dirs(grid)
    ulp = int(np.abs(dirs.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64)).max())
    print("view directions: at most %d ulp from the fp32 restatement" % ulp)
    assert ulp <= 2
    whole = precon.grid_points(c1, c2, reso, device=DEV)
    assert same_bits(whole[0].cpu().numpy(), xyz) and same_bits(whole[1].cpu().numpy(), dirs)


def test_grid_point_at_the_origin_has_direction_zero():
    xyz, dirs = (t.cpu().numpy() for t in precon.grid_points((-1, -1, -1), (1, 1, 1), (3, 3, 3), device=DEV))
    assert (xyz[13] == 0).all() and (dirs[13] == 0).all()
    assert np.isfinite(dirs).all() and np.isfinite(xyz).all()
    others = np.delete(np.arange(27), 13)
    assert np.abs(np.linalg.norm(dirs[others].astype(np.float64), axis=1) - 1.0).max() < 1e-6


# --------------------------------------------------------------------------- meshes
@pytest.mark.parametrize("name", sorted(rr.ANALYTIC))
def test_analytic_fields_against_the_restatement(name):
    field, iso, chi = rr.ANALYTIC[name]
    f = field()
    assert f.size > SCAN_TILE                        # more than one scan tile
    v, t = check_mesh(f, iso, name)
    assert rr.is_closed_manifold(t) and rr.euler_characteristic(len(v), t) == chi and rr.signed_volume(v, t) > 0


def test_all_256_single_cell_cases():
    counts = rr.table()[2]
    ws = torch.empty(precon.workspace_bytes((2, 2, 2)), device=DEV, dtype=torch.uint8)
    for case in range(256):
        _, t = check_mesh(rr.single_cell(case), 0.25, "case %d" % case, workspace=ws)
        assert len(t) == counts[case]


@pytest.mark.parametrize("dims", [(2, 5, 3), (65, 3, 2)])
def test_thin_volumes(dims):
    f = np.random.RandomState(sum(dims)).randn(*dims).astype(np.float32)
    _, t = check_mesh(f, 0.05, str(dims))
    assert len(t) > 0


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_random_volumes(seed):
    f = np.random.RandomState(seed).randn(9, 8, 7).astype(np.float32)
    _, t = check_mesh(f, 0.1, "seed %d" % seed)
    assert len(t) > 0


def test_a_nan_sample_counts_as_outside():
    """The NaN's neighbours are outside too, so no cut edge touches it: the mesh is that of the volume with the NaN replaced by a
    low value, and every coordinate is finite."""
    f = np.random.RandomState(21).randn(6, 7, 5).astype(np.float32)
    for p in ((0, 0, 0), (3, 4, 2)):
        for axis in range(3):
            for step in (-1, 1):
                q = list(p)
                q[axis] += step
                if 0 <= q[axis] < f.shape[axis]:
                    f[tuple(q)] = -2.0
    g = f.copy()
    f[0, 0, 0] = f[3, 4, 2] = np.nan
    g[0, 0, 0] = g[3, 4, 2] = -2.0
    v, t = check_mesh(f, 0.1, "nan")
    gv, gt = rr.extract_mesh(g, 0.1)
    assert np.isfinite(v).all() and same_bits(v, gv) and same_bits(t, gt) and len(t) > 0


def test_volumes_without_a_surface_give_an_empty_mesh():
    f = np.random.RandomState(5).rand(6, 5, 4).astype(np.float32)
    for iso in (2.0, -1.0):                          # entirely below, entirely above
        v, t = precon.extract_mesh(on_dev(f), iso)
        assert tuple(v.shape) == (0, 3) and tuple(t.shape) == (0, 3) and v.dtype == torch.float32 and t.dtype == torch.int32
    torch.cuda.synchronize()


def test_a_volume_that_crosses_both_levels_of_the_scan():
    """(80, 128, 128) rather than the smallest such shape: point 1024 * 1024, where the second tile of tile sums begins, lies at
    x index 64 of 80, inside the ball, so vertices and triangles on both sides of it get their offsets from both levels."""
    dims = (80, 128, 128)
    assert dims[0] * dims[1] * dims[2] > SCAN_TILE * SCAN_TILE and plib.MC_SCAN_TILE == SCAN_TILE
    f = rr.ball_field(dims, centre=np.array([0.11, -0.06, 0.2]), radius=0.7)
    v, t = check_mesh(f, 0.0131, "ball in %s" % (dims,))
    print("ball in %s: %d vertices, %d triangles" % (dims, len(v), len(t)))
    assert rr.is_closed_manifold(t) and rr.euler_characteristic(len(v), t) == 2 and rr.signed_volume(v, t) > 0
    owners = np.floor(v.astype(np.float64)) @ np.array([dims[1] * dims[2], dims[2], 1.0])
    beyond = int((owners >= SCAN_TILE * SCAN_TILE).sum())
    print("vertices owned beyond point 1024 * 1024: %d" % beyond)
    assert 1000 < beyond < len(v) - 1000


def test_bits_are_the_same_from_run_to_run_and_after_another_shape_used_the_workspace():
    a = rr.torus_field()
    b = np.random.RandomState(31).randn(40, 9, 11).astype(np.float32)
    ws = torch.empty(max(precon.workspace_bytes(a.shape), precon.workspace_bytes(b.shape)), device=DEV, dtype=torch.uint8)
    ws.fill_(0xA5)
    da, db = on_dev(a), on_dev(b)
    first = [x.cpu().numpy() for x in precon.extract_mesh(da, 0.011, workspace=ws)]
    again = [x.cpu().numpy() for x in precon.extract_mesh(da, 0.011, workspace=ws)]
    other = [x.cpu().numpy() for x in precon.extract_mesh(db, 0.1, workspace=ws)]
    third = [x.cpu().numpy() for x in precon.extract_mesh(da, 0.011, workspace=ws)]
    fresh = [x.cpu().numpy() for x in precon.extract_mesh(da, 0.011)]
    for got in (again, third, fresh):
        assert same_bits(got[0], first[0]) and same_bits(got[1], first[1])
    rv, rt = rr.extract_mesh(b, 0.1)
    assert same_bits(other[0], rv) and same_bits(other[1], rt)


# --------------------------------------------------------------------------- end to end
def test_end_to_end_sigma_grid_and_marching_cubes(golden):
    g = golden("enc_render")
    seed, ns, H, W = int(g["seed"]), int(g["NS"]), int(g["H"]), int(g["W"])
    net = make_model(pconf.default_mv()["model"]).eval()
    load_mlp(net.mlp_coarse, seed * 10 + 1, 512, 4)
    load_mlp(net.mlp_fine, seed * 10 + 2, 512, 4)
    esd = synth.resnet34_state(seed * 10 + 4, residual_gain=float(g["residual_gain"]))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in esd.items()}, strict=False)
    net = net.to(DEV)
    images, poses = torch.from_numpy(synth.images(seed * 10 + 5, ns, H, W)), torch.from_numpy(g["src_poses"])
    focal, c = torch.tensor(float(g["focal"])), torch.from_numpy(g["c"])[None]
    net.encode(images[None], poses[None], focal, c=c)
    c1, c2, reso, bs = [-1, -1, -1], [1, 1, 1], [16, 16, 16], 1000           # 1000 does not divide 4096
    vol = precon.sigma_grid(net, c1, c2, reso, eval_batch_size=bs)
    assert tuple(vol.shape) == (16, 16, 16) and vol.dtype == torch.float32 and vol.device.type == "cuda"

    grid = rr.gen_grid(c1, c2, reso)
    xyz, dirs = on_dev(grid), on_dev(rr.view_dirs(grid))
    with torch.no_grad():
        ref = torch.cat([net(xyz[None, i:i + bs], coarse=True, viewdirs=dirs[None, i:i + bs])[0, :, 3] for i in range(0, 4096, bs)])
    host = vol.cpu().numpy()
    assert same_bits(host.reshape(-1), ref.cpu().numpy())
    lo, hi = float(host.min()), float(host.max())
    print("sigma volume: %.4f .. %.4f" % (lo, hi))
    assert np.isfinite(host).all() and hi > lo
    levels = np.unique(host)
    k = int(0.7 * len(levels))
    iso = float(np.float32(0.5 * (float(levels[k]) + float(levels[k + 1]))))
    while (host == np.float32(iso)).any():
        k += 1
        iso = float(np.float32(0.5 * (float(levels[k]) + float(levels[k + 1]))))
    assert lo < iso < hi

    v, t = precon.extract_mesh(vol, iso)
    assert len(t) > 0
    expect = v.cpu().numpy().astype(np.float64)
    expect *= (np.array(c2) - np.array(c1)) / np.array(reso)                 # recon.py:73-78: by reso, not reso - 1
    expect = expect + np.array(c1)
    for training in (False, True):
        net.train(training)
        with pytest.warns(UserWarning, match="fake view dirs"):
            mv, mt = precon.marching_cubes(net, c1, c2, reso, isosurface=iso, eval_batch_size=bs)
        assert net.training is training
        assert isinstance(mv, np.ndarray) and mv.dtype == np.float64 and isinstance(mt, np.ndarray) and mt.dtype == np.int32
        assert same_bits(mv, expect) and same_bits(mt, t.cpu().numpy())
    net.eval()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tv, tt = precon.marching_cubes(net, c1, c2, reso, isosurface=iso, eval_batch_size=bs, return_tensors=True)
    assert tv.dtype == torch.float32 and tv.device.type == "cuda" and torch.equal(tt, t)
    assert np.abs(tv.cpu().numpy().astype(np.float64) - expect).max() < 1e-6    # |coordinate| <= 1, fp32 scale and shift

    with pytest.raises(ValueError, match="sigma_idx"):
        precon.sigma_grid(net, c1, c2, reso, sigma_idx=4)
    net.encode(torch.stack([images, images]), torch.stack([poses, poses]), focal, c=c)
    with pytest.raises(plib.PnyError, match="ONE encoded object"):
        precon.sigma_grid(net, c1, c2, reso, eval_batch_size=bs)
