"""
The view-looped kernels at 5 to 16 source views per object (-m gpu), 16 being the ABI's limit (MAX_VIEWS, csrc/pny_common.h):
every MLP-side kernel loops over a.NS or decodes a view from its block index, and no other module runs more than 4 views per
object.  Cameras come from helpers.camera_ring, on which no two views coincide (synth.scene_cameras repeats after 9 views);
tests/test_cpu_many_views.py checks on the oracle alone that these inputs can tell a kernel that drops, repeats or swaps a
view from a correct one.  What can be wrong here and nowhere below 5 views: the 1 / NS scaling for NS that is no power of two,
the running sums of the view-mean order, the stash records' NS-sized strides, the latent gradient's grid and pair-of-tiles
decode, the fixed-point scale of the deterministic latent gradient, a grouped object's view base beyond entry 11 of the
camera array, and the 1 KiB of cameras in the kernel arguments.

  a. the no-grad routes (h2 on 64- and 32-sample tiles, h1, the fp32 kernel with and without projection) against orc.query
     in float64;
  b. the render backward against float64 autograd at 5 and 8 views (short rays: at 16 views no whole ray is relu-safe);
  c. grouped scenes of 2 x 8 and 3 x 5 views against one scene per object;
  d. the deterministic latent gradient at 16 views;
  e. the limit: 17 views raise, 2 x 9 views render per object.
The gradient sweep at these view counts is MANY_VIEW_CASES of tests/test_gpu_grad_shapes.py.  Every bar is one the project
already had at 4 views or fewer (averaging over more views does not enlarge the error); measured values: profiles/many_views.md.
"""
import numpy as np
import pytest
import torch

import pnyolo_oracle as orc
import test_gpu_grad_shapes as gs
from helpers import DEV, RTOL, camera_ring, clean_rays, compare_param_grads, dt, grad_check, load_mlp, maxabs, render_loss, scene_pair
from pixel_nerf_yolo_amd import conf as pconf
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd import synth
from pixel_nerf_yolo_amd.model import make_model
from pixel_nerf_yolo_amd.render import NeRFRenderer
from test_gpu_parity import TOL
from test_gpu_view_mean import D_OUT, H, L, LAT_HW, ROUTES, W, run

pytestmark = pytest.mark.gpu

F64 = torch.float64
VIEWS = (5, 7, 8, 11, 16)
# (n_blocks, combine_layer, views): (5, 3) and (2, 1) (last per-view block = block 0) at every view count; (6, 5), the LDS
# bias-table limit, at 16 views
QUERY_SHAPES = [(nb, cl, ns) for ns in VIEWS for nb, cl in ((5, 3), (2, 1))] + [(6, 5, 16)]
N_POINTS = (70, 200)           # ragged last tile on 64- and on 32-sample tiles; 200 = several tiles
QUERY_SEED = 6500
# the fp32 kernel on the same scenes: (name, projection)
F32_ROUTES = (("f32_projected", "on"), ("f32_reference_order", "off"))


# --------------------------------------------------------------------------- a. no-grad routes
def query_points(n=max(N_POINTS)):
    rs = np.random.RandomState(4343)
    xyz = rs.uniform(-0.3, 0.3, size=(n, 3)).astype(np.float32)
    vd = rs.standard_normal((n, 3)).astype(np.float32)
    vd /= np.linalg.norm(vd, axis=1, keepdims=True)
    return xyz, vd


def query_scene(ns, nb, cl, with_net=True):
    """The scene of a no-grad case: ns views on camera_ring, every view its own random 16 x 16 map (synth.latent)."""
    return scene_pair(ns, H, W, L, D_OUT, nb, cl, QUERY_SEED, lat_hw=LAT_HW, dtype=F64, with_net=with_net,
                      poses=camera_ring(ns)[0])


def build(monkeypatch, ns, nb, cl):
    monkeypatch.setenv("PNYOLO_PROJECTION", "on")
    monkeypatch.setenv("PNYOLO_MLP_PRECISION", "f16x2")
    monkeypatch.delenv("PNYOLO_GRID", raising=False)
    net, sc = query_scene(ns, nb, cl)
    return net.eval(), sc


def run_f32(net, route, xyz, vd):
    """One no-grad coarse query on the fp32 kernel, with the projected latent or in the reference's operation order."""
    name, proj = route
    net.set_matrix_precision("f32")
    net.set_latent_projection(proj)
    with torch.no_grad():
        out = net(dt(xyz)[None], coarse=True, viewdirs=dt(vd)[None])[0].clone()
    torch.cuda.synchronize()
    assert net.last_launch_precision() == "f32", name
    st = net.last_mlp_stats(full=True)
    assert bool(st["projected"]) == (proj == "on") and st["launches"] == 1, name
    net.set_latent_projection("on")
    return out


def all_routes(net, monkeypatch, xyz, vd):
    """{route name: (output, bar)} of one query on every route."""
    outs = {r[0]: (run(net, monkeypatch, r, xyz, vd), r[4]) for r in ROUTES}
    outs.update({r[0]: (run_f32(net, r, xyz, vd), TOL) for r in F32_ROUTES})
    return outs


@pytest.mark.parametrize("nb,cl,ns", QUERY_SHAPES)
def test_routes_against_fp64(monkeypatch, nb, cl, ns):
    net, sc = build(monkeypatch, ns, nb, cl)
    xyz, vd = query_points()
    with torch.no_grad():
        ref = orc.query(sc, xyz, vd, coarse=True)
    assert ref.dtype == F64 and bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 1e-2
    failed = []
    for n in N_POINTS:
        outs = all_routes(net, monkeypatch, xyz[:n], vd[:n])
        for name, (out, bar) in outs.items():
            err = float((out.cpu().to(F64) - ref[:n]).abs().max())
            print("MANY-VIEWS query (%d, %d) NS=%d n=%d %s: max |err| vs float64 %.3e (bar %.1e)" % (nb, cl, ns, n, name, err, bar))
            if not err < bar:
                failed.append((name, n, err, bar))
        assert torch.equal(outs["h2"][0], outs["h2s"][0]), n        # the same sums on 64- and on 32-sample tiles
    assert not failed, failed


@pytest.mark.parametrize("nb,cl", [(5, 3), (2, 1), (6, 5)])
def test_routes_repeat_and_one_workgroup_at_16_views(monkeypatch, nb, cl):
    """Runs repeat bit for bit, and PNYOLO_GRID=1 (one workgroup walks every tile, its slabs and view loop reused tile after
    tile) is bit-equal to the uncapped launch."""
    net, _ = build(monkeypatch, 16, nb, cl)
    xyz, vd = query_points(200)
    free = all_routes(net, monkeypatch, xyz, vd)
    again = all_routes(net, monkeypatch, xyz, vd)
    monkeypatch.setenv("PNYOLO_GRID", "1")
    capped = all_routes(net, monkeypatch, xyz, vd)
    for name in free:
        assert torch.equal(free[name][0], again[name][0]), name
        assert torch.equal(free[name][0], capped[name][0]), name
    assert not torch.equal(free["h2"][0], free["h1"][0])


# --------------------------------------------------------------------------- b. render backward
RENDER = dict(H=32, W=32, kc=8, kf=4, kfd=2, n=16, nb=5, cl=3, near=0.3, far=1.8, net_seed=700, ray_seed=9)
RENDER_VIEWS = (5, 8)
RENDER_LEGS = ("f32", "f16x2")        # the two legs whose relu margin is AMBIG = 1e-5 (fp32 forward)
_RENDER_REF = {}


def render_scene(ns, with_net=True, lat_grad=False):
    c = RENDER
    return scene_pair(ns, c["H"], c["W"], 512, 4, c["nb"], c["cl"], c["net_seed"], lat_grad=lat_grad, dtype=F64, with_net=with_net,
                      poses=camera_ring(ns)[0])


def render_rays(sc, ns):
    """(rays (n, 8), draws, gt (n, 3)): the first n relu-safe rays of the 32 x 32 target frame, in float64 on the oracle."""
    c = RENDER
    rs = np.random.RandomState(c["ray_seed"])
    nc = c["H"] * c["W"]
    rays = orc.gen_rays(camera_ring(ns)[1][None], c["W"], c["H"], 0.9 * c["W"], c["near"], c["far"])[0].reshape(-1, 8)
    kc, kf, kfd = c["kc"], c["kf"], c["kfd"]
    dr = dict(u_coarse=rs.rand(nc, kc).astype(np.float32), u_fine=rs.rand(nc, kf - kfd).astype(np.float32),
              u_fine2=rs.rand(nc, kf - kfd).astype(np.float32), g_depth=rs.randn(nc, kfd).astype(np.float32))
    keep = clean_rays(sc, rays, kc, kf, kfd, dr, c["n"], chunk=48, ambig=gs.AMBIG)      # (the search stops at ray 65 / 329)
    gt = torch.from_numpy(rs.uniform(0, 1, size=(c["n"], 3)).astype(np.float32))
    return rays[torch.from_numpy(keep)], {k: v[keep] for k, v in dr.items()}, gt


def render_reference(ns):
    """Rays and float64 gradients (both MLPs' parameters and the latent) of the case; the same for every leg."""
    if ns not in _RENDER_REF:
        c = RENDER
        _, sc = render_scene(ns, with_net=False, lat_grad=True)
        rays, dr, gt = render_rays(sc, ns)
        ref = orc.render(sc, rays, c["kc"], c["kf"], c["kfd"], dr["u_coarse"], dr["u_fine"], dr["u_fine2"], dr["g_depth"],
                         detach_fine_depth=False)
        assert ref["fine"]["rgb"].dtype == F64
        zd = ref["coarse"]["depth"].detach()[:, None] + torch.from_numpy(dr["g_depth"]).to(F64) * 0.01
        assert int(((zd > c["near"]) & (zd < c["far"])).sum()) > c["n"] * c["kfd"] // 2        # most depth samples are unclamped
        render_loss(ref, gt.to(F64), True).backward()
        assert float(sc.latent.grad.abs().max()) > 0
        _RENDER_REF[ns] = dict(sc=sc, rays=rays, dr=dr, gt=gt, fine_rgb=ref["fine"]["rgb"].detach(), lat=sc.latent.grad.clone())
    return _RENDER_REF[ns]


@pytest.mark.parametrize("legname", RENDER_LEGS)
@pytest.mark.parametrize("ns,lat_grad", [(5, False), (8, False), (5, True)])
def test_render_backward_vs_fp64(ns, lat_grad, legname, monkeypatch):
    """The trainer's loss with the depth terms through the renderer, depth samples attached (the reference's graph), as
    test_gpu_backward.py::test_render_backward_vs_oracle at 2 views: 16 rays x (8 + 4) samples."""
    c = RENDER
    leg = gs.set_leg(legname, monkeypatch)
    r = render_reference(ns)
    net, _ = render_scene(ns, lat_grad=lat_grad)
    ren = NeRFRenderer(n_coarse=c["kc"], n_fine=c["kf"], n_fine_depth=c["kfd"], white_bkgd=True).train()
    ren._detach_fine_depth = False
    ren.draws = r["dr"]
    out = ren(net, r["rays"][None].to(DEV), want_weights=True)
    assert out["fine"]["rgb"].requires_grad
    hip = {p: {k: v[0] for k, v in out[p].items()} for p in ("coarse", "fine")}
    render_loss(hip, r["gt"].to(DEV), True).backward()
    torch.cuda.synchronize()
    assert net.last_backward_precision() == leg["want"]
    e_rgb = float((out["fine"]["rgb"][0].detach().cpu().to(F64) - r["fine_rgb"]).abs().max())
    print("MANY-VIEWS render NS=%d %s lat_grad=%s: fine rgb max |err| %.2e" % (ns, legname, lat_grad, e_rgb))
    assert e_rgb < 1e-4
    worst = compare_param_grads(net, r["sc"])
    print("MANY-VIEWS render NS=%d %s lat_grad=%s: weight worst %.2e of the tensor's max" % (ns, legname, lat_grad, worst))
    if lat_grad:
        g = net.test_latent.grad
        assert g is not None and g.shape == r["lat"].shape
        print("MANY-VIEWS render NS=%d %s: latent worst %.2e of the tensor's max" % (ns, legname, grad_check("latent", g, r["lat"])))


# --------------------------------------------------------------------------- c. grouped scenes with long view lists
def rotated_ring(ns, degrees):
    """camera_ring(ns)'s source poses turned about the world's vertical axis (every camera still looks at the origin)."""
    a = np.deg2rad(degrees)
    rot = np.array([[np.cos(a), -np.sin(a), 0, 0], [np.sin(a), np.cos(a), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64)
    return np.stack([(rot @ p.astype(np.float64)).astype(np.float32) for p in camera_ring(ns)[0]])


@pytest.mark.parametrize("legname", ["f32", "f16x2", "f16x2_default"])
@pytest.mark.parametrize("SB,ns", [(2, 8), (3, 5)])
def test_grouped_long_view_lists_equal_per_object(SB, ns, legname, monkeypatch):
    """One grouped scene of SB x ns = 16 and 15 cameras (object 1 of 2 x 8 starts at entry 8, object 2 of 3 x 5 at entry 10)
    against one scene per object, held as test_gpu_backward.py::test_grouped_super_batch_equals_per_object holds the two
    forms: rendered outputs bit-equal, parameter and latent gradients equal to fp32 summation order.  16 rays x (8 + 4) samples
    per object: shares of 128 and 192 samples, whole tiles in both passes."""
    gs.set_leg(legname, monkeypatch)
    Hh, Ww, kc, kf, kfd, n = 32, 32, 8, 4, 2, 16
    assert (n * kc) % 64 == 0 and (n * (kc + kf)) % 64 == 0
    c = pconf.default_mv()
    rs = np.random.RandomState(50 + ns)
    lat = np.concatenate([synth.latent(1710 + i, ns, 512, Hh // 2, Ww // 2) for i in range(SB)])
    poses = np.stack([rotated_ring(ns, 7.0 * o) for o in range(SB)])
    focal = torch.from_numpy(rs.uniform(26.0, 31.0, size=(SB * ns, 2)).astype(np.float32))     # per view
    cc = torch.from_numpy(rs.uniform(14.0, 18.0, size=(SB, 2)).astype(np.float32))              # per object
    rays = torch.stack([orc.gen_rays(synth.pose_spherical(100.0 + 25 * i, -20.0, 1.3)[None], Ww, Hh, 29.0, 0.3, 1.8)[0]
                        .reshape(-1, 8)[torch.from_numpy(rs.choice(Hh * Ww, n, replace=False))] for i in range(SB)])
    dr = dict(u_coarse=rs.rand(SB * n, kc).astype(np.float32), u_fine=rs.rand(SB * n, kf - kfd).astype(np.float32),
              u_fine2=rs.rand(SB * n, kf - kfd).astype(np.float32), g_depth=rs.randn(SB * n, kfd).astype(np.float32))
    gt = torch.from_numpy(rs.uniform(0, 1, size=(SB, n, 3)).astype(np.float32)).to(DEV)

    def go(group):
        monkeypatch.setenv("PNYOLO_GROUP", "1" if group else "0")
        net = make_model(c["model"], stop_encoder_grad=True)
        load_mlp(net.mlp_coarse, 1701, 512, 4)
        load_mlp(net.mlp_fine, 1702, 512, 4)
        net = net.to(DEV).train()
        lt = torch.from_numpy(lat).to(DEV).requires_grad_()
        net.encode(torch.zeros(SB, ns, 3, Hh, Ww), torch.from_numpy(poses), focal, c=cc, latent=lt)
        assert (net._group_scene() is not None) == group
        ren = NeRFRenderer(n_coarse=kc, n_fine=kf, n_fine_depth=kfd, white_bkgd=True).train()
        ren.draws = dr
        out = ren(net, rays.to(DEV), want_weights=True)
        (torch.nn.functional.mse_loss(out["coarse"]["rgb"], gt) + torch.nn.functional.mse_loss(out["fine"]["rgb"], gt)
         + 0.1 * out["fine"]["depth"].mean()).backward()
        torch.cuda.synchronize()
        assert net._last_call_group == group
        grads = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
        grads["latent"] = lt.grad.clone()
        return {q + "." + k: v.detach().clone() for q in ("coarse", "fine") for k, v in out[q].items()}, grads

    out_g, grad_g = go(True)
    out_s, grad_s = go(False)
    for k in out_s:
        assert bool(torch.isfinite(out_s[k]).all()) and torch.equal(out_g[k], out_s[k]), k
    assert len(grad_g) == len(grad_s) >= 61
    assert grad_s["latent"].shape == (SB * ns, 512, Hh // 2, Ww // 2)
    for v in range(SB * ns):        # every view of every object takes a gradient
        assert float(grad_s["latent"][v].abs().max()) > 0, v
    for k in grad_s:
        scale = float(grad_s[k].abs().max())
        assert float((grad_g[k] - grad_s[k]).abs().max()) <= 2e-6 * max(scale, 1e-20), k


# --------------------------------------------------------------------------- d. deterministic latent gradient
DET_CASE = "5-3_ns16_L512_16x16_2tiles_inside"


@pytest.mark.parametrize("legname", ["f32", "f16x2_default"])
def test_deterministic_latent_gradient_at_16_views(legname, monkeypatch):
    """The fixed-point sums of the deterministic latent gradient, whose term count grows with the views: bit-identical between
    two backwards from identical state, and within RTOL of float64."""
    assert next(iter(gs.MANY_VIEW_CASES)) == DET_CASE and gs.MANY_VIEW_CASES[DET_CASE]["ns"] == 16
    case = gs.MANY_VIEW_CASES[DET_CASE]
    leg = gs.set_leg(legname, monkeypatch)
    r = gs.reference(DET_CASE, case, leg["ambig"])
    net, _ = scene_pair(case["ns"], gs.H, gs.W, case["L"], 4, case["nb"], case["cl"], r["seed"], lat_hw=case["hw"], lat_grad=True,
                        poses=gs.poses_of(case))
    net.set_deterministic(True)
    got = []
    for _ in range(2):
        net.test_latent.grad = None
        for p in net.parameters():
            p.grad = None
        out = net(dt(r["xyz"])[None], coarse=True, viewdirs=dt(r["vd"])[None])
        (out[0] * dt(r["G"])).sum().backward()
        torch.cuda.synchronize()
        assert net.last_latent_grad_deterministic()
        got.append((net.test_latent.grad.clone(), {k: p.grad.clone() for k, p in net.mlp_coarse.named_parameters()}))
    assert torch.equal(got[0][0], got[1][0])
    assert all(torch.equal(got[0][1][k], got[1][1][k]) for k in got[0][1])
    assert float(r["lat"].abs().max()) > 0
    for v in range(case["ns"]):
        assert float(r["lat"][v].abs().max()) > 0, v
    ratio = grad_check("latent", got[0][0], r["lat"], RTOL)
    print("MANY-VIEWS deterministic latent gradient NS=16 %s: worst %.2e of the tensor's max" % (legname, ratio))


# --------------------------------------------------------------------------- e. the limit
def test_17_views_raise():
    net = make_model(pconf.default_mv()["model"]).to(DEV).eval()
    ns = 17
    poses = np.stack([synth.pose_spherical(20.0 * i, -20.0, 1.3) for i in range(ns)])
    lat = torch.from_numpy(synth.latent(1, ns, 512, 16, 16))
    with pytest.raises(plib.PnyError, match=r"ns out of range \[1,16\]"):
        net.encode(torch.zeros(1, ns, 3, 32, 32), torch.from_numpy(poses)[None], torch.tensor(28.8), latent=lat)
    # the handle is still usable: 16 views are accepted
    net.encode(torch.zeros(1, 16, 3, 32, 32), torch.from_numpy(poses[:16])[None], torch.tensor(28.8), latent=lat[:16])
    xyz, vd = query_points(70)
    with torch.no_grad():
        out = net(dt(xyz)[None], coarse=True, viewdirs=dt(vd)[None])
    assert bool(torch.isfinite(out).all())


def test_2x9_views_render_per_object(monkeypatch):
    """SB x NS = 18 views do not fit one grouped scene: the training encode leaves the grouped handle empty and the render and
    its backward run per object."""
    for var in ("PNYOLO_GROUP", "PNYOLO_MLP_PRECISION", "PNYOLO_BWD_PRECISION"):
        monkeypatch.delenv(var, raising=False)
    SB, ns, Hh, Ww, kc, kf, kfd, n = 2, 9, 32, 32, 8, 4, 2, 16
    net = make_model(pconf.default_mv()["model"], stop_encoder_grad=True)
    load_mlp(net.mlp_coarse, 1801, 512, 4)
    load_mlp(net.mlp_fine, 1802, 512, 4)
    net = net.to(DEV).train()
    rs = np.random.RandomState(18)
    lat = torch.from_numpy(np.concatenate([synth.latent(1810 + i, ns, 512, 16, 16) for i in range(SB)])).to(DEV).requires_grad_()
    poses = np.stack([rotated_ring(ns, 7.0 * o) for o in range(SB)])
    net.encode(torch.zeros(SB, ns, 3, Hh, Ww), torch.from_numpy(poses), torch.tensor(28.8), latent=lat)
    assert net._group_scene() is None
    rays = torch.stack([orc.gen_rays(synth.pose_spherical(100.0 + 25 * i, -20.0, 1.3)[None], Ww, Hh, 28.8, 0.3, 1.8)[0]
                        .reshape(-1, 8)[torch.from_numpy(rs.choice(Hh * Ww, n, replace=False))] for i in range(SB)])
    ren = NeRFRenderer(n_coarse=kc, n_fine=kf, n_fine_depth=kfd, white_bkgd=True).train()
    dr = dict(u_coarse=rs.rand(SB * n, kc).astype(np.float32), u_fine=rs.rand(SB * n, kf - kfd).astype(np.float32),
              u_fine2=rs.rand(SB * n, kf - kfd).astype(np.float32), g_depth=rs.randn(SB * n, kfd).astype(np.float32))
    ren.draws = dr
    out = ren(net, rays.to(DEV), want_weights=True)
    assert not net._last_call_group and out["fine"]["rgb"].shape == (SB, n, 3)
    (out["coarse"]["rgb"].square().mean() + out["fine"]["rgb"].square().mean()).backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out["fine"]["rgb"]).all())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.mlp_coarse.parameters())
    assert lat.grad is not None and all(float(lat.grad[v].abs().max()) > 0 for v in range(SB * ns))
    # each object against its own single scene of 9 views: the same tiles through the same kernels
    for o in range(SB):
        one = make_model(pconf.default_mv()["model"], stop_encoder_grad=True)
        load_mlp(one.mlp_coarse, 1801, 512, 4)
        load_mlp(one.mlp_fine, 1802, 512, 4)
        one = one.to(DEV).train()
        one.encode(torch.zeros(1, ns, 3, Hh, Ww), torch.from_numpy(poses[o])[None], torch.tensor(28.8),
                   latent=lat.detach()[o * ns:(o + 1) * ns])
        ren1 = NeRFRenderer(n_coarse=kc, n_fine=kf, n_fine_depth=kfd, white_bkgd=True).train()
        ren1.draws = {k: v[o * n:(o + 1) * n] for k, v in dr.items()}
        out1 = ren1(one, rays[o:o + 1].to(DEV), want_weights=True)
        assert maxabs(out1["fine"]["rgb"][0], out["fine"]["rgb"][o]) == 0.0, o
