"""
The model descriptions pny_model_create accepts, beyond the corner the rest of the suite runs in (-m gpu): the positional code
(num_freqs 0..9, any freq_factor; d_in = 6 + 6 * num_freqs), the output width (d_out 1..64), the latent width (any multiple of
128) and the block count (1..8).  One table, pairwise rather than a product; three bodies:
  a. the no-grad forward on every route against the oracle in float64;
  b. the query backward under the legs of test_gpu_grad_shapes.py against float64 autograd;
  c. the render backward with the depth samples attached (the one path through the depth kernel's own copy of the code
     derivative), and the YOLO renderer at one anchor.
Bars are the routes' and legs' existing ones, imported.  tests/test_cpu_model_desc.py checks the refusals at the ABI and, on the
oracle alone, the conditions on these inputs: enough relu-safe points, and that the float32 oracle is close enough to the
float64 one for the bars to be met by a correct float32 implementation.

Latent map 8 x 8, target frame 32 x 40, 130 query points (two 64-sample tiles and a ragged third; 65 where noted).
"""
import math
import time

import numpy as np
import pytest
import torch

import pnyolo_oracle as orc
import test_gpu_grad_shapes as gs
from helpers import DEV, RTOL, clean_rays, compare_param_grads, dt, grad_check, render_loss, scene_pair
from pixel_nerf_yolo_amd import synth
from pixel_nerf_yolo_amd.render import NeRFRenderer, YoloRenderer
from test_gpu_f16 import QUERY_TOL
from test_gpu_f16_train import GRAD_TOL, LATENT_TOL
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

F64 = torch.float64
H, W = 32, 40
LAT_HW = (8, 8)
PI = math.pi
OUT_GAIN = 0.05        # YOLO mode: raw outputs stay O(1) (synth.mlp_state)
BOX = 0.5              # query points are uniform in [-BOX, BOX]^3 (YOLO mode: the populations of gs.pick_points)

# code = (num_freqs, freq_factor).  Top frequency freq_factor * 2^(num_freqs - 1): the code's argument is formed in fp32 by
# contract, so at a top frequency of 96 or more the fp32 oracle's own gradient gap to float64 is measured per case in
# tests/test_cpu_model_desc.py::test_fp32_oracle_gradient_gap (admission: at most 0.5 x RTOL for every tensor).  Measured there
# (query gradients, points in [-0.5, 0.5]^3; worst tensor's max |g_f32 - g_f64| / max |g_f64|, at margins 1e-5 / 3e-5):
# code9_pi (top 804) 9.5e-6 / 1.1e-5 (lin_in.weight), code9 (384) 2.3e-6 / 2.8e-6, code7 (96) 1.1e-6 / 1.3e-6: all admitted for the
# query backward.  Forward outputs, max |f32 - f64|: 2.1e-5 at code9_pi, 8.0e-6 or less everywhere else.
CASES = {
    "code0": dict(code=(0, 1.5), nb=3, cl=2, ns=2, L=256, d_out=4),
    "code1": dict(code=(1, 1.0), nb=2, cl=1, ns=1, L=128, d_out=4),
    "code9_pi": dict(code=(9, PI), nb=5, cl=3, ns=2, L=512, d_out=4),
    "code9": dict(code=(9, 1.5), nb=3, cl=2, ns=3, L=256, d_out=4),
    "code4_pi_L2048": dict(code=(4, PI), nb=3, cl=2, ns=2, L=2048, d_out=4),
    "L768": dict(code=(6, 1.5), nb=4, cl=2, ns=2, L=768, d_out=4),
    "L384": dict(code=(6, 1.5), nb=3, cl=2, ns=2, L=384, d_out=4),
    "nb1": dict(code=(6, 1.5), nb=1, cl=1000, ns=1, L=128, d_out=4, n=65),
    "nb7": dict(code=(6, 1.5), nb=7, cl=1, ns=3, L=256, d_out=4),
    "nb8": dict(code=(3, 1.0), nb=8, cl=3, ns=2, L=256, d_out=4),
    "nb8_all_view": dict(code=(6, 1.5), nb=8, cl=8, ns=1, L=128, d_out=4),
    "yolo_d1": dict(code=(6, 1.5), nb=3, cl=2, ns=2, L=256, d_out=1, yolo=True),
    "yolo_d7": dict(code=(2, PI), nb=3, cl=2, ns=2, L=256, d_out=7, yolo=True),
    "yolo_d63": dict(code=(6, 1.5), nb=3, cl=2, ns=2, L=256, d_out=63, yolo=True),
    "yolo_d64": dict(code=(6, 1.5), nb=2, cl=1, ns=2, L=128, d_out=64, yolo=True),
    "code7": dict(code=(7, 1.5), nb=3, cl=2, ns=3, L=256, d_out=4),       # code9's stand-in in the render backward (RENDER_CASES)
}
for _c in CASES.values():
    _c.setdefault("n", 130)
    _c.setdefault("yolo", False)
    _c["proj"] = "straddle"         # (YOLO cases: the populations of gs.pick_points, which reads this key)

# what each case is there for, asserted on its own description (test_cases_hold_their_edges)
EDGES = {
    "code0": dict(d_in=6, ncode=3), "code1": dict(d_in=12, lg_refused=True), "code9_pi": dict(d_in=60, top=PI * 256), "code9": dict(d_in=60, top=384.0),
    "code4_pi_L2048": dict(chunks=16, lg_blocks=8), "L768": dict(chunks=6, lg_blocks=3), "L384": dict(chunks=3, lg_refused=True),
    "nb1": dict(nvb=1, lg_refused=True, tiles=2), "nb7": dict(nvb=1, fp32_forward=True), "nb8": dict(nvb=3, post=5, fp32_forward=True),
    "nb8_all_view": dict(nvb=8, fp32_forward=True, lg_refused=True), "yolo_d1": dict(d_out=1), "yolo_d7": dict(d_out=7, anchors=1),
    "yolo_d63": dict(d_out=63, anchors=9), "yolo_d64": dict(d_out=64, lg_refused=True), "code7": dict(d_in=48, top=96.0),
}
H2_MAX_BLOCKS = 6      # include/pnyolo.h: models with more than 6 residual blocks or combine_layer = 0 always run F32 forwards


def d_in_of(case):
    return 6 + 6 * case["code"][0]


def top_frequency(case):
    nf, ff = case["code"]
    return ff * 2.0 ** (nf - 1) if nf > 0 else 0.0


def nvb_of(case):
    return min(case["nb"], case["cl"])


def lg_refused(case):
    """The latent-gradient kernels launch L / 256 blocks: the library refuses other widths."""
    return case["L"] % 256 != 0


def fp32_forward(case):
    return case["nb"] > H2_MAX_BLOCKS or case["cl"] == 0


def seed_of(name):
    return 8000 + 23 * list(CASES).index(name)


def scene(name, with_net=True, lat_grad=False, dtype=F64):
    c = CASES[name]
    return scene_pair(c["ns"], H, W, c["L"], c["d_out"], c["nb"], c["cl"], seed_of(name), yolo=c["yolo"], lat_hw=LAT_HW,
                      lat_grad=lat_grad, dtype=dtype, yolo_flip=False, with_net=with_net, code=c["code"],
                      out_gain=OUT_GAIN if c["yolo"] else 1.0)


def candidates(sc, case, seed, n=None):
    """(xyz, vd) candidates: uniform in the box, in front of every camera; int(POOL * n) + 24 of them (gs.POOL, the pool factor of
    test_gpu_grad_shapes.py)."""
    n = case["n"] if n is None else n
    m = int(gs.POOL * n) + 24
    rs = np.random.RandomState(seed)
    xyz = rs.uniform(-BOX, BOX, size=(m, 3)).astype(np.float32)
    vd = rs.standard_normal((m, 3)).astype(np.float32)
    assert bool((gs.projection(sc, xyz)[1] < 0).all())
    return xyz, vd


def relu_safe(sc, xyz, vd, ambig):
    orc.RELU_TRACE = []
    try:
        with torch.no_grad():
            orc.query(sc, xyz, vd, coarse=True)
        return torch.stack(orc.RELU_TRACE).min(dim=0)[0] >= ambig
    finally:
        orc.RELU_TRACE = None


def pick(sc, case, ambig, seed, n=None):
    """-> (xyz, vd, share): the first n relu-safe candidates at margin `ambig`, and the share of the candidates that is safe.
    YOLO cases: gs.pick_points (culled points, dropped taps; share None)."""
    n = case["n"] if n is None else n
    if case["yolo"]:
        xyz, vd = gs.pick_points(sc, dict(case, n=n), ambig, seed, gs.POOL)
        return xyz, vd, None
    xyz, vd = candidates(sc, case, seed, n)
    ok = relu_safe(sc, xyz, vd, ambig)
    idx = ok.nonzero().flatten()[:n].numpy()
    assert len(idx) == n, "too few relu-safe points: %d of %d candidates, %d needed" % (int(ok.sum()), len(xyz), n)
    return xyz[idx], vd[idx], float(ok.float().mean())


_REF = {}


def reference(name, ambig, n=None, dtype=F64):
    """Inputs and the oracle's outputs and gradients of a case in `dtype` (memoised; the same for every leg with this margin).
    The points are always selected on the float64 oracle."""
    key = (name, ambig, n, dtype)
    if key in _REF:
        return _REF[key]
    case, seed = CASES[name], seed_of(name)
    if dtype == F64:
        _, sc = scene(name, with_net=False, lat_grad=True)
        xyz, vd, share = pick(sc, case, ambig, seed, n)
        if case["yolo"]:
            gs.assert_edges(sc, case, xyz)
    else:
        r64 = reference(name, ambig, n)
        xyz, vd, share = r64["xyz"], r64["vd"], r64["share"]
        _, sc = scene(name, with_net=False, lat_grad=True, dtype=None)
    G = np.random.RandomState(seed + 5).standard_normal((len(xyz), case["d_out"])).astype(np.float32)
    ref = orc.query(sc, xyz, vd, coarse=True)
    assert ref.dtype == (F64 if dtype == F64 else torch.float32) and ref.shape == G.shape
    (ref * torch.from_numpy(G).to(ref.dtype)).sum().backward()
    out = dict(seed=seed, xyz=xyz, vd=vd, G=G, share=share, ref=ref.detach(), lat=sc.latent.grad.clone(),
               params={k: (v.grad.clone() if v.grad is not None else torch.zeros_like(v)) for k, v in sc.mlp_coarse.items()})
    _REF[key] = out
    return out


def test_cases_hold_their_edges():
    """Each case's description has the edge it is in the table for."""
    assert set(EDGES) == set(CASES)
    for name, e in EDGES.items():
        c = CASES[name]
        if "d_in" in e:
            assert d_in_of(c) == e["d_in"], name
        if "ncode" in e:
            assert 3 + 6 * c["code"][0] == e["ncode"], name
        if "top" in e:
            assert abs(top_frequency(c) - e["top"]) < 1e-9, name
        if "chunks" in e:
            assert c["L"] // 128 == e["chunks"] and c["L"] % 128 == 0, name      # the stash's lin_z gather: L / 128 chunks
        if "lg_blocks" in e:
            assert c["L"] // 256 == e["lg_blocks"] and not lg_refused(c), name
        assert lg_refused(c) == bool(e.get("lg_refused")), name
        assert fp32_forward(c) == bool(e.get("fp32_forward")), name
        if "nvb" in e:
            assert nvb_of(c) == e["nvb"], name
        if "post" in e:
            assert c["nb"] - nvb_of(c) == e["post"], name
        if "tiles" in e:
            assert -(-c["n"] // 64) == e["tiles"] and c["n"] % 64 != 0, name
        if "d_out" in e:
            assert c["d_out"] == e["d_out"] and c["yolo"], name
        if "anchors" in e:
            assert c["d_out"] == 7 * e["anchors"], name
        assert c["ns"] == 1 or c["cl"] < c["nb"], name       # a multi-view scene averages its views
    assert all(-(-c["n"] // 64) == 3 and c["n"] % 64 for n_, c in CASES.items() if n_ != "nb1")
    assert {c["code"][0] for c in CASES.values()} >= {0, 1, 2, 3, 4, 6, 9} and {c["nb"] for c in CASES.values()} >= {1, 7, 8}
    assert {c["d_out"] for c in CASES.values()} >= {1, 4, 7, 63, 64} and {c["L"] for c in CASES.values()} >= {128, 384, 768, 2048}


# --------------------------------------------------------------------------- a. no-grad forward, every route
# (name, scene precision, projection, PNYOLO_H2_SPLIT, reported kernel precision, bar); the three f16 routes are those of
# test_gpu_view_mean.py ROUTES
ROUTES = (("f32_raw", "f32", "off", None, "f32", TOL), ("f32_proj", "f32", "on", None, "f32", TOL),
          ("h2", "f16x2", "on", "0", "f16x2", TOL), ("h2s", "f16x2", "on", "1", "f16x2", TOL), ("h1", "f16", "on", None, "f16", QUERY_TOL))


def run_route(net, monkeypatch, route, case, xyz, vd):
    name, prec, proj, split, reported, _ = route
    net.set_matrix_precision(prec)
    net.set_latent_projection(proj)
    if split is None:
        monkeypatch.delenv("PNYOLO_H2_SPLIT", raising=False)
    else:
        monkeypatch.setenv("PNYOLO_H2_SPLIT", split)
    with torch.no_grad():
        out = net(dt(xyz)[None], coarse=True, viewdirs=dt(vd)[None])[0].clone()
    torch.cuda.synchronize()
    want = "f32" if fp32_forward(case) else reported
    assert net.last_launch_precision() == want, (name, net.last_launch_precision(), want)
    st = net.last_mlp_stats(full=True)
    assert st["launches"] == 1 and bool(st["projected"]) == (proj == "on"), (name, st)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_forward_routes_vs_fp64(name, monkeypatch):
    case = CASES[name]
    for var in ("PNYOLO_MLP_PRECISION", "PNYOLO_PROJECTION", "PNYOLO_GRID"):
        monkeypatch.delenv(var, raising=False)
    r = reference(name, gs.AMBIG)
    net, _ = scene(name)
    net = net.eval()
    assert tuple(net.mlp_coarse.lin_in.weight.shape) == (512, d_in_of(case)) and net.d_out == case["d_out"]
    assert bool(torch.isfinite(r["ref"]).all()) and float(r["ref"].abs().max()) > 1e-2
    failed = []
    for route in ROUTES:
        out = run_route(net, monkeypatch, route, case, r["xyz"], r["vd"])
        assert out.shape == r["ref"].shape
        err = float((out.cpu().to(F64) - r["ref"]).abs().max())
        print("MODEL-DESC forward %-15s %-8s max |err| vs float64 %.3e (bar %.1e) max |ref| %.2f"
              % (name, route[0], err, route[5], float(r["ref"].abs().max())))
        if not err < route[5]:
            failed.append((route[0], err, route[5]))
    assert not failed, failed


# --------------------------------------------------------------------------- b. query backward
QUERY_LEGS = ("f32", "f16x2", "f16x2_default")
LG_MESSAGE = "multiple of 256"


def check_weights(net, r, tol, tag):
    worst = 0.0
    for k, p in net.mlp_coarse.named_parameters():
        assert p.grad is not None, k
        assert tuple(p.grad.shape) == tuple(r["params"][k].shape), k
        ratio = grad_check("mlp_coarse." + k, p.grad, r["params"][k], tol)
        print("MODEL-DESC %s %-22s worst %.2e of the tensor's max" % (tag, k, ratio))
        worst = max(worst, ratio)
    return worst


def query_step(net, r):
    out = net(dt(r["xyz"])[None], coarse=True, viewdirs=dt(r["vd"])[None])
    (out[0] * dt(r["G"])).sum().backward()
    torch.cuda.synchronize()
    return out[0].detach()


@pytest.mark.parametrize("legname", QUERY_LEGS)
@pytest.mark.parametrize("name", list(CASES))
def test_query_gradients_vs_fp64(name, legname, monkeypatch):
    """Every MLP parameter gradient (lin_in.weight at (512, d_in)) and, where L % 256 == 0, d loss / d latent.  The backward's
    arithmetic is what include/pnyolo.h documents for the leg; for more than 6 blocks the backward follows the scene's setting
    although the forward runs fp32 (the rule stated there from route_bwd), and the float64 comparison decides whether it holds."""
    case = CASES[name]
    leg = gs.set_leg(legname, monkeypatch)
    t0 = time.time()
    r = reference(name, leg["ambig"])
    tag = "query %-15s %-13s" % (name, legname)
    refused = lg_refused(case)
    net, _ = scene(name, lat_grad=True)
    assert tuple(net.mlp_coarse.lin_in.weight.shape) == (512, d_in_of(case))
    if refused:
        # a backward that asks for the latent gradient is refused with the library's message; the model stays usable
        out = net(dt(r["xyz"])[None], coarse=True, viewdirs=dt(r["vd"])[None])
        with pytest.raises(RuntimeError, match=LG_MESSAGE):
            (out[0] * dt(r["G"])).sum().backward()
        torch.cuda.synchronize()
        for p in net.parameters():
            p.grad = None
        net.test_latent = net.test_latent.detach().clone()     # the second step: the same scene, its latent frozen
        net.test_encode(net.test_latent)
    out = query_step(net, r)
    assert net.last_backward_precision() == leg["want"]
    if fp32_forward(case):
        assert net.last_launch_precision() == "f32"       # the training forward (stash) too: "always run F32"
    err = float((out.cpu().double() - r["ref"]).abs().max())
    print("MODEL-DESC %s forward max |err| %.3e" % (tag, err))
    assert err < 1e-4
    check_weights(net, r, RTOL, tag)
    if refused:
        assert net.test_latent.grad is None
    else:
        g = net.test_latent.grad
        assert g is not None and g.shape == r["lat"].shape and float(r["lat"].abs().max()) > 0
        print("MODEL-DESC %s %-22s worst %.2e of the tensor's max" % (tag, "latent", grad_check("latent", g, r["lat"], RTOL)))
    print("MODEL-DESC %s %.1f s" % (tag, time.time() - t0))


def test_query_gradients_f16_train_code9(monkeypatch):
    """Single-plane f16 training at d_in = 60, on 512 points (F16_TRAIN_MIN_SAMPLES of test_gpu_grad_shapes.py), against its bars."""
    name = "code9"
    leg = gs.set_leg("f16_train", monkeypatch)
    n = gs.F16_TRAIN_MIN_SAMPLES
    r = reference(name, leg["ambig"], n=n)
    assert len(r["xyz"]) == n
    net, _ = scene(name, lat_grad=True)
    net.set_matrix_precision("f16_train")
    query_step(net, r)
    assert net.last_backward_precision() == "f16"
    check_weights(net, r, GRAD_TOL, "query code9 f16_train")
    print("MODEL-DESC query code9 f16_train latent worst %.2e" % grad_check("latent", net.test_latent.grad, r["lat"], LATENT_TOL))


# --------------------------------------------------------------------------- c. render backward, depth samples attached
RENDER = dict(kc=8, kf=4, kfd=2, n=16, near=0.3, far=1.8, ray_seed=9)
# code9 is not admitted here: on its 16 rays the float32 oracle's own gradients are 3.7e-4 of the tensor's max from the float64
# oracle's (mlp_coarse.lin_z.0.weight; tests/test_cpu_model_desc.py RENDER_NOT_ADMITTED asserts that it is above the
# admission bar of 0.5 x RTOL), so RTOL could not be met by any fp32 implementation; code7 (top frequency 96) measures 1.5e-6,
# code0 and code4_pi_L2048 7e-7 and 8e-7.
RENDER_CASES = ("code0", "code4_pi_L2048", "code7")
RENDER_LAT_GRAD = "code0"
# (coarse, fine): added to lin_out.bias[3] of the two MLPs on both sides, so that the median raw density of either MLP on the
# target frame's samples is about + 1.  With the seeded weights as they are the medians are - 0.9 / + 0.1 (code0), - 1.9 / + 1.0
# (code4_pi_L2048), - 1.4 / + 0.8 (code7) and + 0.6 / - 0.8 (code9): code4_pi_L2048's coarse weights sum to 0.006 per ray, its
# coarse depth is 0 and every depth sample clamps to `near`, where it carries no gradient; code9's fine pass renders the white
# background nearly everywhere and mlp_fine's parameters take next to no gradient.
SIGMA_BIAS = {"code0": (1.9, 1.0), "code4_pi_L2048": (2.9, 0.0), "code7": (2.4, 0.2), "code9": (0.4, 1.8)}


def render_scene(name, with_net=True, lat_grad=False, dtype=F64):
    net, sc = scene(name, with_net=with_net, lat_grad=lat_grad, dtype=dtype)
    for i, b in enumerate(SIGMA_BIAS[name]):
        sds = [(sc.mlp_coarse, sc.mlp_fine)[i]] + ([(net.mlp_coarse, net.mlp_fine)[i].state_dict(keep_vars=True)] if with_net else [])
        with torch.no_grad():
            for sd in sds:
                sd["lin_out.bias"][3] += b
    return net, sc


_RENDER_REF = {}


def render_reference(name, dtype=F64):
    key = (name, dtype)
    if key in _RENDER_REF:
        return _RENDER_REF[key]
    c, case = RENDER, CASES[name]
    kc, kf, kfd = c["kc"], c["kf"], c["kfd"]
    if dtype == F64:
        _, sc = render_scene(name, with_net=False, lat_grad=True)
        rs = np.random.RandomState(c["ray_seed"])
        nc = H * W
        _, tgt = synth.scene_cameras(case["ns"])
        rays = orc.gen_rays(tgt[None], W, H, 0.9 * W, c["near"], c["far"])[0].reshape(-1, 8)
        dr = dict(u_coarse=rs.rand(nc, kc).astype(np.float32), u_fine=rs.rand(nc, kf - kfd).astype(np.float32),
                  u_fine2=rs.rand(nc, kf - kfd).astype(np.float32), g_depth=rs.randn(nc, kfd).astype(np.float32))
        keep = clean_rays(sc, rays, kc, kf, kfd, dr, c["n"], chunk=48, ambig=gs.AMBIG)
        gt = torch.from_numpy(rs.uniform(0, 1, size=(c["n"], 3)).astype(np.float32))
        rays, dr = rays[torch.from_numpy(keep)], {k: v[keep] for k, v in dr.items()}
    else:
        r64 = render_reference(name)
        rays, dr, gt = r64["rays"], r64["dr"], r64["gt"]
        _, sc = render_scene(name, with_net=False, lat_grad=True, dtype=None)
    ref = orc.render(sc, rays, kc, kf, kfd, dr["u_coarse"], dr["u_fine"], dr["u_fine2"], dr["g_depth"], detach_fine_depth=False)
    zd = ref["coarse"]["depth"].detach()[:, None] + torch.from_numpy(dr["g_depth"]).to(ref["coarse"]["depth"].dtype) * 0.01
    assert int(((zd > c["near"]) & (zd < c["far"])).sum()) > c["n"] * kfd // 2        # most depth samples are unclamped
    render_loss(ref, gt.to(ref["fine"]["rgb"].dtype), True).backward()
    assert float(sc.latent.grad.abs().max()) > 0
    _RENDER_REF[key] = dict(sc=sc, rays=rays, dr=dr, gt=gt, z_fine=ref["fine"].get("z"), fine_rgb=ref["fine"]["rgb"].detach(), lat=sc.latent.grad.clone())
    return _RENDER_REF[key]


@pytest.mark.parametrize("legname", ["f32", "f16x2"])
@pytest.mark.parametrize("name", RENDER_CASES)
def test_render_backward_vs_fp64(name, legname, monkeypatch):
    """The body of test_gpu_many_views.py::test_render_backward_vs_fp64: 16 relu-safe rays x (8 + 4) samples, the trainer's
    loss with the depth terms, the fine pass's depth samples attached to the coarse depth."""
    c = RENDER
    leg = gs.set_leg(legname, monkeypatch)
    r = render_reference(name)
    lat_grad = name == RENDER_LAT_GRAD
    net, _ = render_scene(name, lat_grad=lat_grad)
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
    print("MODEL-DESC render %-15s %-6s fine rgb max |err| %.2e" % (name, legname, e_rgb))
    assert e_rgb < 1e-4
    worst = compare_param_grads(net, r["sc"])
    print("MODEL-DESC render %-15s %-6s weight worst %.2e of the tensor's max" % (name, legname, worst))
    if lat_grad:
        g = net.test_latent.grad
        assert g is not None and g.shape == r["lat"].shape
        print("MODEL-DESC render %-15s %-6s latent worst %.2e of the tensor's max" % (name, legname, grad_check("latent", g, r["lat"])))


def yolo_render_inputs(name="yolo_d7", n=24, K=16):
    """(sc, rays, u, G): n relu-safe rays of a 16 x 12 target frame, K samples each, on the float64 oracle."""
    case = CASES[name]
    _, sc = scene(name, with_net=False)
    _, tgt_c2w = synth.scene_cameras(case["ns"], radius=4.0, phi=-25.0)
    tgt_w2c = np.linalg.inv(tgt_c2w).astype(np.float32)
    cand = orc.gen_rays_yolo(tgt_w2c[None], 16, 12, [20.0, 22.0], [8.0, 6.0], -6.0, -1.0)[0].reshape(-1, 8)
    rs = np.random.RandomState(21)
    u_all = rs.rand(cand.shape[0], K).astype(np.float32)
    orc.RELU_TRACE = []
    try:
        with torch.no_grad():
            orc.yolo_render(sc, cand, K, u_all, n_anchors=case["d_out"] // 7)
        ok = torch.ones(cand.shape[0], dtype=torch.bool)
        for t in orc.RELU_TRACE:
            ok &= t.reshape(cand.shape[0], -1).min(dim=1)[0] >= gs.AMBIG
    finally:
        orc.RELU_TRACE = None
    keep = ok.nonzero().flatten()[:n]
    assert keep.numel() == n, int(ok.sum())
    G = torch.from_numpy(rs.standard_normal((n, case["d_out"] // 7, 7)).astype(np.float32))
    return sc, cand[keep], u_all[keep.numpy()], G


def test_yolo_render_one_anchor_vs_fp64():
    """YoloRenderer forward and backward at d_out = 7 (one anchor) and the (2, pi) code, as
    test_gpu_backward.py::test_yolo_render_backward_vs_oracle does at 21."""
    name = "yolo_d7"
    sc, rays, u, G = yolo_render_inputs(name)
    n, K = u.shape
    net, _ = scene(name)
    ren = YoloRenderer(K, 128, 1, 1)
    ren.bind_parallel(net)
    ren.draws = dict(u_coarse=u)
    out = ren(rays[None].to(DEV))
    assert out.requires_grad and out.shape == (n, 1, 7)
    (out * G.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    ref = orc.yolo_render(sc, rays, K, u, n_anchors=1)
    scale = max(1.0, float(ref["out"].detach().abs().max()))
    err = float((out.detach().cpu().to(F64) - ref["out"].detach()).abs().max())
    print("MODEL-DESC yolo_render yolo_d7 max |err| %.2e (bar %.1e)" % (err, 1e-4 * scale))
    assert err < 1e-4 * scale
    (ref["out"] * G.to(F64)).sum().backward()
    print("MODEL-DESC yolo_render yolo_d7 weight worst %.2e" % compare_param_grads(net, sc, which=("mlp_coarse",)))
