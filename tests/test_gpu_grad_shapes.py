"""
The backward's latent-gradient and weight-gradient kernels across shapes (-m gpu): each case runs one forward and backward
through the public API (PixelNeRFNet queries, NeRFRenderer) and compares the MLP parameter gradients and d loss / d latent
with torch.autograd through the oracle in float64 (pnyolo_oracle Scene(dtype=torch.float64)).

The cases cross, pairwise rather than as a product, the MLP layout (n_blocks / combine_layer, so 0..6 per-view lin_z
blocks: the K of the latent gradient's lin_z^T GEMM), the view count, the latent width and grid, the number of 64-sample
tiles (one tile: the latent gradient's one-tile kernel; two or more: its pair-of-tiles kernel, an odd count leaving the
last pair half empty; a ragged last tile; >= 40 tiles), where the points project (every tap inside, taps straddling the
grid edge, wholly outside one view but inside another: out-of-range taps are dropped), YOLO mode (d_out 21, L 1792, points
behind a camera culled) and a grouped super-batch whose tile pairs span two objects.  Every case asserts on its own inputs
that its edges occur.  A second table, MANY_VIEW_CASES, runs 5, 8, 11 and 16 views per object (16 is the ABI's limit) on
cameras that are all distinct, through the same body, legs and bars.

Arithmetic legs (the backward's matrix products; test_gpu_backward.py has the same legs as a module fixture):
  f32            fp32 forward, fp32 backward                          1e-4 x each tensor's max, points with relu margin AMBIG
  f16x2          fp32 forward, split-f16 backward                     1e-4, AMBIG
  f16x2_default  the default split-f16 forward and backward           1e-4, AMBIG_DEFAULT
  f16_train      single-plane f16 training (PNY_PRECISION_F16_TRAIN)   test_gpu_f16_train.py's bars, cases of >= 512 samples
                                                                       per pass only (README: the single-plane forward's
                                                                       error on a few dozen rays is larger)
"""
import os
import time

import numpy as np
import pytest
import torch

import pnyolo_oracle as orc
from helpers import DEV, RTOL, camera_ring, clean_rays, dt, grad_check, scene_pair
from pixel_nerf_yolo_amd import conf as pconf
from pixel_nerf_yolo_amd import synth
from pixel_nerf_yolo_amd.model import make_model
from pixel_nerf_yolo_amd.render import NeRFRenderer
from test_gpu_f16_train import GRAD_TOL, LATENT_TOL

pytestmark = pytest.mark.gpu

F64 = torch.float64
AMBIG = 1e-5           # as test_gpu_backward.py: fp32 reference-order forward
AMBIG_DEFAULT = float(os.environ.get("PNYOLO_TEST_AMBIG_DEFAULT", "3e-5"))   # ... the default f16x2 forward
F16_TRAIN_MIN_SAMPLES = 512

LEGS = {
    "f32": dict(mlp="f32", bwd="f32", prec=None, ambig=AMBIG, want="f32"),
    "f16x2": dict(mlp="f32", bwd="f16x2", prec=None, ambig=AMBIG, want="f16x2"),
    "f16x2_default": dict(mlp=None, bwd="f16x2", prec=None, ambig=AMBIG_DEFAULT, want="f16x2"),
    "f16_train": dict(mlp=None, bwd=None, prec="f16_train", ambig=AMBIG_DEFAULT, want="f16"),
}

# query cases: n points per view; tiles = ceil(n / 64).  combine_layer >= n_blocks never averages the views (resnetfc.py:
# 166-170): the reference then returns one row per view and point, a shape only NS = 1 gives meaning to
CASES = {
    "5-3_ns2_L512_16x16_1tile_inside": dict(nb=5, cl=3, ns=2, L=512, hw=(16, 16), n=64, proj="inside"),
    "3-1000_ns1_L512_8x8_2tiles_straddle": dict(nb=3, cl=1000, ns=1, L=512, hw=(8, 8), n=128, proj="straddle"),
    "5-1_ns3_L1792_12x20_3tiles_outside": dict(nb=5, cl=1, ns=3, L=1792, hw=(12, 20), n=192, proj="outside"),
    "4-2_ns4_L512_5x9_5tiles_ragged_straddle": dict(nb=4, cl=2, ns=4, L=512, hw=(5, 9), n=290, proj="straddle"),
    "6-1000_ns1_L1792_12x20_2tiles_ragged_inside": dict(nb=6, cl=1000, ns=1, L=1792, hw=(12, 20), n=100, proj="inside"),
    "5-5_ns1_L512_16x16_16tiles_straddle": dict(nb=5, cl=5, ns=1, L=512, hw=(16, 16), n=1000, proj="straddle"),
    "6-4_ns2_L1792_8x8_41tiles_outside": dict(nb=6, cl=4, ns=2, L=1792, hw=(8, 8), n=2600, proj="outside"),
    "2-0_ns2_L512_8x8_2tiles_inside": dict(nb=2, cl=0, ns=2, L=512, hw=(8, 8), n=90, proj="inside"),
    "yolo_5-3_ns2_L1792_12x20_3tiles_culled": dict(nb=5, cl=3, ns=2, L=1792, hw=(12, 20), n=150, proj="straddle", yolo=True),
}
# 5 to 16 views per object (the ABI's limit) on helpers.camera_ring, whose views are all distinct: the 1 / NS scaling for NS
# that is no power of two, the stash records' NS-sized strides, the latent gradient's grid n_tiles * NS * (L / 256) and its
# pair-of-tiles decode (an odd tile count at 16 views), all 16 cameras of the kernel arguments.  A table of its own, so that
# the seeds of CASES (from a case's place in that table) stay what they were; at these view counts fewer random points are
# relu-safe (tests/test_cpu_many_views.py, profiles/many_views.md), so the points are picked from a pool MANY_VIEW_POOL x the need.
MANY_VIEW_CASES = {
    "5-3_ns16_L512_16x16_2tiles_inside": dict(nb=5, cl=3, ns=16, L=512, hw=(16, 16), n=128, proj="inside"),
    "5-3_ns16_L512_16x16_3tiles_ragged_straddle": dict(nb=5, cl=3, ns=16, L=512, hw=(16, 16), n=130, proj="straddle"),
    "2-1_ns16_L512_8x8_2tiles_outside": dict(nb=2, cl=1, ns=16, L=512, hw=(8, 8), n=128, proj="outside"),
    "6-4_ns11_L1792_8x8_2tiles_straddle": dict(nb=6, cl=4, ns=11, L=1792, hw=(8, 8), n=128, proj="straddle"),
    "5-3_ns5_L512_16x16_2tiles_ragged_outside": dict(nb=5, cl=3, ns=5, L=512, hw=(16, 16), n=70, proj="outside"),
    "3-2_ns8_L512_5x9_4tiles_ragged_straddle": dict(nb=3, cl=2, ns=8, L=512, hw=(5, 9), n=200, proj="straddle"),
}
for _c in MANY_VIEW_CASES.values():
    _c["ring"] = True
POOL, MANY_VIEW_POOL = 1.6, 4.0
# The seed base is chosen on the float64 oracle alone (an input condition): the 16-view "inside" case is the tight one, as only
# ~300 of its 1824 candidates have every tap inside all 16 views and 37 % of those are relu-safe at AMBIG_DEFAULT; of the bases
# 4000, 4100 .. 4500, the bases 4100 and 4500 fill every population of every case at both margins.
MANY_VIEW_SEED = 4100
ALL_CASES = {**CASES, **MANY_VIEW_CASES}
H, W = 32, 40

_MEMO = {}      # (case, ambig) -> inputs and float64 reference: the same for every leg that selects with that margin


def set_leg(name, monkeypatch):
    """The leg's scene defaults (read when a scene is created) through the environment; f16_train is set on the model."""
    cfg = LEGS[name]
    for var, key in (("PNYOLO_MLP_PRECISION", "mlp"), ("PNYOLO_BWD_PRECISION", "bwd")):
        if cfg[key] is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, cfg[key])
    return dict(cfg, name=name)


def tol_of(leg):
    return (GRAD_TOL, LATENT_TOL) if leg["name"] == "f16_train" else (RTOL, RTOL)


def report(case, leg, kind, ratio):
    print("GRAD-SHAPES %-46s %-13s %-6s worst %.2e of the tensor's max" % (case, leg["name"], kind, ratio))


# --------------------------------------------------------------------------- where the points project
def projection(sc, xyz):
    """Per (view, point), in float64 as the oracle's index_latent: the number of the four bilinear taps inside the latent
    grid, and the camera-space z."""
    xyz = torch.as_tensor(np.asarray(xyz), dtype=F64)
    w2c = sc.w2c.to(F64)
    xc = torch.einsum("vij,pj->vpi", w2c[:, :, :3], xyz) + w2c[:, None, :, 3]
    uv = (xc[..., :2] if sc.yolo else -xc[..., :2]) / xc[..., 2:]
    ns = xc.shape[0]
    foc, cc = sc.focal.to(F64).expand(ns, 2), sc.c.to(F64).expand(ns, 2)
    uv = uv * foc[:, None] + cc[:, None]
    Hl, Wl = sc.latent.shape[-2:]
    scale = torch.tensor([Wl / (Wl - 1) * 2.0 / sc.width, Hl / (Hl - 1) * 2.0 / sc.height], dtype=F64)
    g = uv * scale - 1.0
    ix, iy = (g[..., 0] + 1) / 2 * (Wl - 1), (g[..., 1] + 1) / 2 * (Hl - 1)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    taps = torch.zeros_like(ix, dtype=torch.long)
    for xs in (x0, x0 + 1):
        for ys in (y0, y0 + 1):
            taps += ((xs >= 0) & (xs <= Wl - 1) & (ys >= 0) & (ys <= Hl - 1)).long()
    return taps, xc[..., 2]


def pick_points(sc, case, ambig, seed, pool=POOL):
    """n query points with the case's projection edge, every relu unit of the float64 forward at least `ambig` from zero.
    pool: how many candidates of each population are traced, as a multiple of the population's size."""
    n, proj, yolo = case["n"], case["proj"], case.get("yolo", False)
    rs = np.random.RandomState(seed)
    m = 8 * n + 800
    xyz = rs.uniform(-7.0, 7.0, size=(m, 3)) if yolo else rs.uniform(-0.9, 0.9, size=(m, 3))
    xyz = xyz.astype(np.float32)
    vd = rs.standard_normal((m, 3)).astype(np.float32)
    taps, z = projection(sc, xyz)
    live = z < 0        # non-YOLO: in front of the camera; YOLO: where the latent is kept
    groups = []         # (mask, count): the edge populations first, the rest of the points every tap inside every view
    if yolo:
        usable = (z.abs() > 1e-3).all(dim=0)      # finite projections
        groups.append((usable & (~live).any(dim=0), n // 5))     # culled (camera z >= 0) in a view, its latent rows zero
        groups.append((usable & live.all(dim=0) & ((taps > 0) & (taps < 4)).any(dim=0), n // 10))  # a dropped tap
    elif proj == "straddle":
        groups.append((live.all(dim=0) & ((taps > 0) & (taps < 4)).any(dim=0), n // 4))
    elif proj == "outside":
        groups.append((live.all(dim=0) & (taps == 0).any(dim=0) & (taps == 4).any(dim=0), n // 4))
    plain = live.all(dim=0) & (taps == 4).all(dim=0)      # (non-YOLO mode: camera z >= 0 excluded, NaN in the reference)
    groups.append((plain, n - sum(c for _, c in groups)))
    # relu-safe points of each population (the float64 forward's own pre-activations), traced on a pool `pool` x the need
    taken = torch.zeros(m, dtype=torch.bool)
    pools = []
    for mask, cnt in groups:
        cand = (mask & ~taken).nonzero().flatten()[:int(pool * cnt) + 24]
        taken[cand] = True
        pools.append(cand)
    cand = torch.cat(pools)
    orc.RELU_TRACE = []
    try:
        with torch.no_grad():
            orc.query(sc, xyz[cand.numpy()], vd[cand.numpy()], coarse=True)
        ok_c = torch.stack(orc.RELU_TRACE).min(dim=0)[0] >= ambig
    finally:
        orc.RELU_TRACE = None
    ok = torch.zeros(m, dtype=torch.bool)
    ok[cand] = ok_c
    idx = []
    for part, (_, cnt) in zip(pools, groups):
        sel = part[ok[part]][:cnt]
        assert sel.numel() == cnt, "too few relu-safe points of a population: %d of %d" % (sel.numel(), cnt)
        idx.append(sel)
    idx = torch.cat(idx).numpy()[rs.permutation(n)]        # the edge points spread over every tile
    return xyz[idx], vd[idx]


def assert_edges(sc, case, xyz):
    """The case's projection edge really occurs in the chosen points, and every point is usable."""
    proj = case["proj"]
    taps, z = projection(sc, xyz)
    if case.get("yolo"):
        culled = (z >= 0).any(dim=0)
        assert float(culled.float().mean()) >= 0.1, "culled points"
        assert bool((z.abs() > 1e-3).all())
        assert float(((taps > 0) & (taps < 4) & (z < 0)).any(dim=0).float().mean()) >= 0.05     # live points with a dropped tap
        return
    assert bool((z < 0).all()), "non-YOLO points in front of every camera"
    dropped = (taps < 4).any(dim=0)
    if proj == "inside":
        assert not bool(dropped.any())
    elif proj == "straddle":
        assert float(((taps > 0) & (taps < 4)).any(dim=0).float().mean()) >= 0.1
    else:
        assert float(((taps == 0).any(dim=0) & (taps == 4).any(dim=0)).float().mean()) >= 0.1


def seed_of(name):
    """A case's seed, from its place in its own table."""
    if name in CASES:
        return 3000 + 17 * sorted(CASES).index(name)
    return MANY_VIEW_SEED + 17 * sorted(MANY_VIEW_CASES).index(name)


def poses_of(case):
    return camera_ring(case["ns"])[0] if case.get("ring") else None


def pool_of(case):
    return MANY_VIEW_POOL if case.get("ring") else POOL


def reference(name, case, ambig):
    """Inputs and the float64 reference gradients of a case (memoised: the same for every leg with this margin)."""
    key = (name, ambig)
    if key in _MEMO:
        return _MEMO[key]
    seed = seed_of(name)
    yolo = case.get("yolo", False)
    _, sc = scene_pair(case["ns"], H, W, case["L"], 21 if yolo else 4, case["nb"], case["cl"], seed, yolo=yolo, lat_hw=case["hw"],
                       lat_grad=True, dtype=F64, yolo_flip=False, with_net=False, poses=poses_of(case))
    xyz, vd = pick_points(sc, case, ambig, seed, pool_of(case))
    assert_edges(sc, case, xyz)
    G = np.random.RandomState(seed + 5).standard_normal((case["n"], 21 if yolo else 4)).astype(np.float32)
    ref = orc.query(sc, xyz, vd, coarse=True)
    assert ref.dtype == F64
    (ref * torch.from_numpy(G).to(F64)).sum().backward()
    out = dict(seed=seed, xyz=xyz, vd=vd, G=G, ref=ref.detach(), lat=None if sc.latent.grad is None else sc.latent.grad.clone(),
               params={k: (v.grad.clone() if v.grad is not None else torch.zeros_like(v)) for k, v in sc.mlp_coarse.items()})
    _MEMO[key] = out
    return out


def tiles(case):
    return -(-case["n"] // 64)


# every case under the three 1e-4 legs; under f16_train the cases with >= 512 samples per pass (the bars' batch size)
QUERY_PARAMS = [(name, lg) for name in ALL_CASES for lg in LEGS
                if lg != "f16_train" or ALL_CASES[name]["n"] * ALL_CASES[name]["ns"] >= F16_TRAIN_MIN_SAMPLES]


def test_sweep_covers_the_axes():
    """Every value of every axis occurs in some case (the sweep is pairwise, not a product)."""
    cs = list(CASES.values())
    assert {(c["nb"], c["cl"]) for c in cs} >= {(5, 3), (3, 1000), (5, 1), (4, 2), (6, 4), (5, 5), (2, 0)}
    assert any(c["nb"] == 3 and c["cl"] == 1000 and c["ns"] == 1 for c in cs)      # conf/default.conf's model
    assert {min(c["nb"], c["cl"]) for c in cs} >= {0, 1, 2, 3, 4, 5, 6}            # per-view lin_z blocks
    assert {c["ns"] for c in cs} >= {1, 2, 3, 4} and {c["L"] for c in cs} >= {512, 1792}
    assert {c["hw"] for c in cs} >= {(16, 16), (8, 8)} and any(c["hw"][0] != c["hw"][1] for c in cs)
    t = [tiles(c) for c in cs]
    assert 1 in t and 2 in t and any(x >= 3 and x % 2 == 1 for x in t) and any(x >= 40 for x in t)
    assert any(c["n"] % 64 != 0 and tiles(c) >= 2 for c in cs)                      # a ragged last tile
    assert {c["proj"] for c in cs} >= {"inside", "straddle", "outside"} and any(c.get("yolo") and c["L"] == 1792 for c in cs)
    assert sum(lg == "f16_train" for _, lg in QUERY_PARAMS) >= 2
    many = list(MANY_VIEW_CASES.values())
    assert not set(MANY_VIEW_CASES) & set(CASES) and {c["ns"] for c in many} >= {5, 8, 11, 16}
    assert any(c["ns"] == 16 and tiles(c) >= 3 and tiles(c) % 2 == 1 and c["n"] % 64 != 0 for c in many)
    assert {c["proj"] for c in many} >= {"inside", "straddle", "outside"} and any(c["L"] == 1792 for c in many)
    # every leg; f16_train by its rule of >= 512 samples per pass, which all but the 5-view case (70 x 5) meet
    assert all((name, lg) in QUERY_PARAMS for name in MANY_VIEW_CASES for lg in LEGS if lg != "f16_train")
    assert {MANY_VIEW_CASES[name]["ns"] for name, lg in QUERY_PARAMS if lg == "f16_train" and name in MANY_VIEW_CASES} >= {8, 11, 16}


@pytest.mark.parametrize("name,legname", QUERY_PARAMS)
def test_query_gradients_vs_fp64(name, legname, monkeypatch):
    case = ALL_CASES[name]
    leg = set_leg(legname, monkeypatch)
    t0 = time.time()
    r = reference(name, case, leg["ambig"])
    yolo = case.get("yolo", False)
    net, _ = scene_pair(case["ns"], H, W, case["L"], 21 if yolo else 4, case["nb"], case["cl"], r["seed"], yolo=yolo,
                        lat_hw=case["hw"], lat_grad=True, yolo_flip=False, poses=poses_of(case))
    if leg["prec"]:
        net.set_matrix_precision(leg["prec"])
    out = net(dt(r["xyz"])[None], coarse=True, viewdirs=dt(r["vd"])[None])
    (out[0] * dt(r["G"])).sum().backward()
    torch.cuda.synchronize()
    assert net.last_backward_precision() == leg["want"]
    if leg["name"] != "f16_train":
        assert float((out[0].detach().cpu().double() - r["ref"]).abs().max()) < 1e-4
    p_tol, l_tol = tol_of(leg)
    worst = 0.0
    for k, p in net.mlp_coarse.named_parameters():
        assert p.grad is not None, k
        worst = max(worst, grad_check("mlp_coarse." + k, p.grad, r["params"][k], p_tol))
    report(name, leg, "weight", worst)
    g = net.test_latent.grad
    if case["cl"] == 0:
        # no lin_z block: the reference never reads the latent (autograd leaves its grad None); the library returns zeros
        assert r["lat"] is None
        assert g is not None and float(g.abs().max()) == 0.0
    else:
        assert g is not None and g.shape == r["lat"].shape and float(r["lat"].abs().max()) > 0
        report(name, leg, "latent", grad_check("latent", g, r["lat"], l_tol))
    print("GRAD-SHAPES %-46s %-13s %.1f s" % (name, leg["name"], time.time() - t0))


# --------------------------------------------------------------------------- grouped super-batch
@pytest.mark.parametrize("legname", ["f32", "f16x2"])     # 8 rays per object: below f16_train's batch size
def test_grouped_render_gradients_vs_fp64(legname, monkeypatch):
    """SB = 3 objects in ONE grouped scene (the grouped scene needs equal shares of whole tiles), 8 rays x (16 + 8) samples
    each: the coarse pass has 2 tiles per object, the fine pass 3 (tiles 0-2, 3-5, 6-8), so the latent gradient's tile pair
    (2, 3) spans objects 0 and 1 and its last pair (8, -) holds one tile.  fp32 forward only: at the default forward's margin
    (AMBIG_DEFAULT) too few of these 24-sample rays are unambiguous; the query cases hold that leg.  Every object's latent gradient against its own
    float64 reference; the parameter gradients against the sum of the three objects'."""
    leg = set_leg(legname, monkeypatch)
    SB, ns, kc, kf, kfd, n = 3, 2, 16, 8, 4, 8
    HH, WW = 32, 32
    assert (n * kc) % 64 == 0 and (n * (kc + kf)) % 64 == 0 and (n * (kc + kf)) // 64 % 2 == 1
    key = ("grouped", leg["ambig"])
    if key not in _MEMO:
        lat = np.concatenate([synth.latent(1610 + i, ns, 512, 16, 16) for i in range(SB)])
        poses = np.stack([synth.scene_cameras(ns, radius=1.3 + 0.1 * i)[0] for i in range(SB)])
        focal = torch.tensor([[28.0, 28.0], [30.0, 31.0], [27.0, 29.0]])
        sd_c, sd_f = synth.mlp_state(1601), synth.mlp_state(1602)
        mc = {k: torch.from_numpy(v).to(F64).requires_grad_() for k, v in sd_c.items()}
        mf = {k: torch.from_numpy(v).to(F64).requires_grad_() for k, v in sd_f.items()}
        rs = np.random.RandomState(16)
        objs = []
        for i in range(SB):
            sc = orc.Scene(mc, mf, lat[i * ns:(i + 1) * ns], poses[i], focal[i:i + 1], None, WW, HH, dtype=F64)
            sc.mlp_coarse, sc.mlp_fine = mc, mf
            sc.latent = torch.from_numpy(lat[i * ns:(i + 1) * ns]).to(F64).requires_grad_()
            cand = orc.gen_rays(synth.pose_spherical(100.0 + 25 * i, -20.0, 1.3)[None], WW, HH, 29.0, 0.3, 1.8)[0].reshape(-1, 8)
            cand = cand[torch.from_numpy(rs.permutation(cand.shape[0])[:200])]
            nc = cand.shape[0]
            dr = dict(u_coarse=rs.rand(nc, kc).astype(np.float32), u_fine=rs.rand(nc, kf - kfd).astype(np.float32),
                      u_fine2=rs.rand(nc, kf - kfd).astype(np.float32), g_depth=rs.randn(nc, kfd).astype(np.float32))
            keep = clean_rays(sc, cand, kc, kf, kfd, dr, n, ambig=leg["ambig"])
            objs.append((sc, cand[torch.from_numpy(keep)], {k: v[keep] for k, v in dr.items()}))
        gt = torch.from_numpy(rs.uniform(0, 1, size=(SB, n, 3)).astype(np.float32))
        loss = 0.0
        for i, (sc, rays, dr) in enumerate(objs):
            r = orc.render(sc, rays, kc, kf, kfd, dr["u_coarse"], dr["u_fine"], dr["u_fine2"], dr["g_depth"])
            loss = loss + ((r["coarse"]["rgb"] - gt[i].to(F64)).square().sum() + (r["fine"]["rgb"] - gt[i].to(F64)).square().sum()) / (SB * n * 3) \
                + 0.1 * r["fine"]["depth"].sum() / (SB * n)
        loss.backward()
        _MEMO[key] = dict(lat=lat, poses=poses, focal=focal, gt=gt, rays=torch.stack([o[1] for o in objs]),
                          dr={k: np.concatenate([o[2][k] for o in objs]) for k in objs[0][2]},
                          lat_ref=[o[0].latent.grad.clone() for o in objs],
                          params={pre + "." + k: v.grad.clone() for pre, m_ in (("mlp_coarse", mc), ("mlp_fine", mf)) for k, v in m_.items()})
    r = _MEMO[key]
    net = make_model(pconf.default_mv()["model"], stop_encoder_grad=True)
    net.mlp_coarse.load_state_dict({k: torch.from_numpy(v) for k, v in synth.mlp_state(1601).items()})
    net.mlp_fine.load_state_dict({k: torch.from_numpy(v) for k, v in synth.mlp_state(1602).items()})
    net = net.to(DEV).train()
    lt = torch.from_numpy(r["lat"]).to(DEV).requires_grad_()
    net.encode(torch.zeros(SB, ns, 3, HH, WW), torch.from_numpy(r["poses"]), r["focal"], latent=lt)
    assert net._group is not None
    ren = NeRFRenderer(n_coarse=kc, n_fine=kf, n_fine_depth=kfd, white_bkgd=True).train()
    ren.draws = r["dr"]
    out = ren(net, r["rays"].to(DEV), want_weights=True)
    gt = r["gt"].to(DEV)
    (torch.nn.functional.mse_loss(out["coarse"]["rgb"], gt) + torch.nn.functional.mse_loss(out["fine"]["rgb"], gt)
     + 0.1 * out["fine"]["depth"].mean()).backward()
    torch.cuda.synchronize()
    assert net._last_call_group and net.last_backward_precision() == leg["want"]
    worst = 0.0
    for pre in ("mlp_coarse", "mlp_fine"):
        for k, p in getattr(net, pre).named_parameters():
            worst = max(worst, grad_check(pre + "." + k, p.grad, r["params"][pre + "." + k]))
    report("grouped_3x(2|3 tiles)", leg, "weight", worst)
    worst = 0.0
    for i in range(SB):
        assert float(r["lat_ref"][i].abs().max()) > 0
        worst = max(worst, grad_check("latent of object %d" % i, lt.grad[i * ns:(i + 1) * ns], r["lat_ref"][i]))
    report("grouped_3x(2|3 tiles)", leg, "latent", worst)
