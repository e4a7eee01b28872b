"""
The single-plane f16 precision mode (-m gpu; include/pnyolo.h PNY_PRECISION_F16, csrc/mlp_h1.hip).

F16 is opt-in and sits OUTSIDE the 1e-4 parity claim: every operand of the fused MLP's GEMMs is one f16 value (round to
nearest), products accumulate in fp32.  Its bars below were each set from one MI355X measurement with at most 2x margin
(the measured value is written beside each constant).  What it must keep exactly: determinism, independence of the launch a
sample is rendered in, and the AUTO behaviour of everything that is not a no-grad projected forward (training forward,
backward, projection, fp32 fallbacks) -- bit for bit.
"""
import warnings

import numpy as np
import pytest
import torch

import pnyolo_oracle as orc
from helpers import DEV, dt, fine_flip_rays, load_mlp, maxabs, nerf_net, render_debug
from pixel_nerf_yolo_amd import conf as pconf
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd import synth
from pixel_nerf_yolo_amd.model import make_model
from pixel_nerf_yolo_amd.render import NeRFRenderer, make_renderer
from pixel_nerf_yolo_amd.util import gen_rays

pytestmark = pytest.mark.gpu

# bars (absolute), each from one measurement on the MI355X (measured value in the comment), at most 2x margin
QUERY_TOL = 5e-3         # nerf_c2 probes + mlp_shapes: max |d rgb|, |d sigma| (measured 2.79e-3)
RENDER_TOL = 5e-3        # nerf_c2 render golden, coarse samples / pixels / weights / depth (measured 2.65e-3)
FINE_TOL = 4.8e-3        # nerf_c2 render golden, fine pass on the rays whose fine depths equal F32's (measured 2.43e-3)
FINE_MOVED_MAX = 180     # rays of nerf_c2 whose fine depths moved against F32's (measured 93)
YOLO_TOL = 1.4e-3        # yolo_c3 golden, relative to max(1, max |raw|) (measured 7.18e-4)
FRAME_PSNR_MIN = 68.8    # full C2 frame against the F32 render, dB (measured 71.84; 2x the MSE = -3.0 dB)


def report(name, value):
    print("F16-MEASURED %s %.6g" % (name, value))


def set_env(monkeypatch, prec="f16", proj="on"):
    monkeypatch.setenv("PNYOLO_PROJECTION", proj)
    monkeypatch.setenv("PNYOLO_MLP_PRECISION", prec)


# --------------------------------------------------------------------------- ABI and dispatch
def test_abi_accepts_f16_and_reports_the_kernel(golden, monkeypatch):
    set_env(monkeypatch, "auto")
    g = golden("nerf_c2")
    net = nerf_net(g, 7)
    xyz, vd = dt(g["probe_xyz"])[None], dt(g["probe_viewdirs"])[None]
    with torch.no_grad():
        net(xyz, coarse=True, viewdirs=vd)
    assert net.last_launch_precision() == "f16x2"
    L = plib.load()
    h = net._scene(0)
    assert L.pny_scene_set_precision(h, plib.PRECISION["f16"]) == 0
    assert L.pny_scene_set_precision(h, 4) == -1          # PNY_ERR_ARG
    with torch.no_grad():
        net(xyz, coarse=True, viewdirs=vd)
    assert net.last_launch_precision() == "f16" and net.last_launch_f16x2()
    assert net.last_mlp_stats(full=True)["projected"]


@pytest.mark.parametrize("case", ["seven_blocks", "weight_out_of_range"])
def test_fp32_fallbacks_under_f16(golden, monkeypatch, case):
    """What AUTO runs on fp32 runs on fp32 under F16 too: more than 6 residual blocks, a weight beyond the f16 range."""
    set_env(monkeypatch)
    if case == "seven_blocks":
        c = pconf.default_mv()
        c.d["model"]["mlp_coarse"] = {"type": "resnet", "n_blocks": 7, "d_hidden": 512, "d_out": 4, "combine_layer": 3}
        c.d["model"]["mlp_fine"] = {"type": "empty"}
        net = make_model(c["model"]).eval()
        sd = synth.mlp_state(4007, n_blocks=7, combine_layer=3)
        net.mlp_coarse.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        net = net.to(DEV)
        ns, H, W = 3, 32, 32
        net.encode(torch.zeros(1, ns, 3, H, W), torch.from_numpy(synth.scene_cameras(ns)[0])[None], torch.tensor(30.0),
                   latent=torch.from_numpy(synth.latent(4107, ns, 512, H // 2, W // 2)))
        rs = np.random.RandomState(7)
        xyz = dt(rs.uniform(-0.5, 0.5, size=(1, 3000, 3)).astype(np.float32))
        vd = dt(rs.standard_normal((1, 3000, 3)).astype(np.float32))
    else:
        g = golden("nerf_c2")
        net = nerf_net(g, 7)
        xyz, vd = dt(g["probe_xyz"])[None], dt(g["probe_viewdirs"])[None]
        with torch.no_grad():
            net(xyz, coarse=True, viewdirs=vd)
        assert net.last_launch_precision() == "f16"
        with torch.no_grad():
            net.mlp_coarse.blocks[4].fc_1.weight[3, 5] = 1.0e5
            net.invalidate_weights()
    with torch.no_grad():
        out = net(xyz, coarse=True, viewdirs=vd)[0]
    assert net.last_launch_precision() == "f32" and bool(torch.isfinite(out).all())


# --------------------------------------------------------------------------- accuracy against the reference's goldens
def test_query_goldens(golden, monkeypatch):
    set_env(monkeypatch)
    g = golden("nerf_c2")
    net = nerf_net(g, 7)
    xyz, vd = dt(g["probe_xyz"])[None], dt(g["probe_viewdirs"])[None]
    worst = 0.0
    for coarse, key in ((True, "probe_out_coarse"), (False, "probe_out_fine")):
        with torch.no_grad():
            out = net(xyz, coarse=coarse, viewdirs=vd)[0]
        assert net.last_launch_precision() == "f16"
        worst = max(worst, maxabs(out, g[key]))
    gs = golden("mlp_shapes")
    seed, H, W = int(gs["seed"]), int(gs["H"]), int(gs["W"])
    for tag in "abc":
        nb, cl, ns = (int(v) for v in gs[tag + "_cfg"])
        c = pconf.default_mv()
        c.d["model"]["mlp_coarse"] = {"type": "resnet", "n_blocks": nb, "d_hidden": 512, "d_out": 4, "combine_layer": cl}
        c.d["model"]["mlp_fine"] = {"type": "empty"}
        net = make_model(c["model"]).eval()
        sd = synth.mlp_state(seed * 10 + ord(tag), n_blocks=nb, combine_layer=cl)
        net.mlp_coarse.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        net = net.to(DEV)
        lat = torch.from_numpy(synth.latent(seed * 10 + 3, ns, 512, H // 2, W // 2))
        net.encode(torch.zeros(1, ns, 3, H, W), torch.from_numpy(gs[tag + "_poses"])[None], torch.tensor(33.0), latent=lat)
        with torch.no_grad():
            out = net(dt(gs["xyz"])[None], coarse=True, viewdirs=dt(gs["viewdirs"])[None])[0]
        # combine_layer = 0 has nothing to project: fp32 kernel, inside the 1e-4 bar
        assert net.last_launch_precision() == ("f16" if min(cl, nb) > 0 else "f32"), tag
        worst = max(worst, maxabs(out, gs[tag + "_out"]))
    report("query", worst)
    assert worst <= QUERY_TOL


def test_render_c2_golden(golden, monkeypatch):
    g = golden("nerf_c2")
    ren = NeRFRenderer(n_coarse=64, n_fine=32, n_fine_depth=16, depth_std=0.01, white_bkgd=True).eval()
    draws = {k: g[k] for k in ("u_coarse", "u_fine", "u_fine2", "g_depth")}
    res = {}
    for prec in ("f32", "f16"):
        set_env(monkeypatch, prec)
        net = nerf_net(g, 7)
        res[prec] = render_debug(ren, net, g["rays"], draws, 64, 96)
        assert net.last_launch_precision() == prec
    out, dbg = res["f16"]
    n = g["rays"].shape[0]
    assert maxabs(dbg["z_coarse"][0], g["z_coarse"]) == 0.0
    coarse = max(maxabs(dbg["sample_coarse"][0].reshape(-1, 4), g["coarse_out"]),
                 maxabs(out["coarse"]["rgb"][0], g["coarse_rgb"]), maxabs(out["coarse"]["depth"][0], g["coarse_depth"]),
                 maxabs(out["coarse"]["weights"][0], g["coarse_weights"]))
    report("render_coarse", coarse)
    assert coarse <= RENDER_TOL
    # fine pass: on the rays whose fine depths equal those of the F32 render (which itself meets the golden at 1e-4);
    # importance sampling is discontinuous in the coarse weights, so F16's coarse error moves some fine samples
    z32, z16 = res["f32"][1]["z_fine"][0].cpu(), dbg["z_fine"][0].cpu()
    moved = ((z16 - z32).abs().max(dim=1)[0] > 0).nonzero().flatten().tolist()
    rays = torch.from_numpy(g["rays"])
    zf = orc.sample_fine(rays, torch.from_numpy(g["coarse_weights"]), g["u_fine"], g["u_fine2"], 64)
    zd = orc.sample_fine_depth(rays, torch.from_numpy(g["coarse_depth"]), g["g_depth"], 0.01)
    z_ref, _ = torch.sort(torch.cat([torch.from_numpy(g["z_coarse"]), zf, zd], -1), -1)
    bad32 = fine_flip_rays(z32, z_ref, torch.from_numpy(g["coarse_weights"]), g["u_fine"])
    good = torch.ones(n, dtype=torch.bool)
    good[moved] = False
    good[bad32] = False
    fine = max(maxabs(dbg["sample_fine"][0].cpu()[good].reshape(-1, 4), g["fine_out"].reshape(n, 96, 4)[good].reshape(-1, 4)),
               maxabs(out["fine"]["rgb"][0].cpu()[good], g["fine_rgb"][good]),
               maxabs(out["fine"]["depth"][0].cpu()[good], g["fine_depth"][good]),
               maxabs(out["fine"]["weights"][0].cpu()[good], g["fine_weights"][good]))
    report("render_fine", fine)
    report("render_fine_moved", len(moved))
    assert fine <= FINE_TOL and len(moved) <= FINE_MOVED_MAX


def test_yolo_c3_golden(golden, monkeypatch):
    set_env(monkeypatch)
    g = golden("yolo_c3")
    net = make_model(pconf.yolo()["model"]).eval()
    load_mlp(net.mlp_coarse, 31, 1792, 21)
    net = net.to(DEV)
    lat = torch.from_numpy(synth.latent(33, 3, 1792, 16, 16))
    net.encode(torch.zeros(1, 3, 3, 128, 128), torch.from_numpy(g["src_w2c"])[None],
               torch.from_numpy(g["focal"])[None], c=torch.from_numpy(g["c"])[None], latent=lat)
    ren = make_renderer(pconf.yolo())
    par = ren.bind_parallel(net)
    n = g["rays"].shape[0]
    ren._debug_raw = torch.empty(n, 128, 21, device=DEV)
    ren.draws = dict(u_coarse=g["u_coarse"])
    with torch.no_grad():
        out = par(dt(g["rays"])[None])
    torch.cuda.synchronize()
    assert net.last_launch_precision() == "f16"
    scale = max(1.0, float(np.abs(g["raw_out"]).max()))
    err = max(maxabs(ren._debug_raw.reshape(-1, 21), g["raw_out"]), maxabs(out, g["yolo_out"])) / scale
    report("yolo_c3_rel", err)
    assert err <= YOLO_TOL


# --------------------------------------------------------------------------- full frame, determinism, launch independence
def c2_frame():
    """BASELINE config 2 size (128 x 128, 3 views, 64 + 32 (16) samples) as in test_full_frame_properties."""
    NS, H, W = 3, 128, 128
    net = make_model(pconf.default_mv()["model"]).eval()
    load_mlp(net.mlp_coarse, 71, 512, 4)
    load_mlp(net.mlp_fine, 72, 512, 4)
    net = net.to(DEV)
    src, tgt = synth.scene_cameras(NS)
    lat = torch.from_numpy(synth.latent(73, NS, 512, H // 2, W // 2))
    focal, c = torch.tensor(131.25), torch.tensor([[64.0, 64.0]])
    net.encode(torch.zeros(1, NS, 3, H, W), torch.from_numpy(src)[None], focal, c=c, latent=lat)
    rays = gen_rays(dt(tgt)[None], W, H, focal, 0.8, 1.8, c=c[0]).reshape(1, -1, 8)
    ren = NeRFRenderer(n_coarse=64, n_fine=32, n_fine_depth=16, white_bkgd=True).eval()
    n = rays.shape[1]
    rs = np.random.RandomState(11)
    draws = dict(u_coarse=rs.rand(n, 64).astype(np.float32), u_fine=rs.rand(n, 16).astype(np.float32),
                 u_fine2=rs.rand(n, 16).astype(np.float32), g_depth=rs.randn(n, 16).astype(np.float32))
    return net, ren, rays, draws


def render_with(ren, net, rays, draws):
    ren.draws = {k: torch.from_numpy(v) for k, v in draws.items()}
    with torch.no_grad():
        return ren(net, rays.contiguous())


def test_full_frame_psnr_and_ragged_chunks(monkeypatch):
    set_env(monkeypatch, "auto")
    net, ren, rays, draws = c2_frame()
    ref = render_with(ren, net, rays, draws)["fine"]["rgb"][0]
    net.set_matrix_precision("f16")
    whole = render_with(ren, net, rays, draws)
    assert net.last_launch_precision() == "f16"
    rgb = whole["fine"]["rgb"][0]
    mse = float(((rgb - ref) ** 2).mean())
    psnr = 10.0 * np.log10(1.0 / mse)
    report("frame_psnr", psnr)
    report("frame_max_abs_rgb", float((rgb - ref).abs().max()))
    assert psnr >= FRAME_PSNR_MIN
    # the same frame in three ragged chunks (sizes that are not multiples of the 64-sample tile): bit for bit
    n = rays.shape[1]
    cuts = [0, 1237, 1237 + 9001, n]
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        o = render_with(ren, net, rays[:, a:b], {k: v[a:b] for k, v in draws.items()})
        parts.append(o)
    for part in ("coarse", "fine"):
        for key in ("rgb", "depth"):
            joined = torch.cat([p[part][key][0] for p in parts], 0)
            assert torch.equal(joined, whole[part][key][0]), (part, key)


def test_stress_deterministic(golden, monkeypatch):
    """200 000 jittered points: bit-identical over three runs (as test_f16x2_stress_deterministic_and_close_to_f32)."""
    set_env(monkeypatch)
    g = golden("nerf_c2")
    rng = np.random.default_rng(5)
    n = 200_000
    idx = rng.integers(0, g["probe_xyz"].shape[0], n)
    jitter = rng.normal(0.0, 0.02, (n, 3)).astype(np.float32)
    xyz, vd = dt(g["probe_xyz"][idx] + jitter)[None], dt(g["probe_viewdirs"][idx])[None]
    net = nerf_net(g, 7)
    with torch.no_grad():
        runs = [net(xyz, coarse=False, viewdirs=vd)[0] for _ in range(3)]
    assert net.last_launch_precision() == "f16"
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    assert bool(torch.isfinite(runs[0]).all())


# --------------------------------------------------------------------------- non-interference
def small_train_net(prec, seed=900, ns=2, H=32, W=32):
    c = pconf.default_mv()
    net = make_model(c["model"], stop_encoder_grad=True)
    load_mlp(net.mlp_coarse, seed + 1, 512, 4)
    load_mlp(net.mlp_fine, seed + 2, 512, 4)
    net = net.to(DEV).train()
    net.set_matrix_precision(prec)
    poses, tgt = synth.scene_cameras(ns)
    lat = torch.from_numpy(synth.latent(seed + 3, ns, 512, H // 2, W // 2)).to(DEV).requires_grad_(True)
    net.encode(torch.zeros(1, ns, 3, H, W), torch.from_numpy(poses)[None], torch.tensor(0.9 * W), latent=lat)
    return net, lat, tgt


def test_training_step_gradients_equal_auto():
    """F16 changes no training arithmetic: the parameter gradients of one render + backward are bit-identical to an AUTO
    scene's.  The latent gradient is the one output summed with float atomics (csrc/latent_grad.hip): not even two AUTO
    passes agree bit for bit, so it is held to the run-to-run bound of test_latent_gradient_run_to_run_spread (1e-5 of its
    max)."""
    grads = {}
    for prec in ("auto", "f16"):
        net, lat, tgt = small_train_net(prec)
        H = W = 32
        rays = gen_rays(dt(tgt)[None], W, H, torch.tensor(0.9 * W), 0.8, 1.8).reshape(1, -1, 8)[:, :512].contiguous()
        ren = NeRFRenderer(n_coarse=32, n_fine=16, n_fine_depth=8, white_bkgd=True).train()
        rs = np.random.RandomState(3)
        ren.draws = dict(u_coarse=torch.from_numpy(rs.rand(512, 32).astype(np.float32)),
                         u_fine=torch.from_numpy(rs.rand(512, 8).astype(np.float32)),
                         u_fine2=torch.from_numpy(rs.rand(512, 8).astype(np.float32)),
                         g_depth=torch.from_numpy(rs.randn(512, 8).astype(np.float32)))
        out = ren(net, rays, want_weights=True)
        gt = torch.full_like(out["fine"]["rgb"], 0.5)
        loss = torch.nn.functional.mse_loss(out["coarse"]["rgb"], gt) + torch.nn.functional.mse_loss(out["fine"]["rgb"], gt)
        loss.backward()
        torch.cuda.synchronize()
        g = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None and k.startswith("mlp_")}
        g["latent"] = lat.grad.detach().clone()
        grads[prec] = g
    assert len(grads["auto"]) > 10 and grads["auto"].keys() == grads["f16"].keys()
    la, lf = grads["auto"].pop("latent"), grads["f16"].pop("latent")
    scale = float(la.abs().max())
    assert scale > 0 and float((la - lf).abs().max()) <= 1e-5 * scale
    for k in grads["auto"]:
        assert torch.equal(grads["auto"][k], grads["f16"][k]), k


def test_switching_keeps_the_projection_and_equals_fresh_scenes(golden, monkeypatch):
    set_env(monkeypatch, "auto")
    g = golden("nerf_c2")
    xyz, vd = dt(g["probe_xyz"])[None], dt(g["probe_viewdirs"])[None]

    def run(net):
        with torch.no_grad():
            return net(xyz, coarse=False, viewdirs=vd)[0].clone()

    net = nerf_net(g, 7)
    seq = []
    for prec in ("f16", "auto", "f16"):
        net.set_matrix_precision(prec)
        seq.append(run(net))
        assert net.last_launch_precision() == ("f16" if prec == "f16" else "f16x2")
    fresh = {}
    for prec in ("f16", "auto"):
        set_env(monkeypatch, prec)
        fresh[prec] = run(nerf_net(g, 7))
    assert torch.equal(seq[0], fresh["f16"]) and torch.equal(seq[2], fresh["f16"]) and torch.equal(seq[1], fresh["auto"])
    assert not torch.equal(seq[0], seq[1])


def test_refresh_after_optimizer_step_equals_fresh_model(golden, monkeypatch):
    """After an optimizer step (device-side pny_model_refresh, which repacks the single-plane images too) an F16 render
    equals, bit for bit, a freshly built model holding the stepped weights."""
    set_env(monkeypatch)
    g = golden("nerf_c2")
    xyz, vd = dt(g["probe_xyz"])[None], dt(g["probe_viewdirs"])[None]
    net = nerf_net(g, 7)
    with torch.no_grad():
        before = net(xyz, coarse=False, viewdirs=vd)[0].clone()
    opt = torch.optim.Adam([p for k, p in net.named_parameters() if k.startswith("mlp_")], lr=1e-3)
    for p in opt.param_groups[0]["params"]:
        p.grad = torch.randn_like(p) * 1e-2
    opt.step()
    with torch.no_grad():
        after = net(xyz, coarse=False, viewdirs=vd)[0].clone()
    assert net.last_launch_precision() == "f16" and not torch.equal(before, after)
    fresh = nerf_net(g, 7)
    with torch.no_grad():
        fresh.load_state_dict(net.state_dict(), strict=False)
        out = fresh(xyz, coarse=False, viewdirs=vd)[0]
    assert fresh.last_launch_precision() == "f16"
    assert torch.equal(out, after)


# --------------------------------------------------------------------------- range guard (construction of test_gpu_range.py)
def range_net(seed, policy):
    c = pconf.default_mv()
    net = make_model(c["model"], stop_encoder_grad=True)
    for mlp, sd in ((net.mlp_coarse, synth.mlp_state(seed + 1)), (net.mlp_fine, synth.mlp_state(seed + 2))):
        sd = {k: torch.from_numpy(v) for k, v in sd.items()}
        sd["lin_in.weight"] = sd["lin_in.weight"] * 2000.0
        mlp.load_state_dict(sd)
    net = net.to(DEV).eval()
    net.f16_range_policy = policy
    net.set_matrix_precision("f16")
    ns, H, W = 2, 32, 32
    poses, _ = synth.scene_cameras(ns)
    lat = synth.latent(seed + 3, ns, 512, H // 2, W // 2)
    net.encode(torch.zeros(1, ns, 3, H, W), torch.from_numpy(poses)[None], torch.tensor(0.9 * W), latent=torch.from_numpy(lat))
    return net


@pytest.mark.parametrize("policy", ["relaunch", "raise"])
def test_activation_overflow(policy):
    """relu(lin_in(x)) of a few 1e5 (in-range inputs and weights): 'relaunch' repeats the call on fp32 with a warning that
    names f16 -- the fp32 kernels' numbers --, 'raise' raises PnyRangeError."""
    rs = np.random.RandomState(2)
    xyz = dt(rs.uniform(-0.5, 0.5, size=(1, 200, 3)).astype(np.float32)) * 40.0
    vd = dt(rs.standard_normal((1, 200, 3)).astype(np.float32))
    net = range_net(200, policy)
    if policy == "raise":
        with torch.no_grad(), pytest.raises(plib.PnyRangeError, match="f16"):
            net(xyz, coarse=True, viewdirs=vd)
        return
    with torch.no_grad(), pytest.warns(UserWarning, match="f16 .*outside the f16 range"):
        out = net(xyz, coarse=True, viewdirs=vd)
    assert net.last_launch_precision() == "f32" and net.range_status() == 0
    ref = range_net(200, policy).set_matrix_precision("f32")
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("error")
        want = ref(xyz, coarse=True, viewdirs=vd)
    assert torch.equal(out, want)


# --------------------------------------------------------------------------- replicas
def test_bind_parallel_replicas_render_f16(golden, monkeypatch):
    set_env(monkeypatch, "auto")
    g = golden("nerf_c2")
    net = nerf_net(g, 7).set_matrix_precision("f16")
    ren = NeRFRenderer(n_coarse=64, n_fine=32, n_fine_depth=16, depth_std=0.01, white_bkgd=True).eval()
    draws = {k: g[k] for k in ("u_coarse", "u_fine", "u_fine2", "g_depth")}
    rays = dt(g["rays"])[None]
    ren.draws = draws
    with torch.no_grad():
        one = ren.bind_parallel(net)(rays)
    assert net.last_launch_precision() == "f16"
    par = ren.bind_parallel(net, [0, 0])
    ren.draws = draws
    with torch.no_grad():
        two = par(rays)
    reps = [r for r in par._replicas if r is not None] if hasattr(par, "_replicas") else []
    for r in reps:
        assert r._precision == "f16" and r.last_launch_precision() == "f16"
    assert torch.equal(one["fine"]["rgb"], two["fine"]["rgb"]) and torch.equal(one["coarse"]["depth"], two["coarse"]["depth"])
