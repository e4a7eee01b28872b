"""
The DEFAULT source of the renderers' random draws (-m gpu, real MI355X): Philox4x32-10 evaluated inside the kernels from a
64-bit seed (csrc/pny_rng.h), against the oracle's independent restatement of the generator (oracle/pnyolo_oracle.py:
philox_uniform, philox_normal, seeded_draws; pinned on the CPU by tests/test_cpu_philox.py).

  * stage kernels through the ABI, HIP against HIP with only the source of the draw exchanged: bit equality;
  * the in-kernel Box-Muller normal against the float64 normal: NORMAL_ABS_TOL (the one bar of this module that is not inherited);
  * full renders, seeded on the HIP side, against the oracle fed seeded_draws of the seed render.py documents -- at the bars of
    test_gpu_parity.check_render / test_yolo_render_golden;
  * seeded backward against torch.autograd through the oracle on the same draws -- at the bars of test_gpu_backward
    (helpers.RTOL / grad_check), and the number of depth samples the backward locates against the oracle's count.

A draw depends on its ray's index in the launch, so the gradient comparisons cannot leave relu-ambiguous rays out of the launch
(helpers.clean_rays): every candidate is rendered on both sides and the ambiguous ones get zero loss weight.
"""
import numpy as np
import pytest
import torch

import pnyolo_oracle as orc
from helpers import DEV, SEEDED_BWD, compare_param_grads, dt, grad_check, maxabs, renderer_seed, scene_pair, seeded_bwd_case
from pixel_nerf_yolo_amd import conf as pconf
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd import synth
from pixel_nerf_yolo_amd.model import make_model
from pixel_nerf_yolo_amd.render import NeRFRenderer, YoloRenderer
from test_cpu_philox import NORMAL_ABS_TOL
from test_gpu_parity import TOL, small_scene

pytestmark = pytest.mark.gpu

AMBIG = 1e-5          # as tests/test_gpu_backward.py: the fp32 reference-order training forward
SEEDS = [0, 42, 1234 + 7919, 2 ** 40 + 7, 2 ** 64 - 1]    # 1234 + 7919: NeRFRenderer's first seed; two with a non-zero high word


@pytest.fixture(autouse=True, params=["dw_f32", "dw_f16x2"])
def training_forward_arithmetic(request, monkeypatch):
    """The arithmetic legs of tests/test_gpu_backward.py (see there): the comparisons with autograd through the oracle pin the
    fp32 training forward and run under both arithmetics of the backward's matrix products.  Tests marked `one_backward_leg`
    (no MLP backward in them) run once; those marked `f16x2_forward` too keep the shipped default forward arithmetic."""
    if "f16x2_forward" not in request.keywords:
        monkeypatch.setenv("PNYOLO_MLP_PRECISION", "f32")
    monkeypatch.setenv("PNYOLO_BWD_PRECISION", "f32" if request.param == "dw_f32" else "f16x2")


forward_only = [pytest.mark.one_backward_leg, pytest.mark.f16x2_forward]


def _apply(marks):
    def deco(fn):
        for m in marks:
            fn = m(fn)
        return fn
    return deco


def _stage_rays(n, near=0.8, far=1.8):
    r = np.zeros((n, 8), dtype=np.float32)
    r[:, 5] = 1.0
    r[:, 6] = near + 0.001 * (np.arange(n) % 7)
    r[:, 7] = far + 0.002 * (np.arange(n) % 5)
    return r


def _sample_coarse(L, rays_d, n, kc, lindisp, u_d, seed):
    z = torch.full((n, kc), float("nan"), device=DEV)
    plib.check(L.pny_sample_coarse(plib.ptr(rays_d), n, kc, lindisp, plib.ptr(u_d), seed, plib.ptr(z), plib.stream_of(torch.device(DEV))))
    return z


def _sample_fine(L, rays_d, zc, w, depth, n, kc, kf, kfd, std, lindisp, u, u2, g, seed):
    zo = torch.full((n, kc + kf), float("nan"), device=DEV)
    plib.check(L.pny_sample_fine(plib.ptr(rays_d), plib.ptr(zc), plib.ptr(w), plib.ptr(depth), n, kc, kf, kfd, std, lindisp,
                                 plib.ptr(u), plib.ptr(u2), plib.ptr(g), seed, plib.ptr(zo), plib.stream_of(torch.device(DEV))))
    return zo


# --------------------------------------------------------------------------- stage kernels: bit equality
@_apply(forward_only)
def test_sample_coarse_seeded_equals_explicit_oracle_uniforms():
    """pny_sample_coarse(u = NULL, seed) against pny_sample_coarse(u = the oracle's uniforms): the same kernel, the same
    arithmetic after the draw, so the depths are equal bit for bit exactly when every uniform is."""
    L = plib.load()
    for n, kc in [(1, 1), (7, 33), (100, 64), (65, 128), (3, 2)]:      # n * kc a multiple of 4 and not
        rays_d = dt(_stage_rays(n))
        for lindisp in (0, 1):
            for seed in SEEDS:
                u = orc.seeded_draws(seed, n, kc, 0, 0)["u_coarse"]
                u_d = dt(u)
                za = _sample_coarse(L, rays_d, n, kc, lindisp, None, seed)
                zb = _sample_coarse(L, rays_d, n, kc, lindisp, u_d, seed ^ 0x5555)     # (the seed is unused with explicit draws)
                torch.cuda.synchronize()
                assert torch.equal(za, zb), (n, kc, lindisp, seed, maxabs(za, zb))
    # the jitter really is the uniform: t = (z - near) / (far - near) * kc - k reproduces it to fp32 rounding
    n, kc, seed = 100, 64, 42
    r = _stage_rays(n)
    za = _sample_coarse(L, dt(r), n, kc, 0, None, seed).cpu().double().numpy()
    t = (za - r[:, 6:7].astype(np.float64)) / (r[:, 7:8].astype(np.float64) - r[:, 6:7]) * kc - np.arange(kc)
    assert float(np.abs(t - orc.seeded_draws(seed, n, kc, 0, 0)["u_coarse"]).max()) < 1e-4


@_apply(forward_only)
def test_sample_fine_importance_seeded_equals_explicit_oracle_uniforms():
    """pny_sample_fine with n_fine_depth = 0: streams FINE / FINE2 at ray * (kf - kfd) + i, on a sharp peak, uniform weights
    and all-zero weights (cdf = uniform through the 1e-5 floor)."""
    L = plib.load()
    rs = np.random.RandomState(4)
    for n, kc, kf in [(65, 64, 32), (7, 33, 31), (1, 16, 1)]:
        r = _stage_rays(n)
        rays_d = dt(r)
        zc = _sample_coarse(L, rays_d, n, kc, 0, dt(rs.rand(n, kc).astype(np.float32)), 0)
        peak = np.full((n, kc), 1e-4, dtype=np.float32)
        peak[np.arange(n), rs.randint(0, kc, n)] = 0.9
        depth = dt(np.full(n, 1.3, dtype=np.float32))
        for w in (peak, np.full((n, kc), 1.0 / kc, dtype=np.float32), np.zeros((n, kc), dtype=np.float32)):
            w_d = dt(w)
            for lindisp in (0, 1):
                for seed in SEEDS:
                    d = orc.seeded_draws(seed, n, kc, kf, 0)
                    u, u2 = dt(d["u_fine"]), dt(d["u_fine2"])
                    za = _sample_fine(L, rays_d, zc, w_d, depth, n, kc, kf, 0, 0.01, lindisp, None, None, None, seed)
                    zb = _sample_fine(L, rays_d, zc, w_d, depth, n, kc, kf, 0, 0.01, lindisp, u, u2, None, seed ^ 0x5555)
                    torch.cuda.synchronize()
                    assert torch.equal(za, zb), (n, kc, kf, lindisp, seed, maxabs(za, zb))
                    # exchanging the two streams is visible (the comparison would notice u_fine2 == u_fine)
                    if kf > 1 and w is peak and lindisp == 0 and seed == 42:
                        zs = _sample_fine(L, rays_d, zc, w_d, depth, n, kc, kf, 0, 0.01, 0, u, u, None, 0)
                        assert not torch.equal(za, zs)


@_apply(forward_only)
def test_in_kernel_normals_against_float64():
    """pny_sample_fine with n_fine == n_fine_depth read as a normal generator: one coarse depth far below, depth = 0,
    depth_std = 1, near = -8, far = 8 (|g| <= sqrt(2 * 24 * ln 2) = 5.77: nothing clamps, and 0 + g * 1 is exact), so the sorted
    output is the sorted normals of stream DEPTH at ray * kfd + i.  Against the sorted float64 Box-Muller normals of the oracle
    (never against another run of the kernel), 2^16 normals per seed: |g_kernel - g_float64| <= NORMAL_ABS_TOL = 1e-5 (error
    analysis in tests/test_cpu_philox.py), and sample mean / variance against the oracle's own sample at the same bound.
    Measured on the MI355X (5 seeds x 65536 normals): max |g_kernel - g_float64| = 1.6e-6."""
    L = plib.load()
    n, kfd = 1024, 64
    r = np.zeros((n, 8), dtype=np.float32)
    r[:, 5], r[:, 6], r[:, 7] = 1.0, -8.0, 8.0
    rays_d = dt(r)
    zc, w, depth = dt(np.full((n, 1), -100.0, dtype=np.float32)), dt(np.ones((n, 1), dtype=np.float32)), dt(np.zeros(n, dtype=np.float32))
    worst = 0.0
    for seed in SEEDS:
        zo = _sample_fine(L, rays_d, zc, w, depth, n, 1, kfd, kfd, 1.0, 0, None, None, None, seed)
        torch.cuda.synchronize()
        zo = zo.cpu().double().numpy()
        assert np.all(zo[:, 0] == -100.0)
        g = zo[:, 1:]
        g64, g32 = orc.philox_normal(seed, orc.STREAM_DEPTH, np.arange(n * kfd).reshape(n, kfd))
        assert float(np.abs(g).max()) < 8.0                                        # nothing clamped
        err = float(np.abs(g - np.sort(g64, axis=1)).max())
        worst = max(worst, err)
        print("seed %d: max |g_kernel - g_float64| = %.3e (%d normals), mean %.6f var %.6f" % (seed, err, g.size, g.mean(), g.var()))
        assert err <= NORMAL_ABS_TOL, (seed, err)
        assert abs(g.mean() - g64.mean()) <= NORMAL_ABS_TOL and abs(g.var() - g64.var()) <= NORMAL_ABS_TOL, (seed, g.mean(), g64.mean(), g.var(), g64.var())
        # and the explicit path on the oracle's fp32 normals gives the same depths to the same bound (both are g * 1 exactly)
        zb = _sample_fine(L, rays_d, zc, w, depth, n, 1, kfd, kfd, 1.0, 0, None, None, dt(g32), 0)
        assert float(np.abs(zb.cpu().double().numpy() - zo).max()) <= NORMAL_ABS_TOL
    print("max |g_kernel - g_float64| over %d seeds: %.3e" % (len(SEEDS), worst))


@_apply(forward_only)
def test_sample_fine_mixed_seeded_against_explicit_oracle_draws():
    """kf > kfd > 0, depth_std = 0.01: seeded against explicit-from-oracle.  The importance samples are equal bit for bit; a depth
    sample is depth + g * 0.01 with |g - g_oracle| <= NORMAL_ABS_TOL, so the bar is depth_std * NORMAL_ABS_TOL = 1e-7 -- which
    is below one fp32 ulp of a depth in [1, 2), and the sum is rounded once on either side.  The rays of this case therefore
    live in (0.1, 0.45): one ulp of the sum is 3e-8 there and the bar is a bar on the draw."""
    L = plib.load()
    rs = np.random.RandomState(6)
    std = 0.01
    for n, kc, kf, kfd in [(100, 64, 32, 16), (65, 33, 31, 7), (9, 16, 8, 4)]:
        r = _stage_rays(n, near=0.1, far=0.45)
        rays_d = dt(r)
        zc = _sample_coarse(L, rays_d, n, kc, 0, dt(rs.rand(n, kc).astype(np.float32)), 0)
        w_d = dt(rs.rand(n, kc).astype(np.float32) ** 4)
        depth = dt(rs.uniform(0.15, 0.4, n).astype(np.float32))
        depth[0], depth[-1] = float(r[0, 6]) + 1e-4, float(r[-1, 7]) - 1e-4          # some depth samples clamp to near / far
        for seed in SEEDS:
            d = orc.seeded_draws(seed, n, kc, kf, kfd)
            za = _sample_fine(L, rays_d, zc, w_d, depth, n, kc, kf, kfd, std, 0, None, None, None, seed)
            zb = _sample_fine(L, rays_d, zc, w_d, depth, n, kc, kf, kfd, std, 0, dt(d["u_fine"]), dt(d["u_fine2"]), dt(d["g_depth"]), 0)
            torch.cuda.synchronize()
            assert bool((za[:, 1:] >= za[:, :-1]).all())
            assert maxabs(za, zb) <= std * NORMAL_ABS_TOL, (n, kc, kf, kfd, seed, maxabs(za, zb))
            # with the depth draws exchanged for explicit ones, the rest is bit-equal (the importance streams at kimp = kf - kfd)
            zc_ = _sample_fine(L, rays_d, zc, w_d, depth, n, kc, kf, kfd, std, 0, None, None, dt(d["g_depth"]), seed)
            assert torch.equal(zc_, zb)


# --------------------------------------------------------------------------- full renders, forward
def check_seeded_render(ren, net, sc, rays, seed, max_flips=2):
    """test_gpu_parity.check_render with the draws generated in the kernels from `seed` on the HIP side and restated by the
    oracle on the other: TOL on the coarse pass, at most max_flips rays per call over TOL in the fine pass."""
    n = rays.shape[0]
    kc, kf, kfd = int(ren.n_coarse), int(ren.n_fine), int(ren.n_fine_depth)
    assert ren.draws is None and renderer_seed(ren) == seed
    with torch.no_grad():
        out = ren(net, dt(rays)[None], want_weights=True)
    dr = orc.seeded_draws(seed, n, kc, kf, kfd)
    ref = orc.render(sc, rays, kc, kf, kfd, dr["u_coarse"], dr["u_fine"], dr["u_fine2"], dr["g_depth"], depth_std=float(ren.depth_std),
                     white_bkgd=bool(ren.white_bkgd), lindisp=bool(ren.lindisp))
    compare_render(out, ref, 0, n, kc, kf, max_flips)
    return out


def compare_render(out, ref, sb, n, kc, kf, max_flips=2, lo=0):
    for k in ("rgb", "depth", "weights"):
        assert maxabs(out["coarse"][k][sb][lo:lo + n], ref["coarse"][k].detach()) < TOL, k
    if kf > 0:
        diff = (out["fine"]["rgb"][sb][lo:lo + n].detach().cpu() - ref["fine"]["rgb"].detach()).abs().max(dim=1)[0]
        assert int((diff > TOL).sum()) <= max_flips, (int((diff > TOL).sum()), float(diff.max()))
        assert out["fine"]["weights"].shape[-1] == kc + kf
    else:
        assert "fine" not in out


@_apply(forward_only)
@pytest.mark.parametrize("kc,kf,kfd,lindisp,n", [(16, 8, 4, False, 90), (16, 8, 0, False, 90), (16, 8, 8, False, 90), (64, 32, 16, False, 90),
                                                 (33, 31, 7, False, 90), (16, 8, 4, True, 90), (16, 8, 4, False, 1), (16, 8, 4, False, 65),
                                                 (24, 0, 0, False, 65)])
def test_seeded_eval_render_vs_oracle(kc, kf, kfd, lindisp, n):
    net, sc, rays = small_scene()
    sub = rays[torch.arange(0, rays.shape[0], 11)[:n]]
    ren = NeRFRenderer(n_coarse=kc, n_fine=kf, n_fine_depth=kfd, white_bkgd=True, lindisp=lindisp).eval()
    check_seeded_render(ren, net, sc, sub, 1234 + 7919)


@_apply(forward_only)
def test_seeded_render_seed_schedule_over_calls():
    """base_seed + 7919 * (number of the call, from 1): two consecutive calls of one renderer, then base_seed changed by the
    user, then an explicit-draw call in between (it counts as a call)."""
    net, sc, rays = small_scene()
    sub = rays[torch.arange(5, rays.shape[0], 13)[:70]]
    ren = NeRFRenderer(n_coarse=16, n_fine=8, n_fine_depth=4, white_bkgd=True).eval()
    o1 = check_seeded_render(ren, net, sc, sub, 1234 + 7919)
    o2 = check_seeded_render(ren, net, sc, sub, 1234 + 7919 * 2)
    assert not torch.equal(o1["coarse"]["depth"], o2["coarse"]["depth"])
    ren.base_seed = 2 ** 40 + 7          # a seed with a non-zero high word through the whole render path
    check_seeded_render(ren, net, sc, sub, 2 ** 40 + 7 + 7919 * 3)
    ren.draws = orc.seeded_draws(5, 70, 16, 8, 4)
    with torch.no_grad():
        ren(net, dt(sub)[None])
    check_seeded_render(ren, net, sc, sub, 2 ** 40 + 7 + 7919 * 5)
    ren.base_seed = 2 ** 64 - 1          # wraps modulo 2^64
    check_seeded_render(ren, net, sc, sub, (2 ** 64 - 1 + 7919 * 6) % 2 ** 64)


@_apply(forward_only)
@pytest.mark.parametrize("form", ["group", "per_object"])
def test_seeded_super_batch_forms(form, monkeypatch):
    """SB = 2 training renders (the forms are selected as in test_render_backward_super_batch).  Grouped: ONE launch over the
    SB * B rays on one seed, a ray's draws at its global index sb * B + b.  Per object: one launch per object on seed + sb,
    rays numbered from 0."""
    monkeypatch.setenv("PNYOLO_GROUP", "1" if form == "group" else "0")
    SB, ns, H, W, kc, kf, kfd, B = 2, 2, 32, 32, 16, 8, 4, 32
    net = make_model(pconf.default_mv()["model"], stop_encoder_grad=True)
    sd_c, sd_f = synth.mlp_state(2301), synth.mlp_state(2302)
    net.mlp_coarse.load_state_dict({k: torch.from_numpy(v) for k, v in sd_c.items()})
    net.mlp_fine.load_state_dict({k: torch.from_numpy(v) for k, v in sd_f.items()})
    net = net.to(DEV).train()
    lat = np.concatenate([synth.latent(2310 + i, ns, 512, H // 2, W // 2) for i in range(SB)])
    poses = np.stack([synth.scene_cameras(ns, radius=1.3 + 0.1 * i)[0] for i in range(SB)])
    focal = torch.tensor([[28.0, 28.0], [30.0, 31.0]])
    net.encode(torch.zeros(SB, ns, 3, H, W), torch.from_numpy(poses), focal, latent=torch.from_numpy(lat))
    rays = torch.stack([orc.gen_rays(synth.pose_spherical(100.0 + 25 * i, -20.0, 1.3)[None], W, H, 29.0, 0.8, 1.8)[0].reshape(-1, 8)[3::31][:B]
                        for i in range(SB)])
    ren = NeRFRenderer(n_coarse=kc, n_fine=kf, n_fine_depth=kfd, white_bkgd=True).train()
    seed = renderer_seed(ren)
    assert seed == 1234 + 7919
    out = ren(net, rays.to(DEV), want_weights=True)
    assert out["fine"]["rgb"].requires_grad and net._last_call_group == (form == "group")
    (out["coarse"]["rgb"].sum() + out["fine"]["rgb"].sum()).backward()      # (releases the forward's stash reservation)
    grouped = orc.seeded_draws(seed, SB * B, kc, kf, kfd)
    for i in range(SB):
        sc = orc.Scene(sd_c, sd_f, lat[i * ns:(i + 1) * ns], poses[i], focal[i:i + 1], None, W, H)
        d = {k: v[i * B:(i + 1) * B] for k, v in grouped.items()} if form == "group" else orc.seeded_draws(seed + i, B, kc, kf, kfd)
        with torch.no_grad():
            ref = orc.render(sc, rays[i], kc, kf, kfd, d["u_coarse"], d["u_fine"], d["u_fine2"], d["g_depth"])
        compare_render(out, ref, i, B, kc, kf)


@_apply(forward_only)
def test_seeded_bind_parallel_ranges_have_their_own_seeds():
    """bind_parallel(net, [0, 0]) in eval: the rays split into one contiguous range per device (whole 64-ray groups), range i
    rendered on the seed of call number _calls + i + 1 with its rays numbered from 0; the call counts as len(gpus) calls."""
    net, sc, rays = small_scene()
    sub = rays[torch.arange(0, rays.shape[0], 7)[:150]]
    kc, kf, kfd = 16, 8, 4
    ren = NeRFRenderer(n_coarse=kc, n_fine=kf, n_fine_depth=kfd, white_bkgd=True).eval()
    par = ren.bind_parallel(net, [0, 0])
    for call in range(2):
        seeds = [renderer_seed(ren, 1), renderer_seed(ren, 2)]
        assert seeds == [1234 + 7919 * (2 * call + 1), 1234 + 7919 * (2 * call + 2)]
        with torch.no_grad():
            out = par(dt(sub)[None], want_weights=True)
        assert ren._calls == 2 * (call + 1)
        for (lo, hi), seed in zip([(0, 128), (128, 150)], seeds):
            d = orc.seeded_draws(seed, hi - lo, kc, kf, kfd)
            ref = orc.render(sc, sub[lo:hi], kc, kf, kfd, d["u_coarse"], d["u_fine"], d["u_fine2"], d["g_depth"])
            compare_render(out, ref, 0, hi - lo, kc, kf, lo=lo)


def _yolo_case(with_net=True):
    net, sc = scene_pair(2, 64, 64, 1792, 21, 5, 3, 1500, yolo=True, lat_hw=(8, 8), with_net=with_net)
    _, tgt_c2w = synth.scene_cameras(2, radius=4.0, phi=-25.0)
    flipyz = np.diag([1.0, -1.0, -1.0, 1.0]).astype(np.float32)
    tgt_w2c = np.linalg.inv(tgt_c2w @ flipyz).astype(np.float32)
    rays = orc.gen_rays_yolo(tgt_w2c[None], 16, 12, [5.0, 5.5], [8.0, 6.0], 1.0, 6.0)[0].reshape(-1, 8)
    return net, sc, rays


@_apply(forward_only)
def test_seeded_yolo_render_vs_oracle():
    """YoloRenderer (base_seed 4321) without explicit draws against orc.yolo_render on the oracle's coarse uniforms: raw vectors
    and aggregated output at the bars of test_yolo_render_golden (TOL x max(1, max |raw|)), two consecutive calls."""
    net, sc, rays = _yolo_case()
    net.eval()
    K, n = 32, rays.shape[0]
    ren = YoloRenderer(K, 128, 1, 3)
    ren.bind_parallel(net)
    for call in (1, 2):
        seed = renderer_seed(ren)
        assert seed == 4321 + 7919 * call
        ren._debug_raw = torch.empty(n, K, 21, device=DEV)
        with torch.no_grad():
            out = ren(rays[None].to(DEV))
            ref = orc.yolo_render(sc, rays, K, orc.seeded_draws(seed, n, K, 0, 0)["u_coarse"])
        torch.cuda.synchronize()
        scale = max(1.0, float(ref["raw"].abs().max()))
        assert maxabs(ren._debug_raw, ref["raw"]) < TOL * scale
        assert out.shape == (n, 3, 7) and maxabs(out, ref["out"]) < TOL * scale


# --------------------------------------------------------------------------- seeded backward
def _weighted_loss(res, gt, weight):
    """The trainer's loss (MSE on both passes' rgb) plus depth terms (as helpers.render_loss with_depth), every ray's terms
    multiplied by its weight in {0, 1}."""
    w = weight[:, None]
    s = weight.sum()
    loss = ((res["coarse"]["rgb"] - gt).square() * w).sum() / (3 * s) + ((res["fine"]["rgb"] - gt).square() * w).sum() / (3 * s)
    return loss + 0.1 * (res["fine"]["depth"] * weight).sum() / s + 0.05 * (res["coarse"]["depth"].square() * weight).sum() / s


def _located(net, n, kfd):
    """sel of the last pny_render_backward on scene 0 (pny_scene_last_depth_sel): (n, kfd) int32 on the CPU."""
    sel = torch.full((n, kfd), -7, dtype=torch.int32, device=DEV)
    plib.check(plib.load().pny_scene_last_depth_sel(net._scene(0), plib.C.c_void_p(sel.data_ptr()), n * kfd, plib.stream_of(torch.device(DEV))))
    torch.cuda.synchronize()
    return sel.cpu()


def _inside_mask(ref, rays, g_depth, std):
    """(inside, robust): which depth samples the oracle places strictly inside (near, far), and for which of them the answer
    does not hinge on rounding -- the unclamped position is further than TOL (the bar the two sides' coarse depths are held to)
    from both bounds.  The few others (asserted: under 1 %) are left out of the comparison."""
    zd = ref["coarse"]["depth"].detach().double()[:, None] + torch.from_numpy(np.asarray(g_depth)).double() * std
    near, far = rays[:, 6:7].double(), rays[:, 7:8].double()
    robust = torch.minimum((zd - near).abs(), (zd - far).abs()) > TOL
    assert int((~robust).sum()) * 100 < robust.numel()
    return (zd > near) & (zd < far), robust


@pytest.mark.parametrize("mode", ["stash", "chunks"])
def test_seeded_render_backward_vs_oracle(mode, monkeypatch):
    """NeRFRenderer.train() without explicit draws, n_fine_depth > 0, depth samples attached (the reference's graph): gradients
    of both MLPs and of the latent against autograd through the oracle on seeded_draws of the renderer's seed, bars as
    test_render_backward_vs_oracle / test_latent_gradient_vs_oracle_autograd.  All 96 candidate rays are rendered; the rays with a
    relu input within AMBIG carry zero loss weight (helpers.seeded_bwd_case; precondition checked on the CPU in
    test_cpu_philox.py).  "chunks": a stash budget of ~4 tiles -- no reservation, the backward recomputes the seeded forward
    and walks the rays in chunks (as test_backward_recompute_in_chunks).  Also: every depth sample that the oracle puts strictly
    inside (near, far) is located by the backward (sel >= 0) and every clamped one is not."""
    if mode == "chunks":
        monkeypatch.setenv("PNYOLO_STASH_GB", "0.03")
    c = SEEDED_BWD
    kc, kf, kfd, n = c["kc"], c["kf"], c["kfd"], c["n"]
    net, sc, rays, draws, weight, seed = seeded_bwd_case(with_net=True, lat_grad=True)
    assert int(weight.sum()) >= 48 and 2 * int(weight.sum()) >= n
    ren = NeRFRenderer(n_coarse=kc, n_fine=kf, n_fine_depth=kfd, white_bkgd=True).train()
    ren.base_seed = c["base_seed"]
    assert renderer_seed(ren) == seed and ren.draws is None
    gt = torch.from_numpy(np.random.RandomState(8).uniform(0, 1, size=(n, 3)).astype(np.float32))
    out = ren(net, rays[None].to(DEV), want_weights=True)
    assert out["fine"]["rgb"].requires_grad
    assert out["coarse"]["rgb"].grad_fn.deferred == (mode == "stash")
    hip = {p: {k: v[0] for k, v in out[p].items()} for p in ("coarse", "fine")}
    _weighted_loss(hip, gt.to(DEV), weight.to(DEV)).backward()
    ref = orc.render(sc, rays, kc, kf, kfd, draws["u_coarse"], draws["u_fine"], draws["u_fine2"], draws["g_depth"])
    compare_render(out, ref, 0, n, kc, kf)
    clean = weight.bool()
    assert maxabs(out["fine"]["rgb"][0].cpu()[clean], ref["fine"]["rgb"].detach()[clean]) < 1e-4
    inside, robust = _inside_mask(ref, rays, draws["g_depth"], 0.01)
    assert int(inside.sum()) > n * kfd // 2
    sel = _located(net, n, kfd)
    assert torch.equal((sel >= 0)[robust], inside[robust]), "located %d depth samples, the oracle has %d inside (near, far)" % (
        int((sel >= 0)[robust].sum()), int(inside[robust].sum()))
    _weighted_loss(ref, gt, weight).backward()
    assert float(sc.latent.grad.abs().max()) > 0
    grad_check("latent", net.test_latent.grad, sc.latent.grad)
    compare_param_grads(net, sc)


@pytest.mark.one_backward_leg
def test_backward_locates_every_unclamped_depth_sample():
    """The backward re-creates the forward's depth draws (normal_at is compiled into render_kernels.hip and into mlp_bwd.hip) and
    finds each sample in the sorted fine depths by float equality: a last-bit difference between the two compilations would
    drop that sample's gradient silently.  Independent of tolerances: over 300 rays x 16 depth samples, three seeds (one with a
    non-zero high word), near = 0.8 so that many samples clamp, the located set equals the oracle's set of samples strictly
    inside (near, far), and each located position holds that sample's depth.  One leg: no matrix arithmetic is involved."""
    kc, kf, kfd, n = 16, 24, 16, 300
    net, sc = scene_pair(2, 32, 32, 512, 4, 5, 3, 2400)
    _, tgt = synth.scene_cameras(2)
    rays = orc.gen_rays(tgt[None], 32, 32, 0.9 * 32, 0.8, 1.8)[0].reshape(-1, 8)[2::3][:n]
    ren = NeRFRenderer(n_coarse=kc, n_fine=kf, n_fine_depth=kfd, white_bkgd=True, depth_std=0.05).train()
    for base in (1234, 2 ** 40 + 7, 99):
        ren.base_seed = base
        seed = renderer_seed(ren)
        z_fine = torch.empty(1, n, kc + kf, device=DEV)
        ren._debug_out = {"z_fine": z_fine}
        out = ren(net, rays[None].to(DEV))
        ren._debug_out = None
        out["fine"]["rgb"].sum().backward()
        d = orc.seeded_draws(seed, n, kc, kf, kfd)
        with torch.no_grad():
            ref = orc.render(sc, rays, kc, kf, kfd, d["u_coarse"], d["u_fine"], d["u_fine2"], d["g_depth"], depth_std=0.05)
        inside, robust = _inside_mask(ref, rays, d["g_depth"], 0.05)
        sel = _located(net, n, kfd)
        n_in = int(inside.sum())
        assert 0.2 * n * kfd < n_in < 0.95 * n * kfd, n_in             # both kinds are present
        assert torch.equal((sel >= 0)[robust], inside[robust]), "seed %d: located %d depth samples, the oracle has %d inside (near, far)" % (
            seed, int((sel >= 0)[robust].sum()), int(inside[robust].sum()))
        both = inside & robust
        zd = ref["coarse"]["depth"][:, None] + torch.from_numpy(d["g_depth"]) * 0.05
        got = z_fine[0].cpu().reshape(-1)[sel[both].long()]
        assert (sel[both] // (kc + kf) == torch.arange(n)[:, None].expand(n, kfd)[both]).all()
        assert float((got - zd[both]).abs().max()) < TOL


def test_seeded_yolo_render_backward_vs_oracle():
    """YoloRenderer under autograd without explicit draws: pny_yolo_render_backward re-derives the sample depths from the seed.
    All 192 candidate rays in the launch; rays with a relu input within AMBIG get a zero output gradient.  Bars as
    test_yolo_render_backward_vs_oracle."""
    net, sc, rays = _yolo_case()
    K, n = 8, rays.shape[0]
    ren = YoloRenderer(K, 128, 1, 3)
    ren.bind_parallel(net)
    seed = renderer_seed(ren)
    assert seed == 4321 + 7919
    u = orc.seeded_draws(seed, n, K, 0, 0)["u_coarse"]
    orc.RELU_TRACE = []
    with torch.no_grad():
        orc.yolo_render(sc, rays, K, u)
    ok = torch.ones(n, dtype=torch.bool)
    for t in orc.RELU_TRACE:
        ok &= t.reshape(n, -1).min(dim=1)[0] >= AMBIG
    orc.RELU_TRACE = None
    assert int(ok.sum()) >= 48 and 2 * int(ok.sum()) >= n, int(ok.sum())
    G = torch.from_numpy(np.random.RandomState(22).standard_normal((n, 3, 7)).astype(np.float32)) * ok[:, None, None].float()
    out = ren(rays[None].to(DEV))
    assert out.requires_grad and out.shape == (n, 3, 7)
    (out * G.to(DEV)).sum().backward()
    ref = orc.yolo_render(sc, rays, K, u)
    assert maxabs(out, ref["out"].detach()) < 1e-4 * max(1.0, float(ref["out"].detach().abs().max()))
    (ref["out"] * G).sum().backward()
    compare_param_grads(net, sc, which=("mlp_coarse",))
