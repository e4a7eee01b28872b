"""
The single-plane f16 TRAINING mode (-m gpu; include/pnyolo.h PNY_PRECISION_F16_TRAIN; csrc/mlp_h1t.hip, mlp_bwd_h1.hip,
dw_gemm_h1.hip, latent_grad_h1.hip).

F16_TRAIN is opt-in and sits OUTSIDE the 1e-4 parity claim: the training forward, the dX chain, the weight-gradient GEMMs and
the latent gradient multiply one f16 value per operand with fp32 accumulation.  Its bars below were each set from one
MI355X measurement with at most 2x margin (the measured value is written beside each constant).  What it must keep exactly:
determinism of the parameter gradients, exact scaling with the loss (the internal scales are powers of two), the current
transposed images after a refresh, and the behaviour of every other precision on the same model.
"""
import numpy as np
import pytest
import torch

from helpers import DEV, dt, load_mlp
from pixel_nerf_yolo_amd import conf as pconf
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd import synth
from pixel_nerf_yolo_amd.model import make_model
from pixel_nerf_yolo_amd.render import NeRFRenderer
from pixel_nerf_yolo_amd.util import gen_rays

pytestmark = pytest.mark.gpu

# bars, relative to the tensor's max |g| (F32-pinned scene) or to the reference golden's max, each from one measurement on
# the MI355X (measured value in the comment), at most 2x margin; the issue's ceiling is 1e-2
GRAD_TOL = 7e-3          # NeRF head, 512 rays: max over the MLP parameter tensors of max |g - g_f32| / max |g_f32| (measured 3.54e-3, lin_z.0)
LATENT_TOL = 5e-3        # NeRF head, 512 rays: the latent gradient, same measure (measured 2.48e-3)
CHUNK_TOL = 2.6e-3       # the same step recomputed in chunks (fp32 stash forward), parameter gradients (measured 1.28e-3)
YOLO_TOL = 2.4e-3        # YOLO head (d_out 21, L 1792), parameter gradients of mlp_coarse (measured 1.18e-3)
LOSS_REL_TOL = 5e-5      # 200 Adam steps towards a teacher render: |final loss F16_TRAIN - AUTO| / AUTO (measured 2.52e-5)
LOSS_DROP_MAX = 0.85     # ... AUTO's final loss / its first (measured 0.746: the training does move towards the teacher)
# Small batches (the reference golden's 24 rays, the grouped 4 x 16 rays) are measured stage by stage: the single-plane
# BACKWARD against the split-f16 backward on the same single-plane forward (PNYOLO_BWD_PRECISION=f16x2) is held to the bar
# below; the remaining difference to F32 belongs to the single-plane forward (F16's kernel) and is reported.
BWD_TOL = 1.2e-3         # max |g - g_(bwd f16x2)| / max |g_(bwd f16x2)| per tensor (measured 5.82e-4 golden, 4.10e-4 grouped)
FWD_RGB_TOL = 5e-3       # golden case: rendered rgb against the reference's (F16's RENDER_TOL; measured 1.81e-4 against F32)


def report(name, value):
    print("F16T-MEASURED %s %.6g" % (name, value))


def small_train_net(prec, seed=900, ns=2, H=32, W=32, state=None):
    c = pconf.default_mv()
    net = make_model(c["model"], stop_encoder_grad=True)
    load_mlp(net.mlp_coarse, seed + 1, 512, 4)
    load_mlp(net.mlp_fine, seed + 2, 512, 4)
    if state is not None:   # weights of another model, in place before the first library call (finalize packs them)
        net.load_state_dict({k: v.detach().cpu() for k, v in state.items()}, strict=False)
    net = net.to(DEV).train()
    net.set_matrix_precision(prec)
    poses, tgt = synth.scene_cameras(ns)
    lat = torch.from_numpy(synth.latent(seed + 3, ns, 512, H // 2, W // 2)).to(DEV).requires_grad_(True)
    net.encode(torch.zeros(1, ns, 3, H, W), torch.from_numpy(poses)[None], torch.tensor(0.9 * W), latent=lat)
    return net, lat, tgt


def train_step_grads(net, lat, tgt, loss_scale=1.0, n=512, H=32, W=32):
    """One render + backward of 512 rays (32 + 16 (8) samples): the MLP parameter gradients and the latent gradient."""
    rays = gen_rays(dt(tgt)[None], W, H, torch.tensor(0.9 * W), 0.8, 1.8).reshape(1, -1, 8)[:, :n].contiguous()
    ren = NeRFRenderer(n_coarse=32, n_fine=16, n_fine_depth=8, white_bkgd=True).train()
    rs = np.random.RandomState(3)
    ren.draws = dict(u_coarse=torch.from_numpy(rs.rand(n, 32).astype(np.float32)),
                     u_fine=torch.from_numpy(rs.rand(n, 8).astype(np.float32)),
                     u_fine2=torch.from_numpy(rs.rand(n, 8).astype(np.float32)),
                     g_depth=torch.from_numpy(rs.randn(n, 8).astype(np.float32)))
    out = ren(net, rays, want_weights=True)
    gt = torch.full_like(out["fine"]["rgb"], 0.5)
    loss = torch.nn.functional.mse_loss(out["coarse"]["rgb"], gt) + torch.nn.functional.mse_loss(out["fine"]["rgb"], gt)
    (loss * loss_scale).backward()
    torch.cuda.synchronize()
    g = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None and k.startswith("mlp_")}
    g["latent"] = lat.grad.detach().clone()
    return g


def rel_err(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def worst_tensors(errs, n=5):
    top = sorted(errs.items(), key=lambda kv: -kv[1])[:n]
    print("F16T-WORST " + ", ".join("%s %.3g" % kv for kv in top))
    return top[0][1]


# --------------------------------------------------------------------------- dispatch
def test_dispatch_reports_single_plane_forward_and_backward():
    """One render + backward on an F16_TRAIN scene runs the single-plane training forward and chain; the C ABI accepts the
    new value and reports it."""
    net, lat, tgt = small_train_net("f16_train")
    train_step_grads(net, lat, tgt)
    assert net.last_launch_precision() == "f16"
    assert net.last_backward_precision() == "f16"
    # no recompute: the backward started from the stash, which only the training forward writes -- and the only stashing
    # kernel that reports 2 is pny_mlp_h1_kernel<true>
    assert net.last_backward_stats()["flops"][0] == 0.0
    L = plib.load()
    h = net._scene(0)
    assert L.pny_scene_set_precision(h, plib.PRECISION["f16_train"]) == 0
    # the same step on AUTO and F32 scenes reports their kernels
    for prec, want in (("auto", "f16x2"), ("f32", "f32")):
        n2, l2, t2 = small_train_net(prec)
        train_step_grads(n2, l2, t2)
        assert n2.last_backward_precision() == want, prec


def grouped_run(monkeypatch, prec, SB=4, ns=3, n=16, group=True, per_scene=None):
    """The grouped super-batch (one scene over SB objects, deferred weight gradients) of test_gpu_backward's
    test_grouped_super_batch_equals_per_object."""
    H = W = 32
    kc, kf, kfd = 16, 8, 4
    c = pconf.default_mv()
    rs = np.random.RandomState(5)
    lat = np.concatenate([synth.latent(1510 + i, ns, 512, H // 2, W // 2) for i in range(SB)])
    poses = np.stack([synth.scene_cameras(ns, radius=1.3 + 0.05 * i)[0] for i in range(SB)])
    focal = torch.tensor(29.0)
    rays = torch.stack([gen_rays(torch.from_numpy(synth.pose_spherical(100.0 + 25 * i, -20.0, 1.3))[None], W, H, focal, 0.3, 1.8)[0]
                        .reshape(-1, 8)[torch.from_numpy(rs.choice(H * W, n, replace=False))] for i in range(SB)])
    dr = dict(u_coarse=rs.rand(SB * n, kc).astype(np.float32), u_fine=rs.rand(SB * n, kf - kfd).astype(np.float32),
              u_fine2=rs.rand(SB * n, kf - kfd).astype(np.float32), g_depth=rs.randn(SB * n, kfd).astype(np.float32))
    gt = torch.from_numpy(rs.uniform(0, 1, size=(SB, n, 3)).astype(np.float32)).to(DEV)
    monkeypatch.setenv("PNYOLO_GROUP", "1" if group else "0")
    net = make_model(c["model"], stop_encoder_grad=True)
    load_mlp(net.mlp_coarse, 1501, 512, 4)
    load_mlp(net.mlp_fine, 1502, 512, 4)
    net = net.to(DEV).train()
    net.set_matrix_precision(prec)
    net.encode(torch.zeros(SB, ns, 3, H, W), torch.from_numpy(poses), focal, latent=torch.from_numpy(lat).to(DEV))
    assert (net._group is not None) == group
    for i, p in enumerate(per_scene or []):   # per-object scenes of one model, each with its own precision
        assert plib.load().pny_scene_set_precision(net._scene(i), plib.PRECISION[p]) == 0
    ren = NeRFRenderer(n_coarse=kc, n_fine=kf, n_fine_depth=kfd, white_bkgd=True).train()
    ren.draws = dr
    out = ren(net, rays.to(DEV), want_weights=True)
    (torch.nn.functional.mse_loss(out["coarse"]["rgb"], gt) + torch.nn.functional.mse_loss(out["fine"]["rgb"], gt)).backward()
    torch.cuda.synchronize()
    return net, {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}


def test_dispatch_grouped_super_batch(monkeypatch):
    net, g16 = grouped_run(monkeypatch, "f16_train")
    assert net._last_call_group
    assert net.last_launch_precision() == "f16" and net.last_backward_precision() == "f16"
    assert net.last_flush_precision() == "f16" and net.last_backward_stats()["flops"][0] == 0.0
    monkeypatch.setenv("PNYOLO_BWD_PRECISION", "f16x2")   # the same single-plane forward, split-f16 backward
    netx, gfx = grouped_run(monkeypatch, "f16_train")
    assert netx.last_backward_precision() == "f16x2" and netx.last_flush_precision() == "f16x2"
    monkeypatch.delenv("PNYOLO_BWD_PRECISION")
    bwd = worst_tensors({k: rel_err(g16[k], gfx[k]) for k in gfx})
    report("grouped_bwd_rel_err", bwd)
    _, g32 = grouped_run(monkeypatch, "f32")
    report("grouped_fwd_owned_rel_err", worst_tensors({k: rel_err(gfx[k], g32[k]) for k in g32}))
    report("grouped_total_rel_err", worst_tensors({k: rel_err(g16[k], g32[k]) for k in g32}))
    assert bwd <= BWD_TOL


# --------------------------------------------------------------------------- accuracy
def test_gradients_against_f32():
    """The same draws on an F32-pinned scene: every MLP parameter gradient and the latent gradient within the bars."""
    g16 = train_step_grads(*small_train_net("f16_train"))
    g32 = train_step_grads(*small_train_net("f32"))
    assert g16.keys() == g32.keys() and len(g32) > 60
    lat = rel_err(g16.pop("latent"), g32.pop("latent"))
    errs = {k: rel_err(g16[k], g32[k]) for k in g32}
    worst = worst_tensors(errs)
    report("nerf_param_grad_rel_err_max", worst)
    report("nerf_param_grad_rel_err_median", float(np.median(list(errs.values()))))
    report("nerf_latent_grad_rel_err", lat)
    assert worst <= GRAD_TOL, max(errs, key=errs.get)
    assert lat <= LATENT_TOL


def golden_grads(g, prec):
    seed, ns, H, W = int(g["seed"]), int(g["NS"]), int(g["H"]), int(g["W"])
    kc, kf, kfd = int(g["Kc"]), int(g["Kf"]), int(g["Kfd"])
    net = make_model(pconf.default_mv()["model"], stop_encoder_grad=True)
    load_mlp(net.mlp_coarse, seed * 10 + 1, 512, 4)
    load_mlp(net.mlp_fine, seed * 10 + 2, 512, 4)
    net = net.to(DEV).train()
    net.set_matrix_precision(prec)
    lat = torch.from_numpy(synth.latent(seed * 10 + 3, ns, 512, H // 2, W // 2))
    net.encode(torch.zeros(1, ns, 3, H, W), torch.from_numpy(g["poses"])[None], torch.tensor(float(g["focal"])),
               c=torch.from_numpy(g["c"]), latent=lat)
    ren = NeRFRenderer(n_coarse=kc, n_fine=kf, n_fine_depth=kfd, depth_std=0.01, white_bkgd=True).train()
    ren.draws = dict(u_coarse=g["draw0_rand_like"], u_fine=g["draw1_rand"], u_fine2=g["draw2_rand_like"], g_depth=g["draw3_randn_like"])
    out = ren(net, dt(g["rays"])[None], want_weights=True)
    gt = dt(g["gt"])[None]
    loss = torch.nn.functional.mse_loss(out["coarse"]["rgb"], gt) + torch.nn.functional.mse_loss(out["fine"]["rgb"], gt)
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None and k.startswith("mlp_")}
    return net, out, grads


def test_gradients_against_reference_golden(golden, monkeypatch):
    """tests/golden/nerf_grads.npz (the reference's own gradients, 24 rays) in the form of
    test_training_gradients_reference_golden, stage by stage: the single-plane forward's rendered rgb against the reference's
    (F16's bar), the single-plane backward against the split-f16 backward on that same forward (BWD_TOL); the digests'
    error against the reference -- what the forward's own error does to the gradients of this small batch -- is reported."""
    g = golden("nerf_grads")
    net, out, g16 = golden_grads(g, "f16_train")
    assert net.last_backward_precision() == "f16"
    fwd = max(float((out["coarse"]["rgb"][0].cpu() - torch.from_numpy(g["coarse_rgb"])).abs().max()),
              float((out["fine"]["rgb"][0].cpu() - torch.from_numpy(g["fine_rgb"])).abs().max()))
    report("golden_fwd_rgb_err", fwd)
    assert fwd <= FWD_RGB_TOL
    monkeypatch.setenv("PNYOLO_BWD_PRECISION", "f16x2")
    netx, _, gfx = golden_grads(g, "f16_train")
    assert netx.last_backward_precision() == "f16x2"
    monkeypatch.delenv("PNYOLO_BWD_PRECISION")
    bwd = worst_tensors({k: rel_err(g16[k], gfx[k]) for k in gfx})
    report("golden_bwd_rel_err", bwd)
    errs = {}
    for name, grad in g16.items():
        stat, idx, val = g["g:%s:stat" % name], g["g:%s:idx" % name], g["g:%s:val" % name]
        f = grad.cpu().reshape(-1).double()
        errs[name] = float(((f[torch.from_numpy(idx)] - torch.from_numpy(val)).abs() / max(float(stat[2]), 1e-12)).max())
    report("golden_digest_rel_err_fwd_owned", worst_tensors(errs))
    assert bwd <= BWD_TOL


def yolo_grads(prec):
    from pixel_nerf_yolo_amd.render import YoloRenderer
    from test_gpu_backward import scene_pair
    n, K = 40, 32
    net, _ = scene_pair(2, 64, 64, 1792, 21, 5, 3, 1500, yolo=True, lat_hw=(8, 8))
    net.set_matrix_precision(prec)
    _, tgt_c2w = synth.scene_cameras(2, radius=4.0, phi=-25.0)
    flipyz = np.diag([1.0, -1.0, -1.0, 1.0]).astype(np.float32)
    tgt_w2c = np.linalg.inv(tgt_c2w @ flipyz).astype(np.float32)
    import pnyolo_oracle as orc
    rays = orc.gen_rays_yolo(tgt_w2c[None], 16, 12, [5.0, 5.5], [8.0, 6.0], 1.0, 6.0)[0].reshape(-1, 8)[:n]
    rs = np.random.RandomState(21)
    u = rs.rand(n, K).astype(np.float32)
    G = torch.from_numpy(rs.standard_normal((n, 3, 7)).astype(np.float32))
    ren = YoloRenderer(K, 128, 1, 3)
    ren.bind_parallel(net)
    ren.draws = dict(u_coarse=u)
    out = ren(rays[None].to(DEV))
    (out * G.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return net, {k: p.grad.detach().clone() for k, p in net.mlp_coarse.named_parameters() if p.grad is not None}


def test_yolo_head_gradients_against_f32():
    """The YOLO head (d_out 21, L 1792, pny_yolo_render_backward): mlp_coarse's gradients against an F32-pinned scene."""
    net, g16 = yolo_grads("f16_train")
    assert net.last_backward_precision() == "f16"
    _, g32 = yolo_grads("f32")
    errs = {k: rel_err(g16[k], g32[k]) for k in g32}
    worst = max(errs.values())
    report("yolo_param_grad_rel_err_max", worst)
    assert worst <= YOLO_TOL, max(errs, key=errs.get)


# --------------------------------------------------------------------------- determinism and scaling
def test_parameter_gradients_deterministic():
    a = train_step_grads(*small_train_net("f16_train"))
    b = train_step_grads(*small_train_net("f16_train"))
    la, lb = a.pop("latent"), b.pop("latent")
    assert float((la - lb).abs().max()) <= 1e-5 * float(la.abs().max())
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_recompute_in_chunks_deterministic(monkeypatch):
    """A stash budget below the batch: the backward recomputes the forward chunk by chunk (as test_backward_recompute_in_chunks
    does for AUTO) and still runs the single-plane chain and GEMMs; two such runs are bit-identical and close to F32."""
    monkeypatch.setenv("PNYOLO_STASH_GB", "0.07")
    net, lat, tgt = small_train_net("f16_train")
    a = train_step_grads(net, lat, tgt)
    assert net.last_backward_precision() == "f16"
    b = train_step_grads(*small_train_net("f16_train"))
    la, lb = a.pop("latent"), b.pop("latent")
    assert float((la - lb).abs().max()) <= 1e-5 * float(la.abs().max())
    for k in a:
        assert torch.equal(a[k], b[k]), k
    c = train_step_grads(*small_train_net("f32"))
    c.pop("latent")
    worst = max(rel_err(a[k], c[k]) for k in c)
    report("chunked_grad_rel_err", worst)
    assert worst <= CHUNK_TOL


@pytest.mark.parametrize("k", [-20, 0, 20])
def test_gradients_scale_exactly_with_the_loss(k):
    base = train_step_grads(*small_train_net("f16_train"))
    scaled = train_step_grads(*small_train_net("f16_train"), loss_scale=2.0 ** k)
    base.pop("latent"), scaled.pop("latent")
    for name in base:
        assert torch.equal(scaled[name], base[name] * 2.0 ** k), name


# --------------------------------------------------------------------------- training
def train_losses(prec, steps=200, lr=1e-4):
    """Reduced form of bench.py's training step (frozen trunk, supplied latent): 200 Adam steps on one scene, fixed draws
    per step, the same init for every precision.  The target is a learnable image: the F32 render of a teacher network
    (other weights, same scene), so the loss falls well below its start instead of settling on a noise floor."""
    torch.manual_seed(0)
    net, _, tgt = small_train_net(prec, seed=910)
    H = W = 32
    n = 256
    opt = torch.optim.Adam([p for k, p in net.named_parameters() if k.startswith("mlp_")], lr=lr)
    all_rays = gen_rays(dt(tgt)[None], W, H, torch.tensor(0.9 * W), 0.8, 1.8).reshape(-1, 8)
    rs = np.random.RandomState(11)
    teacher, _, _ = small_train_net("f32", seed=930)
    teacher.eval()
    tren = NeRFRenderer(n_coarse=32, n_fine=16, n_fine_depth=8, white_bkgd=True).eval()
    tr = np.random.RandomState(12)
    tren.draws = dict(u_coarse=torch.from_numpy(tr.rand(H * W, 32).astype(np.float32)),
                      u_fine=torch.from_numpy(tr.rand(H * W, 8).astype(np.float32)),
                      u_fine2=torch.from_numpy(tr.rand(H * W, 8).astype(np.float32)),
                      g_depth=torch.from_numpy(tr.randn(H * W, 8).astype(np.float32)))
    with torch.no_grad():
        gt_img = tren(teacher, all_rays[None].contiguous())["fine"]["rgb"][0].detach().clone()
    ren = NeRFRenderer(n_coarse=32, n_fine=16, n_fine_depth=8, white_bkgd=True).train()
    losses = []
    for step in range(steps):
        idx = torch.from_numpy(rs.choice(H * W, n, replace=False)).to(DEV)
        ren.draws = dict(u_coarse=torch.from_numpy(rs.rand(n, 32).astype(np.float32)),
                         u_fine=torch.from_numpy(rs.rand(n, 8).astype(np.float32)),
                         u_fine2=torch.from_numpy(rs.rand(n, 8).astype(np.float32)),
                         g_depth=torch.from_numpy(rs.randn(n, 8).astype(np.float32)))
        out = ren(net, all_rays[idx][None].contiguous())
        gt = gt_img[idx][None]
        loss = torch.nn.functional.mse_loss(out["coarse"]["rgb"], gt) + torch.nn.functional.mse_loss(out["fine"]["rgb"], gt)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    return net, losses


def test_training_converges_like_auto():
    net16, l16 = train_losses("f16_train")
    assert net16.last_backward_precision() == "f16"
    _, la = train_losses("auto")
    f16, fa = np.mean(l16[-10:]), np.mean(la[-10:])
    report("loss_first", la[0])
    report("loss_final_auto", fa)
    report("loss_final_f16_train", f16)
    report("loss_rel_diff", abs(f16 - fa) / fa)
    report("loss_drop_auto", fa / la[0])
    assert fa <= LOSS_DROP_MAX * la[0]
    assert abs(f16 - fa) <= LOSS_REL_TOL * fa


# --------------------------------------------------------------------------- refresh and mixed flushes
def test_refresh_keeps_transposed_images_current():
    """After an optimizer step (device-side pny_model_refresh) the F16_TRAIN gradients equal those of a freshly built model
    holding the stepped weights, bit for bit."""
    net, lat, tgt = small_train_net("f16_train")
    g0 = train_step_grads(net, lat, tgt)
    opt = torch.optim.Adam([p for k, p in net.named_parameters() if k.startswith("mlp_")], lr=1e-3)
    opt.step()
    net.zero_grad(set_to_none=True)
    lat.grad = None
    g1 = train_step_grads(net, lat, tgt)
    assert not torch.equal(g0["mlp_fine.blocks.0.fc_0.weight"], g1["mlp_fine.blocks.0.fc_0.weight"])
    # a model whose FIRST library call finalizes the stepped weights: every image, the transposed single-plane ones
    # included, is packed from them on the host path, none by a refresh
    fresh, flat, _ = small_train_net("f16_train", state=net.state_dict())
    g2 = train_step_grads(fresh, flat, tgt)
    g1.pop("latent"), g2.pop("latent")
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


def test_mixed_flushes(monkeypatch):
    """One scene per object, one deferred flush over all their tiles: all F16_TRAIN runs the single-plane GEMM, one AUTO
    contributor among them the split-f16 GEMM, one F32 contributor the fp32 GEMM, and each scene reports its own chain.
    (An all-AUTO flush cannot be matched bit for bit: the F16_TRAIN scenes' stashes hold single-plane forward values.)  An
    AUTO model's gradients do not change when one of its scenes was F16_TRAIN before (the transposed images exist)."""
    name = {"f16_train": "f16", "auto": "f16x2", "f32": "f32"}
    for mix, flush in ((["f16_train"] * 4, "f16"), (["f16_train", "auto", "f16_train", "f16_train"], "f16x2"),
                       (["f16_train", "f32", "f16_train", "f16_train"], "f32")):
        net, g = grouped_run(monkeypatch, "auto", group=False, per_scene=mix)
        assert [net.last_backward_precision(i) for i in range(4)] == [name[m] for m in mix]
        assert net.last_flush_precision() == flush, mix
        assert all(bool(torch.isfinite(v).all()) for v in g.values())
    _, g_auto = grouped_run(monkeypatch, "auto", group=False)
    _, g_had = grouped_run(monkeypatch, "auto", group=False, per_scene=["f16_train", "auto", "auto", "auto"])
    _, g_had_then_auto = grouped_run(monkeypatch, "f16_train", group=False, per_scene=["auto"] * 4)
    for k in g_auto:
        assert torch.equal(g_auto[k], g_had_then_auto[k]), k
    assert any(not torch.equal(g_auto[k], g_had[k]) for k in g_auto)


# --------------------------------------------------------------------------- range guard
def test_activation_overflow_in_training_forward():
    """relu(lin_in(x)) of a few 1e5 in the TRAINING forward (pny_mlp_h1_kernel<true>; construction of test_gpu_f16's
    test_activation_overflow): the kernel reports PNY_RANGE_ACTIVATION, the backward -- the next call on the model -- raises
    PnyRangeError and is not repeated on other kernels.  A software flag, not a fault."""
    net = make_model(pconf.default_mv()["model"], stop_encoder_grad=True)
    for mlp, sd in ((net.mlp_coarse, synth.mlp_state(201)), (net.mlp_fine, synth.mlp_state(202))):
        sd = {k: torch.from_numpy(v) for k, v in sd.items()}
        sd["lin_in.weight"] = sd["lin_in.weight"] * 2000.0
        mlp.load_state_dict(sd)
    net = net.to(DEV).train()
    net.set_matrix_precision("f16_train")
    ns, H, W = 2, 32, 32
    poses, tgt = synth.scene_cameras(ns)
    net.encode(torch.zeros(1, ns, 3, H, W), torch.from_numpy(poses)[None], torch.tensor(0.9 * W),
               latent=torch.from_numpy(synth.latent(203, ns, 512, H // 2, W // 2)))
    n = 256
    rays = gen_rays(dt(tgt)[None], W, H, torch.tensor(0.9 * W), 0.8, 1.8).reshape(1, -1, 8)[:, :n].contiguous() * 1.0
    rays[..., :3] *= 40.0
    ren = NeRFRenderer(n_coarse=32, n_fine=16, n_fine_depth=8, white_bkgd=True).train()
    # (the fine pass may already meet the flag raised by the coarse pass: the error is expected from either call)
    with pytest.raises(plib.PnyRangeError, match="f16"):
        out = ren(net, rays)
        torch.cuda.synchronize()
        assert net.last_launch_precision() == "f16" and net.range_status() & 1
        (out["coarse"]["rgb"].sum() + out["fine"]["rgb"].sum()).backward()
    assert net.range_status(clear=True) & 1
