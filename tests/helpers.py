"""Shared builders for the parity tests: the same seeded scenes tools/make_golden.py used."""
import numpy as np
import torch

from pixel_nerf_yolo_amd import conf as pconf
from pixel_nerf_yolo_amd import synth
from pixel_nerf_yolo_amd.model import make_model


def load_mlp(mlp, seed, d_latent, d_out):
    sd = synth.mlp_state(seed, d_latent=d_latent, d_out=d_out)
    mlp.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)


def latent_dims(g):
    """(channels, Hl, Wl) of a fixture_nerf golden; older fixtures are ResNet-34 sized (512, H/2, W/2)."""
    H, W = int(g["H"]), int(g["W"])
    if "d_latent" in g:
        return int(g["d_latent"]), int(g["Hl"]), int(g["Wl"])
    return 512, H // 2, W // 2


def nerf_net(g, seed, device="cuda:0"):
    """PixelNeRFNet (HIP path) configured and seeded exactly like tools/make_golden.fixture_nerf."""
    c = pconf.default_mv()
    has_fine = int(g["Kf"]) > 0
    if not has_fine:
        c.d["model"]["mlp_fine"] = {"type": "empty"}
    L, hl, wl = latent_dims(g)
    if L != 512:
        c.d["model"]["encoder"]["backbone"] = "custom"   # BASELINE configs 3-5: d_latent = 1792, latent supplied
    net = make_model(c["model"]).eval()
    load_mlp(net.mlp_coarse, seed * 10 + 1, L, 4)
    if has_fine:
        load_mlp(net.mlp_fine, seed * 10 + 2, L, 4)
    net = net.to(device)
    ns, H, W = int(g["NS"]), int(g["H"]), int(g["W"])
    lat = torch.from_numpy(synth.latent(seed * 10 + 3, ns, L, hl, wl))
    images = torch.zeros(1, ns, 3, H, W)
    net.encode(images, torch.from_numpy(g["src_poses"])[None], torch.tensor(float(g["focal"])),
               c=torch.from_numpy(g["c"])[None], latent=lat)
    return net


def oracle_scene(g, seed):
    import pnyolo_oracle as orc
    ns, H, W = int(g["NS"]), int(g["H"]), int(g["W"])
    L, hl, wl = latent_dims(g)
    mc = synth.mlp_state(seed * 10 + 1, d_latent=L)
    mf = synth.mlp_state(seed * 10 + 2, d_latent=L) if int(g["Kf"]) > 0 else None
    lat = synth.latent(seed * 10 + 3, ns, L, hl, wl)
    return orc.Scene(mc, mf, lat, g["src_poses"], g["focal"], g["c"][None], W, H)


def camera_ring(ns):
    """(ns source poses, target pose) for any view count up to the ABI's 16: no two views share a camera.
    synth.scene_cameras steps theta by 40 degrees, so its view 9 is its view 0 again and a kernel that confused the two
    would go unnoticed; here theta steps by 22.5 degrees (16 views: 3 .. 340.5), the elevation cycles through five values
    and the radius grows with the view."""
    src = np.stack([synth.pose_spherical(22.5 * i + 3.0, -35.0 + 4.0 * (i % 5), 1.3 + 0.03 * i) for i in range(ns)])
    return src, synth.pose_spherical(120.0, -20.0, 1.3)


# --------------------------------------------------------------------------- MLP (query) backward
def scene_pair(ns, H, W, L, d_out, n_blocks, combine_layer, seed, yolo=False, lat_hw=None, lat_grad=False, dtype=None,
               yolo_flip=True, with_net=True, poses=None, code=None, out_gain=1.0):
    """The same seeded scene as a HIP net (trainable MLP, frozen encoder) and as oracle state with requires_grad.
    lat_grad: the latent is a leaf that requires grad on both sides (net.test_latent on the GPU, sc.latent on the CPU).
    dtype: the oracle's arithmetic and the dtype of its leaves (None = f32; torch.float64 = the arbiter of the shape sweeps).
    yolo_flip=False (YOLO mode): world->cam extrinsics of cameras looking down -z, so that the scene lies at z < 0, where YOLO
    mode keeps the latent (models.py:224,254-264 zero it at z >= 0); the default flips y / z, which puts the scene at z > 0.
    with_net=False: the oracle scene alone (net is None; no GPU needed).
    poses (non-YOLO mode): (ns, 4, 4) source poses instead of synth.scene_cameras(ns), e.g. camera_ring(ns)[0].
    code: (num_freqs, freq_factor) of the positional code on both sides (None = the shipped 6, 1.5): conf model.code of the net,
    d_in = 6 + 6 * num_freqs of the weights, Scene(num_freqs, freq_factor) of the oracle.
    out_gain: synth.mlp_state's scale of lin_out.weight (YOLO mode's raw outputs).
    A d_latent that no backbone yields (neither 512 nor 1792), and a d_out that the conf cannot state (YOLO mode: no multiple
    of 7), are set on the model after construction and both MLPs rebuilt at them, before the first library call."""
    import pnyolo_oracle as orc
    from pixel_nerf_yolo_amd.model import make_mlp
    c = pconf.yolo() if yolo else pconf.default_mv()
    m = c.d["model"]
    if L != 512 and not yolo:
        m["encoder"]["backbone"] = "custom"
    num_freqs, freq_factor = (6, 1.5) if code is None else (int(code[0]), float(code[1]))
    d_in = 6 + 6 * num_freqs
    if code is not None:
        m["code"].update({"num_freqs": num_freqs, "freq_factor": freq_factor})
    if yolo and d_out % 7 == 0:
        m["mlp_coarse"].update({"d_out": 7, "num_anchors_per_scale": d_out // 7})
    elif not yolo:
        m["mlp_coarse"]["d_out"] = m["mlp_fine"]["d_out"] = d_out
    m["mlp_coarse"].update({"n_blocks": n_blocks, "combine_layer": combine_layer})
    if not yolo:
        m["mlp_fine"].update({"n_blocks": n_blocks, "combine_layer": combine_layer})
    net = make_model(c["model"], stop_encoder_grad=True)
    assert net.d_in == d_in and net.code.num_freqs == num_freqs and float(net.code.freq_factor) == freq_factor
    if net.d_latent != L or net.d_out != d_out:
        net.d_latent = net.latent_size = L
        net.d_out = d_out
        for k in ("mlp_coarse", "mlp_fine"):
            if getattr(net, k) is not None:
                mlp = make_mlp(c["model"][k], d_in, L)
                if mlp.d_out != d_out:
                    mlp.lin_out, mlp.d_out = torch.nn.Linear(mlp.d_hidden, d_out), d_out
                setattr(net, k, mlp)
    kw = dict(d_latent=L, d_out=d_out, n_blocks=n_blocks, combine_layer=combine_layer, d_in=d_in, out_gain=out_gain)
    sd_c = synth.mlp_state(seed + 1, **kw)
    net.mlp_coarse.load_state_dict({k: torch.from_numpy(v) for k, v in sd_c.items()})
    sd_f = None
    if net.mlp_fine is not None:
        sd_f = synth.mlp_state(seed + 2, **kw)
        net.mlp_fine.load_state_dict({k: torch.from_numpy(v) for k, v in sd_f.items()})
    hl, wl = lat_hw or (H // 2, W // 2)
    lat = synth.latent(seed + 3, ns, L, hl, wl)
    if yolo:
        src_c2w, _ = synth.scene_cameras(ns, radius=4.0, phi=-25.0)
        flipyz = np.diag([1.0, -1.0, -1.0, 1.0] if yolo_flip else [1.0, 1.0, 1.0, 1.0]).astype(np.float32)
        poses = np.stack([np.linalg.inv(p @ flipyz) for p in src_c2w]).astype(np.float32)
        focal, cc = torch.tensor([[40.0, 44.0]]), torch.tensor([[W * 0.5, H * 0.5 - 2]])
    else:
        if poses is None:
            poses, _ = synth.scene_cameras(ns)
        poses = np.asarray(poses, dtype=np.float32)
        assert poses.shape == (ns, 4, 4)
        focal, cc = torch.tensor(0.9 * W), torch.tensor([[W * 0.5, H * 0.5]])
    if with_net:
        net = net.to(DEV).train()
        net.test_latent = torch.from_numpy(lat).to(DEV).requires_grad_() if lat_grad else torch.from_numpy(lat)
        net.encode(torch.zeros(1, ns, 3, H, W), torch.from_numpy(poses)[None], focal, c=cc, latent=net.test_latent)
        # the same scene again on another latent tensor (e.g. a frozen copy): net.test_encode(latent)
        net.test_encode = lambda latent: net.encode(torch.zeros(1, ns, 3, H, W), torch.from_numpy(poses)[None], focal, c=cc, latent=latent)
    else:
        net = None
    leaf_dt = torch.float32 if dtype is None else dtype
    mc = {k: torch.from_numpy(v).to(leaf_dt).requires_grad_() for k, v in sd_c.items()}
    mf = None if sd_f is None else {k: torch.from_numpy(v).to(leaf_dt).requires_grad_() for k, v in sd_f.items()}
    sc = orc.Scene(mc, mf, lat, poses, focal, cc, W, H, yolo=yolo, n_blocks=n_blocks, combine_layer=combine_layer, dtype=dtype,
                   num_freqs=num_freqs, freq_factor=freq_factor)
    sc.mlp_coarse, sc.mlp_fine = mc, mf          # Scene() re-wraps tensors: keep the leaves
    if lat_grad:
        sc.latent = torch.from_numpy(lat).to(leaf_dt).requires_grad_()
    return net, sc


RTOL = 1e-4      # every gradient tensor within 1e-4 x its own max |.| (gradients sum 10^4..10^5 fp32 products)


def grad_check(name, got, ref, rtol=RTOL):
    ref = torch.as_tensor(np.asarray(ref), dtype=torch.float32)
    scale = max(float(ref.abs().max()), 1e-20)
    err = float((got.detach().cpu().float() - ref).abs().max())
    assert err <= rtol * scale, "%s: max |err| %.3e vs max |grad| %.3e (ratio %.2e)" % (name, err, scale, err / scale)
    return err / scale


def compare_param_grads(net, sc, which=("mlp_coarse", "mlp_fine"), rtol=RTOL):
    worst = 0.0
    for pre in which:
        mlp, ref = getattr(net, pre), getattr(sc, pre)
        if mlp is None:
            continue
        for k, p in mlp.named_parameters():
            assert p.grad is not None, pre + "." + k
            r = ref[k].grad if ref[k].grad is not None else torch.zeros_like(ref[k])
            worst = max(worst, grad_check(pre + "." + k, p.grad, r, rtol))
    return worst


def render_loss(out, gt, with_depth=False):
    loss = torch.nn.functional.mse_loss(out["coarse"]["rgb"], gt) + torch.nn.functional.mse_loss(out["fine"]["rgb"], gt)
    if with_depth:
        loss = loss + 0.1 * out["fine"]["depth"].mean() + 0.05 * out["coarse"]["depth"].square().mean()
    return loss


def maxabs(a, b):
    a = torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a), dtype=torch.float32)
    b = torch.as_tensor(np.asarray(b.detach().cpu() if torch.is_tensor(b) else b), dtype=torch.float32)
    return float((a - b).abs().max())


DEV = "cuda:0"


def dt(x, device=DEV):
    return torch.as_tensor(np.asarray(x), dtype=torch.float32, device=device).contiguous()


def render_debug(ren, net, rays, draws, kc, kt, device=DEV):
    """Render with explicit draws and capture the per-sample / z buffers through the ABI."""
    n = rays.shape[0]
    dbg = {"z_coarse": torch.empty(1, n, kc, device=device), "sample_coarse": torch.empty(1, n, kc, 4, device=device)}
    if kt > kc:
        dbg["z_fine"] = torch.empty(1, n, kt, device=device)
        dbg["sample_fine"] = torch.empty(1, n, kt, 4, device=device)
    ren._debug_out = dbg
    ren.draws = draws
    with torch.no_grad():
        out = ren(net, dt(rays, device)[None], want_weights=True)
    torch.cuda.synchronize()
    ren._debug_out = None
    return out, dbg


def fine_flip_rays(z_hip, z_ref, weights_ref, u_fine):
    """Rays whose sorted fine depths differ from the reference's; each must be explained by a draw that sits within
    1e-5 of a cdf edge (importance sampling is discontinuous in the coarse weights)."""
    bad = ((z_hip - z_ref).abs().max(dim=1)[0] > 1e-6).nonzero().flatten().tolist()
    w = weights_ref + 1e-5
    cdf = torch.cumsum(w / w.sum(-1, keepdim=True), -1)
    for r in bad:
        margin = (cdf[r][None, :] - torch.as_tensor(u_fine[r])[:, None]).abs().min()
        assert float(margin) < 1e-5, "ray %d differs without a near-edge draw (margin %.2e)" % (r, float(margin))
    return bad


def check_against_nerf_golden(g, out, dbg, tol, max_flips=2):
    """HIP render (out, dbg from render_debug) against a fixture_nerf-style golden: bit-exact coarse depths, per-sample
    rgb / sigma, weights and pixels within `tol` ABSOLUTE; fine pass on the rays whose bins did not flip."""
    import pnyolo_oracle as orc
    n, kc, kf, kfd = g["rays"].shape[0], int(g["Kc"]), int(g["Kf"]), int(g["Kfd"])
    if "z_coarse" in g:
        assert maxabs(dbg["z_coarse"][0], g["z_coarse"]) == 0.0
    assert maxabs(dbg["sample_coarse"][0].reshape(-1, 4), g["coarse_out"]) < tol
    for k in ("rgb", "depth", "weights"):
        assert maxabs(out["coarse"][k][0], g["coarse_" + k]) < tol, k
    if kf == 0:
        return []
    rays = torch.from_numpy(g["rays"])
    zc = orc.sample_coarse(rays, kc, g["u_coarse"])
    samps = [zc]
    if kf - kfd > 0:
        samps.append(orc.sample_fine(rays, torch.from_numpy(g["coarse_weights"]), g["u_fine"], g["u_fine2"], kc))
    if kfd > 0:
        samps.append(orc.sample_fine_depth(rays, torch.from_numpy(g["coarse_depth"]), g["g_depth"], 0.01))
    z_ref, _ = torch.sort(torch.cat(samps, -1), -1)
    bad = fine_flip_rays(dbg["z_fine"][0].cpu(), z_ref, torch.from_numpy(g["coarse_weights"]), g["u_fine"])
    assert len(bad) <= max_flips, bad
    good = torch.ones(n, dtype=torch.bool)
    good[bad] = False
    kt = kc + kf
    assert maxabs(dbg["sample_fine"][0].cpu()[good].reshape(-1, 4), g["fine_out"].reshape(n, kt, 4)[good].reshape(-1, 4)) < tol
    for k in ("rgb", "depth", "weights"):
        assert maxabs(out["fine"][k][0].cpu()[good], g["fine_" + k][good]) < tol, k
    assert maxabs(out["fine"]["rgb"][0], g["fine_rgb"]) < 2e-2   # a moved sample changes the quadrature, not the scene
    return bad


# --------------------------------------------------------------------------- relu-safe points / rays (gradient comparisons)
# The backward tests run under two backward arithmetics (fixture legs `dw_f32` / `dw_f16x2`) on the SAME seeded inputs: the
# selection of unambiguous points / rays -- an oracle pass over all candidates on the CPU -- is the same in both legs and is
# remembered per (test, parameters without the leg, call number).
_SELECT_MEMO = {}
_SELECT_CALLS = {}


def _select_key(kind, extra):
    import os
    import re
    cur = os.environ.get("PYTEST_CURRENT_TEST", "")
    leg = re.search(r"\[(dw_f32|dw_f16x2)-?", cur)
    base = re.sub(r"(dw_f32|dw_f16x2)-?", "", cur.split(" ")[0])
    if not leg:
        return None
    cnt_key = (cur.split(" ")[0], kind)
    _SELECT_CALLS[cnt_key] = _SELECT_CALLS.get(cnt_key, 0) + 1
    return (base, kind, _SELECT_CALLS[cnt_key], extra)


def clean_points(sc, xyz, vd, n, ambig=1e-5):
    """First n of the candidate points whose relu inputs (both MLPs, traced through the oracle) all satisfy |h| >= ambig."""
    import pnyolo_oracle as orc
    key = _select_key("points", (int(len(xyz)), int(n), float(ambig), float(np.asarray(xyz, dtype=np.float64).sum())))
    if key is not None and key in _SELECT_MEMO:
        return _SELECT_MEMO[key].copy()
    out = _clean_points(sc, xyz, vd, n, ambig)
    if key is not None:
        _SELECT_MEMO[key] = out.copy()
    return out


def _clean_points(sc, xyz, vd, n, ambig):
    import pnyolo_oracle as orc
    orc.RELU_TRACE = []
    with torch.no_grad():
        orc.query(sc, xyz, vd, coarse=True)
        if sc.mlp_fine is not None:
            orc.query(sc, xyz, vd, coarse=False)
    ok = torch.stack(orc.RELU_TRACE).min(dim=0)[0] >= ambig
    orc.RELU_TRACE = None
    idx = ok.nonzero().flatten()[:n]
    assert idx.numel() == n, "not enough unambiguous candidates (%d of %d)" % (int(ok.sum()), len(xyz))
    return idx.numpy()


def clean_rays(sc, rays, kc, kf, kfd, draws, n, chunk=160, ambig=1e-5, **kw):
    """First n of the candidate rays all of whose samples (coarse and fine pass) are unambiguous.  Rays are independent in the
    oracle, so the candidates are traced chunk by chunk and the search stops once n are found (the oracle on the CPU is what
    these tests spend their time in)."""
    key = _select_key("rays", (int(rays.shape[0]), kc, kf, kfd, int(n), float(ambig), float(np.asarray(rays, dtype=np.float64).sum()),
                               float(np.asarray(draws["u_coarse"], dtype=np.float64).sum())))
    if key is not None and key in _SELECT_MEMO:
        return _SELECT_MEMO[key].copy()
    out = _clean_rays(sc, rays, kc, kf, kfd, draws, n, chunk, ambig, **kw)
    if key is not None:
        _SELECT_MEMO[key] = out.copy()
    return out


def _clean_rays(sc, rays, kc, kf, kfd, draws, n, chunk=160, ambig=1e-5, **kw):
    import pnyolo_oracle as orc
    found, N = [], rays.shape[0]
    for lo in range(0, N, chunk):
        hi = min(N, lo + chunk)
        orc.RELU_TRACE = []
        kw_c = {k: (v[lo:hi] if hasattr(v, "shape") and len(v.shape) > 0 and v.shape[0] == N else v) for k, v in kw.items()}
        with torch.no_grad():
            orc.render(sc, rays[lo:hi], kc, kf, kfd, draws["u_coarse"][lo:hi], draws["u_fine"][lo:hi], draws["u_fine2"][lo:hi],
                       draws["g_depth"][lo:hi], **kw_c)
        ok = torch.ones(hi - lo, dtype=torch.bool)
        for t in orc.RELU_TRACE:                   # (n*K,) per traced relu; K = kc or kc + kf
            ok &= t.reshape(hi - lo, -1).min(dim=1)[0] >= ambig
        orc.RELU_TRACE = None
        found += (ok.nonzero().flatten() + lo).tolist()
        if len(found) >= n:
            return np.asarray(found[:n])
    raise AssertionError("not enough unambiguous rays (%d of %d)" % (len(found), N))


# --------------------------------------------------------------------------- seeded (Philox) draws
def renderer_seed(ren, call=1, sb=0):
    """The seed NeRFRenderer / YoloRenderer document for their `call`-th call from now (render.py: base_seed + 7919 * _calls,
    _calls counted from 1; `+ sb` per object in the per-object super-batch form), written out here a second time."""
    return (int(ren.base_seed) + 7919 * (int(ren._calls) + call) + sb) & 0xFFFFFFFFFFFFFFFF


def clean_ray_mask(sc, rays, kc, kf, kfd, draws, ambig=1e-5, chunk=160, **kw):
    """Boolean (n,) mask of the rays all of whose relu inputs (both passes, traced through the oracle) satisfy |h| >= ambig.
    For seeded renders: a draw depends on the ray's index in the launch, so unclean rays cannot be left out of the launch --
    they are rendered on both sides and given zero loss weight."""
    import pnyolo_oracle as orc
    N = rays.shape[0]
    ok = torch.ones(N, dtype=torch.bool)
    for lo in range(0, N, chunk):
        hi = min(N, lo + chunk)
        orc.RELU_TRACE = []
        with torch.no_grad():
            orc.render(sc, rays[lo:hi], kc, kf, kfd, draws["u_coarse"][lo:hi], draws["u_fine"][lo:hi], draws["u_fine2"][lo:hi],
                       draws["g_depth"][lo:hi], **kw)
        for t in orc.RELU_TRACE:
            ok[lo:hi] &= t.reshape(hi - lo, -1).min(dim=1)[0] >= ambig
        orc.RELU_TRACE = None
    return ok


# The seeded backward comparison (tests/test_gpu_seeded.py) and its CPU-side precondition (tests/test_cpu_philox.py): the scene
# of test_render_backward_vs_oracle (every depth sample inside (near, far)), 96 candidate rays in launch order, the first seed
# of a renderer with base_seed 45: 54 unambiguous rays (base seeds 1..49 give 33..54).  Few samples per ray: a ray is out if ANY
# relu input of its (2 kc + kf) samples x views x units is within the margin.
SEEDED_BWD = dict(ns=2, H=32, W=32, kc=6, kf=4, kfd=2, n=96, net_seed=700, base_seed=45, near=0.3, far=1.8)


def seeded_bwd_case(with_net, base_seed=None, lat_grad=False):
    """(net, sc, rays (n, 8), draws, weight (n,) in {0, 1}, seed): the scenario of SEEDED_BWD.  draws are the oracle's
    restatement of what the kernels generate for the renderer's first call; weight marks the unambiguous rays."""
    import pnyolo_oracle as orc
    c = SEEDED_BWD
    net, sc = scene_pair(c["ns"], c["H"], c["W"], 512, 4, 5, 3, c["net_seed"], with_net=with_net, lat_grad=lat_grad)
    _, tgt = synth.scene_cameras(c["ns"])
    cand = orc.gen_rays(tgt[None], c["W"], c["H"], 0.9 * c["W"], c["near"], c["far"])[0].reshape(-1, 8)
    rays = cand[torch.from_numpy(np.random.RandomState(31).choice(cand.shape[0], c["n"], replace=False))]
    seed = ((c["base_seed"] if base_seed is None else base_seed) + 7919) & 0xFFFFFFFFFFFFFFFF
    draws = orc.seeded_draws(seed, c["n"], c["kc"], c["kf"], c["kfd"])
    weight = clean_ray_mask(sc, rays, c["kc"], c["kf"], c["kfd"], draws).float()
    return net, sc, rays, draws, weight, seed
