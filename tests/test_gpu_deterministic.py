"""The deterministic latent gradient (-m gpu): include/pnyolo.h pny_model_set_deterministic, PixelNeRFNet.set_deterministic.

  * repeatability: three backward passes of one batch with the mode on give bit-identical latent and MLP gradients, for the
    NeRF render on single scenes (side streams) and on the grouped super-batch, the YOLO render on a supplied L = 1792 latent,
    and the query backward, each under the default arithmetic (split f16), F16_TRAIN and F32.  The shapes put thousands of
    samples on a 16 x 16 or 64 x 64 latent: far more than enough for the float-atomic path to reorder its sums;
  * accuracy: within 1e-5 of the gradient's max of the float-atomic path (same inputs, same arithmetic; the MLP gradients are
    bit-identical to that path's), and against autograd through the oracle in float64 at the latent-gradient tests' bar;
  * end to end, the reference's default training graph (trunk trained, SB = 4 objects x 3 views, 128 rays each, 64 + 32
    samples) under torch.use_deterministic_algorithms(True) with the default 'auto' mode: two steps from identical state give
    torch.equal gradients for every trunk and MLP parameter and the latent, and three Adam steps torch.equal parameters;
  * flag plumbing ('auto' follows torch's flag; False under it raises, or warns under warn_only) and bind_parallel(net, [0, 0]).
"""
import os
import warnings

import numpy as np
import pytest
import torch

os.environ.setdefault("CUBLAS_WORKSPACE_CONFIG", ":4096:8")   # (torch's requirement for BLAS under its deterministic flag)

import pnyolo_oracle as orc  # noqa: E402
from helpers import DEV, RTOL, clean_points, dt, grad_check, scene_pair  # noqa: E402
from pixel_nerf_yolo_amd import conf as pconf  # noqa: E402
from pixel_nerf_yolo_amd import synth  # noqa: E402
from pixel_nerf_yolo_amd.model import make_model  # noqa: E402
from pixel_nerf_yolo_amd.render import NeRFRenderer, YoloRenderer  # noqa: E402
from test_gpu_trunk import trunk_net  # noqa: E402

pytestmark = pytest.mark.gpu

PRECISIONS = {"auto": None, "f16_train": "f16_train", "f32": "f32"}


@pytest.fixture
def torch_flag():
    """Restores torch's deterministic flag (and warn_only) after the test."""
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    yield
    torch.use_deterministic_algorithms(was, warn_only=warn)


def clear_env(monkeypatch):
    for var in ("PNYOLO_MLP_PRECISION", "PNYOLO_BWD_PRECISION", "PNYOLO_GROUP", "PNYOLO_SCENE_STREAMS", "PNYOLO_STASH_GB"):
        monkeypatch.delenv(var, raising=False)


def mlp_grads(net):
    return {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None and k.startswith("mlp_")}


# --------------------------------------------------------------------------- the four backward paths
def nerf_case(seed):
    """SB = 2 objects x 2 views, 128 x 128 images (64 x 64 latent that requires grad), 128 rays x (32 + 16) samples each."""
    SB, ns, H, W, kc, kf, kfd, B = 2, 2, 128, 128, 32, 16, 8, 128
    net = make_model(pconf.default_mv()["model"], stop_encoder_grad=True)
    net.mlp_coarse.load_state_dict({k: torch.from_numpy(v) for k, v in synth.mlp_state(seed).items()})
    net.mlp_fine.load_state_dict({k: torch.from_numpy(v) for k, v in synth.mlp_state(seed + 1).items()})
    net = net.to(DEV).train()
    lat = torch.from_numpy(np.concatenate([synth.latent(seed + 2 + i, ns, 512, H // 2, W // 2) for i in range(SB)])).to(DEV)
    lat.requires_grad_()
    poses = np.stack([synth.scene_cameras(ns, radius=1.3 + 0.1 * i)[0] for i in range(SB)])
    focal, cc = torch.tensor(0.9 * W), torch.tensor([[W * 0.5, H * 0.5]])
    net.encode(torch.zeros(SB, ns, 3, H, W), torch.from_numpy(poses), focal, c=cc, latent=lat)
    rs = np.random.RandomState(seed)
    rays = torch.stack([orc.gen_rays(synth.pose_spherical(100.0 + 25 * i, -20.0, 1.3)[None], W, H, 0.9 * W, 0.3, 1.8)[0]
                        .reshape(-1, 8)[torch.from_numpy(rs.choice(H * W, B, replace=False))] for i in range(SB)]).to(DEV)
    n = SB * B
    draws = dict(u_coarse=rs.rand(n, kc).astype(np.float32), u_fine=rs.rand(n, kf - kfd).astype(np.float32),
                 u_fine2=rs.rand(n, kf - kfd).astype(np.float32), g_depth=rs.randn(n, kfd).astype(np.float32))
    gt = torch.from_numpy(rs.uniform(0, 1, size=(SB, B, 3)).astype(np.float32)).to(DEV)
    ren = NeRFRenderer(n_coarse=kc, n_fine=kf, n_fine_depth=kfd, white_bkgd=True).train()

    def step():
        ren.draws = draws
        out = ren(net, rays, want_weights=True)
        (torch.nn.functional.mse_loss(out["coarse"]["rgb"], gt) + torch.nn.functional.mse_loss(out["fine"]["rgb"], gt)).backward()
    return net, lat, step


def yolo_case(seed):
    """YOLO mode, a supplied L = 1792 latent (2 views, 16 x 16) that requires grad, 768 rays x 32 samples."""
    K = 32
    net, _ = scene_pair(2, 64, 64, 1792, 21, 5, 3, seed, yolo=True, lat_hw=(16, 16), lat_grad=True)
    _, tgt_c2w = synth.scene_cameras(2, radius=4.0, phi=-25.0)
    tgt_w2c = np.linalg.inv(tgt_c2w @ np.diag([1.0, -1.0, -1.0, 1.0]).astype(np.float32)).astype(np.float32)
    rays = orc.gen_rays_yolo(tgt_w2c[None], 32, 24, [10.0, 11.0], [16.0, 12.0], 1.0, 6.0)[0].reshape(-1, 8).to(DEV)
    rs = np.random.RandomState(seed)
    u = rs.rand(rays.shape[0], K).astype(np.float32)
    G = torch.from_numpy(rs.standard_normal((rays.shape[0], 3, 7)).astype(np.float32)).to(DEV)
    ren = YoloRenderer(K, 128, 1, 3)
    ren.bind_parallel(net)

    def step():
        ren.draws = dict(u_coarse=u)
        (ren(rays[None]) * G).sum().backward()
    return net, net.test_latent, step


def query_case(seed, n=4096):
    """net(xyz) on n points along rays of a target view, 2 views, 64 x 64 latent."""
    net, _ = scene_pair(2, 128, 128, 512, 4, 5, 3, seed, lat_grad=True)
    _, tgt = synth.scene_cameras(2)
    rs = np.random.RandomState(seed)
    r = orc.gen_rays(tgt[None], 128, 128, 115.2, 0.3, 1.8)[0].reshape(-1, 8)[torch.from_numpy(rs.choice(128 * 128, n, replace=False))]
    t = torch.from_numpy(rs.uniform(0.8, 1.8, size=(n, 1)).astype(np.float32))
    xyz = (r[:, :3] + t * r[:, 3:6]).to(DEV)
    vd = r[:, 3:6].contiguous().to(DEV)
    G = torch.from_numpy(rs.standard_normal((n, 4)).astype(np.float32)).to(DEV)

    def step():
        (net(xyz[None], coarse=True, viewdirs=vd[None])[0] * G).sum().backward()
    return net, net.test_latent, step


def make_case(path, seed):
    if path in ("render", "group"):
        return nerf_case(seed)   # (PNYOLO_GROUP decides the grouped scene at encode())
    return yolo_case(seed) if path == "yolo" else query_case(seed)


def run(net, lat, step):
    lat.grad = None
    for p in net.parameters():
        p.grad = None
    step()
    torch.cuda.synchronize()
    return lat.grad.clone(), mlp_grads(net)


@pytest.mark.parametrize("prec", list(PRECISIONS))
@pytest.mark.parametrize("path", ["render", "group", "yolo", "query"])
def test_latent_gradient_bit_repeatable(path, prec, monkeypatch):
    clear_env(monkeypatch)
    monkeypatch.setenv("PNYOLO_GROUP", "1" if path == "group" else "0")
    net, lat, step = make_case(path, 5100)
    if PRECISIONS[prec]:
        net.set_matrix_precision(PRECISIONS[prec])
    net.set_deterministic(True)
    runs = [run(net, lat, step) for _ in range(3)]
    assert net.last_latent_grad_deterministic()
    if path != "yolo":
        assert net.last_backward_precision() == {"auto": "f16x2", "f16_train": "f16", "f32": "f32"}[prec]
    g0, m0 = runs[0]
    assert float(g0.abs().max()) > 0 and len(m0) >= (20 if path in ("yolo", "query") else 60)
    for g, m in runs[1:]:
        assert torch.equal(g, g0), "latent gradient differs by %.3e" % float((g - g0).abs().max())
        assert all(torch.equal(m[k], m0[k]) for k in m0)


@pytest.mark.parametrize("prec", list(PRECISIONS))
@pytest.mark.parametrize("path", ["render", "group", "yolo", "query"])
def test_latent_gradient_matches_the_atomic_path(path, prec, monkeypatch):
    """Same inputs, same arithmetic: the deterministic sum within 1e-5 of the gradient's max of the float-atomic one; the MLP
    gradients (which the mode does not touch) bit-identical."""
    clear_env(monkeypatch)
    monkeypatch.setenv("PNYOLO_GROUP", "1" if path == "group" else "0")
    net, lat, step = make_case(path, 5200)
    if PRECISIONS[prec]:
        net.set_matrix_precision(PRECISIONS[prec])
    net.set_deterministic(False)
    g_at, m_at = run(net, lat, step)
    assert not net.last_latent_grad_deterministic()
    net.set_deterministic(True)
    g_det, m_det = run(net, lat, step)
    assert net.last_latent_grad_deterministic()
    scale = float(g_at.abs().max())
    err = float((g_det - g_at).abs().max())
    print("%s %s: deterministic vs atomic latent gradient %.2e of its max" % (path, prec, err / scale))
    assert scale > 0 and err <= 1e-5 * scale
    assert all(torch.equal(m_det[k], m_at[k]) for k in m_at)


def test_latent_gradient_vs_fp64_oracle(monkeypatch):
    """Mode on, fp32 arithmetic, points clear of every relu kink: d loss / d latent against torch.autograd through the oracle
    in float64 within RTOL of its max (the bar of tests/test_gpu_grad_shapes.py)."""
    clear_env(monkeypatch)
    monkeypatch.setenv("PNYOLO_MLP_PRECISION", "f32")
    monkeypatch.setenv("PNYOLO_BWD_PRECISION", "f32")
    n = 600
    net, sc = scene_pair(2, 32, 32, 512, 4, 5, 3, 5300, lat_hw=(8, 8), lat_grad=True, dtype=torch.float64)
    net.set_deterministic(True)
    rs = np.random.RandomState(5301)
    xyz = rs.uniform(-0.5, 0.5, size=(3 * n, 3)).astype(np.float32)
    vd = rs.standard_normal((3 * n, 3)).astype(np.float32)
    keep = clean_points(sc, xyz, vd, n)
    xyz, vd = xyz[keep], vd[keep]
    G = rs.standard_normal((n, 4)).astype(np.float32)
    (net(dt(xyz)[None], coarse=True, viewdirs=dt(vd)[None])[0] * dt(G)).sum().backward()
    torch.cuda.synchronize()
    assert net.last_latent_grad_deterministic()
    ref = orc.query(sc, xyz, vd, coarse=True)
    (ref * torch.from_numpy(G).to(ref.dtype)).sum().backward()
    grad_check("latent", net.test_latent.grad.cpu().double(), sc.latent.grad, RTOL)


# --------------------------------------------------------------------------- end to end, trunk trained
def trunk_case(seed, SB=4, NS=3, B=128, H=128, W=128, kc=64, kf=32, kfd=16):
    """The reference's default training graph: trunk trained (batch statistics), SB objects x NS views, B rays each."""
    net, _ = trunk_net(seed, True, mlp_seed=seed + 1)
    images = torch.from_numpy(synth.images(seed + 2, SB * NS, H, W)).reshape(SB, NS, 3, H, W)
    poses = torch.from_numpy(np.stack([synth.scene_cameras(NS, radius=1.3 + 0.1 * i)[0] for i in range(SB)]))
    focal, cc = torch.tensor(0.9 * W), torch.tensor([[W * 0.5, H * 0.5]])
    rs = np.random.RandomState(seed + 3)
    rays = torch.stack([orc.gen_rays(synth.pose_spherical(100.0 + 25 * i, -20.0, 1.3)[None], W, H, 0.9 * W, 0.3, 1.8)[0]
                        .reshape(-1, 8)[torch.from_numpy(rs.choice(H * W, B, replace=False))] for i in range(SB)]).to(DEV)
    n = SB * B
    draws = dict(u_coarse=rs.rand(n, kc).astype(np.float32), u_fine=rs.rand(n, kf - kfd).astype(np.float32),
                 u_fine2=rs.rand(n, kf - kfd).astype(np.float32), g_depth=rs.randn(n, kfd).astype(np.float32))
    gt = torch.from_numpy(rs.uniform(0, 1, size=(SB, B, 3)).astype(np.float32)).to(DEV)
    ren = NeRFRenderer(n_coarse=kc, n_fine=kf, n_fine_depth=kfd, white_bkgd=True).train()
    state = {k: v.clone() for k, v in net.state_dict().items()}

    def step(call=None):
        net.encode(images, poses, focal, c=cc)
        lat = net.differentiable_latent()
        lat.retain_grad()
        ren.draws = draws
        out = (call or (lambda r, want_weights: ren(net, r, want_weights)))(rays, want_weights=True)
        loss = torch.nn.functional.mse_loss(out["coarse"]["rgb"], gt) + torch.nn.functional.mse_loss(out["fine"]["rgb"], gt)
        loss.backward()
        torch.cuda.synchronize()
        return lat
    return net, ren, state, step


def all_grads(net):
    return {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}


def test_end_to_end_training_is_bit_reproducible(torch_flag, monkeypatch):
    clear_env(monkeypatch)
    torch.use_deterministic_algorithms(True)
    net, ren, state, step = trunk_case(5400)
    assert net._deterministic == "auto"
    runs = []
    for _ in range(2):
        net.load_state_dict(state)
        net.zero_grad(set_to_none=True)
        lat = step()
        runs.append((lat.grad.clone(), all_grads(net)))
    assert net.last_latent_grad_deterministic()
    (l0, g0), (l1, g1) = runs
    n_trunk = sum(k.startswith("encoder.") for k in g0)
    n_mlp = sum(k.startswith("mlp_") for k in g0)
    assert n_trunk >= 80 and n_mlp >= 60 and set(g0) == set(g1)
    assert torch.equal(l0, l1), "latent gradient differs by %.3e" % float((l0 - l1).abs().max())
    bad = [k for k in g0 if not torch.equal(g0[k], g1[k])]
    assert not bad, "%d of %d parameter gradients differ: %s" % (len(bad), len(g0), bad[:5])
    # three Adam steps from identical state, twice
    finals = []
    for _ in range(2):
        net.load_state_dict(state)
        opt = torch.optim.Adam([p for p in net.parameters() if p.requires_grad], lr=1e-4)
        for _ in range(3):
            opt.zero_grad(set_to_none=True)
            step()
            opt.step()
        torch.cuda.synchronize()
        finals.append({k: v.clone() for k, v in net.state_dict().items()})
    bad = [k for k in finals[0] if not torch.equal(finals[0][k], finals[1][k])]
    assert not bad, "%d of %d tensors differ after three Adam steps: %s" % (len(bad), len(finals[0]), bad[:5])


def test_bind_parallel_replicas_inherit_the_mode(monkeypatch):
    """bind_parallel(net, [0, 0]): two replicas, each with half of the rays; two trunk-trained steps with the mode on give
    bit-identical gradients."""
    clear_env(monkeypatch)
    net, ren, state, step = trunk_case(5500, SB=2, NS=2, B=128, H=64, W=64, kc=32, kf=16, kfd=8)
    net.set_deterministic(True)
    call = ren.bind_parallel(net, [0, 0])
    runs = []
    for _ in range(2):
        net.load_state_dict(state)
        net.zero_grad(set_to_none=True)
        lat = step(call)
        runs.append((lat.grad.clone(), all_grads(net)))
    assert all(r is None or r._deterministic is True for r in call._replicas)
    assert any(r is not None and r is not net and r.last_latent_grad_deterministic() for r in call._replicas)
    (l0, g0), (l1, g1) = runs
    assert torch.equal(l0, l1)
    assert len(g0) >= 140 and all(torch.equal(g0[k], g1[k]) for k in g0)


# --------------------------------------------------------------------------- flag plumbing
def test_auto_follows_torch_flag_and_explicit_false_raises(torch_flag, monkeypatch):
    clear_env(monkeypatch)
    net, lat, step = query_case(5600, n=1024)
    assert net._deterministic == "auto"
    torch.use_deterministic_algorithms(False)
    run(net, lat, step)
    assert not net.last_latent_grad_deterministic()
    torch.use_deterministic_algorithms(True)
    run(net, lat, step)
    assert net.last_latent_grad_deterministic()
    torch.use_deterministic_algorithms(False)      # back to the atomic path
    run(net, lat, step)
    assert not net.last_latent_grad_deterministic()
    net.set_deterministic(True)                    # explicit True without torch's flag
    run(net, lat, step)
    assert net.last_latent_grad_deterministic()
    net.set_deterministic(False)
    torch.use_deterministic_algorithms(True)
    with pytest.raises(RuntimeError, match="deterministic"):
        run(net, lat, step)
    torch.use_deterministic_algorithms(True, warn_only=True)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        g, _ = run(net, lat, step)
    assert any("deterministic" in str(x.message) for x in w)
    assert not net.last_latent_grad_deterministic() and float(g.abs().max()) > 0
    torch.use_deterministic_algorithms(False)
    net.set_deterministic("auto")
    run(net, lat, step)
    assert not net.last_latent_grad_deterministic()
