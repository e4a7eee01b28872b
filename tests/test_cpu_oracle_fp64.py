"""The oracle's trunk in float64 (spatial_encoder(dtype=torch.float64)), the arbiter of tests/test_gpu_trunk.py, against its
default float32 arithmetic (which tests/test_oracle_golden.py holds to the reference): the same function to fp32 rounding,
forward and autograd.  CPU only."""
import numpy as np
import pytest
import torch

import pnyolo_oracle as orc
from pixel_nerf_yolo_amd import synth


def _state(enc, dtype):
    return {k: torch.from_numpy(v.copy()).to(dtype).requires_grad_("running" not in k)
            for k, v in enc.items() if "num_batches" not in k}


@pytest.mark.parametrize("training", [False, True])
def test_oracle_trunk_fp64_matches_fp32(training):
    n, H, W = 2, 32, 40
    enc = synth.resnet34_state(1803, residual_gain=0.25)
    images = synth.images(1804, n, H, W)
    G = torch.from_numpy(np.random.RandomState(5).standard_normal((n, 512, H // 2, W // 2)))
    sd32, sd64 = _state(enc, torch.float32), _state(enc, torch.float64)
    lat32, lv32 = orc.spatial_encoder(sd32, images, training=training)
    lat64, lv64 = orc.spatial_encoder(sd64, images, training=training, dtype=torch.float64)
    assert lat32.dtype == torch.float32 and lat64.dtype == torch.float64 and all(t.dtype == torch.float64 for t in lv64)
    # the default is the float32 arithmetic itself, bit for bit
    sd32b = _state(enc, torch.float32)
    assert torch.equal(orc.spatial_encoder(sd32b, images, training=training, dtype=torch.float32)[0], lat32)
    scale = max(1.0, float(lat64.abs().max()))
    assert float((lat32.double() - lat64).abs().max()) <= 1e-5 * scale
    (lat32 * G.float()).sum().backward()
    (lat64 * G).sum().backward()
    checked = 0
    for k, t in sd64.items():
        if t.grad is None:
            assert k.startswith(("encoder.model.layer4", "encoder.model.fc")) or "running" in k, k
            continue
        g32 = sd32[k].grad.double()
        assert float((g32 - t.grad).abs().max()) <= 2e-5 * float(t.grad.abs().max()), k
        checked += 1
    assert checked >= 80
    # batch statistics step the float64 running statistics in place, as they step the float32 ones
    for k, t in sd64.items():
        if "running" in k and not k.startswith("encoder.model.layer4"):
            moved = not torch.equal(t, torch.from_numpy(enc[k]).double())
            assert moved == training, k
            assert float((sd32[k].double() - t).abs().max()) <= 1e-6 * max(1.0, float(t.abs().max())), k


def test_oracle_trunk_fp64_gradients_reach_fp32_leaves():
    """Leaves of another dtype are converted differentiably: fp32 parameters receive the fp64 graph's gradients."""
    enc = synth.resnet34_state(1803, residual_gain=0.25)
    sd32 = _state(enc, torch.float32)
    lat = orc.spatial_encoder(sd32, synth.images(1804, 1, 32, 32), dtype=torch.float64)[0]
    assert lat.dtype == torch.float64
    lat.sum().backward()
    assert sd32["encoder.model.conv1.weight"].grad is not None
    assert sd32["encoder.model.conv1.weight"].grad.dtype == torch.float32


# --------------------------------------------------------------------------- query / render (the MLP side)
def _mlp_scene(dtype, yolo, L, d_out, seed):
    """One seeded scene whose MLP parameters and latent are leaves of `dtype` (the float64 arbiter of tests/test_gpu_grad_shapes.py
    against the default float32 arithmetic)."""
    ns, H, W = 2, 32, 40
    mc = {k: torch.from_numpy(v).to(dtype).requires_grad_() for k, v in synth.mlp_state(seed, d_latent=L, d_out=d_out).items()}
    mf = None if yolo else {k: torch.from_numpy(v).to(dtype).requires_grad_()
                            for k, v in synth.mlp_state(seed + 1, d_latent=L, d_out=d_out).items()}
    lat = torch.from_numpy(synth.latent(seed + 2, ns, L, 8, 12)).to(dtype).requires_grad_()
    if yolo:
        # world->cam extrinsics of cameras looking down -z: the scene lies at z < 0, where YOLO mode keeps the latent
        # (models.py:224,254-264 zero it at z >= 0)
        c2w, _ = synth.scene_cameras(ns, radius=4.0, phi=-25.0)
        poses = np.stack([np.linalg.inv(p) for p in c2w]).astype(np.float32)
        focal, cc = torch.tensor([[40.0, 44.0]]), torch.tensor([[W * 0.5, H * 0.5 - 2]])
    else:
        poses, _ = synth.scene_cameras(ns)
        focal, cc = torch.tensor(0.9 * W), torch.tensor([[W * 0.5, H * 0.5]])
    sc = orc.Scene(mc, mf, lat, poses, focal, cc, W, H, yolo=yolo, dtype=None if dtype == torch.float32 else dtype)
    sc.mlp_coarse, sc.mlp_fine, sc.latent = mc, mf, lat      # Scene() re-wraps tensors: keep the leaves
    return sc


def _leaves(sc):
    out = {"latent": sc.latent}
    for pre in ("mlp_coarse", "mlp_fine"):
        for k, v in (getattr(sc, pre) or {}).items():
            out[pre + "." + k] = v
    return out


def _agree(sc32, sc64, y32, y64, fwd_tol=2e-5, grad_tol=5e-5):
    """fp32 and fp64 of the same function: outputs within fp32 rounding, every gradient tensor within a few 1e-5 of its max."""
    assert y32.dtype == torch.float32 and y64.dtype == torch.float64
    assert float((y32.double() - y64).abs().max()) <= fwd_tol * max(1.0, float(y64.abs().max()))
    G = torch.from_numpy(np.random.RandomState(7).standard_normal(tuple(y64.shape)))
    (y32 * G.float()).sum().backward()
    (y64 * G).sum().backward()
    l32, l64 = _leaves(sc32), _leaves(sc64)
    checked = 0
    for k, t in l64.items():
        assert (t.grad is None) == (l32[k].grad is None), k
        if t.grad is None:          # a query of the coarse MLP leaves the fine one alone
            assert k.startswith("mlp_fine."), k
            continue
        assert t.grad.dtype == torch.float64, k
        g32 = l32[k].grad.double()
        checked += 1
        assert float((g32 - t.grad).abs().max()) <= grad_tol * max(float(t.grad.abs().max()), 1e-30), k
    assert checked >= 30 and float(l64["latent"].grad.abs().max()) > 0


def test_oracle_query_render_fp64_matches_fp32():
    """NeRF head: a query and a coarse + fine render with attached depth samples; the fp64 scene's traced pre-activations are
    float64 (the relu-ambiguity selection of the GPU sweeps traces the arbiter's own arithmetic)."""
    rs = np.random.RandomState(3)
    xyz, vd = rs.uniform(-0.5, 0.5, size=(50, 3)).astype(np.float32), rs.standard_normal((50, 3)).astype(np.float32)
    sc32, sc64 = _mlp_scene(torch.float32, False, 512, 4, 61), _mlp_scene(torch.float64, False, 512, 4, 61)
    orc.RELU_TRACE = []
    try:
        y64 = orc.query(sc64, xyz, vd)
        assert orc.RELU_TRACE and all(t.dtype == torch.float64 for t in orc.RELU_TRACE)
    finally:
        orc.RELU_TRACE = None
    _agree(sc32, sc64, orc.query(sc32, xyz, vd), y64)
    # the default is the float32 arithmetic itself, bit for bit
    assert torch.equal(orc.query(sc32, xyz, vd, dtype=torch.float32), orc.query(sc32, xyz, vd))

    _, tgt = synth.scene_cameras(2)
    n, kc, kf, kfd = 12, 16, 8, 4
    rays = orc.gen_rays(tgt[None], 40, 32, 36.0, 0.3, 1.8)[0].reshape(-1, 8)[torch.from_numpy(rs.choice(32 * 40, n, replace=False))]
    dr = dict(u_coarse=rs.rand(n, kc).astype(np.float32), u_fine=rs.rand(n, kf - kfd).astype(np.float32),
              u_fine2=rs.rand(n, kf - kfd).astype(np.float32), g_depth=rs.randn(n, kfd).astype(np.float32))
    sc32, sc64 = _mlp_scene(torch.float32, False, 512, 4, 71), _mlp_scene(torch.float64, False, 512, 4, 71)

    def ren(sc):
        r = orc.render(sc, rays, kc, kf, kfd, dr["u_coarse"], dr["u_fine"], dr["u_fine2"], dr["g_depth"])
        return torch.cat([r[p][k].reshape(n, -1) for p in ("coarse", "fine") for k in ("rgb", "depth")], 1)
    r32, r64 = ren(sc32), ren(sc64)
    _agree(sc32, sc64, r32, r64)


def test_oracle_yolo_render_fp64_matches_fp32():
    """YOLO head: d_out 21, L 1792, points behind a camera culled (their latent rows are zero on both sides)."""
    rs = np.random.RandomState(4)
    n, kc = 40, 12
    o = rs.standard_normal((n, 3))
    o = 7.0 * o / np.linalg.norm(o, axis=1, keepdims=True)
    d = -o / 7.0 + 0.1 * rs.standard_normal((n, 3))        # from behind the cameras through the middle of the scene
    rays = torch.from_numpy(np.concatenate([o, d, np.full((n, 1), 0.5), np.full((n, 1), 12.0)], 1).astype(np.float32))
    u = rs.rand(n, kc).astype(np.float32)
    sc32, sc64 = _mlp_scene(torch.float32, True, 1792, 21, 81), _mlp_scene(torch.float64, True, 1792, 21, 81)
    # rays none of whose relu units is within fp32 rounding of zero (the gradient is discontinuous there)
    orc.RELU_TRACE = []
    try:
        with torch.no_grad():
            orc.yolo_render(sc64, rays, kc, u)
        ok = torch.stack([t.reshape(n, -1).min(dim=1)[0] for t in orc.RELU_TRACE]).min(dim=0)[0] >= 1e-5
    finally:
        orc.RELU_TRACE = None
    keep = ok.nonzero().flatten()[:12]
    assert keep.numel() == 12
    rays, u = rays[keep], u[keep.numpy()]
    r64 = orc.yolo_render(sc64, rays, kc, u)
    pts = (r64["z"].unsqueeze(2) * rays[:, None, 3:6].double() + rays[:, None, :3].double()).reshape(-1, 3)
    zc = torch.einsum("vij,pj->vpi", sc64.w2c[:, :, :3], pts)[..., 2] + sc64.w2c[:, None, 2, 3]
    assert int((zc >= 0).sum()) > 0 and int((zc < 0).sum()) > 0      # culled and live samples both occur
    _agree(sc32, sc64, orc.yolo_render(sc32, rays, kc, u)["out"], r64["out"])
