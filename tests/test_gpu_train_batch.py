"""The training batch sampler on the GPU (-m gpu): util.sample_train_batch -> pny_sample_train_batch -> train_batch_kernel.

  * replay of tests/golden/train_batch.npz (the reference's trainer on CPU, tools/make_train_batch_golden.py): pix exact,
    rgb_gt bit-equal to the reference's, rays bit-equal to this package's gen_rays at those pixels and within 1e-6 of the
    reference's (the bar test_gen_rays_golden sets for the same arithmetic);
  * seeded: pix equal to the CPU restatement (tests/train_batch_ref.py), every pixel inside its box / the image, the same
    seed the same bits, another seed another batch, object s of a four-object call equal to a one-object call at
    draw_offset = s * B, torch.manual_seed governing seed=None; NV = 1, SB = 1, B = 1, 128 and 1000, H != W;
  * through the trainer's call: one training step (grouped scene, SB = 2) fed by sample_train_batch(draws=...) against
    one fed by the reference-style preparation with the same draws -- coarse / fine rgb and every MLP gradient bit-equal
    under set_deterministic(True);
  * no hidden waiting: the call returns while its stream is still busy behind work enqueued before it.
"""
import numpy as np
import pytest
import torch

import train_batch_ref as tb
from helpers import DEV
from pixel_nerf_yolo_amd import conf as pconf
from pixel_nerf_yolo_amd import synth
from pixel_nerf_yolo_amd.model import make_model
from pixel_nerf_yolo_amd.render import NeRFRenderer
from pixel_nerf_yolo_amd.util import gen_rays, sample_train_batch

pytestmark = pytest.mark.gpu

CASES = ("a_uni", "a_box", "b_uni", "b_box")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def fixture_inputs(g, key):
    case, mode = key.split("_")
    focal = torch.from_numpy(g[case + "_focal"])
    focal = focal.reshape(()) if focal.numel() == 1 else focal                 # a: the scalar; b: (SB, 2)
    c = torch.from_numpy(g[case + "_c"]) if case + "_c" in g else None
    bboxes = torch.from_numpy(g[case + "_bboxes"]) if mode == "box" else None
    names = ("image_ids", "u_x", "u_y") if mode == "box" else ("pix_inds",)
    draws = {n: torch.from_numpy(g["%s_%s" % (key, n)]) for n in names}
    return torch.from_numpy(g[case + "_images"]), torch.from_numpy(g[case + "_poses"]), focal, c, bboxes, draws


def own_rays_at(poses, W, H, focal, z_near, z_far, c, pix):
    """This package's gen_rays of every view of every object, gathered at pix (SB, B, 3) [view, y, x]."""
    SB = poses.shape[0]
    out = []
    for s in range(SB):
        f = focal if focal.dim() == 0 or focal.shape[0] != SB else focal[s]
        cc = None if c is None else (c if c.dim() == 1 or c.shape[0] != SB else c[s])
        full = gen_rays(poses[s], W, H, f, z_near, z_far, c=cc, device=DEV)
        p = pix[s].long()
        out.append(full[p[:, 0], p[:, 1], p[:, 2]])
    return torch.stack(out)


# --------------------------------------------------------------------------- replay of the reference's batches
@pytest.mark.parametrize("where", ["cpu_inputs", "gpu_inputs"])
@pytest.mark.parametrize("key", CASES)
def test_replay_of_the_reference_batches(golden, key, where):
    g = golden("train_batch")
    SB, NV, H, W, B = (int(v) for v in g["shape"])
    z_near, z_far = float(g["z"][0]), float(g["z"][1])
    images, poses, focal, c, bboxes, draws = fixture_inputs(g, key)
    if where == "gpu_inputs":
        poses, focal = poses.to(DEV), focal.to(DEV)
        c, bboxes = (None if c is None else c.to(DEV)), (None if bboxes is None else bboxes.to(DEV))
        draws = {k: v.to(DEV) for k, v in draws.items()}
    rays, rgb, pix = sample_train_batch(images.to(DEV), poses, focal, z_near, z_far, B, c=c, bboxes=bboxes, draws=draws)
    torch.cuda.synchronize()
    assert rays.shape == (SB, B, 8) and rgb.shape == (SB, B, 3) and pix.shape == (SB, B, 3) and pix.dtype == torch.int32
    assert np.array_equal(pix.cpu().numpy(), g[key + "_pix"])
    assert torch.equal(bits(rgb), bits(torch.from_numpy(g[key + "_rgb_gt"])))
    own = own_rays_at(poses.cpu(), W, H, focal.cpu(), z_near, z_far, None if c is None else c.cpu(), pix)
    assert torch.equal(bits(rays), bits(own))
    err = float((rays.cpu() - torch.from_numpy(g[key + "_rays"])).abs().max())
    print("%s: rays max |sampled - reference| = %.3e" % (key, err))
    assert err < 1e-6


def test_replay_clamps_out_of_range_draws(golden):
    """Replayed values outside their range land on the nearest valid pixel (nothing is read out of bounds)."""
    g = golden("train_batch")
    SB, NV, H, W, B = (int(v) for v in g["shape"])
    images, poses, focal, c, _, _ = fixture_inputs(g, "a_uni")
    bad = torch.tensor([[-5, NV * H * W, 2 ** 40, 7]] * SB)
    _, _, pix = sample_train_batch(images.to(DEV), poses, focal, 0.8, 1.8, 4, draws={"pix_inds": bad})
    assert pix[0].cpu().tolist() == [[0, 0, 0], [NV - 1, H - 1, W - 1], [NV - 1, H - 1, W - 1], [0, 0, 7]]
    boxes = torch.tensor([-3.0, -2.0, W + 4.0, H + 9.0]).expand(SB, NV, 4)
    _, _, pix = sample_train_batch(images.to(DEV), poses, focal, 0.8, 1.8, 2, bboxes=boxes,
                                   draws={"image_ids": torch.tensor([[-1, NV + 3]] * SB), "u_x": torch.tensor([[0.0, 0.999]] * SB),
                                          "u_y": torch.tensor([[0.0, 0.999]] * SB)})
    assert pix[1].cpu().tolist() == [[0, 0, 0], [NV - 1, H - 1, W - 1]]


# --------------------------------------------------------------------------- seeded
def seeded_scene(SB, NV, H, W, seed, focal_kind):
    images = torch.from_numpy(synth.images(seed, SB * NV, H, W)).reshape(SB, NV, 3, H, W).to(DEV)
    poses = torch.from_numpy(np.stack([np.stack([synth.pose_spherical(29.0 * v + 13.0 * s, -15.0 - 2.0 * v, 1.2 + 0.1 * s)
                                                 for v in range(NV)]) for s in range(SB)])).to(DEV)
    rs = np.random.RandomState(seed)
    if focal_kind == "scalar":
        focal, c = torch.tensor(0.9 * W), None
    elif focal_kind == "per_object":
        focal, c = torch.from_numpy(rs.uniform(0.8 * W, 1.1 * W, size=SB).astype(np.float32)), torch.tensor([W * 0.45, H * 0.55])
    else:
        focal = torch.from_numpy(rs.uniform(0.8 * W, 1.1 * W, size=(SB, 2)).astype(np.float32))
        c = torch.from_numpy(rs.uniform(0.4, 0.6, size=(SB, 2)).astype(np.float32) * np.array([W, H], dtype=np.float32))
    lo = np.stack([rs.randint(0, W // 2, size=(SB, NV)), rs.randint(0, H // 2, size=(SB, NV))], -1)
    hi = lo + np.stack([rs.randint(0, W // 2, size=(SB, NV)), rs.randint(0, H // 2, size=(SB, NV))], -1)
    boxes = torch.from_numpy(np.concatenate([lo, hi], -1).astype(np.float32))     # cmin rmin cmax rmax, inside the image
    return images, poses, focal, c, boxes


SHAPES = [   # SB, NV, H, W, B, focal
    (4, 5, 24, 16, 128, "scalar"),
    (1, 1, 16, 24, 1, "per_object"),
    (1, 3, 20, 12, 1000, "pair"),
    (3, 1, 12, 20, 128, "pair"),
    (4, 50, 128, 128, 128, "per_object"),     # the SRN training shape
    (2, 7, 30, 40, 1000, "scalar"),
]


@pytest.mark.parametrize("mode", ["uniform", "bbox"])
@pytest.mark.parametrize("SB,NV,H,W,B,focal_kind", SHAPES)
def test_seeded_batches(SB, NV, H, W, B, focal_kind, mode):
    seed = 2 ** 40 + 7 + 13 * B
    images, poses, focal, c, boxes = seeded_scene(SB, NV, H, W, 8100 + B, focal_kind)
    bb = boxes if mode == "bbox" else None
    rays, rgb, pix = sample_train_batch(images, poses, focal, 0.5, 2.5, B, c=c, bboxes=bb, seed=seed)
    torch.cuda.synchronize()
    p = pix.cpu().numpy()
    assert np.array_equal(p, tb.seeded_pix(seed, SB, B, NV, H, W, bboxes=None if bb is None else bb.numpy()))
    assert p[..., 0].min() >= 0 and p[..., 0].max() < NV and p[..., 1].min() >= 0 and p[..., 1].max() < H
    assert p[..., 2].min() >= 0 and p[..., 2].max() < W
    if bb is not None:
        box = bb.numpy()[np.arange(SB)[:, None], p[..., 0]]
        assert bool(((p[..., 2] >= box[..., 0]) & (p[..., 2] <= box[..., 2]) & (p[..., 1] >= box[..., 1]) & (p[..., 1] <= box[..., 3])).all())
    # the rays and colours of those pixels
    own = own_rays_at(poses.cpu(), W, H, focal, 0.5, 2.5, c, pix)
    assert torch.equal(bits(rays), bits(own))
    pl = pix.long()
    s_idx = torch.arange(SB, device=DEV)[:, None].expand(SB, B)
    want = images[s_idx, pl[..., 0], :, pl[..., 1], pl[..., 2]] * 0.5 + 0.5
    assert torch.equal(bits(rgb), bits(want))
    # same seed, same bits; another seed, another batch
    rays2, rgb2, pix2 = sample_train_batch(images, poses, focal, 0.5, 2.5, B, c=c, bboxes=bb, seed=seed)
    assert torch.equal(pix2, pix) and torch.equal(bits(rays2), bits(rays)) and torch.equal(bits(rgb2), bits(rgb))
    if NV * H * W > 1000 or B > 100:
        _, _, pix3 = sample_train_batch(images, poses, focal, 0.5, 2.5, B, c=c, bboxes=bb, seed=seed + 1)
        assert not torch.equal(pix3, pix)


@pytest.mark.parametrize("mode", ["uniform", "bbox"])
def test_an_objects_batch_does_not_depend_on_the_others(mode):
    SB, NV, H, W, B, seed = 4, 5, 24, 16, 128, 991
    images, poses, focal, c, boxes = seeded_scene(SB, NV, H, W, 8200, "pair")
    bb = boxes if mode == "bbox" else None
    rays, rgb, pix = sample_train_batch(images, poses, focal, 0.5, 2.5, B, c=c, bboxes=bb, seed=seed)
    for s in range(SB):
        r1, g1, p1 = sample_train_batch(images[s:s + 1], poses[s:s + 1], focal[s:s + 1], 0.5, 2.5, B, c=c[s:s + 1],
                                        bboxes=None if bb is None else bb[s:s + 1], seed=seed, draw_offset=s * B)
        assert torch.equal(p1[0], pix[s]) and torch.equal(bits(r1[0]), bits(rays[s])) and torch.equal(bits(g1[0]), bits(rgb[s]))
    if mode == "uniform":      # without the offset the lone object draws object 0's pixels
        _, _, p0 = sample_train_batch(images[2:3], poses[2:3], focal[2:3], 0.5, 2.5, B, c=c[2:3], seed=seed)
        assert torch.equal(p0[0], pix[0]) and not torch.equal(p0[0], pix[2])


def test_default_seed_follows_torch_manual_seed():
    images, poses, focal, c, _ = seeded_scene(2, 5, 24, 16, 8300, "scalar")
    torch.manual_seed(77)
    _, _, a = sample_train_batch(images, poses, focal, 0.5, 2.5, 128)
    _, _, b = sample_train_batch(images, poses, focal, 0.5, 2.5, 128)
    torch.manual_seed(77)
    _, _, a2 = sample_train_batch(images, poses, focal, 0.5, 2.5, 128)
    assert torch.equal(a, a2) and not torch.equal(a, b)          # one fresh seed per call


# --------------------------------------------------------------------------- through the trainer's call
def reference_style_batch(images, poses, focal, c, z_near, z_far, pix_inds):
    """PixelNerfTrainer.calc_losses:84-123 on this package's parent API: per-object gen_rays, the NHWC copy, two gathers."""
    SB, NV, _, H, W = images.shape
    all_rays, all_rgb = [], []
    for obj in range(SB):
        images_0to1 = images[obj] * 0.5 + 0.5
        cam_rays = gen_rays(poses[obj], W, H, focal[obj], z_near, z_far, c=None if c is None else c[obj])
        rgb_gt_all = images_0to1.permute(0, 2, 3, 1).contiguous().reshape(-1, 3)
        all_rgb.append(rgb_gt_all[pix_inds[obj]])
        all_rays.append(cam_rays.view(-1, 8)[pix_inds[obj]].to(device=images.device))
    return torch.stack(all_rays), torch.stack(all_rgb)


def test_training_step_fed_by_the_sampler_equals_the_reference_style_step(monkeypatch):
    for var in ("PNYOLO_MLP_PRECISION", "PNYOLO_BWD_PRECISION", "PNYOLO_SCENE_STREAMS", "PNYOLO_STASH_GB"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("PNYOLO_GROUP", "1")
    SB, NV, NS, H, W, B, kc, kf, kfd = 2, 6, 2, 64, 64, 128, 32, 16, 8
    net = make_model(pconf.default_mv()["model"], stop_encoder_grad=True)
    net.mlp_coarse.load_state_dict({k: torch.from_numpy(v) for k, v in synth.mlp_state(8401).items()})
    net.mlp_fine.load_state_dict({k: torch.from_numpy(v) for k, v in synth.mlp_state(8402).items()})
    net = net.to(DEV).train()
    net.set_deterministic(True)
    images = torch.from_numpy(synth.images(8403, SB * NV, H, W)).reshape(SB, NV, 3, H, W).to(DEV)
    poses = torch.from_numpy(np.stack([np.stack([synth.pose_spherical(40.0 * v + 15.0 * s, -20.0, 1.3 + 0.1 * s)
                                                 for v in range(NV)]) for s in range(SB)])).to(DEV)
    focal = torch.tensor([0.9 * W, 0.95 * W])                       # data["focal"] (SB,)
    lat = torch.from_numpy(np.concatenate([synth.latent(8404 + i, NS, 512, H // 2, W // 2) for i in range(SB)])).to(DEV)
    rs = np.random.RandomState(8405)
    pix_inds = torch.from_numpy(rs.randint(0, NV * H * W, size=(SB, B)))           # torch.randint's role, on the CPU
    n = SB * B
    draws = dict(u_coarse=rs.rand(n, kc).astype(np.float32), u_fine=rs.rand(n, kf - kfd).astype(np.float32),
                 u_fine2=rs.rand(n, kf - kfd).astype(np.float32), g_depth=rs.randn(n, kfd).astype(np.float32))
    ren = NeRFRenderer(n_coarse=kc, n_fine=kf, n_fine_depth=kfd, white_bkgd=True).train()

    def step(all_rays, all_rgb_gt):
        net.zero_grad(set_to_none=True)
        net.encode(images[:, :NS].contiguous(), poses[:, :NS].contiguous(), focal, latent=lat)
        ren.draws = draws
        out = ren(net, all_rays, want_weights=True)
        loss = torch.nn.functional.mse_loss(out["coarse"]["rgb"], all_rgb_gt) + torch.nn.functional.mse_loss(out["fine"]["rgb"], all_rgb_gt)
        loss.backward()
        torch.cuda.synchronize()
        grads = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None and k.startswith("mlp_")}
        return out["coarse"]["rgb"].detach().clone(), out["fine"]["rgb"].detach().clone(), grads

    rays_a, gt_a, pix = sample_train_batch(images, poses, focal, 0.8, 1.8, B, draws={"pix_inds": pix_inds})
    rays_b, gt_b = reference_style_batch(images, poses, focal, None, 0.8, 1.8, pix_inds)
    assert np.array_equal(pix.cpu().numpy(), tb.flat_to_pix(pix_inds.numpy(), H, W))
    assert torch.equal(bits(rays_a), bits(rays_b)) and torch.equal(bits(gt_a), bits(gt_b))
    c_a, f_a, g_a = step(rays_a, gt_a)
    c_b, f_b, g_b = step(rays_b, gt_b)
    assert net._h_group is not None, "the step ran on the grouped scene"
    assert len(g_a) >= 60 and set(g_a) == set(g_b) and all(float(v.abs().max()) > 0 for k, v in g_a.items() if k.endswith("lin_out.weight"))
    assert torch.equal(bits(c_a), bits(c_b)) and torch.equal(bits(f_a), bits(f_b))
    bad = [k for k in g_a if not torch.equal(bits(g_a[k]), bits(g_b[k]))]
    assert not bad, "%d of %d MLP gradients differ: %s" % (len(bad), len(g_a), bad[:5])


# --------------------------------------------------------------------------- no hidden waiting
def test_the_call_does_not_wait_for_its_stream():
    """All inputs on the device; a queue of large matrix products (about a second of GPU work) is enqueued first.  The
    call must come back with that stream still busy -- stream.query(), no timing threshold -- and its results, read after
    the stream drained, are those of an undisturbed call."""
    SB, NV, H, W, B, seed = 4, 50, 128, 128, 128, 4242
    images, poses, focal, c, boxes = seeded_scene(SB, NV, H, W, 8500, "pair")
    focal, c, boxes = focal.to(DEV), c.to(DEV), boxes.to(DEV)
    pix_inds = torch.randint(0, NV * H * W, (SB, B)).to(DEV)
    calls = [dict(seed=seed), dict(bboxes=boxes, seed=seed), dict(draws={"pix_inds": pix_inds})]
    quiet = [sample_train_batch(images, poses, focal, 0.5, 2.5, B, c=c, **kw) for kw in calls]      # (also loads the kernel)
    m = torch.randn(8192, 8192, device=DEV)
    out = torch.empty_like(m)
    torch.mm(m, m, out=out)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(DEV)
    for _ in range(60):
        torch.mm(m, m, out=out)
    assert not stream.query(), "the queue of matrix products was too short to test anything"
    busy = [sample_train_batch(images, poses, focal, 0.5, 2.5, B, c=c, **kw) for kw in calls]
    still_busy = not stream.query()
    torch.cuda.synchronize()
    assert still_busy, "sample_train_batch waited for the stream"
    for q, b in zip(quiet, busy):
        assert torch.equal(q[2], b[2]) and torch.equal(bits(q[0]), bits(b[0])) and torch.equal(bits(q[1]), bits(b[1]))
