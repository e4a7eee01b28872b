"""
The ResNet-34 trunk on the library's kernels (-m gpu, real MI355X) against torch.autograd through the oracle's trunk in
float64 (oracle/pnyolo_oracle.py spatial_encoder(dtype=torch.float64)), on synth.resnet34_state weights and synth.images:
  * the training trunk (pny_trunk_train_forward / _backward, csrc/encoder_train.hip) at the benchmark's and the reference's
    training shape and at odd, non-square, smallest and DTU-like sizes, with batch norm on batch or running statistics;
  * the inference trunk (csrc/encoder.hip, folded batch norm) at the same shapes, super-batches included;
  * what encode() does below the trunk's minimum size;
  * the trunk after its parameters moved to new storage (load_state_dict(assign=True), p.data = ...);
  * a training encode() superseded before its graph's backward;
  * a latent whose gradient autograd sums from more than one consumer, in the full loop images -> trunk -> renderer -> loss.
Bounds (those of tests/test_gpu_backward.py): the latent within 2e-4 x max(1, max |latent|), every trunk parameter gradient
within RTOL = 1e-4 of its tensor's max, the stepped running statistics within 2e-6 x max(1, max |.|).
"""
import time

import numpy as np
import pytest
import torch

import pnyolo_oracle as orc
from helpers import DEV, RTOL, clean_rays, compare_param_grads, grad_check, load_mlp, maxabs, render_loss
from pixel_nerf_yolo_amd import conf as pconf
from pixel_nerf_yolo_amd import synth
from pixel_nerf_yolo_amd.model import make_model
from pixel_nerf_yolo_amd.render import NeRFRenderer

pytestmark = pytest.mark.gpu
f64 = torch.float64
SPIN_CYCLES = 20_000_000      # torch.cuda._sleep: ~10 ms of one wave spinning on the clock


def trunk_net(seed, pool=True, mlp_seed=None):
    """A net whose trunk trains (stop_encoder_grad=False) with synth.resnet34_state(seed) and, if mlp_seed, seeded MLPs."""
    c = pconf.default_mv()
    c.d["model"]["encoder"]["use_first_pool"] = pool
    net = make_model(c["model"], stop_encoder_grad=False)
    enc = synth.resnet34_state(seed, residual_gain=0.25)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in enc.items()}, strict=False)
    if mlp_seed is not None:
        load_mlp(net.mlp_coarse, mlp_seed, 512, 4)
        load_mlp(net.mlp_fine, mlp_seed + 1, 512, 4)
    return net.to(DEV).train(), enc


def oracle_state(enc):
    """float64 copies of the trunk state: parameters are leaves that take a gradient, running statistics step in place."""
    return {k: torch.from_numpy(np.array(v, dtype=np.float64)).requires_grad_("running" not in k)
            for k, v in enc.items() if "num_batches" not in k}


def oracle_trunk(sd64, images, pool, training):
    return orc.spatial_encoder(sd64, torch.as_tensor(images).reshape(-1, *images.shape[-3:]), use_first_pool=pool,
                               training=training, dtype=f64)[0]


def no_torch_trunk(monkeypatch, net):
    monkeypatch.setattr(type(net.encoder), "forward_torch", lambda self, x: (_ for _ in ()).throw(AssertionError("torch trunk used")))


def check_latent(lat, ref):
    scale = max(1.0, float(ref.detach().abs().max()))
    err = maxabs(lat, ref.detach())
    assert err <= 2e-4 * scale, "latent: max |err| %.3e vs max(1, max |latent|) %.3e" % (err, scale)
    return err / scale


def check_trunk_grads(net, sd64):
    """Every trunk parameter gradient against the oracle's (layer4 / fc take none); returns the worst error / tensor max."""
    worst, checked, bad = 0.0, 0, []
    for k, p in net.encoder.model.named_parameters():
        if k.startswith(("layer4", "fc")):
            assert p.grad is None, k
            continue
        ref = sd64["encoder.model." + k].grad
        assert p.grad is not None and ref is not None, k
        try:
            worst = max(worst, grad_check("encoder.model." + k, p.grad, ref))
        except AssertionError as e:       # (every failing tensor in the message: the pattern is the diagnosis)
            bad.append(str(e))
        checked += 1
    assert not bad, "\n".join(bad)
    assert checked >= 80
    return worst


def check_running_stats(net, sd64, steps):
    sd = net.state_dict()
    for k, t in sd64.items():
        if "running" in k and not k.startswith("encoder.model.layer4"):
            assert maxabs(sd[k], t) <= 2e-6 * max(1.0, float(t.abs().max())), k
    for b in net._trunk_bn_modules():
        assert int(b.num_batches_tracked) == steps


def train_step(net, images, poses, G, focal):
    net.zero_grad()
    net.encode(images, poses, focal)
    lat = net.differentiable_latent()
    assert lat is not None
    (lat * G).sum().backward()
    return lat.detach()


def report(tag, **errs):
    print("TRUNK %s: %s" % (tag, " ".join("%s %.2e" % kv for kv in errs.items())))


# --------------------------------------------------------------------------- B1: the training trunk, shape matrix
# (SB, NS, H, W, first pool, batch norm, weight seed): n = SB * NS images.  Levels (pool): 128 -> 64 / 32 / 16 / 8; 33 x 47 ->
# 17 x 24 / 9 x 12 / 5 x 6 / 3 x 3; 32 x 40 -> 16 x 20 / 8 x 10 / 4 x 5 / 2 x 3; (no pool) 75 x 100 -> 38 x 50 / 38 x 50 /
# 19 x 25 / 10 x 13; 150 x 200 -> 75 x 100 / 38 x 50 / 19 x 25 / 10 x 13.
# Relu units at zero.  The trunk's gradient is discontinuous in every relu input (test_gpu_backward.py, the batch-statistics
# test): a unit within fp32 rounding of zero may be masked either way by ANY fp32 evaluation, and with a random G one flipped
# unit moves every gradient below it by ~1/sqrt(P) of its max (a sum of random-signed terms gets one O(1) term more or less).
# Traced on the MI355X: at 2 x 3 x 128 x 128 / seed 7356 the trunk's gradients were 2e-3 .. 3e-2 from fp64 in conv1 .. layer2.1;
# setting ONE layer2 unit (9.1e-8 of its relu's max from zero) the other way in the fp64 graph reproduces the per-tensor error
# to 1 % (conv1.weight 16.1 vs 16.5, layer2.0.downsample.0.weight 27.9 vs 27.9); at 3 x 75 x 100 / 3275 a layer1 unit 2.5e-8
# from zero does the same (1.55 / 6.23 / 8.77 vs 1.546 / 6.225 / 8.774); at 7356 a second unit (layer1.2's bn1 relu) is needed
# for layer1.2.bn1.bias, and only with both set together.  No seed avoids such units at these sizes, so the
# reference accounts for them (fp64_grads_with_flips): each unit within FLIP_TOL of zero may be set either way, if that brings
# the fp64 gradients closer to the GPU's, and every tensor must then be within RTOL.  Seeds were screened by comparing the
# oracle in fp32 and fp64 on the CPU (rejected above 2e-5): 32 x 40: 3172 (1.4e-2); 2 x 3 x 128 x 128: 3356, 4356, 5356, 6356.
# The benchmark's 4 x 3 images of 128 x 128 are not used: none of 36 seeds (3356 + 1000 k) passed that screen (12.6 M relu units);
# 2 x 3 images put conv1 above bn_grid's cap as well (P = 24 576 > 16 384).
FLIP_TOL = 1e-6          # |pre-activation| / max |pre-activation of that relu|: ~10x fp32's rounding of a 576..2304-term sum
FLIP_MAX = 32
SHAPES = [
    (2, 3, 128, 128, True, "batch", 7356),    # the benchmark's image size on batch statistics: bn_grid's capped path
    (1, 3, 33, 47, True, "batch", 3180),      # odd and non-square at every level
    (1, 2, 32, 40, True, "eval", 4172),       # the smallest legal height
    (1, 3, 75, 100, False, "batch", 3275),    # odd stride-2 inputs, conf/exp/sn64.conf (no first pool)
    (1, 5, 150, 200, True, "eval", 3450),     # DTU at half scale, n odd (conv1 above the cap, running statistics)
    (1, 16, 32, 32, True, "batch", 5516),     # 16 views of one object, the ABI's limit (screen: 3516 5.5e-4, 4516 5.9e-2, 5516 2.0e-6)
]


def fp64_grads_with_flips(net, enc, images, pool, training, G):
    """fp64 gradients of (trunk(images) * G).sum() for the trunk parameters, with the units within FLIP_TOL of zero set the way
    that brings them closest to the GPU's gradients (greedy, one unit at a time, each flip's effect computed exactly in fp64 and
    kept, together with the flips kept before it, if it lowers the summed per-tensor relative error).
    Returns ({name: gradient}, [(relu call, unit, margin) of the units set the other way])."""
    x = torch.as_tensor(images).reshape(-1, *images.shape[-3:])
    gpu = {"encoder.model." + k: p.grad.detach().cpu().double() for k, p in net.encoder.model.named_parameters() if p.grad is not None}
    state = {}

    def relu(h):
        i = state["call"]
        state["call"] += 1
        if state["rec"] is not None:
            state["rec"].append(h.detach())
        units = [j for c, j in state["flip"] if c == i]
        if units:
            m = (h > 0).flatten().clone()
            m[units] = ~m[units]
            return torch.where(m.view_as(h), h, torch.zeros((), dtype=h.dtype))
        return torch.relu(h)

    def run(flip=(), rec=None):
        state.update(call=0, flip=list(flip), rec=rec)
        sd = oracle_state(enc)
        out = orc.spatial_encoder(sd, x, use_first_pool=pool, training=training, dtype=f64, relu=relu)[0]
        (out * G.to(f64)).sum().backward()
        return {k: sd[k].grad for k in gpu}

    rec = []
    ref = run(rec=rec)
    cands = []
    for i, h in enumerate(rec):
        a = h.abs().flatten()
        near = (a < FLIP_TOL * float(a.max())).nonzero().flatten()
        cands += [(float(a[j]) / float(a.max()), i, int(j)) for j in near]
    cands = sorted(cands)[:FLIP_MAX]

    def worst(g):      # (summed over the tensors: a flip that fixes one tensor counts while another flip dominates the max)
        return sum(float((gpu[k] - g[k]).abs().max()) / max(float(g[k].abs().max()), 1e-20) for k in gpu)
    used = []
    for margin, i, j in cands:
        trial = run(flip=[(c, u) for c, u, _ in used] + [(i, j)])      # (the whole set of flips, evaluated together)
        if worst(trial) < worst(ref):
            ref = trial
            used.append((i, j, margin))
    return ref, used


@pytest.mark.parametrize("SB,NS,H,W,pool,bn,seed", SHAPES, ids=["%dx%d-%dx%d-%s-%s" % (s[0], s[1], s[2], s[3],
                                                                                         "pool" if s[4] else "nopool", s[5]) for s in SHAPES])
def test_training_trunk_shapes_vs_fp64_autograd(SB, NS, H, W, pool, bn, seed, monkeypatch):
    """pny_trunk_train_forward / _backward through net.encode() and (latent * G).sum().backward(), G a fixed random upstream
    gradient: the latent, every trunk parameter gradient, the running statistics and num_batches_tracked against the fp64
    oracle.  bn = eval: every BatchNorm2d in eval() mode under autograd (running statistics, no stepping).  In the largest case
    (the most weight-gradient pixel slices) the step runs twice and the gradients must be bit-identical (no atomics)."""
    t0 = time.time()
    net, enc = trunk_net(seed, pool)
    if bn == "eval":
        net.encoder.eval()
    no_torch_trunk(monkeypatch, net)
    images = torch.from_numpy(np.stack([synth.images(seed + 1 + i, NS, H, W) for i in range(SB)]))
    poses = torch.from_numpy(np.stack([synth.scene_cameras(NS, radius=1.3 + 0.1 * i)[0] for i in range(SB)]))
    n, hl, wl = SB * NS, (H + 1) // 2, (W + 1) // 2
    G = torch.from_numpy(np.random.RandomState(5).standard_normal((n, 512, hl, wl)).astype(np.float32))
    reps = 2 if n * H * W == max(s[0] * s[1] * s[2] * s[3] for s in SHAPES) else 1
    grads = []
    for _ in range(reps):
        lat = train_step(net, images, poses, G.to(DEV), torch.tensor(0.9 * W))
        assert lat.shape == (n, 512, hl, wl)
        grads.append({k: p.grad.detach().clone() for k, p in net.encoder.model.named_parameters() if p.grad is not None})
    torch.cuda.synchronize()
    for g in grads[1:]:
        assert all(torch.equal(grads[0][k], g[k]) for k in grads[0]), "trunk gradients are not bit-reproducible"
    sd64 = oracle_state(enc)
    for _ in range(reps):       # (batch statistics: the running statistics step once per pass)
        with torch.no_grad():
            ref = oracle_trunk(sd64, images, pool, training=bn == "batch")
    e_lat = check_latent(lat, ref)
    check_running_stats(net, sd64, reps if bn == "batch" else 0)
    grads64, flips = fp64_grads_with_flips(net, enc, images, pool, bn == "batch", G)
    for k, g in grads64.items():      # (the gradients do not depend on the running statistics)
        sd64[k].grad = g
    e_grad = check_trunk_grads(net, sd64)
    report("train n=%d %dx%d pool=%s bn=%s" % (n, H, W, pool, bn), latent=e_lat, grad=e_grad, units_flipped=len(flips),
           flip_margin=max([f[2] for f in flips], default=0.0), seconds=time.time() - t0)


# --------------------------------------------------------------------------- B2: the inference trunk at the same shapes
INFER = [
    (3, 4, 128, 128, True),     # super-batch of 3 objects: pny_scenes_encode, one pass over 12 images
    (1, 3, 33, 47, True),
    (2, 1, 32, 40, True),
    (3, 1, 75, 100, False),
    (5, 1, 150, 200, True),
    (1, 16, 32, 32, True),      # 16 views of one object, the ABI's limit
]


@pytest.mark.parametrize("SB,NS,H,W,pool", INFER, ids=["%dx%d-%dx%d-%s" % (s[0], s[1], s[2], s[3], "pool" if s[4] else "nopool")
                                                          for s in INFER])
def test_inference_trunk_shapes_vs_fp64(SB, NS, H, W, pool):
    """Eval-mode encode() (csrc/encoder.hip: folded batch norm, maxpool_kernel, upsample_concat_kernel; SB > 1 one
    pny_scenes_encode pass over every object's views) against the fp64 oracle's latent, object by object."""
    seed = 3200 + H + W
    net, enc = trunk_net(seed, pool)
    net.eval()
    images = torch.from_numpy(np.stack([synth.images(seed + 1 + i, NS, H, W) for i in range(SB)]))
    poses = torch.from_numpy(np.stack([synth.scene_cameras(NS, radius=1.3 + 0.1 * i)[0] for i in range(SB)]))
    with torch.no_grad():
        net.encode(images, poses, torch.tensor(0.9 * W))
        lat = torch.cat([net.latent(sb) for sb in range(SB)])
        ref = oracle_trunk(oracle_state(enc), images, pool, training=False)
    assert lat.shape == ref.shape == (SB * NS, 512, (H + 1) // 2, (W + 1) // 2)
    report("infer SB=%d NS=%d %dx%d pool=%s" % (SB, NS, H, W, pool), latent=check_latent(lat, ref))


# --------------------------------------------------------------------------- B3: below the trunk's minimum size
@pytest.mark.parametrize("H,W", [(30, 64), (64, 31), (16, 16)])
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_encode_below_minimum_size_raises(H, W, mode):
    """Both of the library's trunks need H, W >= 32 (every pyramid level at least 2 x 2; pny_scene_encode and
    pny_trunk_train_forward refuse smaller images).  encode() on them raises a ValueError that says so, before it changes any
    state, in training and in inference; the same net then encodes a legal size."""
    net, _ = trunk_net(3300)
    if mode == "eval":
        net.eval()
    poses = torch.from_numpy(synth.scene_cameras(2)[0])
    with pytest.raises(ValueError, match="at least 32 x 32"):
        net.encode(torch.from_numpy(synth.images(3301, 2, H, W)), poses, torch.tensor(0.9 * W))
    assert net._last_encode is None
    net.encode(torch.from_numpy(synth.images(3301, 2, 32, 32)), poses, torch.tensor(28.8))
    assert net._last_encode["H"] == 32


def test_encode_below_minimum_size_on_the_aten_trunk(monkeypatch):
    """The ATen training graph (PNYOLO_TRUNK=torch: SpatialEncoder.forward_torch) takes any size, as before: a training
    encode() of 30 x 64 images runs there and its latent carries the gradient to the trunk's parameters."""
    monkeypatch.setenv("PNYOLO_TRUNK", "torch")
    net, _ = trunk_net(3300)
    net.encode(torch.from_numpy(synth.images(3301, 2, 30, 64)), torch.from_numpy(synth.scene_cameras(2)[0]), torch.tensor(57.6))
    lat = net.differentiable_latent()
    assert lat is not None and lat.shape == (2, 512, 15, 32)
    lat.sum().backward()
    assert net.encoder.model.conv1.weight.grad is not None and float(net.encoder.model.conv1.weight.grad.abs().max()) > 0


# --------------------------------------------------------------------------- B4: parameters moved to new storage
@pytest.mark.parametrize("how", ["assign", "data"])
def test_training_trunk_after_parameters_rebound(how, monkeypatch):
    """One training step, then the trunk's parameters move to NEW storage with DIFFERENT values -- load_state_dict(...,
    assign=True) (parameters and running statistics) or p.data = ... (parameters) -- while the old tensors stay alive; the
    next training step must read the new weights: the latent and every gradient against the fp64 oracle on the new state.
    (The trunk's pack-job table holds the conv weights' device pointers; pny_model_bind_param re-resolves them.)"""
    ns, H, W, pool = 2, 64, 48, True
    net, enc = trunk_net(3400, pool)
    no_torch_trunk(monkeypatch, net)
    images = torch.from_numpy(synth.images(3401, ns, H, W))
    poses = torch.from_numpy(synth.scene_cameras(ns)[0])
    G = torch.from_numpy(np.random.RandomState(6).standard_normal((ns, 512, H // 2, W // 2)).astype(np.float32)).to(DEV)
    train_step(net, images, poses, G, torch.tensor(0.9 * W))
    old = [t.data for t in net.state_dict(keep_vars=True).values()]      # the old storage, kept alive: the stale read is well defined
    enc_b = synth.resnet34_state(3402, residual_gain=0.25)
    if how == "assign":
        new = {k: torch.from_numpy(v).to(DEV) for k, v in enc_b.items()}
        net.load_state_dict(new, strict=False, assign=True)
    else:
        with torch.no_grad():
            for k, p in net.encoder.model.named_parameters():
                if "encoder.model." + k in enc_b:       # (layer4 / fc: not part of the trunk)
                    p.data = torch.from_numpy(enc_b["encoder.model." + k]).to(DEV)
    state = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items() if k.startswith("encoder.model.")}
    tracked = int(net.encoder.model.bn1.num_batches_tracked)
    for k, p in net.encoder.model.named_parameters():
        if "encoder.model." + k not in enc_b:
            continue
        assert np.array_equal(state["encoder.model." + k], enc_b["encoder.model." + k])
        assert all(p.data_ptr() != t.data_ptr() for t in old)
    lat = train_step(net, images, poses, G, torch.tensor(0.9 * W))
    sd64 = oracle_state(state)
    ref = oracle_trunk(sd64, images, pool, training=True)
    (ref * G.cpu().to(f64)).sum().backward()
    e_lat = check_latent(lat, ref)
    e_grad = check_trunk_grads(net, sd64)
    check_running_stats(net, sd64, tracked + 1)
    del old
    report("rebind %s" % how, latent=e_lat, grad=e_grad)


# --------------------------------------------------------------------------- B5: a superseded training forward
def test_superseded_training_forward_refuses_backward(monkeypatch):
    """Two training encode() calls before any backward (gradient accumulation over two batches): the library keeps the saved
    activations of the later one only, so backward through the FIRST graph raises a RuntimeError that names the cause and
    leaves no gradient; backward through the second graph alone matches the fp64 oracle."""
    ns, H, W, pool = 2, 48, 64, True
    net, enc = trunk_net(3500, pool)
    no_torch_trunk(monkeypatch, net)
    img_a, img_b = torch.from_numpy(synth.images(3501, ns, H, W)), torch.from_numpy(synth.images(3502, ns, H, W))
    poses = torch.from_numpy(synth.scene_cameras(ns)[0])
    G = torch.from_numpy(np.random.RandomState(7).standard_normal((ns, 512, H // 2, W // 2)).astype(np.float32))
    net.zero_grad()
    net.encode(img_a, poses, torch.tensor(0.9 * W))
    lat_a = net.differentiable_latent()
    net.encode(img_b, poses, torch.tensor(0.9 * W))
    lat_b = net.differentiable_latent()
    with pytest.raises(RuntimeError, match="superseded"):
        (lat_a * G.to(DEV)).sum().backward()
    assert all(p.grad is None for p in net.encoder.parameters())
    (lat_b * G.to(DEV)).sum().backward()
    sd64 = oracle_state(enc)
    with torch.no_grad():
        oracle_trunk(sd64, img_a, pool, training=True)          # (steps the running statistics, as the first encode did)
    ref = oracle_trunk(sd64, img_b, pool, training=True)
    (ref * G.to(f64)).sum().backward()
    e_lat = check_latent(lat_b, ref)
    e_grad = check_trunk_grads(net, sd64)
    check_running_stats(net, sd64, 2)
    report("superseded", latent=e_lat, grad=e_grad)


# --------------------------------------------------------------------------- B6: a latent gradient with several consumers
class _SlowIdentity(torch.autograd.Function):
    """Identity whose backward holds the current stream in a timed spin BEFORE it writes its output: a reader of that gradient
    (or of anything autograd sums from it) on another stream that does not wait for this stream reads it unwritten."""

    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        torch.cuda._sleep(SPIN_CYCLES)
        return g.clone()


@pytest.mark.parametrize("variant", ["one_render", "two_renders", "extra_term", "bind_parallel", "supplied_then_native"])
def test_shared_latent_gradient_full_loop(variant, monkeypatch):
    """images -> native training trunk (batch statistics) -> renderer -> loss, trunk and MLP gradients against autograd
    through the oracle (fp64 trunk, the renderer as the other backward tests run it).  one_render: d loss / d latent is the
    tensor the render backward returned, and the trunk's side stream starts behind that backward's event (beside the
    weight-gradient flush).  Otherwise it is not, and the side stream must wait for the caller's whole stream:
      two_renders           two renders with different rays on one encode();
      extra_term            one render plus a loss term on net.differentiable_latent() whose backward runs after the render's
                            and writes its gradient behind a timed spin (_SlowIdentity);
      bind_parallel         bind_parallel(net, [0, 0]): two replicas' latent-gradient shares, summed by autograd;
      supplied_then_native  a training render on a caller-supplied latent, then a native-trunk step whose loss is a term on
                            the latent alone (the render's event of the earlier step must not order this one).
    Which ordering ran is asserted (net._last_trunk_wait); that is the deterministic part.  The spin only widens the window in
    which a wrong ordering reads an unwritten gradient: whether it does so depends on how the runtime maps the two streams
    onto hardware queues (on the unfixed tree only bind_parallel's gradients came out wrong)."""
    monkeypatch.setenv("PNYOLO_MLP_PRECISION", "f32")      # the fp32 forward: relu masks as the oracle's (test_gpu_backward.py)
    ns, H, W, kc, kf, kfd, pool = 2, 64, 64, 16, 8, 4, True
    net, enc = trunk_net(3600, pool, mlp_seed=3601)
    no_torch_trunk(monkeypatch, net)
    images = torch.from_numpy(synth.images(3603, ns, H, W))[None]      # one object, ns views
    poses, tgt = synth.scene_cameras(ns)
    focal, cc = torch.tensor(0.9 * W), torch.tensor([[W * 0.5, H * 0.5]])
    rs = np.random.RandomState(3604)
    hl, wl = H // 2, W // 2
    G2 = torch.from_numpy(rs.standard_normal((ns, 512, hl, wl)).astype(np.float32))
    # oracle: fp64 trunk on batch statistics, fp32 renderer on its latent
    sd64 = oracle_state(enc)
    if variant == "supplied_then_native":
        ref = oracle_trunk(sd64, images, pool, training=True)
        (ref * G2.to(f64)).sum().backward()
    else:
        ref = oracle_trunk(sd64, images, pool, training=True)
        mc = {k: torch.from_numpy(v).requires_grad_() for k, v in synth.mlp_state(3601).items()}
        mf = {k: torch.from_numpy(v).requires_grad_() for k, v in synth.mlp_state(3602).items()}
        sc = orc.Scene(mc, mf, ref.detach().float().numpy(), poses, focal, cc, W, H)
        sc.mlp_coarse, sc.mlp_fine, sc.latent = mc, mf, ref.float()
        n_sets = 2 if variant == "two_renders" else 1
        n = 128                                              # bind_parallel splits a call of >= 64 rays per device
        cand = orc.gen_rays(tgt[None], W, H, 0.9 * W, 0.3, 1.8)[0].reshape(-1, 8)
        cand = cand[torch.from_numpy(rs.choice(H * W, 1200, replace=False))]
        dr = dict(u_coarse=rs.rand(1200, kc).astype(np.float32), u_fine=rs.rand(1200, kf - kfd).astype(np.float32),
                  u_fine2=rs.rand(1200, kf - kfd).astype(np.float32), g_depth=rs.randn(1200, kfd).astype(np.float32))
        keep = clean_rays(sc, cand, kc, kf, kfd, dr, n * n_sets)
        sets = [(cand[torch.from_numpy(keep[i * n:(i + 1) * n])], {k: v[keep[i * n:(i + 1) * n]] for k, v in dr.items()},
                 torch.from_numpy(rs.uniform(0, 1, size=(n, 3)).astype(np.float32))) for i in range(n_sets)]
        loss = 0.5 * (sc.latent * G2).sum() if variant == "extra_term" else 0.0
        for rays, d, gt in sets:
            out = orc.render(sc, rays, kc, kf, kfd, d["u_coarse"], d["u_fine"], d["u_fine2"], d["g_depth"])
            loss = loss + render_loss(out, gt, True)
        loss.backward()
    # HIP
    ren = NeRFRenderer(n_coarse=kc, n_fine=kf, n_fine_depth=kfd, white_bkgd=True).train()
    if variant == "supplied_then_native":
        # step 1: a training render on a caller-supplied latent (its backward records the latent-gradient event)
        lt = torch.from_numpy(synth.latent(3605, ns, 512, hl, wl)).to(DEV).requires_grad_()
        net.encode(images, torch.from_numpy(poses)[None], focal, c=cc, latent=lt)
        rays = orc.gen_rays(tgt[None], W, H, 0.9 * W, 0.3, 1.8)[0].reshape(-1, 8)[:64].to(DEV)
        render_loss(ren(net, rays[None], want_weights=True), torch.full((1, 64, 3), 0.5, device=DEV), True).backward()
        assert lt.grad is not None
        # step 2: the native trunk, a loss on the latent alone
        net.zero_grad()
        net.encode(images, torch.from_numpy(poses)[None], focal, c=cc)
        (_SlowIdentity.apply(net.differentiable_latent()) * G2.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        assert net._last_trunk_wait == "stream"
        e_grad = check_trunk_grads(net, sd64)
        report("shared latent %s" % variant, grad=e_grad)
        return
    net.zero_grad()
    net.encode(images, torch.from_numpy(poses)[None], focal, c=cc)
    lat = net.differentiable_latent()
    loss = 0.5 * (_SlowIdentity.apply(lat) * G2.to(DEV)).sum() if variant == "extra_term" else 0.0   # (before the render:
    call = ren.bind_parallel(net, [0, 0]) if variant == "bind_parallel" else (lambda r, want_weights: ren(net, r, want_weights))
    for rays, d, gt in sets:                                                                         # its backward runs after)
        ren.draws = d
        out = call(rays[None].to(DEV), want_weights=True)
        loss = loss + render_loss({p: {k: v[0] for k, v in out[p].items()} for p in ("coarse", "fine")}, gt.to(DEV), True)
    loss.backward()
    torch.cuda.synchronize()
    assert net._last_trunk_wait == ("event" if variant == "one_render" else "stream")
    e_lat = check_latent(lat, ref)
    e_mlp = compare_param_grads(net, sc)
    e_grad = check_trunk_grads(net, sd64)
    report("shared latent %s" % variant, latent=e_lat, mlp=e_mlp, grad=e_grad)
