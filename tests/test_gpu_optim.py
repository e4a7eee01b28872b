"""
The one-launch Adam optimizer on the GPU (-m gpu): pixel_nerf_yolo_amd.optim.Adam, csrc/optim.hip, include/pnyolo.h pny_optim_*.

The yardstick is the fp64 restatement of Adam in tests/test_cpu_optim.py (pinned there to torch.optim.Adam in fp64).  THE BAR
(every comparison of values below): run torch.optim.Adam(foreach=False) in fp32 on the same device and inputs and take its
maximum |error| against fp64 per step (over every tensor of the step); the kernel's maximum |error| must not exceed twice that
plus one fp32 ulp of the largest parameter.  Both are roundings of the same formula in a different operation order (lerp and
addcdiv against the kernel's order), so neither bounds the other more tightly than a factor of two.  The moments are held
to the same rule, each with the ulp of ITS OWN largest value (for exp_avg_sq that is tighter than the parameters' ulp).  The
replayed training loop applies the rule to each of its 60 tensors on its own.

Every comparison prints both sides' figures before it asserts (run with -s).  For scale: torch's own fp32 error on a CPU, on
the inputs of test_tensors_against_fp64, is 7.4e-9 after one step and 3.9e-8 after ten; the ulp at 0.05 is 3.7e-9 and a step
moves a parameter by 1e-4.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import DEV, dt, scene_pair
from pixel_nerf_yolo_amd import conf as pconf
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd import synth
from pixel_nerf_yolo_amd.model import make_model
from pixel_nerf_yolo_amd.optim import Adam
from pixel_nerf_yolo_amd.render import NeRFRenderer, YoloRenderer
from test_cpu_optim import adam_fp64, gradients

import pnyolo_oracle as orc

pytestmark = pytest.mark.gpu


# --------------------------------------------------------------------------- the bar
def within_bar(tag, e_k, e_t, largest):
    """The kernel's max |error| `e_k` and torch fp32's `e_t`, both against fp64, under the rule of the module docstring;
    `largest` is the largest fp64 magnitude of the quantity compared."""
    ulp = float(np.spacing(np.float32(largest)))
    print("%s: kernel %.3e, torch fp32 %.3e, ulp %.3e" % (tag, e_k, e_t, ulp))
    assert e_k <= 2.0 * e_t + ulp, "%s: kernel max |err| %.3e, torch fp32 %.3e, ulp %.3e" % (tag, e_k, e_t, ulp)


def max_err(x, exact):
    return float((x.detach().double() - exact.view(x.shape)).abs().max())


def make_params(values, offsets=None):
    """fp32 parameters on the GPU holding `values` (numpy); offsets[i] > 0 makes parameter i a view that starts that many
    elements into its own buffer (a storage pointer that is not 16-byte aligned)."""
    out = []
    for i, val in enumerate(values):
        off = 0 if offsets is None else offsets[i]
        buf = torch.zeros(val.size + off + 5, device=DEV, dtype=torch.float32)
        view = buf[off:off + val.size].view(val.shape)
        view.copy_(torch.from_numpy(np.ascontiguousarray(val, dtype=np.float32)))
        p = torch.nn.Parameter(view)
        assert p.data_ptr() == buf.data_ptr() + 4 * off
        out.append(p)
    return out


def run_fp64(values, grads, lrs, weight_decay=0.0):
    """[(p, m, v) per tensor] per step, float64 on the GPU, from the fp32 initial values and the fp32 gradients."""
    state = [(torch.from_numpy(np.asarray(v, dtype=np.float32)).to(DEV).double(),) for v in values]
    state = [(p, torch.zeros_like(p), torch.zeros_like(p)) for (p,) in state]
    steps = []
    for t, (gs, lr) in enumerate(zip(grads, lrs), start=1):
        state = [(s if g is None else adam_fp64(s[0], g.double(), s[1], s[2], t, lr, weight_decay=weight_decay))
                 for s, g in zip(state, gs)]
        steps.append(state)
    return steps


def run_fp32(classes, values, grads, lrs, weight_decay=0.0, offsets=None):
    """The same steps in fp32 with classes[t] as the optimizer of step t (a change of class goes through state_dict() /
    load_state_dict()).  Returns [(p, m, v) clones per tensor] per step."""
    ps = make_params(values, offsets)
    opt, steps = None, []
    for cls, gs, lr in zip(classes, grads, lrs):
        if opt is None or type(opt) is not cls:
            kw = dict(foreach=False) if cls is torch.optim.Adam else {}
            new = cls(ps, lr=lr, weight_decay=weight_decay, **kw)
            if opt is not None:
                new.load_state_dict(opt.state_dict())
            opt = new
        for p, g in zip(ps, gs):
            p.grad = None if g is None else g.clone().view(p.shape)
        opt.param_groups[0]["lr"] = lr
        opt.step()
        steps.append([(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone())
                      for p in ps])
    torch.cuda.synchronize()
    return steps


def compare_runs(tag, got, ref32, exact, per_tensor=False):
    """Every step and quantity (parameters, exp_avg, exp_avg_sq) under the bar: the maximum over all tensors of the step, as
    the rule is stated, or with per_tensor every tensor on its own (the replayed training loop)."""
    summary = []
    for t, (a, b, c) in enumerate(zip(got, ref32, exact), start=1):
        for q, name in enumerate(("param", "exp_avg", "exp_avg_sq")):
            e_k = [max_err(x[q], z[q]) for x, z in zip(a, c)]
            e_t = [max_err(y[q], z[q]) for y, z in zip(b, c)]
            big = [float(z[q].abs().max()) for z in c]
            if per_tensor:
                for i in range(len(a)):
                    within_bar("%s step %d tensor %d %s" % (tag, t, i, name), e_k[i], e_t[i], big[i])
            else:
                within_bar("%s step %d %s" % (tag, t, name), max(e_k), max(e_t), max(big))
            if q == 0:
                summary.append((max(e_k), max(e_t)))
    print("%s: parameters, max |err| vs fp64 (kernel, torch fp32): step 1 %.2e %.2e, step %d %.2e %.2e"
          % (tag, summary[0][0], summary[0][1], len(summary), summary[-1][0], summary[-1][1]))
    return summary


SHAPES = [(1,), (3,), (4,), (511,), (512, 512), (512, 512, 3, 3), (1000,), (4099,)]
OFFSETS = [0, 0, 0, 0, 0, 0, 1, 3]


def tensor_case(seed, steps=10, shapes=SHAPES):
    rs = np.random.RandomState(seed)
    values = [(0.05 * rs.standard_normal(s)).astype(np.float32) for s in shapes]
    grads = [[torch.from_numpy(gradients(rs, s).astype(np.float32)).to(DEV) for s in shapes] for _ in range(steps)]
    return values, grads


# --------------------------------------------------------------------------- 1. tensors against fp64
@pytest.mark.parametrize("case", ["plain", "weight_decay", "lr_decay"])
def test_tensors_against_fp64(case):
    """Sizes 1, 3, 4, 511, 512 x 512, 2.4 M and two views that start 1 and 3 elements into a buffer, in ONE parameter group (one
    launch per step); ten steps, gradients N(0, 1) x 10^U(-6, 0), lr 1e-4."""
    values, grads = tensor_case(101)
    wd = 1e-2 if case == "weight_decay" else 0.0
    lrs = [1e-4 * (0.9 ** t if case == "lr_decay" else 1.0) for t in range(10)]
    exact = run_fp64(values, grads, lrs, wd)
    ref32 = run_fp32([torch.optim.Adam] * 10, values, grads, lrs, wd, OFFSETS)
    got = run_fp32([Adam] * 10, values, grads, lrs, wd, OFFSETS)
    compare_runs(case, got, ref32, exact)
    moved = float((got[-1][4][0].double() - torch.from_numpy(values[4]).to(DEV).double()).abs().max())
    assert 1e-4 <= moved < 4e-3         # ten steps of up to ~1e-4 each: the comparison is not of two idle optimizers


def test_every_alignment_gives_the_same_bits():
    """The C ABI directly: the same 4099 values stepped where all four pointers are 16-byte aligned (float4 body, scalar tail),
    where all four start 1, 2 or 3 elements later (scalar head, float4 body, scalar tail) and where they disagree (scalar
    throughout) end bit-identical; the elements around every view keep their guard value."""
    L = plib.load()
    n, rs = 4099, np.random.RandomState(7)
    src = [dt(rs.standard_normal(n).astype(np.float32) * s) for s in (0.05, 1.0, 0.01, 1e-4)]   # p, g, m, v (v >= 0 below)
    src[3] = src[3].abs()
    h = C.c_void_p()
    plib.check(L.pny_optim_create(C.byref(h), 0))
    layouts = [(0, 0, 0, 0), (1, 1, 1, 1), (2, 2, 2, 2), (3, 3, 3, 3), (1, 0, 3, 2), (0, 0, 0, 1)]
    bufs = []
    for offs in layouts:
        four = []
        for s, o in zip(src, offs):
            b = torch.full((n + 16,), 777.0, device=DEV)
            b[4 + o:4 + o + n] = s
            four.append((b, 4 + o))
        bufs.append(four)
        ptrs = [C.c_void_p(b.data_ptr() + 4 * o) for b, o in four]
        i = L.pny_optim_add_tensor(h, ptrs[0], ptrs[2], ptrs[3], n)
        assert i == len(bufs) - 1
    grads = (C.c_void_p * len(layouts))(*[b[1][0].data_ptr() + 4 * b[1][1] for b in bufs])
    hyper = plib.AdamHyper(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, step=3)
    plib.check(L.pny_optim_adam_step(h, C.byref(hyper), grads, 0, len(layouts), None, plib.stream_of(torch.device(DEV))))
    torch.cuda.synchronize()
    L.pny_optim_destroy(h)
    first = [b[o:o + n] for b, o in bufs[0]]
    assert not torch.equal(first[0], src[0]) and torch.equal(first[1], src[1])      # stepped; the gradient is read only
    for four in bufs:
        for k, (b, o) in enumerate(four):
            assert torch.equal(b[o:o + n], first[k]), k
            assert bool((b[:o] == 777.0).all()) and bool((b[o + n:] == 777.0).all())


# --------------------------------------------------------------------------- 2. skipped parameters, two groups
def test_skipped_parameters_and_two_groups():
    rs = np.random.RandomState(21)
    shapes = [(300,), (17, 5), (4096,), (33,)]
    values = [(0.05 * rs.standard_normal(s)).astype(np.float32) for s in shapes]
    ps = make_params(values)
    opt = Adam([dict(params=ps[:2], lr=1e-2), dict(params=ps[2:])], lr=1e-4)
    ref = [torch.from_numpy(v).to(DEV).double() for v in values]
    st = [(r, torch.zeros_like(r), torch.zeros_like(r)) for r in ref]
    taken = [0, 0, 0, 0]
    for t in range(3):
        gs = [torch.from_numpy(gradients(rs, s).astype(np.float32)).to(DEV) for s in shapes]
        skip = {0: (1,), 1: (1, 3), 2: ()}[t]       # tensor 1 joins at the third step: its own launch (another step count)
        for i, (p, g) in enumerate(zip(ps, gs)):
            p.grad = None if i in skip else g
        before = [p.detach().clone() for p in ps]
        versions = [p._version for p in ps]
        opt.step()
        torch.cuda.synchronize()
        for i, p in enumerate(ps):
            if i in skip:
                assert torch.equal(p.detach(), before[i]) and p._version == versions[i]
            else:
                taken[i] += 1
                st[i] = adam_fp64(st[i][0], gs[i].double(), st[i][1], st[i][2], taken[i], 1e-2 if i < 2 else 1e-4)
                assert p._version > versions[i]
                assert float((p.detach().double() - st[i][0]).abs().max()) < 1e-6
                # (a group that took the other group's lr would be off by ~1e-2 per step)
            assert (float(opt.state[p]["step"]) if opt.state[p] else 0.0) == float(taken[i])
    assert taken == [3, 1, 3, 2] and set(opt.state_dict()["state"]) == {0, 1, 2, 3}


# --------------------------------------------------------------------------- 3. state interchange on the device
@pytest.mark.parametrize("order", ["torch_then_kernel", "kernel_then_torch"])
def test_state_interchange_on_the_device(order):
    values, grads = tensor_case(303, steps=6, shapes=[(4,), (511,), (512, 512), (1000,)])
    lrs = [1e-4] * 6
    a, b = (torch.optim.Adam, Adam) if order == "torch_then_kernel" else (Adam, torch.optim.Adam)
    exact = run_fp64(values, grads, lrs)
    ref32 = run_fp32([torch.optim.Adam] * 6, values, grads, lrs)
    got = run_fp32([a] * 3 + [b] * 3, values, grads, lrs)
    compare_runs(order, got, ref32, exact)


# --------------------------------------------------------------------------- 4. reproducibility
def test_two_runs_are_bit_identical():
    values, grads = tensor_case(404)
    lrs = [1e-4] * 10
    r0 = run_fp32([Adam] * 10, values, grads, lrs, 1e-2, OFFSETS)[-1]
    r1 = run_fp32([Adam] * 10, values, grads, lrs, 1e-2, OFFSETS)[-1]
    assert all(torch.equal(x, y) for a, b in zip(r0, r1) for x, y in zip(a, b))


# --------------------------------------------------------------------------- scenes for the model tests
def nerf_setup(seed, SB=2, ns=2, H=64, W=64, kc=16, kf=8, kfd=4, B=128):
    net = make_model(pconf.default_mv()["model"], stop_encoder_grad=True)
    net.mlp_coarse.load_state_dict({k: torch.from_numpy(v) for k, v in synth.mlp_state(seed).items()})
    net.mlp_fine.load_state_dict({k: torch.from_numpy(v) for k, v in synth.mlp_state(seed + 1).items()})
    net = net.to(DEV).train()
    lat = torch.from_numpy(np.concatenate([synth.latent(seed + 2 + i, ns, 512, H // 2, W // 2) for i in range(SB)])).to(DEV)
    poses = torch.from_numpy(np.stack([synth.scene_cameras(ns, radius=1.3 + 0.1 * i)[0] for i in range(SB)]))
    focal, cc = torch.tensor(0.9 * W), torch.tensor([[W * 0.5, H * 0.5]])
    rs = np.random.RandomState(seed)
    rays = torch.stack([orc.gen_rays(synth.pose_spherical(100.0 + 25 * i, -20.0, 1.3)[None], W, H, 0.9 * W, 0.3, 1.8)[0]
                        .reshape(-1, 8)[torch.from_numpy(rs.choice(H * W, B, replace=False))] for i in range(SB)]).to(DEV)
    n = SB * B
    draws = dict(u_coarse=rs.rand(n, kc).astype(np.float32), u_fine=rs.rand(n, kf - kfd).astype(np.float32),
                 u_fine2=rs.rand(n, kf - kfd).astype(np.float32), g_depth=rs.randn(n, kfd).astype(np.float32))
    gt = torch.from_numpy(rs.uniform(0, 1, size=(SB, B, 3)).astype(np.float32)).to(DEV)
    ren = NeRFRenderer(n_coarse=kc, n_fine=kf, n_fine_depth=kfd, white_bkgd=True)

    def encode():
        net.encode(torch.zeros(SB, ns, 3, H, W), poses, focal, c=cc, latent=lat)

    def render(call=None):
        ren.draws = draws
        out = (call or (lambda r, want_weights: ren(net, r, want_weights=want_weights)))(rays, want_weights=True)
        return out

    def loss():
        out = render()
        return torch.nn.functional.mse_loss(out["coarse"]["rgb"], gt) + torch.nn.functional.mse_loss(out["fine"]["rgb"], gt)
    return dict(net=net, ren=ren, encode=encode, render=render, loss=loss, rays=rays)


def yolo_setup(seed, K=16):
    net, _ = scene_pair(2, 64, 64, 1792, 21, 5, 3, seed, yolo=True, lat_hw=(16, 16))
    _, tgt_c2w = synth.scene_cameras(2, radius=4.0, phi=-25.0)
    tgt_w2c = np.linalg.inv(tgt_c2w @ np.diag([1.0, -1.0, -1.0, 1.0]).astype(np.float32)).astype(np.float32)
    rays = orc.gen_rays_yolo(tgt_w2c[None], 16, 12, [10.0, 11.0], [8.0, 6.0], 1.0, 6.0)[0].reshape(-1, 8).to(DEV)
    rs = np.random.RandomState(seed)
    u = rs.rand(rays.shape[0], K).astype(np.float32)
    G = torch.from_numpy(rs.standard_normal((rays.shape[0], 3, 7)).astype(np.float32)).to(DEV)
    ren = YoloRenderer(K, 128, 1, 3)
    ren.bind_parallel(net)

    def render():
        ren.draws = dict(u_coarse=u)
        return ren(rays[None])
    return dict(net=net, render=render, loss=lambda: (render() * G).sum() * 1e-3)


def mlp_params(net):
    return [p for k, p in net.named_parameters() if k.startswith("mlp_")]


def fresh_copy(setup_fn, seed, net, precision):
    """A second, freshly built net that receives `net`'s parameter values through load_state_dict: the upload and
    finalize path."""
    other = setup_fn(seed)
    if precision != "auto":
        other["net"].set_matrix_precision(precision)
    other["net"].load_state_dict({k: v.clone() for k, v in net.state_dict().items()})
    other["net"].invalidate_weights()     # (a net that has rendered before would otherwise refresh on the device)
    return other


# --------------------------------------------------------------------------- 5. packed operands are current
@pytest.mark.parametrize("precision", ["auto", "f32", "f16", "f16_train"])
@pytest.mark.parametrize("renderer", ["nerf", "yolo"])
def test_packed_operands_are_current_after_a_step(renderer, precision):
    setup_fn, seed = (nerf_setup, 5100) if renderer == "nerf" else (yolo_setup, 5200)
    s = setup_fn(seed)
    net = s["net"]
    if precision != "auto":
        net.set_matrix_precision(precision)
    params = mlp_params(net)
    opt = Adam(params, lr=1e-3, model=net)
    start = [p.detach().clone() for p in params]
    for _ in range(3):
        if renderer == "nerf":
            s["encode"]()
        opt.zero_grad(set_to_none=True)
        s["loss"]().backward()
        versions = [p._version for p in params]
        opt.step()
        assert all(p._version > v for p, v in zip(params, versions))
        assert net._weights_key() == net._synced_key
    torch.cuda.synchronize()
    assert net.range_status() == 0
    assert sum(not torch.equal(p.detach(), q) for p, q in zip(params, start)) >= len(params) - 12   # (fc_1 starts at zero)
    net.eval()
    other = fresh_copy(setup_fn, seed, net, precision)
    other["net"].eval()
    with torch.no_grad():
        if renderer == "nerf":
            s["encode"]()
            other["encode"]()
        a, b = s["render"](), other["render"]()
    assert net._weights_key() == net._synced_key
    if renderer == "nerf":
        for part in ("coarse", "fine"):
            for k in ("rgb", "depth"):
                assert torch.equal(a[part][k], b[part][k]), (part, k)
        assert bool(torch.isfinite(a["fine"]["rgb"]).all())
    else:
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())


# --------------------------------------------------------------------------- 6. replay of a training loop
def test_replay_of_a_training_loop():
    """Four steps of the bench-shaped loop (SB = 4 objects x 3 views of 128 x 128, 128 rays each, 64 + 32 samples, frozen
    trunk) with torch.optim.Adam, recording every step's 60 gradients; the same gradients fed to this class (and to fp64) from
    the same initial state.  Replaying recorded gradients is deliberate: two live loops diverge through Adam's sign-like update
    on small elements, which says nothing about either side."""
    s = nerf_setup(6100, SB=4, ns=3, H=128, W=128, kc=64, kf=32, kfd=16, B=128)
    net = s["net"]
    params = mlp_params(net)
    assert len(params) == 60
    values = [p.detach().cpu().numpy().copy() for p in params]
    opt = torch.optim.Adam(params, lr=1e-4)
    grads = []
    for _ in range(4):
        s["encode"]()
        opt.zero_grad(set_to_none=True)
        s["loss"]().backward()
        grads.append([p.grad.detach().clone().reshape(-1).view(p.shape) for p in params])
        opt.step()
    torch.cuda.synchronize()
    assert all(float(g.abs().max()) > 0 for g in grads[0][:2])
    lrs = [1e-4] * 4
    exact = run_fp64(values, grads, lrs)
    ref32 = run_fp32([torch.optim.Adam] * 4, values, grads, lrs)
    got = run_fp32([Adam] * 4, values, grads, lrs)
    compare_runs("replay", got, ref32, exact, per_tensor=True)
    # (the live loop used ATen's default multi-tensor Adam; the foreach=False reference lands on the same bits or next to them)
    for p, r in zip(params, ref32[-1]):
        assert float((p.detach() - r[0]).abs().max()) <= 1e-6


# --------------------------------------------------------------------------- 7. trained trunk
def test_trained_trunk_step():
    from test_gpu_deterministic import trunk_case
    net, ren, state, step = trunk_case(7100, SB=2, NS=2, B=128, H=64, W=64, kc=16, kf=8, kfd=4)
    params = [p for p in net.parameters() if p.requires_grad]
    enc = [p for k, p in net.named_parameters() if k.startswith("encoder.") and p.grad is None and p.requires_grad]
    opt = Adam(params, lr=1e-3, model=net)
    step()
    stepped = [p for p in params if p.grad is not None]
    assert sum(1 for k, p in net.named_parameters() if k.startswith("encoder.") and p.grad is not None) >= 80 and enc
    before = [p.detach().clone() for p in stepped]
    net._enc_stale = False
    opt.step()
    torch.cuda.synchronize()
    assert net._enc_stale and net._weights_key() == net._synced_key
    assert all(not torch.equal(p.detach(), b) for p, b in zip(stepped, before) if float(p.grad.abs().max()) > 0)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    images = torch.from_numpy(synth.images(7102, 4, 64, 64)).reshape(2, 2, 3, 64, 64)
    poses = torch.from_numpy(np.stack([synth.scene_cameras(2, radius=1.3 + 0.1 * i)[0] for i in range(2)]))
    focal, cc = torch.tensor(0.9 * 64), torch.tensor([[32.0, 32.0]])
    other, _ = __import__("test_gpu_trunk").trunk_net(7100, True, mlp_seed=7101)
    other.load_state_dict(sd)
    # a training encode uses the stepped values (same parameters and running statistics on both sides)
    lats = []
    for n_ in (net, other):
        n_.train()
        n_.encode(images, poses, focal, c=cc)
        lats.append(n_.differentiable_latent().detach().clone())
    assert torch.equal(lats[0], lats[1])
    # the inference trunk's folded copy is rebuilt from the stepped values (_enc_stale honoured)
    outs = []
    for n_ in (net, other):
        n_.eval()
        with torch.no_grad():
            n_.encode(images, poses, focal, c=cc)
            outs.append(torch.cat([n_.latent(sb) for sb in range(2)]).clone())
    assert torch.equal(outs[0], outs[1])
    stale = make_model(pconf.default_mv()["model"]).to(DEV).eval()
    stale.load_state_dict(state)
    with torch.no_grad():
        stale.encode(images, poses, focal, c=cc)
        assert not torch.equal(outs[0], torch.cat([stale.latent(sb) for sb in range(2)]))


# --------------------------------------------------------------------------- 8. range
def test_weight_driven_out_of_the_f16_range_is_reported_by_its_step():
    """One lin_in weight is driven past 65504 by one step (its own group, a large lr, a unit gradient: Adam's first step moves
    an element by lr).  The refresh chained into the step reports it: PNY_RANGE_WEIGHT is up before any further render, and
    the next no-grad call returns the fp32 kernels' finite result (as tests/test_gpu_range.py expects of a refresh)."""
    import warnings
    from test_gpu_range import fp32_result, make_net, points
    net = make_net(800)
    xyz, vd = points(150, 8)
    with torch.no_grad():
        net(xyz, coarse=True, viewdirs=vd)
        assert net.last_launch_f16x2()
    w = net.mlp_coarse.lin_in.weight
    rest = [p for p in mlp_params(net) if p is not w]
    opt = Adam([dict(params=[w], lr=1.0e5), dict(params=rest)], lr=1e-4, model=net)
    w.grad = torch.zeros_like(w)
    w.grad[5, 9] = 1.0
    moved_from = float(w[5, 9])
    opt.step()
    torch.cuda.synchronize()
    assert abs(float(w[5, 9]) - moved_from) > 9.0e4
    assert net.range_status() & 4, "the step's refresh did not report the weight"
    assert net._weights_key() == net._synced_key
    with torch.no_grad(), warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = net(xyz, coarse=True, viewdirs=vd)
    assert any("weight" in str(x.message) for x in rec)
    assert bool(torch.isfinite(out).all()) and not net.last_launch_f16x2()
    ref = make_net(800).set_matrix_precision("f32")
    ref.load_state_dict({k: v.clone() for k, v in net.state_dict().items()})
    with torch.no_grad():
        assert torch.equal(out, ref(xyz, coarse=True, viewdirs=vd))
    assert fp32_result is not None


# --------------------------------------------------------------------------- 9. bind_parallel(net, [0, 0])
def test_bind_parallel_replicas_render_the_stepped_weights():
    s = nerf_setup(9100, SB=1, ns=2, B=256)
    net, ren = s["net"], s["ren"]
    call = ren.bind_parallel(net, [0, 0])
    opt = Adam(mlp_params(net), lr=1e-3, model=net)
    s["encode"]()
    net.eval()
    with torch.no_grad():
        first = s["render"](call)            # both replicas exist and hold the initial weights
    net.train()
    for _ in range(2):
        s["encode"]()
        opt.zero_grad(set_to_none=True)
        s["loss"]().backward()
        opt.step()
    net.eval()
    with torch.no_grad():
        s["encode"]()
        split = s["render"](call)
        single = s["render"]()
    assert any(r is not None and r is not net for r in call._replicas)
    for part in ("coarse", "fine"):
        assert torch.equal(split[part]["rgb"], single[part]["rgb"]), part
        assert not torch.equal(split[part]["rgb"], first[part]["rgb"])
