"""The latent of a list of feature maps on the device (-m gpu): include/pnyolo.h pny_latent_levels, pny_latent_levels_backward,
pny_scene_set_latent_levels; PixelNeRFNet.encode(latent=[...]).  Cases, references and bars: tests/latent_levels_ref.py.

  * stage sweep, forward and backward, against float64: every element written and nothing behind the buffers, a level of the
    latent's own size copied bit for bit, NULL levels of the backward left alone, two runs bit-identical;
  * marker pixels: a channel offset or stride that is off cannot hide inside a bar;
  * scenes (d_latent = 128, per-object and grouped): the assembled latent read back, renders and queries bit-equal to the
    same calls on that read-back tensor, no stale projected map after a second encode;
  * gradients (d_latent = 256, what the latent-gradient kernels take) through NeRFRenderer and YoloRenderer against the tensor
    path (the same maps through F.interpolate + cat under autograd, fed as latent=tensor) at level sizes whose blends are
    exact (GRAD_SIZES says why), None for a map that takes none, half-precision maps, no graph when nothing takes a
    gradient, bit-identical repeats; bind_parallel(net, [0, 0]).
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import latent_levels_ref as lr
from helpers import DEV
from pixel_nerf_yolo_amd import conf as pconf
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd import synth
from pixel_nerf_yolo_amd.lib import check, ptr, stream_of
from pixel_nerf_yolo_amd.model import make_mlp, make_model
from pixel_nerf_yolo_amd.render import NeRFRenderer, YoloRenderer
from pixel_nerf_yolo_amd.util import gen_rays

pytestmark = pytest.mark.gpu

GUARD_BITS = 0x7FC12345          # a quiet NaN with a payload: "never written" and "not changed" are both visible
GUARD = 4096                     # floats behind every destination


def guarded(numel):
    """(the destination, the whole allocation as int32): numel floats and GUARD more, all set to the guard NaN."""
    whole = torch.full((numel + GUARD,), GUARD_BITS, dtype=torch.int32, device=DEV)
    return whole.view(torch.float32)[:numel], whole


def guard_intact(whole, numel):
    return bool((whole[numel:] == GUARD_BITS).all())


def arrays(c):
    n = len(c["sizes"])
    return ((C.c_int * n)(*c["channels"]), (C.c_int * n)(*[s[0] for s in c["sizes"]]), (C.c_int * n)(*[s[1] for s in c["sizes"]]))


def assemble(c, maps_dev):
    """pny_latent_levels into a guarded NaN-filled buffer -> ((n, h0, w0, L) view, whole allocation, numel)."""
    L = plib.load()
    (h0, w0), ltot = c["sizes"][0], sum(c["channels"])
    numel = c["n"] * h0 * w0 * ltot
    out, whole = guarded(numel)
    ch, hs, ws = arrays(c)
    ptrs = (C.c_void_p * len(maps_dev))(*[m.data_ptr() for m in maps_dev])
    check(L.pny_latent_levels(ptrs, ch, hs, ws, len(maps_dev), c["n"], ptr(out), stream_of(DEV)))
    torch.cuda.synchronize()
    return out.view(c["n"], h0, w0, ltot), whole, numel


def adjoint(c, d_lat_dev, skip=()):
    """pny_latent_levels_backward into guarded NaN-filled buffers -> [(view, whole, numel) per level]; `skip`: NULL levels."""
    L = plib.load()
    outs = [guarded(c["n"] * ch * h * w) + (c["n"] * ch * h * w,) for ch, (h, w) in zip(c["channels"], c["sizes"])]
    ch, hs, ws = arrays(c)
    ptrs = (C.c_void_p * len(outs))(*[None if i in skip else o[0].data_ptr() for i, o in enumerate(outs)])
    check(L.pny_latent_levels_backward(ptr(d_lat_dev), ptrs, ch, hs, ws, len(outs), c["n"], stream_of(DEV)))
    torch.cuda.synchronize()
    return outs


@pytest.fixture(scope="module")
def references():
    """Per case id: the float32 inputs and their float64 latent / gradients, computed once."""
    out = {}
    for c in lr.all_cases():
        maps, g = lr.inputs(c)
        out[lr.case_id(c)] = (maps, g, lr.latent_ref(maps), lr.grads_ref(maps, g))
    return out


@pytest.mark.parametrize("name", sorted(lr.SIZES))
def test_stage_sweep_forward(references, name):
    worst = 0.0
    for c in lr.cases(name):
        key = lr.case_id(c)
        maps, _, ref, _ = references[key]
        maps_dev = [m.to(DEV) for m in maps]
        got, whole, numel = assemble(c, maps_dev)
        assert bool(torch.isfinite(got).all()), key + ": an element was not written"
        assert guard_intact(whole, numel), key + ": written behind the latent"
        err = lr.rel_err(got.cpu(), lr.nhwc(ref), "act")
        worst = max(worst, err)
        print("%s: forward error %.3e (bar %.3e)" % (key, err, lr.FWD_BAR))
        assert err <= lr.FWD_BAR, key
        off = 0
        for m, md in zip(maps, maps_dev):
            if m.shape[-2:] == maps[0].shape[-2:]:
                assert torch.equal(got[..., off:off + m.shape[1]], md.permute(0, 2, 3, 1)), key + ": a same-size level is not a copy"
            off += m.shape[1]
        again, _, _ = assemble(c, maps_dev)
        assert torch.equal(got, again), key + ": two runs differ"
    print("%s: worst forward error %.3e" % (name, worst))


@pytest.mark.parametrize("name", sorted(lr.SIZES))
def test_stage_sweep_backward(references, name):
    for j, c in enumerate(lr.cases(name)):
        key = lr.case_id(c)
        _, g, _, ref = references[key]
        d_lat = lr.nhwc(g).to(DEV)
        outs = adjoint(c, d_lat)
        for i, ((got, whole, numel), r) in enumerate(zip(outs, ref)):
            assert bool(torch.isfinite(got).all()), "%s: level %d not wholly written" % (key, i)
            assert guard_intact(whole, numel), "%s: written behind level %d" % (key, i)
            err = lr.rel_err(got.view(r.shape).cpu(), r, "grad")
            print("%s: level %d backward error %.3e (bar %.3e)" % (key, i, err, lr.BWD_BAR))
            assert err <= lr.BWD_BAR, (key, i)
        skip = {j % len(outs)} | ({len(outs) - 1} if len(outs) > 2 else set())
        again = adjoint(c, d_lat, skip=skip)
        for i, ((got, whole, numel), (first, _, _)) in enumerate(zip(again, outs)):
            if i in skip:
                assert bool((whole == GUARD_BITS).all()), "%s: NULL level %d was touched" % (key, i)
            else:
                assert torch.equal(got, first) and guard_intact(whole, numel), "%s: level %d differs between two runs" % (key, i)
    c = lr.cases(name)[0]
    assert all(bool((o[1] == GUARD_BITS).all()) for o in adjoint(c, lr.nhwc(references[lr.case_id(c)][1]).to(DEV), skip=set(range(8))))


@pytest.mark.parametrize("name", sorted(lr.SIZES))
def test_markers_land_in_their_channels_and_nowhere_else(references, name):
    for c in lr.cases(name):
        key = lr.case_id(c)
        plain, _ = assemble(c, [m.to(DEV) for m in references[key][0]])[:2]
        marked_maps, _ = lr.inputs(c, markers=True)
        got, whole, numel = assemble(c, [m.to(DEV) for m in marked_maps])
        assert guard_intact(whole, numel)
        ref = lr.nhwc(lr.latent_ref(marked_maps))
        assert float(ref.abs().max()) >= 0.99 * lr.MARKER                    # (the marker reaches the latent in every case)
        assert lr.rel_err(got.cpu(), ref, "act") <= lr.FWD_BAR, key
        changed = (got != plain).reshape(-1, got.shape[-1]).any(dim=0).cpu()
        allowed = torch.zeros_like(changed)
        allowed[lr.marker_channels(c)] = True
        assert not bool((changed & ~allowed).any()), "%s: channels %s changed" % (key, torch.nonzero(changed & ~allowed).flatten().tolist())
        # level 0 is a copy: its marker sits at the last pixel of its two channels, exactly
        assert float(got[0, -1, -1, 0]) == lr.MARKER and float(got[-1, -1, -1, c["channels"][0] - 1]) == lr.MARKER


# --------------------------------------------------------------------------- scenes
D_LATENT = 128
SPLITS = ((24, 40, 64), (3, 61, 64))
LEVEL_SIZES = ((8, 10), (4, 5), (11, 13))
H = W = 32


def small_net(yolo=False, train=False, seed=6100, d_latent=D_LATENT):
    """A model at a small d_latent (the Python model sizes its MLPs by the backbone's channel count: they are rebuilt)."""
    c = pconf.yolo() if yolo else pconf.default_mv()
    m = c.d["model"]
    m["encoder"]["backbone"] = "custom"
    kinds = ("mlp_coarse",) if yolo else ("mlp_coarse", "mlp_fine")
    for k in kinds:
        m[k].update({"n_blocks": 3, "combine_layer": 2})
    net = make_model(c["model"], stop_encoder_grad=True)
    net.d_latent = net.latent_size = d_latent
    for i, k in enumerate(kinds):
        mlp = make_mlp(c["model"][k], net.d_in, d_latent)
        sd = synth.mlp_state(seed + i, d_latent=d_latent, d_out=net.d_out, n_blocks=3, combine_layer=2)
        mlp.load_state_dict({n: torch.from_numpy(v) for n, v in sd.items()}, strict=True)
        setattr(net, k, mlp)
    net = net.to(DEV)
    return net.train() if train else net.eval()


def level_maps(split, n, seed, sizes=LEVEL_SIZES):
    rs = np.random.RandomState(seed)
    return [torch.from_numpy(rs.randn(n, ch, h, w).astype(np.float32)).to(DEV) for ch, (h, w) in zip(split, sizes)]


def cameras(SB, NS):
    poses = np.stack([synth.scene_cameras(NS, radius=1.3 + 0.1 * i)[0] for i in range(SB)])
    return torch.zeros(SB, NS, 3, H, W), torch.from_numpy(poses), torch.tensor(0.9 * W)


def target_rays(SB, B, seed=3):
    rs = np.random.RandomState(seed)
    rows = []
    for i in range(SB):
        tgt = torch.from_numpy(synth.pose_spherical(100.0 + 25 * i, -20.0, 1.3))[None].to(DEV)
        r = gen_rays(tgt, W, H, torch.tensor(0.9 * W), 0.8, 1.8).reshape(-1, 8)
        rows.append(r[torch.from_numpy(rs.choice(H * W, B, replace=False)).to(DEV)])
    return torch.stack(rows).contiguous()


def nerf_draws(n, kc, kf, kfd, seed=11):
    rs = np.random.RandomState(seed)
    return dict(u_coarse=rs.rand(n, kc).astype(np.float32), u_fine=rs.rand(n, kf - kfd).astype(np.float32),
                u_fine2=rs.rand(n, kf - kfd).astype(np.float32), g_depth=rs.randn(n, kfd).astype(np.float32))


def query_points(SB, n, seed=17):
    rs = np.random.RandomState(seed)
    xyz = torch.from_numpy(rs.uniform(-0.3, 0.3, size=(SB, n, 3)).astype(np.float32)).to(DEV)
    vd = Fn.normalize(torch.from_numpy(rs.standard_normal((SB, n, 3)).astype(np.float32)), dim=-1).to(DEV)
    return xyz, vd


def read_back(net, SB):
    return torch.cat([net.latent(sb) for sb in range(SB)])


def same_outputs(a, b):
    return all(torch.equal(a[p][k], b[p][k]) for p in a for k in a[p])


@pytest.mark.parametrize("split", SPLITS, ids=lambda s: "x".join(str(v) for v in s))
@pytest.mark.parametrize("grouped", (False, True), ids=("per_object", "grouped"))
def test_scene_latent_render_and_query_equal_the_read_back_tensor(split, grouped):
    SB, NS, B, kc, kf, kfd = 2, 2, 128, 16, 8, 4
    net = small_net(train=grouped)                      # (train() with trainable MLPs and SB > 1: encode() fills the grouped scene)
    images, poses, focal = cameras(SB, NS)
    maps = level_maps(split, SB * NS, 6200 + split[0])
    rays, (xyz, vd) = target_rays(SB, B), query_points(SB, 256)
    ren = NeRFRenderer(n_coarse=kc, n_fine=kf, n_fine_depth=kfd, white_bkgd=True)
    ren = ren.train() if grouped else ren.eval()

    def calls():
        ren.draws = nerf_draws(SB * B, kc, kf, kfd)
        if grouped:
            out = ren(net, rays, want_weights=True)
            assert net._last_grouped()
            out = {p: {k: v.detach() for k, v in d.items()} for p, d in out.items()}
        else:
            with torch.no_grad():
                out = ren(net, rays, want_weights=True)
        with torch.no_grad():
            q = net(xyz, coarse=True, viewdirs=vd)
        torch.cuda.synchronize()
        return out, q

    net.encode(images, poses, focal, latent=maps)
    assert (net._group_scene() is not None) == grouped
    out_l, q_l = calls()
    lat = read_back(net, SB)
    ref = lr.latent_ref([m.cpu() for m in maps])
    err = lr.rel_err(lat.cpu(), ref, "act")
    print("read-back latent error %.3e (bar %.3e)" % (err, lr.FWD_BAR))
    assert lat.shape == ref.shape and err <= lr.FWD_BAR
    net.encode(images, poses, focal, latent=lat)
    out_t, q_t = calls()
    assert same_outputs(out_l, out_t) and torch.equal(q_l, q_t)
    assert float(q_l.abs().max()) > 0 and bool(torch.isfinite(q_l).all())


def test_scene_entry_checks_the_model_and_the_view_count():
    L = plib.load()
    net = small_net()
    images, poses, focal = cameras(1, 2)
    maps = level_maps(SPLITS[0], 2, 6300)
    net.encode(images, poses, focal, latent=maps)
    s, err = net._scene(0), L.pny_last_error

    def rc(split, n):
        m = level_maps(split, n, 6301)
        ptrs = (C.c_void_p * 3)(*[t.data_ptr() for t in m])
        ch, hs, ws = ((C.c_int * 3)(*v) for v in (split, [v[0] for v in LEVEL_SIZES], [v[1] for v in LEVEL_SIZES]))
        return L.pny_scene_set_latent_levels(s, ptrs, ch, hs, ws, 3, n, stream_of(DEV))

    assert rc((24, 40, 60), 2) == -1 and err().decode().startswith("pny_scene_set_latent_levels:") and b"d_latent" in err()
    assert rc(SPLITS[0], 17) == -1 and err().decode().startswith("pny_scene_set_latent_levels:")
    assert rc(SPLITS[1], 2) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="d_latent is 128"):
        net.encode(images, poses, focal, latent=maps[:2])


def test_second_encode_serves_no_stale_projected_map():
    SB, NS, B, kc = 1, 2, 512, 32
    net = small_net().set_latent_projection("on")
    images, poses, focal = cameras(SB, NS)
    rays = target_rays(SB, B)
    ren = NeRFRenderer(n_coarse=kc, n_fine=0, n_fine_depth=0, white_bkgd=True).eval()

    def render():
        ren.draws = dict(u_coarse=np.random.RandomState(5).rand(SB * B, kc).astype(np.float32))
        with torch.no_grad():
            out = ren(net, rays)
        torch.cuda.synchronize()
        assert net.last_mlp_stats(full=True)["projected"]
        return out

    maps_a, maps_b = level_maps(SPLITS[0], NS, 6400), level_maps(SPLITS[0], NS, 6401)
    net.encode(images, poses, focal, latent=maps_a)
    out_a = render()
    net.encode(images, poses, focal, latent=maps_b)
    out_b = render()
    lat_b = read_back(net, SB)
    fresh = small_net().set_latent_projection("on")
    net, old = fresh, net
    net.encode(images, poses, focal, latent=lat_b)
    out_ref = render()
    assert same_outputs(out_b, out_ref)
    assert not torch.equal(out_a["coarse"]["rgb"], out_b["coarse"]["rgb"])
    del old


# --------------------------------------------------------------------------- gradients
# (the latent-gradient kernels take d_latent in multiples of 256: the scene tests' splits with the last level widened)
D_GRAD = 256
GRAD_SPLITS = ((24, 40, 192), (3, 61, 192))
# The list path and the tensor path are compared through the whole render, and the MLP's relu makes that comparison discrete: a
# latent that differs in its last bit flips the odd pre-activation near zero, and one flipped unit moves a map's gradient by
# 1e-4 .. 1e-3 of its max (measured: 6.2e-4 through the YOLO renderer at the sizes of the scene tests, where ATen's blend on
# the device, contracted to fused multiply-adds, and the kernel's differ by 1.4e-7).  The backward bar bounds the adjoint, not
# that lottery, so these tests use level sizes whose blends are exact in float32 whatever the contraction -- scale 1/2 (weights
# 0, 1/2, 1: every product exact, every sum rounded once) and scale 2 (weights 0 and 1) -- and assert that both paths hand the
# renderer the same latent bits.  Arbitrary weights are the stage sweep's and the scene tests' ground.
GRAD_SIZES = ((9, 5), (5, 3), (17, 9))


def tensor_path_latent(maps):
    size0 = tuple(maps[0].shape[-2:])
    return torch.cat([Fn.interpolate(m, size0, mode="bilinear", align_corners=True) for m in maps], dim=1)


def leaves(split, n, seed, frozen=(), sizes=LEVEL_SIZES):
    maps = level_maps(split, n, seed, sizes)
    for i, m in enumerate(maps):
        m.requires_grad_(i not in frozen)
    return maps


def check_map_grads(got_maps, ref_maps, frozen, what):
    for i, (a, b) in enumerate(zip(got_maps, ref_maps)):
        if i in frozen:
            assert a.grad is None and b.grad is None, "%s: map %d takes no gradient" % (what, i)
            continue
        assert a.grad is not None and a.grad.shape == a.shape and a.grad.dtype == a.dtype and a.grad.device == a.device
        err = lr.rel_err(a.grad.cpu(), b.grad.cpu(), "grad")
        print("%s: map %d gradient vs the tensor path %.3e (bar %.3e)" % (what, i, err, lr.BWD_BAR))
        assert err <= lr.BWD_BAR, (what, i)


@pytest.mark.parametrize("split", GRAD_SPLITS, ids=lambda s: "x".join(str(v) for v in s))
def test_map_gradients_through_the_nerf_renderer(split):
    SB, NS, B, kc, kf, kfd = 2, 2, 128, 16, 8, 4
    net = small_net(train=True, d_latent=D_GRAD)
    net.set_deterministic(True)
    images, poses, focal = cameras(SB, NS)
    rays = target_rays(SB, B)
    gt = torch.from_numpy(np.random.RandomState(7).uniform(0, 1, size=(SB, B, 3)).astype(np.float32)).to(DEV)
    ren = NeRFRenderer(n_coarse=kc, n_fine=kf, n_fine_depth=kfd, white_bkgd=True).train()
    frozen, latents = (1,), []

    def step(latent_of):
        maps = leaves(split, SB * NS, 6500 + split[0], frozen, GRAD_SIZES)
        net.zero_grad(set_to_none=True)
        net.encode(images, poses, focal, latent=latent_of(maps))
        assert net._group_scene() is not None
        latents.append(read_back(net, SB))
        ren.draws = nerf_draws(SB * B, kc, kf, kfd)
        out = ren(net, rays, want_weights=True)
        (Fn.mse_loss(out["coarse"]["rgb"], gt) + Fn.mse_loss(out["fine"]["rgb"], gt)).backward()
        torch.cuda.synchronize()
        return maps

    got = step(lambda maps: maps)
    assert net.last_latent_grad_deterministic()
    ref = step(tensor_path_latent)
    assert torch.equal(latents[0], latents[1]), "the two paths' latents differ: the gradients are not comparable at the bar"
    check_map_grads(got, ref, frozen, "nerf %s" % (split,))
    again = step(lambda maps: maps)
    assert all(torch.equal(a.grad, b.grad) for i, (a, b) in enumerate(zip(got, again)) if i not in frozen)


@pytest.mark.parametrize("split", GRAD_SPLITS, ids=lambda s: "x".join(str(v) for v in s))
def test_map_gradients_through_the_yolo_renderer(split):
    NS, K = 2, 32
    net = small_net(yolo=True, train=True, d_latent=D_GRAD)
    net.set_deterministic(True)
    # world->cam extrinsics of cameras looking down -z: the scene lies at z < 0, where YOLO mode keeps the latent; the target
    # rays run from a camera of the same ring through the scene (near 2, far 6 at radius 4)
    src_c2w, tgt_c2w = synth.scene_cameras(NS, radius=4.0, phi=-25.0)
    poses = torch.from_numpy(np.stack([np.linalg.inv(p) for p in src_c2w]).astype(np.float32))
    focal, cc = torch.tensor([[40.0, 44.0]]), torch.tensor([[W * 0.5, H * 0.5 - 2]])
    rays = gen_rays(torch.from_numpy(tgt_c2w)[None].to(DEV), 16, 16, torch.tensor(14.4), 2.0, 6.0).reshape(-1, 8).contiguous()
    rs = np.random.RandomState(9)
    u = rs.rand(rays.shape[0], K).astype(np.float32)
    G = torch.from_numpy(rs.standard_normal((rays.shape[0], 3, 7)).astype(np.float32)).to(DEV)
    ren = YoloRenderer(K, 128, 1, 3)
    ren.bind_parallel(net)
    frozen, latents = (0,), []

    def step(latent_of):
        maps = leaves(split, NS, 6600 + split[0], frozen, GRAD_SIZES)
        net.zero_grad(set_to_none=True)
        net.encode(torch.zeros(1, NS, 3, H, W), poses[None], focal, c=cc, latent=latent_of(maps))
        latents.append(read_back(net, 1))
        ren.draws = dict(u_coarse=u)
        (ren(rays[None]) * G).sum().backward()
        torch.cuda.synchronize()
        return maps

    got = step(lambda maps: maps)
    ref = step(tensor_path_latent)
    assert torch.equal(latents[0], latents[1]), "the two paths' latents differ: the gradients are not comparable at the bar"
    assert all(float(m.grad.abs().max()) > 0 for i, m in enumerate(ref) if i not in frozen)
    check_map_grads(got, ref, frozen, "yolo %s" % (split,))
    again = step(lambda maps: maps)
    assert all(torch.equal(a.grad, b.grad) for i, (a, b) in enumerate(zip(got, again)) if i not in frozen)


def test_half_precision_maps_take_gradients_in_their_own_dtype_and_the_query_backward_reaches_them():
    net = small_net(train=True, d_latent=D_GRAD)
    net.set_deterministic(True)
    images, poses, focal = cameras(1, 2)
    maps = [m.half().requires_grad_() for m in level_maps(GRAD_SPLITS[0], 2, 6700)]
    net.encode(images, poses, focal, latent=maps)
    xyz, vd = query_points(1, 256)
    net(xyz, coarse=True, viewdirs=vd).square().sum().backward()
    torch.cuda.synchronize()
    for m in maps:
        assert m.grad is not None and m.grad.dtype == torch.float16 and m.grad.shape == m.shape
        assert bool(torch.isfinite(m.grad).all())
    assert any(float(m.grad.float().abs().max()) > 0 for m in maps)


def test_no_graph_when_nothing_takes_a_gradient():
    net = small_net(train=True)
    for p in net.parameters():
        p.requires_grad_(False)
    images, poses, focal = cameras(1, 2)
    net.encode(images, poses, focal, latent=level_maps(SPLITS[0], 2, 6800))
    assert net.differentiable_latent() is None
    ren = NeRFRenderer(n_coarse=16, n_fine=0, n_fine_depth=0, white_bkgd=True).train()
    out = ren(net, target_rays(1, 64))
    xyz, vd = query_points(1, 64)
    q = net(xyz, coarse=True, viewdirs=vd)
    assert not out["coarse"]["rgb"].requires_grad and out["coarse"]["rgb"].grad_fn is None
    assert not q.requires_grad and q.grad_fn is None


def test_bind_parallel_replicas_render_the_assembled_latent():
    """(A replica is built from the master's configuration, so this model has the configuration's own d_latent, 1792.)"""
    SB, NS, B, kc = 1, 2, 256, 16
    c = pconf.default_mv()
    c.d["model"]["encoder"]["backbone"] = "custom"
    c.d["model"]["mlp_fine"] = {"type": "empty"}
    net = make_model(c["model"], stop_encoder_grad=True).eval()
    net.mlp_coarse.load_state_dict({k: torch.from_numpy(v) for k, v in synth.mlp_state(6901, d_latent=1792).items()}, strict=True)
    net = net.to(DEV)
    images, poses, focal = cameras(SB, NS)
    net.encode(images, poses, focal, latent=level_maps((256, 512, 1024), NS, 6900))
    rays = target_rays(SB, B)
    ren = NeRFRenderer(n_coarse=kc, n_fine=0, n_fine_depth=0, white_bkgd=True).eval()
    u = np.random.RandomState(5).rand(SB * B, kc).astype(np.float32)
    with torch.no_grad():
        ren.draws = dict(u_coarse=u)
        single = ren(net, rays)
        ren.draws = dict(u_coarse=u)
        call = ren.bind_parallel(net, [0, 0])
        double = call(rays)
    torch.cuda.synchronize()
    assert any(r is not None and r is not net for r in call._replicas)
    assert same_outputs(single, double)
