"""
Which kernel each call runs (-m gpu): a table of the routes of csrc/render_api.hip route_mlp / train_api.hip route_bwd, as the calls
report them (last_launch_precision, the `projected` flag of last_mlp_stats, last_backward_precision, last_flush_precision, the
recompute term of last_backward_stats).  The expected values are written out from the rules of include/pnyolo.h
(pny_scene_set_projection, pny_scene_set_precision, PNY_PRECISION_*), not computed by a copy of the routing code.

Tiny models (2 residual blocks, combine_layer 1, d_latent 128 / 256, a 4 x 4 latent map, 1 / 2 views) with in-range random
weights: nothing here is an error path (tests/test_gpu_range.py covers those), and no value is compared but for bit-identity.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import DEV
from pixel_nerf_yolo_amd import conf as pconf
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd import synth
from pixel_nerf_yolo_amd.model import make_mlp, make_model
from pixel_nerf_yolo_amd.render import NeRFRenderer
from pixel_nerf_yolo_amd.util import gen_rays

pytestmark = pytest.mark.gpu

HL = WL = 4                 # latent map: AUTO projection of a scene without f16 kernels starts at 2 * HL * WL = 32 points
H = W = 32
PRECISIONS = ("auto", "f32", "f16x2", "f16", "f16_train")
PROJECTIONS = ("off", "on", "auto")


def tiny_net(L=256, ns=2, nb=2, cl=1, prec=None, proj=None, train=False, seed=5100):
    """(net, target pose): a model of nb blocks at d_latent L on a supplied (ns, L, 4, 4) latent.  The Python model sizes its
    MLPs by the backbone's channel count (512 / 1792); the two MLPs are rebuilt at L before the first library call."""
    c = pconf.default_mv()
    m = c.d["model"]
    m["encoder"]["backbone"] = "custom"       # no trunk: the latent is supplied
    for k in ("mlp_coarse", "mlp_fine"):
        m[k].update({"n_blocks": nb, "combine_layer": cl})
    net = make_model(c["model"], stop_encoder_grad=True)
    net.d_latent = net.latent_size = L
    for i, k in enumerate(("mlp_coarse", "mlp_fine")):
        mlp = make_mlp(c["model"][k], net.d_in, L)
        sd = synth.mlp_state(seed + i, d_latent=L, n_blocks=nb, combine_layer=cl)
        mlp.load_state_dict({n: torch.from_numpy(v) for n, v in sd.items()}, strict=True)
        setattr(net, k, mlp)
    net = net.to(DEV)
    net = net.train() if train else net.eval()
    if prec is not None:
        net.set_matrix_precision(prec)
    if proj is not None:
        net.set_latent_projection(proj)
    poses, tgt = synth.scene_cameras(ns)
    net.encode(torch.zeros(1, ns, 3, H, W), torch.from_numpy(poses)[None], torch.tensor(0.9 * W),
               latent=torch.from_numpy(synth.latent(seed + 7, ns, L, HL, WL)))
    return net, tgt


def rays_of(tgt, n):
    r = gen_rays(torch.from_numpy(tgt)[None].to(DEV), W, H, torch.tensor(0.9 * W), 0.8, 1.8).reshape(-1, 8)
    return r[torch.from_numpy(np.random.RandomState(9).choice(H * W, n, replace=False)).to(DEV)].contiguous()


def query(net, n):
    rs = np.random.RandomState(n)
    xyz = torch.from_numpy(rs.uniform(-0.3, 0.3, size=(1, n, 3)).astype(np.float32)).to(DEV)
    vd = torch.nn.functional.normalize(torch.from_numpy(rs.standard_normal((1, n, 3)).astype(np.float32)), dim=-1).to(DEV)
    with torch.no_grad():
        out = net(xyz, coarse=True, viewdirs=vd)
    torch.cuda.synchronize()
    return out


def render(net, tgt, n_rays, kc, kf=0):
    ren = NeRFRenderer(n_coarse=kc, n_fine=kf, n_fine_depth=kf // 2, white_bkgd=True).eval()
    with torch.no_grad():
        out = ren(net, rays_of(tgt, n_rays)[None])
    torch.cuda.synchronize()
    return out


def reported(net):
    return net.last_launch_precision(), bool(net.last_mlp_stats(full=True)["projected"])


# --------------------------------------------------------------------------- no-grad query and render
# (kernel, projected) of a launch of at least 2 * HL * WL points on a model the f16 kernels support.  OFF: the reference's
# operation order, always fp32.  A projected launch runs fp32 on an F32 scene, the split kernel on AUTO / F16X2, the
# single-plane kernel on F16 / F16_TRAIN.
NOGRAD = {
    ("auto", "off"): ("f32", False), ("auto", "on"): ("f16x2", True), ("auto", "auto"): ("f16x2", True),
    ("f32", "off"): ("f32", False), ("f32", "on"): ("f32", True), ("f32", "auto"): ("f32", True),
    ("f16x2", "off"): ("f32", False), ("f16x2", "on"): ("f16x2", True), ("f16x2", "auto"): ("f16x2", True),
    ("f16", "off"): ("f32", False), ("f16", "on"): ("f16", True), ("f16", "auto"): ("f16", True),
    ("f16_train", "off"): ("f32", False), ("f16_train", "on"): ("f16", True), ("f16_train", "auto"): ("f16", True),
}
# d_latent, views, query points: one tile / one sample into the second tile
SHAPES = {"L128_ns1_64pts": (128, 1, 64), "L256_ns2_65pts": (256, 2, 65)}


def test_table_is_complete():
    assert set(NOGRAD) == {(p, z) for p in PRECISIONS for z in PROJECTIONS}


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("proj", PROJECTIONS)
@pytest.mark.parametrize("prec", PRECISIONS)
def test_no_grad_query_and_render(prec, proj, shape):
    L, ns, n = SHAPES[shape]
    net, tgt = tiny_net(L, ns, prec=prec, proj=proj)
    out = query(net, n)
    assert out.shape == (1, n, 4) and bool(torch.isfinite(out).all())
    assert reported(net) == NOGRAD[prec, proj]
    res = render(net, tgt, 4, 16, 8)             # 64 coarse and 96 fine points
    assert bool(torch.isfinite(res["fine"]["rgb"]).all())
    assert reported(net) == NOGRAD[prec, proj]
    assert net.last_mlp_stats(full=True)["launches"] == 2


@pytest.mark.parametrize("proj", ("on", "auto"))
@pytest.mark.parametrize("prec", PRECISIONS)
def test_seven_blocks_run_fp32(prec, proj):
    """More than 6 residual blocks: no f16 kernel exists, every precision mode reports fp32."""
    net, tgt = tiny_net(128, 2, nb=7, prec=prec, proj=proj)
    query(net, 65)
    assert reported(net) == ("f32", True)        # 65 >= 2 * HL * WL: projected under AUTO too
    render(net, tgt, 4, 16, 8)
    assert reported(net) == ("f32", True)


@pytest.mark.parametrize("n_rays,kc,projected", [(11, 3, True), (4, 8, True), (1, 31, False)])
def test_auto_projection_threshold_on_f32_scene(n_rays, kc, projected):
    """AUTO projection without f16 kernels: from 2 * HL * WL = 32 points per launch (33, 32) and not below (31)."""
    net, tgt = tiny_net(128, 2, prec="f32", proj="auto")
    render(net, tgt, n_rays, kc)
    assert reported(net) == ("f32", projected)


def test_auto_projects_every_launch_with_f16_kernels():
    net, tgt = tiny_net(128, 2, prec="auto", proj="auto")
    render(net, tgt, 1, 31)
    assert reported(net) == ("f16x2", True)


def test_split_shape_is_bit_identical(monkeypatch):
    """PNYOLO_H2_SPLIT=0 / 1: the split-f16 kernel on 64- and on 32-sample tiles, the same arithmetic per sample."""
    outs = []
    for v in ("0", "1"):
        monkeypatch.setenv("PNYOLO_H2_SPLIT", v)
        net, _ = tiny_net(256, 2, prec="auto")
        outs.append(query(net, 64))
        assert reported(net) == ("f16x2", True)
    assert torch.equal(outs[0], outs[1])


# --------------------------------------------------------------------------- training step
KC, KF, KFD, B = 16, 8, 4, 4        # 64 coarse points = 1 tile, 96 fine points = 2 tiles per pass


def train_step(prec, proj=None):
    """One render + backward through autograd: the reservation render.py makes fits both passes exactly."""
    net, tgt = tiny_net(256, 2, prec=prec, proj=proj, train=True)
    ren = NeRFRenderer(n_coarse=KC, n_fine=KF, n_fine_depth=KFD, white_bkgd=True).train()
    out = ren(net, rays_of(tgt, B)[None], want_weights=True)
    fwd = reported(net)
    (out["coarse"]["rgb"].sum() + out["fine"]["rgb"].sum()).backward()
    torch.cuda.synchronize()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for _, p in net.trainable_mlp_parameters())
    return fwd, net.last_backward_precision(), net.last_flush_precision(), net.last_backward_stats()["flops"][0]


# stash forward (kernel, projected), dX chain, flush: an F16 scene trains as AUTO; the stashing forward projects whenever it
# runs an f16 kernel and runs fp32 on the raw latent otherwise
TRAIN = {
    "auto": (("f16x2", True), "f16x2", "f16x2"),
    "f32": (("f32", False), "f32", "f32"),
    "f16": (("f16x2", True), "f16x2", "f16x2"),
    "f16_train": (("f16", True), "f16", "f16"),
}


@pytest.mark.parametrize("prec", sorted(TRAIN))
def test_training_step_with_fitting_reservation(prec):
    fwd, bwd, flush, recompute = train_step(prec)
    assert (fwd, bwd, flush) == TRAIN[prec]
    assert recompute == 0.0                      # the backward started from the forward's stash


def test_stash_forward_ignores_projection_off():
    fwd, bwd, _, recompute = train_step("auto", proj="off")
    assert fwd == ("f16x2", True) and bwd == "f16x2" and recompute == 0.0


@pytest.mark.parametrize("env,bwd", [("f32", "f32"), ("f16x2", "f16x2")])
def test_backward_precision_override(monkeypatch, env, bwd):
    monkeypatch.setenv("PNYOLO_BWD_PRECISION", env)
    fwd, got, flush, recompute = train_step("auto")
    assert fwd == ("f16x2", True)                # the override is the backward's alone
    assert (got, flush) == (bwd, bwd) and recompute == 0.0


def abi_train_step(coarse_tiles, fine_tiles, immediate):
    """The same step through the C ABI with a reservation of the caller's choice on an AUTO scene with projection OFF (so that
    a stashing forward, which forces the projection, and a plain one report differently)."""
    L = plib.load()
    net, tgt = tiny_net(256, 2, prec="auto", proj="off", train=True)
    dev = torch.device(DEV)
    st = plib.stream_of(dev)
    net._sync()
    plib.check(L.pny_model_defer_weight_grads(net._h_model, 1, 2, coarse_tiles, fine_tiles))
    ren = NeRFRenderer(n_coarse=KC, n_fine=KF, n_fine_depth=KFD, white_bkgd=True).train()
    rays = rays_of(tgt, B)[None]
    res, sv = ren._render(net, rays, want_weights=True, save=True, stash=True)
    fwd = reported(net)                          # of the fine pass, the last launch
    grads = net.bind_mlp_grads()
    g = torch.full((B, 3), 0.01, device=dev)
    saved = plib.RenderSaved(z_coarse=sv["z_coarse"][0].data_ptr(), sample_coarse=sv["sample_coarse"][0].data_ptr(),
                             z_fine=sv["z_fine"][0].data_ptr(), sample_fine=sv["sample_fine"][0].data_ptr(),
                             depth_coarse=res["coarse"]["depth"][0].data_ptr())
    up = plib.RenderGrads(rgb_coarse=g.data_ptr(), rgb_fine=g.data_ptr())
    plib.check(L.pny_render_backward(net._scene(0), plib.ptr(sv["rays"][0]), B, C.byref(sv["opts"][0]), C.byref(saved),
                                     C.byref(up), plib.ACC_ADD | (plib.ACC_IMMEDIATE if immediate else 0), st))
    if not immediate:
        plib.check(L.pny_model_flush_weight_grads(net._h_model, plib.ACC_ADD, st))
    plib.check(L.pny_model_defer_weight_grads(net._h_model, 0, 0, 0, 0))
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in grads)
    return fwd, net.last_backward_precision(), net.last_backward_stats()["flops"]


def test_reservation_one_tile_too_small():
    """The fine pass needs 2 tiles.  With both reserved it stashes (forced projection, split kernel) and the backward starts at
    the chain; with one reserved the call falls through to the plain forward -- projection OFF: fp32 on the raw latent -- and
    the backward, told that the reservation is not its own (accumulate bit 2), recomputes both passes."""
    fwd, bwd, flops = abi_train_step(1, 2, immediate=False)
    assert fwd == ("f16x2", True) and bwd == "f16x2" and flops[0] == 0.0
    fwd, bwd, flops = abi_train_step(1, 1, immediate=True)
    assert fwd == ("f32", False) and bwd == "f16x2"
    assert flops[0] > 0.0 and flops[0] == flops[2]     # every forward GEMM recomputed once


def reservation_net(lat_grad):
    """(net, target pose, latent or None) of the foreign-backward test: the AUTO training net; lat_grad = a latent that requires
    grad under the deterministic latent gradient, so that every gradient of the step has a fixed order of summation."""
    net, tgt = tiny_net(256, 2, prec="auto", train=True)
    lat = None
    if lat_grad:
        net.set_deterministic(True)
        lat = torch.from_numpy(synth.latent(5107, 2, 256, HL, WL)).to(DEV).requires_grad_()
        net.encode(torch.zeros(1, 2, 3, H, W), torch.from_numpy(synth.scene_cameras(2)[0])[None], torch.tensor(0.9 * W), latent=lat)
    return net, tgt, lat


def render_loss(net, tgt):
    ren = NeRFRenderer(n_coarse=KC, n_fine=KF, n_fine_depth=KFD, white_bkgd=True).train()
    out = ren(net, rays_of(tgt, B)[None], want_weights=True)
    return out["coarse"]["rgb"].sum() + out["fine"]["rgb"].sum()


def query_loss(net, n=65):      # two tiles, the second partial
    rs = np.random.RandomState(n)
    xyz = torch.from_numpy(rs.uniform(-0.3, 0.3, size=(1, n, 3)).astype(np.float32)).to(DEV)
    vd = torch.nn.functional.normalize(torch.from_numpy(rs.standard_normal((1, n, 3)).astype(np.float32)), dim=-1).to(DEV)
    return net(xyz, coarse=True, viewdirs=vd).sum()


@pytest.mark.parametrize("lat_grad", (False, True), ids=("frozen_trunk", "deterministic_latent_grad"))
def test_backward_on_someone_elses_reservation(lat_grad):
    """A query's backward while a training render's reservation is outstanding: it computes its weight gradients at once from
    the scene's own stash and leaves the reservation alone, so the render's backward still starts at the chain.  The weight-gradient
    reduction has a fixed order and a two-term fp32 sum does not depend on its order: every gradient equals, bit for bit, the
    sum of the two backwards run alone on fresh identical nets."""
    net, tgt, lat = reservation_net(lat_grad)
    l_render = render_loss(net, tgt)             # stashes into the reservation it made
    l_query = query_loss(net)
    l_query.backward()                           # not the reservation's owner
    l_render.backward()
    torch.cuda.synchronize()
    assert net.last_backward_stats()["flops"][0] == 0.0      # the render's backward recomputed nothing
    alone = []
    for loss in (lambda n_, t_: render_loss(n_, t_), lambda n_, t_: query_loss(n_)):
        other, tgt2, lat2 = reservation_net(lat_grad)
        loss(other, tgt2).backward()
        torch.cuda.synchronize()
        assert lat2 is None or bool(torch.isfinite(lat2.grad).all())
        alone.append({k: p.grad for k, p in other.trainable_mlp_parameters()})
    named = net.trainable_mlp_parameters()
    assert len(named) > 0 and set(alone[0]) == set(alone[1]) == {k for k, _ in named}
    for k, p in named:
        assert torch.equal(p.grad, alone[0][k] + alone[1][k]), k
    if lat_grad:
        assert net.last_latent_grad_deterministic() and bool(torch.isfinite(lat.grad).all())
