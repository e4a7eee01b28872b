"""
lin_out of the two-plane f16 MLP kernels as a split-K product on the matrix cores (-m gpu; csrc/mlp_h2.hip h2linout_product /
h2linout_reduce, the PACK_H2O image of csrc/pack.hip): wave w multiplies the lin_out fragments of its own 64
(or 2 x 64) features with the planes it has just written, one partial per 64-k chunk goes to the wave's own plane rows, and
behind one barrier the eight chunks are added in chunk order, + b_out, the output head, the store.  What can go wrong is a
mapping -- k-step <-> wave, output row <-> accumulator quad <-> partial slot, chunk <-> wave on the 32-sample shape, the zero
rows of the padded n-tile, the second n-tile for d_out > 32 --, an ordering (planes read before the wave wrote them, partials
over rows still to be read, readers behind the next tile's prologue), the store guard of a ragged tile, or an image that does
not follow the weights.

Reference: the oracle in float64 on the same points.  Bar: the project's absolute 1e-4 of the f16x2 routes (TOL of
test_gpu_parity.py); the split arithmetic measures 1.7e-6 against float64 at K = 512 (csrc/mlp_h2.hip header), and the
sibling files (test_gpu_wave_gather.py, test_gpu_view_mean.py) 2e-6 .. 4e-6 for the whole MLP.  Every output depends on all 512
features of h through lin_out, so a permuted k-step, chunk, sample or output row is an O(1) error.

(n_blocks, combine_layer) = (3, 3) has no post-mean block, lin_out follows the view mean's fc_1 directly; it runs with one view
only: with combine_layer >= n_blocks the reference never averages the views (resnetfc.py:166-170), and a multi-view scene has
no meaning there (test_gpu_model_desc.py asserts the same of its table).  Geometry of test_gpu_model_desc.py: latent 8 x 8,
frame 32 x 40, points uniform in [-0.5, 0.5]^3, YOLO mode with the scene at z < 0 and raw outputs of O(1).
"""
import os

import numpy as np
import pytest
import torch

import pnyolo_oracle as orc
from helpers import dt, scene_pair
from pixel_nerf_yolo_amd.optim import Adam
from test_gpu_parity import TOL
from test_gpu_view_mean import ROUTES, run

pytestmark = pytest.mark.gpu

F64 = torch.float64
BAR = 1e-4
H, W = 32, 40
LAT_HW = (8, 8)
L = 256
OUT_GAIN = 0.05
BOX = 0.5
# a single sample; one short of, exactly and one over a 64-sample tile (two and three 32-sample tiles); two tiles and a ragged third
N_POINTS = (1, 63, 64, 65, 130)
N = max(N_POINTS)
# (n_blocks, combine_layer, views): (6, 5) is the largest LDS bias table
SHAPES = ((5, 3, 1), (5, 3, 2), (5, 3, 3), (3, 3, 1), (6, 5, 1), (6, 5, 2), (6, 5, 3))
# (d_out, YOLO mode): 4 = the NeRF head and the 16-byte store; 7 and 35 = one and two padded n-tiles, output quads that end
# inside a quad, output_head's YOLO branch
HEADS = ((4, False), (7, True), (35, True))
H2_ROUTES = ROUTES[:2]          # the 64-sample shape and the 32-sample shape (PNYOLO_H2_SPLIT=1)
H1_ROUTE = ROUTES[2]
GOLDEN_H1 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lin_out_h1.npz")


def test_the_bar_is_the_projects():
    assert TOL == BAR and [r[0] for r in H2_ROUTES] == ["h2", "h2s"] and H1_ROUTE[0] == "h1"


def build(monkeypatch, nb, cl, ns, d_out, yolo, seed=9100):
    monkeypatch.setenv("PNYOLO_PROJECTION", "on")
    monkeypatch.setenv("PNYOLO_MLP_PRECISION", "f16x2")
    for var in ("PNYOLO_GRID", "PNYOLO_BWD_PRECISION"):
        monkeypatch.delenv(var, raising=False)
    net, sc = scene_pair(ns, H, W, L, d_out, nb, cl, seed, yolo=yolo, lat_hw=LAT_HW, dtype=F64, yolo_flip=False,
                         out_gain=OUT_GAIN if yolo else 1.0)
    return net.eval(), sc


def points(n=N):
    rs = np.random.RandomState(5151)
    xyz = rs.uniform(-BOX, BOX, size=(n, 3)).astype(np.float32)
    vd = rs.standard_normal((n, 3)).astype(np.float32)
    vd /= np.linalg.norm(vd, axis=1, keepdims=True)
    return xyz, vd


def fp64(sc, xyz, vd):
    with torch.no_grad():
        ref = orc.query(sc, xyz, vd, coarse=True).to(F64)
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 1e-2
    return ref


def stash_forward(net, monkeypatch, xyz, vd):
    """The training forward (the STASH instantiation) on the 64-sample shape: a query with gradients, and its backward."""
    monkeypatch.delenv("PNYOLO_H2_SPLIT", raising=False)
    net.train()
    net.set_matrix_precision("f16x2")
    out = net(dt(xyz)[None], coarse=True, viewdirs=dt(vd)[None])
    out.sum().backward()
    torch.cuda.synchronize()
    assert net.last_launch_precision() == "f16x2" and net.last_mlp_stats(full=True)["projected"]
    for p in net.parameters():
        p.grad = None
    net.eval()
    return out[0].detach().clone()


@pytest.mark.parametrize("d_out,yolo", HEADS)
@pytest.mark.parametrize("nb,cl,ns", SHAPES)
def test_lin_out_against_fp64(monkeypatch, nb, cl, ns, d_out, yolo):
    """Both shapes at every point count and the training forward against float64; and without a bar: the shapes agree bit for
    bit, a run repeats, and the first n points rendered as a batch of n equal the same points inside the batch of 130 (n = 1: a
    point rendered alone), and the last point of the ragged tile rendered alone equals itself inside the batch."""
    net, sc = build(monkeypatch, nb, cl, ns, d_out, yolo)
    xyz, vd = points()
    ref = fp64(sc, xyz, vd)
    assert tuple(ref.shape) == (N, d_out)
    tag = "lin_out (%d, %d) NS=%d d_out=%d" % (nb, cl, ns, d_out)
    failed, full = [], {}
    for route in H2_ROUTES:
        for n in sorted(N_POINTS, reverse=True):
            out = run(net, monkeypatch, route, xyz[:n], vd[:n])
            assert tuple(out.shape) == (n, d_out)
            err = float((out.cpu().to(F64) - ref[:n]).abs().max())
            print("%s n=%d %s: max |err| vs float64 %.3e (bar %.1e)" % (tag, n, route[0], err, BAR))
            if not err < BAR:
                failed.append((route[0], n, err))
            if n == N:
                full[route[0]] = out
                assert torch.equal(run(net, monkeypatch, route, xyz, vd), out), route[0]
            else:
                assert torch.equal(out, full[route[0]][:n]), (route[0], n)
    assert torch.equal(full["h2"], full["h2s"])
    for route in H2_ROUTES:          # the last point of the ragged tile, rendered alone: sample 0 of a tile instead of sample 1
        alone = run(net, monkeypatch, route, xyz[N - 1:], vd[N - 1:])
        assert torch.equal(alone[0], full[route[0]][N - 1]), route[0]
    out = stash_forward(net, monkeypatch, xyz, vd)
    err = float((out.cpu().to(F64) - ref).abs().max())
    print("%s n=%d training forward: max |err| vs float64 %.3e (bar %.1e)" % (tag, N, err, BAR))
    if not err < BAR:
        failed.append(("stash", N, err))
    assert not failed, failed


def test_several_tiles_per_workgroup(monkeypatch):
    """PNYOLO_GRID=1: one workgroup walks every tile, so the partials of a tile lie in the rows the next tile's prologue and
    planes overwrite; bit-equal to the uncapped launch."""
    net, _ = build(monkeypatch, 5, 3, 3, 4, False)
    xyz, vd = points()
    for route in H2_ROUTES:
        monkeypatch.delenv("PNYOLO_GRID", raising=False)
        free = run(net, monkeypatch, route, xyz, vd)
        monkeypatch.setenv("PNYOLO_GRID", "1")
        assert torch.equal(run(net, monkeypatch, route, xyz, vd), free), route[0]


@pytest.mark.parametrize("d_out,yolo", [(4, False), (35, True)])
def test_image_follows_the_weights(monkeypatch, d_out, yolo):
    """One step of the one-launch Adam on lin_out alone (its chained pny_model_refresh repacks the images), then on every MLP
    tensor: the outputs match float64 of the stepped weights -- and are far from float64 of the weights before, so a lin_out
    image that had stayed behind would miss the bar."""
    net, sc = build(monkeypatch, 5, 3, 2, d_out, yolo)
    xyz, vd = points()
    old = fp64(sc, xyz, vd)
    params = dict(net.mlp_coarse.named_parameters())
    opt = Adam(list(params.values()), lr=2e-3, model=net)
    gen = torch.Generator(device="cpu").manual_seed(77)
    for stepped in (("lin_out.weight", "lin_out.bias"), tuple(params)):
        run(net, monkeypatch, H2_ROUTES[0], xyz, vd)
        for k, p in params.items():
            p.grad = torch.randn(p.shape, generator=gen).to(p.device) if k in stepped else None
        opt.step()
        torch.cuda.synchronize()
        sc.mlp_coarse = {k: v.detach().cpu().to(F64) for k, v in net.mlp_coarse.state_dict().items()}
        ref = fp64(sc, xyz, vd)
        moved = float((ref - old).abs().max())
        assert moved > 100 * BAR, moved
        for route in H2_ROUTES:
            err = float((run(net, monkeypatch, route, xyz, vd).cpu().to(F64) - ref).abs().max())
            print("lin_out d_out=%d after a step of %d tensors, %s: max |err| vs float64 %.3e (bar %.1e; the step moved the outputs by %.2e)"
                  % (d_out, len(stepped), route[0], err, BAR, moved))
            assert err < BAR, (route[0], err)
        old = ref


def h1_output(monkeypatch):
    """The single-plane route's case: (5, 3), three views, d_out = 4, 130 points."""
    net, _ = build(monkeypatch, 5, 3, 3, 4, False)
    xyz, vd = points()
    return run(net, monkeypatch, H1_ROUTE, xyz, vd).cpu()


def test_single_plane_route_keeps_its_bits(monkeypatch):
    """The single-plane kernel keeps the fp32 lin_out on w_out as stored: its output equals, bit for bit, the one recorded from
    the build before the split-K product (tests/golden/lin_out_h1.npz)."""
    with np.load(GOLDEN_H1) as f:
        want = torch.from_numpy(f["out"])
    got = h1_output(monkeypatch)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert torch.equal(got, want), float((got - want).abs().max())
