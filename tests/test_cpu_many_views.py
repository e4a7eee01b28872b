"""
The inputs of the many-view GPU tests (tests/test_gpu_many_views.py, MANY_VIEW_CASES of tests/test_gpu_grad_shapes.py), checked
on the oracle alone: these are conditions on the inputs, not measurements, and they are what makes a pass of those tests mean
something.  No GPU.
  * helpers.camera_ring(16): no two views share a camera, and every query point lies in front of every camera;
  * every case of MANY_VIEW_CASES selects its relu-safe points at both margins from a pool 4 x the need, with its edges;
  * the render-backward cases find their 16 relu-safe rays at 5 and at 8 views, most depth samples unclamped;
  * every view counts: with any ONE view's latent zeroed the float64 output of the 16-view scenes moves by more than 10 x the
    bar somewhere, so a kernel that drops or repeats a view cannot pass.
"""
import numpy as np
import pytest
import torch

import pnyolo_oracle as orc
import test_gpu_grad_shapes as gs
import test_gpu_many_views as mv
from helpers import camera_ring
from test_gpu_parity import TOL

F64 = torch.float64


def test_camera_ring_views_are_distinct():
    src, tgt = camera_ring(16)
    assert src.shape == (16, 4, 4) and src.dtype == np.float32 and tgt.shape == (4, 4)
    for i in range(16):
        for j in range(i + 1, 16):
            assert np.linalg.norm(src[i, :3, 3] - src[j, :3, 3]) > 0.05, (i, j)       # camera centres
            assert np.abs(src[i, :3, :3] - src[j, :3, :3]).max() > 0.05, (i, j)      # rotations
        assert np.linalg.norm(tgt[:3, 3] - src[i, :3, 3]) > 0.05, i
    for ns in (5, 7, 8, 11):      # a shorter ring is the head of the long one
        assert np.array_equal(camera_ring(ns)[0], src[:ns])


def test_query_points_lie_in_front_of_every_camera():
    _, sc = mv.query_scene(16, 2, 1, with_net=False)
    xyz, _ = mv.query_points()
    taps, z = gs.projection(sc, xyz)
    assert z.shape == (16, max(mv.N_POINTS)) and bool((z < -0.5).all())
    corners = np.array([[x, y, zz] for x in (-0.3, 0.3) for y in (-0.3, 0.3) for zz in (-0.3, 0.3)], dtype=np.float32)
    assert bool((gs.projection(sc, corners)[1] < -0.5).all())       # the whole cube the points are drawn from
    assert bool((taps == 4).any(dim=1).all())                       # every view sees some of the points whole


@pytest.mark.parametrize("ambig", [gs.AMBIG, gs.AMBIG_DEFAULT])
@pytest.mark.parametrize("name", list(gs.MANY_VIEW_CASES))
def test_many_view_cases_select_their_points(name, ambig):
    case = gs.MANY_VIEW_CASES[name]
    assert gs.pool_of(case) == 4.0 and gs.seed_of(name) >= gs.MANY_VIEW_SEED
    r = gs.reference(name, case, ambig)          # pick_points and assert_edges, then the float64 forward and backward
    assert r["xyz"].shape == (case["n"], 3) and r["ref"].dtype == F64
    assert r["lat"] is not None and r["lat"].shape[0] == case["ns"]
    for v in range(case["ns"]):                  # every view's map takes a gradient
        assert float(r["lat"][v].abs().max()) > 0, v


def test_existing_cases_keep_their_seeds_and_pool():
    assert [gs.seed_of(n) for n in sorted(gs.CASES)] == [3000 + 17 * i for i in range(len(gs.CASES))]
    assert all(gs.pool_of(c) == 1.6 and gs.poses_of(c) is None for c in gs.CASES.values())


@pytest.mark.parametrize("ns", mv.RENDER_VIEWS)
def test_render_cases_find_their_rays(ns):
    r = mv.render_reference(ns)                  # clean_rays; asserts that most depth samples are unclamped
    assert r["rays"].shape == (mv.RENDER["n"], 8) and r["lat"].shape[0] == ns
    for v in range(ns):
        assert float(r["lat"][v].abs().max()) > 0, v


@pytest.mark.parametrize("nb,cl", [(5, 3), (2, 1), (6, 5)])
def test_every_view_counts_at_16_views(nb, cl):
    _, sc = mv.query_scene(16, nb, cl, with_net=False)
    xyz, vd = mv.query_points()
    full = sc.latent
    with torch.no_grad():
        ref = orc.query(sc, xyz, vd, coarse=True)
        for v in range(16):
            lat = full.clone()
            lat[v] = 0
            sc.latent = lat
            for n in mv.N_POINTS:
                moved = float((orc.query(sc, xyz[:n], vd[:n], coarse=True) - ref[:n]).abs().max())
                assert moved > 10 * TOL, "view %d of (%d, %d), %d points: the output moves by %.2e only" % (v, nb, cl, n, moved)
    sc.latent = full
