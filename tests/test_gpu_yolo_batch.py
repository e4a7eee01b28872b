"""
The one-launch YOLO training batch on the GPU (include/pnyolo.h pny_yolo_train_batch, util.yolo_train_batch):
  * the three cases of tests/golden/yolo_train_batch.npz (the reference's own trainer lines, tools/make_yolo_batch_golden.py):
    targets bit-equal to the reference's, rays bit-equal to the rows of pny_gen_rays_range(yolo_mode = 1) called per scale with
    the fp32 focal / cell and c / cell, and within 1e-5 of the reference's rays -- the bar test_gen_rays_golden
    (tests/test_gpu_parity.py) sets for its gen_rays_yolo case; the per-scale results are views of two flat buffers;
  * repeated view ids give repeated blocks; 16 views x 4 scales, the documented limit;
  * one YOLO training step fed by the batch and watched by FiniteMonitor against the same step fed from util.gen_rays_yolo
    plus indexing: loss terms and every parameter gradient bit-identical, the report clean, and an Inf written into one
    bound gradient buffer named by it.
"""
import numpy as np
import pytest
import torch

import yolo_batch_ref as yb
from helpers import DEV, scene_pair
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd import loss as ploss
from pixel_nerf_yolo_amd import synth
from pixel_nerf_yolo_amd.render import YoloRenderer
from pixel_nerf_yolo_amd.util import FiniteMonitor, gen_rays_range, gen_rays_yolo, stage_yolo_targets, yolo_train_batch

pytestmark = pytest.mark.gpu

RAY_TOL = 1e-5     # tests/test_gpu_parity.py::test_gen_rays_golden, the gen_rays_yolo case


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def run_case(k, views=None, grids=None):
    views = k["views"] if views is None else views
    grids = [torch.from_numpy(t).to(DEV) for t in (k["grids"] if grids is None else grids)]
    return yolo_train_batch(torch.from_numpy(k["poses"]), views, k["focal"], k["c"], grids, k["H"], k["W"], k["cells"], *k["z"])


def own_rays(k, views):
    """pny_gen_rays_range(poses[view], 1, Ws, Hs, focal / cell, c / cell, yolo_mode = 1) per scale and selected view."""
    poses, focal, c = torch.from_numpy(k["poses"]), torch.from_numpy(k["focal"]), torch.from_numpy(k["c"])
    out = []
    for cell in k["cells"]:
        hs, ws = k["H"] // cell, k["W"] // cell
        f, cc = focal / cell, c / cell                           # fp32 tensor divisions, as YoloTrainer.py:107-108
        assert f.dtype == torch.float32
        out.append(torch.cat([gen_rays_range(poses[int(v)][None], ws, hs, f, k["z"][0], k["z"][1], 0, hs * ws, c=cc, yolo=True, device=DEV)
                              for v in views]))
    return out


@pytest.mark.parametrize("case", yb.CASES)
def test_replay_of_the_reference_batches(golden, case):
    k = yb.fixture_case(golden("yolo_train_batch"), case)
    rays, targets = run_case(k)
    torch.cuda.synchronize()
    off = k["offsets"].tolist()
    assert len(rays) == len(targets) == len(k["cells"])
    own = own_rays(k, k["views"])
    for s in range(len(k["cells"])):
        n = off[s + 1] - off[s]
        assert rays[s].shape == (n, 8) and targets[s].shape == (n, k["A"], 6)
        assert torch.equal(bits(targets[s]), bits(torch.from_numpy(k["targets"][s]))), "scale %d: targets" % s
        assert torch.equal(bits(rays[s]), bits(own[s])), "scale %d: rays differ from pny_gen_rays_range" % s
        err = float((rays[s].cpu() - torch.from_numpy(k["rays"][s])).abs().max())
        print("%s scale %d: rays max |batch - reference| = %.3e" % (case, s, err))
        assert err < RAY_TOL
        # views of the two flat buffers, at the offsets expected
        assert rays[s].data_ptr() == rays[0].data_ptr() + off[s] * 8 * 4
        assert targets[s].data_ptr() == targets[0].data_ptr() + off[s] * k["A"] * 6 * 4
        assert rays[s]._base is rays[0]._base and targets[s]._base is targets[0]._base and rays[s]._base is not None
    assert rays[0]._base.shape == (off[-1], 8) and rays[0].data_ptr() % 16 == 0
    # the trainer's mini-batches are splits of the views
    parts = torch.split(rays[0].unsqueeze(0), 64, dim=1)
    assert sum(p.shape[1] for p in parts) == off[1] and parts[0].data_ptr() == rays[0].data_ptr()


def test_repeated_and_reordered_views(golden):
    k = yb.fixture_case(golden("yolo_train_batch"), "a")
    views = [2, 2, 4, 0, 2]
    rays, targets = run_case(k, views=views)
    want_t = yb.gather_targets(k["grids"], views)
    own = own_rays(k, views)
    for s, cell in enumerate(k["cells"]):
        per = (k["H"] // cell) * (k["W"] // cell)
        assert np.array_equal(targets[s].cpu().numpy(), want_t[s]) and torch.equal(bits(rays[s]), bits(own[s]))
        blocks_r, blocks_t = rays[s].reshape(len(views), per, 8), targets[s].reshape(len(views), per, -1)
        for i in (1, 4):                                         # the repeats of view 2 are repeats of its block
            assert torch.equal(bits(blocks_r[i]), bits(blocks_r[0])) and torch.equal(bits(blocks_t[i]), bits(blocks_t[0]))
        assert not torch.equal(bits(blocks_r[2]), bits(blocks_r[0]))
    # the single-view call is the first block of each scale
    r1, t1 = run_case(k, views=[2])
    for s in range(len(k["cells"])):
        assert torch.equal(bits(r1[s]), bits(rays[s][:r1[s].shape[0]])) and torch.equal(bits(t1[s]), bits(targets[s][:t1[s].shape[0]]))


def test_sixteen_views_and_four_scales():
    """The documented limit: NS = 16 selected views (of NV = 3, so with repeats) x 4 scales of an 8 x 8 image; one more is refused."""
    rs = np.random.RandomState(16)
    flipyz = np.diag([1.0, -1.0, -1.0, 1.0])
    poses = np.stack([np.linalg.inv(synth.pose_spherical(50.0 * v + 5.0, -25.0, 4.0).astype(np.float64) @ flipyz) for v in range(3)]).astype(np.float32)
    k = dict(NV=3, H=8, W=8, A=3, cells=[1, 2, 4, 8], poses=poses, focal=np.array([9.5, 10.25], dtype=np.float32),
             c=np.array([3.75, 4.5], dtype=np.float32), z=(1.0, 6.0), grids=yb.coded_grids(3, 8, 8, [1, 2, 4, 8], 3))
    views = rs.randint(0, 3, size=16).tolist()
    rays, targets = run_case(k, views=views)
    assert [r.shape[0] for r in rays] == [1024, 256, 64, 16]
    want_t, own = yb.gather_targets(k["grids"], views), own_rays(k, views)
    for s in range(4):
        assert np.array_equal(targets[s].cpu().numpy(), want_t[s]) and torch.equal(bits(rays[s]), bits(own[s]))
    with pytest.raises(plib.PnyError, match="n_views"):
        run_case(k, views=views + [0])


# --------------------------------------------------------------------------- through the trainer's loop
def realistic_grids(k, seed):
    """Target grids with the dataset's value ranges (obj in {1, 0, -1}, boxes, class index): the fixture's grids encode
    positions instead, which YoloLoss cannot digest."""
    rs = np.random.RandomState(seed)
    out = []
    for cell in k["cells"]:
        shape = (k["NV"], k["H"] // cell, k["W"] // cell, k["A"])
        t = np.empty(shape + (6,), dtype=np.float32)
        u = rs.rand(*shape)
        t[..., 0] = np.where(u < 0.25, 1.0, np.where(u < 0.35, -1.0, 0.0))
        t[..., 1:3] = rs.uniform(0.0, 1.0, size=shape + (2,))
        t[..., 3:5] = rs.uniform(0.02, 0.9, size=shape + (2,))
        t[..., 5] = rs.randint(0, 2, size=shape)
        out.append(t)
    return out


def test_training_step_fed_by_the_batch_equals_the_step_fed_by_gen_rays_yolo(golden):
    k = yb.fixture_case(golden("yolo_train_batch"), "a")
    A, K, MB = k["A"], 16, 64
    net, _ = scene_pair(2, 64, 64, 1792, 7 * A, 5, 3, 1900, yolo=True, lat_hw=(8, 8))
    net.set_deterministic(True)
    ren = YoloRenderer(K, 128, len(k["cells"]), A)
    ren.bind_parallel(net)
    crit = ploss.YoloLoss(A, 1.0, 20.0, 1.0, 1.0)
    rs = np.random.RandomState(1901)
    anchors = [torch.from_numpy(rs.uniform(0.1, 0.6, size=(A, 2)).astype(np.float32)).to(DEV) for _ in k["cells"]]
    u_all = rs.rand(int(k["offsets"][-1]), K).astype(np.float32)             # the renderer's draws, fixed per ray
    poses, views = torch.from_numpy(k["poses"]), torch.from_numpy(k["views"])
    focal, c = torch.from_numpy(k["focal"]), torch.from_numpy(k["c"])
    # the dataset's nested structure -> one device tensor per scale
    grids_np = realistic_grids(k, 1902)
    nested = [tuple(torch.from_numpy(g[v:v + 1].copy()) for g in grids_np) for v in range(k["NV"])]
    grids = stage_yolo_targets(nested, DEV)
    names = [n for n, _ in net.named_parameters()]
    params = [p for _, p in net.named_parameters()]
    mon = FiniteMonitor(("render", "targets", "grads"), DEV)
    mon.watch("grads", params, names, grads=True)

    def step(all_rays, all_targets, watch):
        net.zero_grad(set_to_none=True)
        terms, r0 = [], 0
        for s, (rays_on_scale, bboxes_on_scale) in enumerate(zip(all_rays, all_targets)):
            for rays, bboxes_gt in zip(torch.split(rays_on_scale.unsqueeze(0), MB, dim=1), torch.split(bboxes_on_scale.unsqueeze(0), MB, dim=1)):
                n = rays.shape[1]
                ren.draws = dict(u_coarse=u_all[r0:r0 + n])
                r0 += n
                render = ren(rays.to(DEV)).reshape(1, n, A, 7)
                out = crit(render, bboxes_gt, anchors[s])
                out[0].backward(retain_graph=True)
                if watch:
                    mon.check("render", render)
                    mon.check("targets", bboxes_gt)
                    mon.check("grads")
                terms.append(torch.stack([o.detach() for o in out]).clone())
        torch.cuda.synchronize()
        grads = {n: p.grad.clone() for n, p in zip(names, params) if p.grad is not None}
        return torch.stack(terms), grads

    # (a) the new front end
    rays_a, targets_a = yolo_train_batch(poses, views, focal, c, grids, k["H"], k["W"], k["cells"], *k["z"])
    # (b) YoloTrainer.py:93-129 on the existing API
    rays_b, targets_b = [], []
    for s, cell in enumerate(k["cells"]):
        hs, ws = k["H"] // cell, k["W"] // cell
        rays_b.append(gen_rays_yolo(poses[views], ws, hs, focal / cell, c / cell, *k["z"], device=DEV).reshape(-1, 8))
        targets_b.append(grids[s][views.to(DEV)].reshape(-1, A, 6))
    for s in range(len(k["cells"])):
        assert torch.equal(bits(rays_a[s]), bits(rays_b[s])) and torch.equal(bits(targets_a[s]), bits(targets_b[s]))
    mon.reset()
    t_a, g_a = step(rays_a, targets_a, watch=True)
    report = mon.report()
    t_b, g_b = step(rays_b, targets_b, watch=False)
    assert t_a.shape == (2 + 1 + 1, 5) and bool(t_a.isfinite().all()) and float(t_a[:, 0].min()) > 0
    assert torch.equal(bits(t_a), bits(t_b)), "loss terms differ"
    assert len(g_a) >= 20 and set(g_a) == set(g_b) and any(float(v.abs().max()) > 0 for v in g_a.values())
    bad = [n for n in g_a if not torch.equal(bits(g_a[n]), bits(g_b[n]))]
    assert not bad, "%d of %d gradients differ: %s" % (len(bad), len(g_a), bad[:5])
    assert report == {"render": (False, False, None), "targets": (False, False, None), "grads": (False, False, None)}
    # an Inf in one bound gradient buffer: the report names that parameter, and only the grads group
    victim = "mlp_coarse.blocks.2.fc_0.weight"
    assert victim in g_a
    dict(zip(names, params))[victim].grad.view(-1)[12345] = float("inf")
    mon.reset()
    mon.check("render", rays_a[0])
    mon.check("grads")
    assert mon.report() == {"render": (False, False, None), "targets": (False, False, None), "grads": (False, True, victim)}
    mon.close()
