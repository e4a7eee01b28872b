"""
The losses of all mini-batches of a YOLO training step in one launch (csrc/loss.hip yolo_loss_batches_kernel,
pny_yolo_loss_batches, loss.YoloLoss.forward_batches) on the GPU:
  * every mini-batch's terms, counts and gradient rows bit-equal to pny_yolo_loss on that slice with that scale's anchors,
    and within the project's bars of the fp64 restatement of the trainer's loop (tests/loss_batches_ref.py);
  * the step values bit-equal to the host's fp64 sum of the fp32 terms in mini-batch order;
  * mini-batches without an object cell, with every target ignored, with a class outside [0, C);
  * bit reproducibility, no hidden waiting, autograd behaviour, util.yolo_train_batch(flat=True);
  * one training step both ways: the trainer's loop on the per-mini-batch API against one render, one loss, one backward.
The project's bars (tests/test_gpu_loss.py): terms within 1e-4 absolute, gradients within 1e-4 of the tensor's max.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import loss_batches_ref
import loss_ref
from helpers import DEV, scene_pair
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd import loss as ploss
from pixel_nerf_yolo_amd import synth
from pixel_nerf_yolo_amd.render import YoloRenderer
from pixel_nerf_yolo_amd.util import FiniteMonitor, stage_yolo_targets, yolo_train_batch

pytestmark = pytest.mark.gpu

T_ABS, G_REL = 1e-4, 1e-4
WEIGHTS = (1.0, 20.0, 1.0, 1.0)
# (rows per scale, ray_batch_size, A, C)
CASES = [((1,), 1, 3, 2), ((5,), 2, 3, 2), ((165,), 128, 3, 2), ((7, 3), 4, 3, 2), ((64, 16, 4, 1), 64, 3, 2), ((300,), 2, 3, 2),
         ((37,), 16, 1, 1), ((37,), 16, 3, 5), ((400,), 400, 3, 2)]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits_or_both_nan(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    return bool(((bits(a) == bits(b)) | (a.isnan() & b.isnan())).all())


def check_terms(got, want, tol=T_ABS, what="terms"):
    """NaN exactly where the yardstick has NaN; everything else within tol absolute."""
    got, want = got.detach().cpu().to(torch.float64).flatten(), torch.as_tensor(want).to(torch.float64).flatten()
    assert torch.equal(got.isnan(), want.isnan()), "%s: NaN pattern %s, expected %s" % (what, got.tolist(), want.tolist())
    ok = ~want.isnan()
    err = float((got[ok] - want[ok]).abs().max()) if bool(ok.any()) else 0.0
    assert err <= tol, "%s: max|err| %.2e > %.0e" % (what, err, tol)
    return err


def check_grad(got, want, rel=G_REL, what="gradient"):
    got, want = got.detach().cpu().to(torch.float64), torch.as_tensor(want).detach().cpu().to(torch.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.equal(got.isnan(), want.isnan()), what + ": NaN pattern differs"
    ok = ~want.isnan()
    if not bool(ok.any()):
        return 0.0
    scale = max(float(want[ok].abs().max()), 1e-30)
    err = float((got[ok] - want[ok]).abs().max()) / scale
    assert err <= rel, "%s: max|err| / max|gradient| %.2e > %.0e (max|gradient| %.3e)" % (what, err, rel, scale)
    return err


def yolo_inputs(rows, A, Cn, seed, f_obj=0.3, f_ign=0.1):
    """The value ranges of tests/golden/losses.npz (tools/make_loss_golden.py) for sum(rows) cells, and one (A, 2) set of
    anchors per scale -> pred (N, A, 5 + C), target (N, A, 6), anchors (S, A, 2), on the CPU."""
    rs = np.random.RandomState(seed)
    n = int(sum(rows))
    pred = np.empty((n, A, 5 + Cn), dtype=np.float32)
    pred[..., 0] = rs.uniform(1e-3, 1.0 - 1e-3, size=(n, A))
    pred[..., 1:3] = rs.randn(n, A, 2)
    pred[..., 3:5] = rs.uniform(-2.0, 2.0, size=(n, A, 2))
    pred[..., 5:] = rs.randn(n, A, Cn)
    target = np.empty((n, A, 6), dtype=np.float32)
    u = rs.rand(n, A)
    target[..., 0] = np.where(u < f_obj, 1.0, np.where(u < f_obj + f_ign, -1.0, 0.0))
    target[..., 1:3] = rs.uniform(0.0, 1.0, size=(n, A, 2))
    target[..., 3:5] = rs.uniform(0.02, 0.9, size=(n, A, 2))
    target[..., 5] = rs.randint(0, Cn, size=(n, A))
    anchors = rs.uniform(0.1, 0.6, size=(len(rows), A, 2)).astype(np.float32)
    return torch.from_numpy(pred), torch.from_numpy(target), torch.from_numpy(anchors)


def batches_abi(pred, target, anchors, rows, batch_rows, weights=WEIGHTS, want_grad=True):
    """pny_yolo_loss_batches -> (terms (M, 5), counts (M, 2), step (6,), d_pred | None) on the CPU; outputs pre-filled (every
    element must be overwritten), inputs checked bit-unchanged."""
    p, t, a = pred.to(DEV).contiguous(), target.to(DEV).contiguous(), anchors.to(DEV).contiguous()
    keep = (bits(p), bits(t), bits(a))
    A, row = p.shape[-2], p.shape[-1]
    b = plib.YoloBatchesDesc(len(rows), batch_rows, (C.c_int64 * 4)(*rows))
    L = plib.load()
    M = L.pny_yolo_loss_batches_count(C.byref(b))
    assert M == len(loss_batches_ref.segments(rows, batch_rows))
    terms = torch.full((M, 5), 7.0, device=DEV)
    counts = torch.full((M, 2), -1, device=DEV, dtype=torch.int32)
    step = torch.full((6,), 7.0, device=DEV)
    d = torch.full_like(p, 7.0) if want_grad else None
    desc = plib.YoloLossDesc(A, row - 5, *weights)
    plib.check(L.pny_yolo_loss_batches(C.byref(desc), C.byref(b), plib.ptr(p), plib.ptr(t), plib.ptr(a), plib.ptr(terms),
                                       C.c_void_p(counts.data_ptr()), plib.ptr(step), plib.ptr(d), plib.stream_of(DEV)))
    torch.cuda.synchronize()
    assert torch.equal(bits(p), keep[0]) and torch.equal(bits(t), keep[1]) and torch.equal(bits(a), keep[2]), "an input was modified"
    return terms.cpu(), counts.cpu(), step.cpu(), None if d is None else d.cpu()


def slice_abi(pred, target, anchors, weights=WEIGHTS):
    """pny_yolo_loss on one slice (n, A, row) with one scale's anchors (A, 2) -> (terms (5,), counts (2,), d_pred), on the CPU."""
    p, t, a = pred.to(DEV).contiguous(), target.to(DEV).contiguous(), anchors.to(DEV).contiguous()
    A, row = p.shape[-2], p.shape[-1]
    terms = torch.full((5,), 7.0, device=DEV)
    counts = torch.full((2,), -1, device=DEV, dtype=torch.int32)
    d = torch.full_like(p, 7.0)
    desc = plib.YoloLossDesc(A, row - 5, *weights)
    plib.check(plib.load().pny_yolo_loss(C.byref(desc), plib.ptr(p), plib.ptr(t), plib.ptr(a), p.shape[0], plib.ptr(terms),
                                         C.c_void_p(counts.data_ptr()), plib.ptr(d), plib.stream_of(DEV)))
    torch.cuda.synchronize()
    return terms.cpu(), counts.cpu(), d.cpu()


def host_step(terms_seg):
    """The host's fp64 sum of the fp32 rows in mini-batch order, divided by M for entries 1 .. 5, rounded to fp32."""
    return loss_batches_ref.step_values(terms_seg).to(torch.float32)


# --------------------------------------------------------------------------- slices equal the existing launch
@pytest.mark.parametrize("rows,batch_rows,A,Cn", CASES)
def test_every_mini_batch_equals_the_existing_launch_on_its_slice(rows, batch_rows, A, Cn):
    pred, target, anchors = yolo_inputs(rows, A, Cn, 6000 + 13 * sum(rows) + 5 * batch_rows + A + Cn)
    terms, counts, step, d = batches_abi(pred, target, anchors, rows, batch_rows)
    want_t, want_c, want_g, _ = loss_batches_ref.yolo_batches(pred, target, anchors, WEIGHTS, rows, batch_rows)
    segs = loss_batches_ref.segments(rows, batch_rows)
    one_group = all(n * A <= 1024 for _, _, n in segs)        # LOSS_YOLO_PER_GROUP: the existing launch is one workgroup
    assert one_group == (rows != (400,)), "only the 400-row mini-batch is one the existing launch would split"
    if len(rows) > 1:
        assert not torch.equal(anchors[0], anchors[1])
    for m, (s, r0, n) in enumerate(segs):
        t1, c1, d1 = slice_abi(pred[r0:r0 + n], target[r0:r0 + n], anchors[s])
        assert torch.equal(counts[m], c1) and torch.equal(bits(d[r0:r0 + n]), bits(d1)), "mini-batch %d (scale %d, rows %d + %d)" % (m, s, r0, n)
        if one_group:
            assert torch.equal(bits(terms[m]), bits(t1)), "mini-batch %d: terms %s, the slice's %s" % (m, terms[m].tolist(), t1.tolist())
    assert torch.equal(counts.to(torch.int64), want_c)
    e_t = check_terms(terms, want_t)
    e_g = check_grad(d, want_g)
    # the step values: bit-equal to the host's sum of what the kernel stored
    want_step = host_step(terms)
    assert same_bits_or_both_nan(step, want_step), "step %s, the host's sum %s" % (step.tolist(), want_step.tolist())
    assert torch.equal(step.isnan(), want_step.isnan())
    print("rows %s B %d A %d C %d: M %d, terms max|err| %.2e, gradient err / max %.2e, step %s"
          % (rows, batch_rows, A, Cn, len(segs), e_t, e_g, step.tolist()))
    # without a gradient buffer and without counts: the same terms
    t2, _, s2, _ = batches_abi(pred, target, anchors, rows, batch_rows, want_grad=False)
    assert same_bits_or_both_nan(t2, terms) and same_bits_or_both_nan(s2, step)


# --------------------------------------------------------------------------- edge mini-batches
@pytest.mark.parametrize("kind", ["no_object", "all_ignored", "class_out_of_range"])
def test_edge_mini_batches(kind):
    """One of five mini-batches of 8 rows is made an edge case; NaN appears exactly where the restatement has it, and the other
    mini-batches' terms and gradient rows are the bits of a run on the untouched inputs."""
    rows, B, A, Cn, bad = (40,), 8, 3, 3, 2
    weights = (2.0, 20.0, 3.0, 4.0)
    pred, target, anchors = yolo_inputs(rows, A, Cn, 6100)
    clean = batches_abi(pred, target, anchors, rows, B, weights)
    assert bool((clean[1] > 0).all()) and bool(clean[0].isfinite().all()) and bool(clean[2].isfinite().all())
    lo, hi = bad * B, (bad + 1) * B
    edge, valid = target.clone(), None
    if kind == "no_object":
        edge[lo:hi, :, 0] = torch.where(edge[lo:hi, :, 0] == 1, torch.zeros(()), edge[lo:hi, :, 0])
    elif kind == "all_ignored":
        edge[lo:hi, :, 0] = -1.0
    else:
        cells = (edge[lo:hi, :, 0] == 1).nonzero()
        cells = cells[[0, len(cells) - 1]]
        valid = edge.clone()
        for (r, an), v in zip(cells.tolist(), (float(Cn), -1.0)):
            edge[lo + r, an, 5] = v
            valid[lo + r, an, 5] = 0.0
    terms, counts, step, d = batches_abi(pred, edge, anchors, rows, B, weights)
    want_t, want_c, want_g, _ = loss_batches_ref.yolo_batches(pred, edge if valid is None else valid, anchors, weights, rows, B)
    if kind == "no_object":
        assert counts[bad, 0] == 0 and terms[bad, [1, 2, 4]].tolist() == [0.0, 0.0, 0.0], "the three object terms must be exactly 0"
        assert abs(float(terms[bad, 0]) - 3.0 * float(terms[bad, 3])) <= 1e-6 * float(terms[bad, 0]), "total = w_noobj * no_object"
        assert bool(terms.isfinite().all()) and bool(step.isfinite().all()) and bool(d.isfinite().all())
    elif kind == "all_ignored":
        assert counts[bad].tolist() == [0, 0] and bool(terms[bad, 0].isnan()) and bool(terms[bad, 3].isnan())
        assert terms[bad, [1, 2, 4]].tolist() == [0.0, 0.0, 0.0] and not bool(d[lo:hi].any()), "ignored anchors receive a zero gradient"
    else:
        want_t, want_g = want_t.clone(), want_g.clone()
        want_t[bad, 0] = want_t[bad, 4] = float("nan")
        for r, an in cells.tolist():
            want_g[lo + r, an, 5:] = float("nan")
    assert torch.equal(counts.to(torch.int64), want_c)
    check_terms(terms, want_t)
    check_grad(d, want_g)
    # NaN in the step values exactly where the trainer's sums of the restatement's terms have it
    want_step = loss_batches_ref.step_values(want_t)
    assert torch.equal(step.isnan(), want_step.isnan()), (step.tolist(), want_step.tolist())
    assert kind == "no_object" or (bool(step[0].isnan()) and bool(step[1].isnan()) and int(step.isnan().sum()) == 3)
    assert same_bits_or_both_nan(step, host_step(terms))
    check_terms(step, want_step, tol=T_ABS * 5, what="step values (sums of 5 terms)")
    others = [m for m in range(5) if m != bad]
    keep_rows = torch.cat([torch.arange(m * B, (m + 1) * B) for m in others])
    assert torch.equal(bits(terms[others]), bits(clean[0][others])) and torch.equal(counts[others], clean[1][others])
    assert torch.equal(bits(d[keep_rows]), bits(clean[3][keep_rows]))


# --------------------------------------------------------------------------- reproducibility, no hidden waiting
def test_same_inputs_give_the_same_bits():
    for rows, B in (((165,), 128), ((300,), 2), ((64, 16, 4, 1), 64)):
        pred, target, anchors = yolo_inputs(rows, 3, 2, 6200 + sum(rows))
        a, b = batches_abi(pred, target, anchors, rows, B), batches_abi(pred, target, anchors, rows, B)
        assert all(same_bits_or_both_nan(x.float(), y.float()) for x, y in zip(a, b))
        assert torch.equal(a[1], b[1])


def test_forward_batches_does_not_wait_for_its_stream():
    """A queue of large matrix products is enqueued first; forward_batches and its backward must come back with that stream
    still busy -- stream.query(), no timing threshold -- and give the bits of an undisturbed call."""
    rows, B = (128, 32, 8), 48
    pred, target, anchors = (x.to(DEV) for x in yolo_inputs(rows, 3, 2, 6300))
    crit = ploss.YoloLoss(3, *WEIGHTS)

    def call():
        p = pred.clone().requires_grad_()
        loss_sum, step = crit.forward_batches(p, target, anchors, rows, B)
        loss_sum.backward()
        return step, p.grad, crit.batch_terms, crit.batch_counts.float()

    quiet = call()                                        # (also loads the kernel and allocates the stream's workspace)
    torch.cuda.synchronize()
    m = torch.randn(8192, 8192, device=DEV)
    out = torch.empty_like(m)
    torch.mm(m, m, out=out)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(DEV)
    for _ in range(60):
        torch.mm(m, m, out=out)
    assert not stream.query(), "the queue of matrix products was too short to test anything"
    busy = call()
    still_busy = not stream.query()
    torch.cuda.synchronize()
    assert still_busy, "forward_batches or its backward waited for the stream"
    assert all(torch.equal(bits(q), bits(b)) for q, b in zip(quiet, busy))


# --------------------------------------------------------------------------- the Python module
def test_forward_batches_autograd_behaviour():
    rows, B = (7, 3), 4
    pred, target, anchors = yolo_inputs(rows, 3, 2, 6400)
    terms, counts, step, base = batches_abi(pred, target, anchors, rows, B)
    t, a = target.to(DEV), anchors.to(DEV)
    crit = ploss.YoloLoss(3, *WEIGHTS)
    p = pred.to(DEV).requires_grad_()
    keep = (bits(p), bits(t))
    loss_sum, step_terms = crit.forward_batches(p, t, a, rows, B)
    assert loss_sum.dim() == 0 and step_terms.shape == (6,) and loss_sum.data_ptr() == step_terms.data_ptr()
    assert loss_sum.requires_grad and not step_terms.requires_grad
    assert crit.batch_terms.shape == (3, 5) and crit.batch_counts.shape == (3, 2) and crit.batch_terms.device == p.device
    assert crit.batch_counts.dtype == torch.int32
    loss_sum.backward(retain_graph=True)
    assert torch.equal(bits(p.grad), bits(base)) and torch.equal(bits(step_terms), bits(step))
    assert torch.equal(bits(crit.batch_terms), bits(terms)) and torch.equal(crit.batch_counts.cpu(), counts)
    loss_sum.backward(retain_graph=True)                   # twice accumulates twice
    check_grad(p.grad, 2.0 * base, rel=1e-6)
    assert torch.equal(bits(p), keep[0]) and torch.equal(bits(t), keep[1]), "an input was modified"
    # a grad_output other than 1 scales the gradient
    p = pred.to(DEV).requires_grad_()
    (crit.forward_batches(p, t, a, rows, B)[0] * 3.0).backward()
    check_grad(p.grad, 3.0 * base, rel=1e-6)
    assert crit.saved_grad is not None
    # no gradient buffer without grad mode or without an input that requires grad; the same bits
    with torch.no_grad():
        quiet = crit.forward_batches(p, t, a, rows, B)
    assert crit.saved_grad is None and not quiet[0].requires_grad and torch.equal(bits(quiet[1]), bits(step))
    assert crit.forward_batches(pred.to(DEV), t, a, rows, B)[0].requires_grad is False and crit.saved_grad is None
    # the trainer's shapes: a leading 1 on pred and target, the anchors as a list per scale; the gradient has pred's shape
    p4 = pred[None].to(DEV).requires_grad_()
    loss4, step4 = crit.forward_batches(p4, t[None], [a[0], a[1]], rows, B)
    loss4.backward()
    assert p4.grad.shape == p4.shape and torch.equal(bits(p4.grad[0]), bits(base)) and torch.equal(bits(step4), bits(step))
    # a non-contiguous pred is made contiguous and left unchanged
    wide = torch.zeros(10, 3, 12, device=DEV)
    wide[..., 2:9] = pred.to(DEV)
    pv = wide[..., 2:9].detach().requires_grad_()
    assert not pv.is_contiguous()
    crit.forward_batches(pv, t, a, rows, B)[0].backward()
    assert torch.equal(bits(pv.grad), bits(base)) and torch.equal(bits(wide[..., 2:9]), bits(pred))
    # shape errors name the argument
    p = pred.to(DEV)
    for args, name in (((p, t, a, (7, 4), B), "rows_per_scale"), ((p, t, a, (10,), B), "anchors"), ((p, t[:9], a, rows, B), "target"),
                       ((p[:, :2], t, a, rows, B), "pred"), ((p, t, a[:, :2], rows, B), "anchors"), ((p, t, a, (), B), "rows_per_scale"),
                       ((p[None, None], t, a, rows, B), "pred")):
        with pytest.raises(ValueError, match=name):
            crit.forward_batches(*args)
    with pytest.raises(plib.PnyError, match="batch_rows"):
        crit.forward_batches(p, t, a, rows, 0)
    with pytest.raises(plib.PnyError, match="fp32"):
        crit.forward_batches(p.double(), t, a, rows, B)


# --------------------------------------------------------------------------- the flat batch and the step, both ways
def step_scene(seed):
    """3 views of an 8 x 8 image, cells 1, 2, 4, the selected views 2 and 0: rows (128, 32, 8)."""
    H = W = 8
    cells, views = [1, 2, 4], torch.tensor([2, 0])
    flipyz = np.diag([1.0, -1.0, -1.0, 1.0])
    poses = torch.from_numpy(np.stack([np.linalg.inv(synth.pose_spherical(100.0 + 20.0 * v, -25.0, 4.0).astype(np.float64) @ flipyz)
                                       for v in range(3)]).astype(np.float32))
    focal, c = torch.tensor([2.5, 2.75]), torch.tensor([4.0, 4.0])
    rs = np.random.RandomState(seed)
    A, nested = 3, []
    for v in range(3):                     # dataset-like values: 25 % object, 10 % ignored
        per_scale = []
        for cell in cells:
            shape = (1, H // cell, W // cell, A)
            t = np.empty(shape + (6,), dtype=np.float32)
            u = rs.rand(*shape)
            t[..., 0] = np.where(u < 0.25, 1.0, np.where(u < 0.35, -1.0, 0.0))
            t[..., 1:3] = rs.uniform(0.0, 1.0, size=shape + (2,))
            t[..., 3:5] = rs.uniform(0.02, 0.9, size=shape + (2,))
            t[..., 5] = rs.randint(0, 2, size=shape)
            per_scale.append(torch.from_numpy(t))
        nested.append(tuple(per_scale))
    grids = stage_yolo_targets(nested, DEV)
    return dict(poses=poses, views=views, focal=focal, c=c, grids=grids, H=H, W=W, cells=cells, z=(1.0, 6.0), A=A)


def test_yolo_train_batch_flat_returns_the_buffers_of_the_per_scale_views():
    k = step_scene(6500)
    args = (k["poses"], k["views"], k["focal"], k["c"], k["grids"], k["H"], k["W"], k["cells"]) + k["z"]
    rays, targets, rows = yolo_train_batch(*args, flat=True)
    lists = yolo_train_batch(*args)
    assert rows == [128, 32, 8] and rays.shape == (168, 8) and targets.shape == (168, k["A"], 6)
    assert rays._base is None and targets._base is None and rays.is_contiguous() and targets.is_contiguous()
    assert len(lists) == 2 and [r.shape[0] for r in lists[0]] == rows
    off = 0
    for s, n in enumerate(rows):
        # the per-scale views of the default call are slices of buffers of this very shape, at these offsets
        assert lists[0][s]._base.shape == rays.shape and lists[1][s]._base.shape == targets.shape
        assert lists[0][s].data_ptr() == lists[0][0]._base.data_ptr() + off * 8 * 4
        assert lists[1][s].data_ptr() == lists[1][0]._base.data_ptr() + off * k["A"] * 6 * 4
        assert rays[off:off + n].data_ptr() == rays.data_ptr() + off * 8 * 4
        assert torch.equal(bits(rays[off:off + n]), bits(lists[0][s])) and torch.equal(bits(targets[off:off + n]), bits(lists[1][s]))
        off += n
    assert torch.equal(bits(rays), bits(lists[0][0]._base)) and torch.equal(bits(targets), bits(lists[1][0]._base))


@pytest.mark.parametrize("precision", ["auto", "f32"])
def test_one_pass_step_equals_the_trainers_loop(precision):
    """One training step of 168 rays in 5 mini-batches (48, 48, 32, 32, 8 rows over three scales), both ways on the same model,
    rays, targets and per-ray draws:
      A  the trainer's loop (YoloTrainer.py:149-208) on the per-mini-batch API: render, YoloLoss, backward(retain_graph=True);
      B  one render of all rays, forward_batches, one backward.
    Render and terms within 1e-4 absolute; every MLP parameter gradient and the latent's within 2e-4 of the tensor's max: each
    leg is held to 1e-4 against fp64 by the gradient tests (test_gpu_backward.py, test_gpu_loss.py), hence twice that between
    the two.  Measured on an MI355X: see DESIGN.md 4.4 item 16."""
    k = step_scene(6600)
    A, K, MB = k["A"], 16, 48
    net, _ = scene_pair(2, 64, 64, 1792, 7 * A, 5, 3, 6601, yolo=True, lat_hw=(8, 8), lat_grad=True)
    net.set_deterministic(True)
    net.set_matrix_precision(precision)
    ren = YoloRenderer(K, 128, len(k["cells"]), A)
    render_par = ren.bind_parallel(net)
    crit = ploss.YoloLoss(A, *WEIGHTS)
    rs = np.random.RandomState(6602)
    anchors = [torch.from_numpy(rs.uniform(0.1, 0.6, size=(A, 2)).astype(np.float32)).to(DEV) for _ in k["cells"]]
    args = (k["poses"], k["views"], k["focal"], k["c"], k["grids"], k["H"], k["W"], k["cells"]) + k["z"]
    rays, targets, rows = yolo_train_batch(*args, flat=True)
    rays_list, targets_list = yolo_train_batch(*args)
    assert rows == [128, 32, 8]
    u_all = rs.rand(sum(rows), K).astype(np.float32)                      # the renderer's draws, fixed per ray
    names = [n for n, p in net.named_parameters() if n.startswith("mlp_")]

    def grads():
        torch.cuda.synchronize()
        g = {n: p.grad.clone() for n, p in net.named_parameters() if n in names and p.grad is not None}
        g["latent"] = net.test_latent.grad.clone()
        return g

    def reset():
        net.zero_grad(set_to_none=True)
        net.test_latent.grad = None

    # A: the trainer's loop
    reset()
    renders, terms_a, totals, r0, mini_batch = [], [], [0.0] * 5, 0, 0
    for s, (rays_on_scale, bboxes_on_scale) in enumerate(zip(rays_list, targets_list)):
        for r, bboxes_gt in zip(torch.split(rays_on_scale.unsqueeze(0), MB, dim=1), torch.split(bboxes_on_scale.unsqueeze(0), MB, dim=1)):
            mini_batch += 1
            n = r.shape[1]
            ren.draws = dict(u_coarse=u_all[r0:r0 + n])
            r0 += n
            render = render_par(r.to(DEV)).reshape(1, n, A, 7)
            out = crit(render, bboxes_gt, anchors[s])
            out[0].backward(retain_graph=True)
            for j, o in enumerate(out):
                totals[j] += o.item()
            renders.append(render.detach()[0].clone())
            terms_a.append(torch.stack([o.detach() for o in out]).cpu())
    logged_a = [t / mini_batch for t in totals]
    g_a, render_a, terms_a = grads(), torch.cat(renders), torch.stack(terms_a)
    # B: one render, one loss, one backward
    reset()
    ren.draws = dict(u_coarse=u_all)
    render = render_par(rays[None]).reshape(1, sum(rows), A, 7)
    loss_sum, step_terms = crit.forward_batches(render, targets[None], anchors, rows, MB)
    loss_sum.backward()
    g_b = grads()
    step = step_terms.tolist()
    counts = crit.batch_counts.cpu()
    assert mini_batch == 5 and crit.batch_terms.shape == (5, 5)
    assert bool((counts > 0).all()), "every mini-batch has an object and a no-object cell: %s" % counts.tolist()
    e_r = float((render.detach()[0] - render_a).abs().max())
    print("[%s] render: max |B - A| %.3e, bit-equal: %s" % (precision, e_r, torch.equal(bits(render[0]), bits(render_a))))
    e_t = float((crit.batch_terms.cpu() - terms_a).abs().max())
    e_l = max(abs(a - b) for a, b in zip(logged_a, step[1:]))
    e_s = abs(step[0] - totals[0])
    print("[%s] terms per mini-batch: max |B - A| %.3e; logged values %.3e; sum of totals %.3e (%s)" % (precision, e_t, e_l, e_s, step))
    assert set(g_a) == set(g_b) and len(g_a) >= 20
    worst = {}
    for n in g_a:
        scale = float(g_a[n].abs().max())
        worst[n] = float((g_b[n] - g_a[n]).abs().max()) / max(scale, 1e-30)
    assert float(g_a["latent"].abs().max()) > 0 and sum(float(g.abs().max()) > 0 for g in g_a.values()) >= 20
    w_mlp = max((v, n) for n, v in worst.items() if n != "latent")
    print("[%s] gradients: worst MLP tensor %.3e of its max (%s, %d tensors); latent %.3e of its max"
          % (precision, w_mlp[0], w_mlp[1], len(worst) - 1, worst["latent"]))
    assert e_r <= 1e-4, "render"
    assert e_t <= 1e-4 and e_l <= 1e-4, "terms"
    bad = {n: v for n, v in worst.items() if not v <= 2e-4}
    assert not bad, "gradients beyond 2e-4 of their max: %s" % bad
