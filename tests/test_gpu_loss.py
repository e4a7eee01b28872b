"""
The one-launch training losses (csrc/loss.hip, pixel_nerf_yolo_amd.loss) on the GPU:
  * golden replay: every case of tests/golden/losses.npz (the reference's own modules, tools/make_loss_golden.py) through the
    Python modules and through the raw ABI; inputs bit-unchanged afterwards;
  * shape sweep against the fp64 restatement (tests/loss_ref.py) at the smallest shapes where the kernels can go wrong: one
    item, around one wave, the trainer's mini-batch, more than one workgroup (the ticket path); the edge cases of the means,
    of BCELoss's clamp and of the class index;
  * bit reproducibility, autograd behaviour, the trainers' call sites, no hidden waiting.
The project's bars: terms within 1e-4 absolute, gradients within 1e-4 of the tensor's max |gradient|.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import loss_ref
from helpers import DEV, scene_pair
from pixel_nerf_yolo_amd import conf as pconf
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd import loss as ploss
from pixel_nerf_yolo_amd import synth
from pixel_nerf_yolo_amd.model import make_model
from pixel_nerf_yolo_amd.render import NeRFRenderer, YoloRenderer
from pixel_nerf_yolo_amd.util import sample_train_batch

pytestmark = pytest.mark.gpu

T_ABS, G_REL = 1e-4, 1e-4
YOLO_CASES = ("y128", "y37", "ynoobj", "ya1c1", "ya3c5")
RGB_CASES = ("mse_mse", "l1_mse", "coarse_only")
WEIGHTS = (1.0, 20.0, 1.0, 1.0)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def cf(l1):
    return pconf.Conf({"use_l1": bool(l1)})


def check_terms(got, want, tol=T_ABS, what="terms"):
    """NaN exactly where the yardstick has NaN; everything else within tol absolute."""
    got, want = got.detach().cpu().to(torch.float64).flatten(), torch.as_tensor(want).to(torch.float64).flatten()
    assert torch.equal(got.isnan(), want.isnan()), "%s: NaN pattern %s, expected %s" % (what, got.tolist(), want.tolist())
    ok = ~want.isnan()
    err = float((got[ok] - want[ok]).abs().max()) if bool(ok.any()) else 0.0
    assert err <= tol, "%s: %s, expected %s (max|err| %.2e > %.0e)" % (what, got.tolist(), want.tolist(), err, tol)
    return err


def check_grad(got, want, rel=G_REL, what="gradient"):
    got, want = got.detach().cpu().to(torch.float64), torch.as_tensor(want).to(torch.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.equal(got.isnan(), want.isnan()), what + ": NaN pattern differs"
    ok = ~want.isnan()
    if not bool(ok.any()):
        return 0.0
    scale = max(float(want[ok].abs().max()), 1e-30)
    err = float((got[ok] - want[ok]).abs().max()) / scale
    assert err <= rel, "%s: max|err| / max|gradient| %.2e > %.0e (max|gradient| %.3e)" % (what, err, rel, scale)
    return err


def yolo_inputs(cells, A, C, seed, f_obj=0.1, f_ign=0.1):
    """The value ranges of the fixture (tools/make_loss_golden.py)."""
    rs = np.random.RandomState(seed)
    pred = np.empty((1, cells, A, 5 + C), dtype=np.float32)
    pred[..., 0] = rs.uniform(1e-3, 1.0 - 1e-3, size=(1, cells, A))
    pred[..., 1:3] = rs.randn(1, cells, A, 2)
    pred[..., 3:5] = rs.uniform(-2.0, 2.0, size=(1, cells, A, 2))
    pred[..., 5:] = rs.randn(1, cells, A, C)
    target = np.empty((1, cells, A, 6), dtype=np.float32)
    u = rs.rand(1, cells, A)
    target[..., 0] = np.where(u < f_obj, 1.0, np.where(u < f_obj + f_ign, -1.0, 0.0))
    target[..., 1:3] = rs.uniform(0.0, 1.0, size=(1, cells, A, 2))
    target[..., 3:5] = rs.uniform(0.02, 0.9, size=(1, cells, A, 2))
    target[..., 5] = rs.randint(0, C, size=(1, cells, A))
    anchors = rs.uniform(0.1, 0.6, size=(A, 2)).astype(np.float32)
    return torch.from_numpy(pred), torch.from_numpy(target), torch.from_numpy(anchors)


def yolo_module(pred, target, anchors, weights=WEIGHTS):
    """Through pixel_nerf_yolo_amd.loss.YoloLoss -> (terms (5,), d total / d pred, counts), inputs checked bit-unchanged."""
    p, t, a = pred.to(DEV).requires_grad_(), target.to(DEV), anchors.to(DEV)
    keep = (bits(p), bits(t), bits(a))
    crit = ploss.YoloLoss(pred.shape[-2], *weights)
    out = crit(p, t, a)
    assert len(out) == 5 and all(o.dim() == 0 and o.device == p.device for o in out)
    assert crit.terms.shape == (5,) and all(o.data_ptr() == crit.terms.data_ptr() + 4 * i for i, o in enumerate(out)), \
        "the five values are views of one device tensor"
    out[0].backward()
    assert torch.equal(bits(p), keep[0]) and torch.equal(bits(t), keep[1]) and torch.equal(bits(a), keep[2]), "an input was modified"
    return torch.stack([o.detach() for o in out]).cpu(), p.grad.cpu(), crit.counts.cpu()


def yolo_abi(pred, target, anchors, weights=WEIGHTS, want_grad=True):
    p, t, a = pred.to(DEV).contiguous(), target.to(DEV).contiguous(), anchors.to(DEV).contiguous()
    keep = (bits(p), bits(t), bits(a))
    A, row = p.shape[-2], p.shape[-1]
    terms = torch.full((5,), 7.0, device=DEV)
    counts = torch.full((2,), -1, device=DEV, dtype=torch.int32)
    d = torch.full_like(p, 7.0) if want_grad else None     # (every element must be overwritten)
    desc = plib.YoloLossDesc(A, row - 5, *weights)
    plib.check(plib.load().pny_yolo_loss(C.byref(desc), plib.ptr(p), plib.ptr(t), plib.ptr(a), p.numel() // (A * row), plib.ptr(terms),
                                         C.c_void_p(counts.data_ptr()), plib.ptr(d), plib.stream_of(DEV)))
    torch.cuda.synchronize()
    assert torch.equal(bits(p), keep[0]) and torch.equal(bits(t), keep[1]) and torch.equal(bits(a), keep[2]), "an input was modified"
    return terms.cpu(), None if d is None else d.cpu(), counts.cpu()


def rgb_abi(coarse, fine, gt, l1, lam, want_grad=True):
    c, g = coarse.to(DEV).contiguous(), gt.to(DEV).contiguous()
    f = None if fine is None else fine.to(DEV).contiguous()
    keep = [bits(x) for x in (c, g)] + ([bits(f)] if f is not None else [])
    terms = torch.full((3,), 7.0, device=DEV)
    d_c = torch.full_like(c, 7.0) if want_grad else None
    d_f = torch.full_like(f, 7.0) if want_grad and f is not None else None
    desc = plib.RgbLossDesc(int(l1[0]), int(l1[1]), float(lam[0]), float(lam[1]))
    plib.check(plib.load().pny_rgb_loss(C.byref(desc), plib.ptr(c), plib.ptr(f), plib.ptr(g), c.numel(), plib.ptr(terms), plib.ptr(d_c),
                                        plib.ptr(d_f), plib.stream_of(DEV)))
    torch.cuda.synchronize()
    now = [bits(x) for x in (c, g)] + ([bits(f)] if f is not None else [])
    assert all(torch.equal(a, b) for a, b in zip(keep, now)), "an input was modified"
    return terms.cpu(), None if d_c is None else d_c.cpu(), None if d_f is None else d_f.cpu()


def rgb_module(coarse, fine, gt, l1, lam):
    c, g = coarse.to(DEV).requires_grad_(), gt.to(DEV)
    f = None if fine is None else fine.to(DEV).requires_grad_()
    crit = ploss.NerfLoss(cf(l1[0]), cf(l1[1]), float(lam[0]), float(lam[1]))
    loss, terms = crit(c, f, g)
    assert loss.dim() == 0 and terms.shape == (3,) and loss.data_ptr() == terms.data_ptr() + 8 and not terms.requires_grad
    loss.backward()
    return terms.detach().cpu(), c.grad.cpu(), None if f is None else f.grad.cpu()


# --------------------------------------------------------------------------- golden replay
@pytest.mark.parametrize("way", ["module", "abi"])
@pytest.mark.parametrize("name", YOLO_CASES)
def test_yolo_replay_of_the_reference(golden, name, way):
    g = golden("losses")
    pred, target, anchors = (torch.from_numpy(g["%s_%s" % (name, k)]) for k in ("pred", "target", "anchors"))
    terms, grad, counts = (yolo_module if way == "module" else yolo_abi)(pred, target, anchors, tuple(float(w) for w in g[name + "_weights"]))
    e_t = check_terms(terms, g[name + "_terms"])
    e_g = check_grad(grad, g[name + "_d_pred"])
    assert counts.tolist() == [int((target[..., 0] == 1).sum()), int((target[..., 0] == 0).sum())]
    if name == "ynoobj":
        assert terms[1] == 0 and terms[2] == 0 and terms[4] == 0 and float(terms[0]) == float(terms[3]) * float(g[name + "_weights"][2])
    print("%s (%s): terms max|err| %.2e, gradient err / max %.2e" % (name, way, e_t, e_g))


@pytest.mark.parametrize("way", ["module", "abi"])
@pytest.mark.parametrize("name", RGB_CASES)
def test_rgb_replay_of_the_reference(golden, name, way):
    g = golden("losses")
    coarse, gt = torch.from_numpy(g[name + "_coarse"]), torch.from_numpy(g[name + "_gt"])
    fine = torch.from_numpy(g[name + "_fine"]) if name + "_fine" in g else None
    l1, lam = g[name + "_use_l1"], g[name + "_lambdas"]
    terms, d_c, d_f = (rgb_module if way == "module" else rgb_abi)(coarse, fine, gt, l1, lam)
    e_t = check_terms(terms, g[name + "_terms"])
    e_c = check_grad(d_c, g[name + "_d_coarse"])
    e_f = check_grad(d_f, g[name + "_d_fine"]) if fine is not None else 0.0
    print("%s (%s): terms max|err| %.2e, gradient err / max %.2e, %.2e" % (name, way, e_t, e_c, e_f))
    if way == "module":   # the criteria of get_rgb_loss on their own, as the trainer's unchanged lines call them
        for x, use_l1, raw in ((coarse, l1[0], g[name + "_raw"][0]),) + (((fine, l1[1], g[name + "_raw"][1]),) if fine is not None else ()):
            crit = ploss.get_rgb_loss(cf(use_l1), True)
            xx = x.to(DEV).requires_grad_()
            v = crit(xx, gt.to(DEV))
            v.backward()
            assert v.dim() == 0 and abs(float(v.detach()) - float(raw)) <= T_ABS
            check_grad(xx.grad, loss_ref.rgb_with_grads(x, None, gt, use_l1_coarse=bool(use_l1))[1])


# --------------------------------------------------------------------------- shape sweep against the restatement
@pytest.mark.parametrize("A,C", [(1, 1), (1, 2), (1, 5), (3, 1), (3, 2), (3, 5)])
@pytest.mark.parametrize("cells", [1, 63, 64, 65, 384, 5000])
def test_yolo_sweep(cells, A, C):
    """1 item .. one wave +- 1 .. the trainer's 128 x 3 .. 5000 cells (more than one workgroup: the ticket path)."""
    pred, target, anchors = yolo_inputs(cells, A, C, 1000 + 7 * cells + 3 * A + C, f_obj=0.3 if cells < 100 else 0.05)
    want_t, want_g, n_obj, n_noobj = loss_ref.yolo_with_grads(pred, target, anchors, WEIGHTS)
    assert cells < 5000 or cells * A > 1024, "the largest size must take more than one workgroup (1024 items each)"
    terms, grad, counts = yolo_abi(pred, target, anchors)
    assert counts.tolist() == [n_obj, n_noobj]
    check_terms(terms, want_t)
    check_grad(grad, want_g)
    if cells in (1, 384):    # and through the module
        terms_m, grad_m, _ = yolo_module(pred, target, anchors)
        assert torch.equal(bits(terms_m), bits(terms)) and torch.equal(bits(grad_m), bits(grad))


def test_yolo_no_object_cell():
    pred, target, anchors = yolo_inputs(65, 3, 2, 2001, f_obj=0.0)
    want_t, want_g, n_obj, _ = loss_ref.yolo_with_grads(pred, target, anchors, (2.0, 20.0, 3.0, 4.0))
    terms, grad, counts = yolo_abi(pred, target, anchors, (2.0, 20.0, 3.0, 4.0))
    assert n_obj == 0 and counts[0] == 0
    assert float(terms[1]) == 0.0 and float(terms[2]) == 0.0 and float(terms[4]) == 0.0, "the three object terms must be exactly 0"
    assert abs(float(terms[0]) - 3.0 * float(terms[3])) <= 1e-6 * float(terms[0]), "total = w_noobj * no_object"
    check_terms(terms, want_t)
    check_grad(grad, want_g)


def test_yolo_no_no_object_cell():
    pred, target, anchors = yolo_inputs(65, 3, 2, 2002, f_obj=0.4, f_ign=0.6)
    target[..., 0] = torch.where(target[..., 0] == 0, torch.ones(()), target[..., 0])
    want_t, want_g, _, n_noobj = loss_ref.yolo_with_grads(pred, target, anchors, WEIGHTS)
    terms, grad, counts = yolo_abi(pred, target, anchors)
    assert n_noobj == 0 and counts[1] == 0
    assert bool(terms[0].isnan()) and bool(terms[3].isnan()) and bool(terms[[1, 2, 4]].isfinite().all())
    check_terms(terms, want_t)
    assert bool(grad.isfinite().all())
    check_grad(grad, want_g)


def test_yolo_every_target_ignored():
    pred, target, anchors = yolo_inputs(64, 3, 2, 2003)
    target[..., 0] = -1.0
    terms, grad, counts = yolo_abi(pred, target, anchors)
    assert counts.tolist() == [0, 0]
    assert terms[[1, 2, 4]].tolist() == [0.0, 0.0, 0.0] and bool(terms[0].isnan()) and bool(terms[3].isnan())
    assert not bool(grad.any()), "ignored anchors receive a zero gradient"


def test_yolo_bce_clamp_at_exactly_0_and_1():
    """p_obj exactly 0.0 and 1.0 on no-object cells: the logarithm is clamped at -100 and the gradient is ATen's
    (p - 0) / max(p (1 - p), 1e-12) / n: against torch.nn.BCELoss on the CPU."""
    pred, target, anchors = yolo_inputs(40, 3, 2, 2004, f_obj=0.0, f_ign=0.0)
    pred[0, 0::4, :, 0] = 0.0
    pred[0, 1::4, :, 0] = 1.0
    p = pred[..., 0:1].clone().requires_grad_()
    ref = torch.nn.BCELoss()(p, torch.zeros_like(p))
    ref.backward()
    assert float(ref.detach()) > 100.0 * 0.25 and float(p.grad.max()) > 1e9
    terms, grad, _ = yolo_abi(pred, target, anchors, (1.0, 1.0, 1.0, 1.0))
    check_terms(terms[[0, 3]], torch.stack([ref.detach(), ref.detach()]))
    check_grad(grad[..., 0:1], p.grad)
    assert not bool(grad[..., 1:].any())
    rel = ((grad[..., 0:1] - p.grad).abs() / p.grad.abs().clamp(min=1e-30))[p.grad != 0]
    assert float(rel.max()) <= 1e-4 and bool((grad[..., 0:1][p.grad == 0] == 0).all()), "each element against ATen's, not only the largest"


def test_yolo_class_out_of_range():
    """Nothing is read out of bounds; the class term, the total and that cell's logit gradients are NaN, everything else is what
    the restatement gives with a valid class in those cells."""
    Cn = 3
    pred, target, anchors = yolo_inputs(64, 3, Cn, 2005, f_obj=0.3)
    obj = (target[..., 0] == 1).nonzero()
    bad = obj[[0, len(obj) // 2, len(obj) - 1]]
    valid = target.clone()
    for (b, c, a), v in zip(bad.tolist(), (float(Cn), -1.0, 1.0e9)):
        target[b, c, a, 5] = v
        valid[b, c, a, 5] = 0.0
    want_t, want_g, _, _ = loss_ref.yolo_with_grads(pred, valid, anchors, WEIGHTS)
    terms, grad, _ = yolo_abi(pred, target, anchors)
    assert bool(terms[4].isnan()) and bool(terms[0].isnan())
    check_terms(terms[1:4], want_t[1:4])
    mask = torch.zeros_like(grad, dtype=torch.bool)
    for b, c, a in bad.tolist():
        mask[b, c, a, 5:] = True
    assert bool(grad[mask].isnan().all()) and bool(grad[~mask].isfinite().all())
    want_g = want_g.clone()
    want_g[mask] = float("nan")
    check_grad(grad, want_g)


@pytest.mark.parametrize("l1", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("n", [1, 3, 383, 384, 1536, 100003])
def test_rgb_sweep(n, l1):
    """1 element .. the 128-ray batch +- 1 .. 4 x 128 rays .. 100 003 elements (49 workgroups: the ticket path); both criteria
    in both passes, lambdas other than 1, with and without a fine pass."""
    rs = np.random.RandomState(3000 + n)
    coarse, fine, gt = (torch.from_numpy(rs.uniform(0, 1, size=(n,)).astype(np.float32)) for _ in range(3))
    lam = (0.7, 1.3)
    for f in (fine, None):
        want_t, want_c, want_f = loss_ref.rgb_with_grads(coarse, f, gt, use_l1_coarse=bool(l1[0]), use_l1_fine=bool(l1[1]),
                                                         lambda_coarse=lam[0], lambda_fine=lam[1])
        terms, d_c, d_f = rgb_abi(coarse, f, gt, l1, lam)
        check_terms(terms, want_t)
        check_grad(d_c, want_c)
        if f is not None:
            check_grad(d_f, want_f)
        else:
            assert float(terms[1]) == 0.0 and float(terms[2]) == float(terms[0])
    if n in (3, 1536):
        terms_m, c_m, f_m = rgb_module(coarse.reshape(-1, 3), fine.reshape(-1, 3), gt.reshape(-1, 3), l1, lam)
        terms, d_c, d_f = rgb_abi(coarse, fine, gt, l1, lam)
        assert torch.equal(bits(terms_m), bits(terms)) and torch.equal(bits(c_m.flatten()), bits(d_c)) and torch.equal(bits(f_m.flatten()), bits(d_f))


def test_rgb_l1_gradient_is_zero_where_prediction_equals_ground_truth():
    rs = np.random.RandomState(3100)
    gt = torch.from_numpy(rs.uniform(0, 1, size=(50, 3)).astype(np.float32))
    coarse = gt.clone()
    coarse[::2] += 0.25
    coarse[1::4] -= 0.125
    terms, d_c, _ = rgb_abi(coarse, None, gt, (1, 0), (2.0, 1.0))
    want_t, want_c, _ = loss_ref.rgb_with_grads(coarse, None, gt, use_l1_coarse=True, lambda_coarse=2.0)
    same = coarse == gt
    assert bool(same.any()) and bool((d_c[same] == 0).all()), "sign(0) = 0"
    check_terms(terms, want_t)
    check_grad(d_c, want_c)


# --------------------------------------------------------------------------- bit reproducibility
def test_same_inputs_give_the_same_bits():
    for cells in (384, 5000):
        pred, target, anchors = yolo_inputs(cells, 3, 2, 4000 + cells)
        a, b = yolo_abi(pred, target, anchors), yolo_abi(pred, target, anchors)
        assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1])) and torch.equal(a[2], b[2])
    rs = np.random.RandomState(4100)
    coarse, fine, gt = (torch.from_numpy(rs.uniform(0, 1, size=(100003,)).astype(np.float32)) for _ in range(3))
    a, b = rgb_abi(coarse, fine, gt, (0, 1), (0.7, 1.3)), rgb_abi(coarse, fine, gt, (0, 1), (0.7, 1.3))
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


# --------------------------------------------------------------------------- autograd behaviour
def test_autograd_behaviour():
    pred, target, anchors = yolo_inputs(37, 3, 2, 5000, f_obj=0.2)
    _, base, _ = yolo_module(pred, target, anchors)
    t, a = target.to(DEV), anchors.to(DEV)
    crit = ploss.YoloLoss(3, *WEIGHTS)
    # a grad_output other than 1 scales the gradient
    p = pred.to(DEV).requires_grad_()
    (crit(p, t, a)[0] * 3.0).backward()
    check_grad(p.grad, 3.0 * base, rel=1e-6)
    # backward(retain_graph=True) twice, as YoloTrainer.py:186 may: twice the gradient
    p = pred.to(DEV).requires_grad_()
    total = crit(p, t, a)[0]
    total.backward(retain_graph=True)
    total.backward(retain_graph=True)
    check_grad(p.grad, 2.0 * base, rel=1e-6)
    assert crit.saved_grad is not None
    # no gradient buffer without grad mode or without an input that requires grad; the terms are the same bits
    with torch.no_grad():
        quiet = crit(p, t, a)
    assert crit.saved_grad is None and not quiet[0].requires_grad and torch.equal(bits(quiet[0]), bits(total))
    assert crit(pred.to(DEV), t, a)[0].requires_grad is False and crit.saved_grad is None
    # non-contiguous pred (and target): made contiguous, left unchanged
    wide = torch.zeros(1, 37, 3, 12, device=DEV)
    wide[..., 2:9] = pred.to(DEV)
    pv = wide[..., 2:9].detach().requires_grad_()
    tv = torch.cat([t, t], dim=-1)[..., :6]
    assert not pv.is_contiguous() and not tv.is_contiguous()
    crit(pv, tv, a)[0].backward()
    assert torch.equal(bits(pv.grad), bits(base)) and torch.equal(bits(wide[..., 2:9]), bits(pred))
    # the same for the rgb losses
    rs = np.random.RandomState(5001)
    c, f, g = (torch.from_numpy(rs.uniform(0, 1, size=(2, 50, 3)).astype(np.float32)).to(DEV) for _ in range(3))
    nerf = ploss.NerfLoss(cf(1), cf(0), 0.7, 1.3)
    c1, f1 = c.clone().requires_grad_(), f.clone().requires_grad_()
    loss, _ = nerf(c1, f1, g)
    loss.backward(retain_graph=True)
    gc, gf = c1.grad.clone(), f1.grad.clone()
    (loss * 0.5).backward()
    check_grad(c1.grad, 1.5 * gc.cpu(), rel=1e-6)
    check_grad(f1.grad, 1.5 * gf.cpu(), rel=1e-6)
    with torch.no_grad():
        nerf(c1, f1, g)
    assert nerf.saved_grads == (None, None)
    loss, _ = nerf(c1, f.clone(), g)                    # only the coarse pass requires grad
    assert nerf.saved_grads[0] is not None and nerf.saved_grads[1] is None
    ct = c.transpose(0, 1).detach().requires_grad_()    # non-contiguous
    nerf(ct, f.transpose(0, 1), g.transpose(0, 1))[0].backward()
    assert torch.equal(bits(ct.grad.transpose(0, 1)), bits(gc))
    with pytest.raises(plib.PnyError, match="fp32"):
        nerf(c.double(), f, g)


# --------------------------------------------------------------------------- through the trainers' call sites
def test_nerf_training_step_with_nerf_loss_equals_the_aten_loss_lines(monkeypatch):
    """One training step of SB = 2 x 32 rays, 8 + 4 samples, deterministic mode: NerfLoss against PixelNerfTrainer.py:147-154
    in ATen on the same renders.  MLP gradients within 1e-4 of each tensor's max; the three terms within 1e-6 (both sides are
    fp32-rounded sums of 192 O(1) values)."""
    for var in ("PNYOLO_MLP_PRECISION", "PNYOLO_BWD_PRECISION", "PNYOLO_SCENE_STREAMS", "PNYOLO_STASH_GB"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("PNYOLO_GROUP", "1")
    SB, NV, NS, H, W, B, kc, kf, kfd = 2, 4, 2, 64, 64, 32, 8, 4, 2
    lam_c, lam_f = 0.7, 1.3
    net = make_model(pconf.default_mv()["model"], stop_encoder_grad=True)
    net.mlp_coarse.load_state_dict({k: torch.from_numpy(v) for k, v in synth.mlp_state(8601).items()})
    net.mlp_fine.load_state_dict({k: torch.from_numpy(v) for k, v in synth.mlp_state(8602).items()})
    net = net.to(DEV).train()
    net.set_deterministic(True)
    images = torch.from_numpy(synth.images(8603, SB * NV, H, W)).reshape(SB, NV, 3, H, W).to(DEV)
    poses = torch.from_numpy(np.stack([np.stack([synth.pose_spherical(40.0 * v + 15.0 * s, -20.0, 1.3 + 0.1 * s)
                                                 for v in range(NV)]) for s in range(SB)])).to(DEV)
    focal = torch.tensor([0.9 * W, 0.95 * W])
    lat = torch.from_numpy(np.concatenate([synth.latent(8604 + i, NS, 512, H // 2, W // 2) for i in range(SB)])).to(DEV)
    rs = np.random.RandomState(8605)
    n = SB * B
    draws = dict(u_coarse=rs.rand(n, kc).astype(np.float32), u_fine=rs.rand(n, kf - kfd).astype(np.float32),
                 u_fine2=rs.rand(n, kf - kfd).astype(np.float32), g_depth=rs.randn(n, kfd).astype(np.float32))
    ren = NeRFRenderer(n_coarse=kc, n_fine=kf, n_fine_depth=kfd, white_bkgd=True).train()
    all_rays, all_rgb_gt, _ = sample_train_batch(images, poses, focal, 0.8, 1.8, B, seed=8606)
    fused = ploss.NerfLoss(cf(0), cf(0), lam_c, lam_f)
    mse = torch.nn.MSELoss()

    def step(which):
        net.zero_grad(set_to_none=True)
        net.encode(images[:, :NS].contiguous(), poses[:, :NS].contiguous(), focal, latent=lat)
        ren.draws = draws
        out = ren(net, all_rays, want_weights=True)
        coarse, fine = out["coarse"]["rgb"], out["fine"]["rgb"]
        if which == "fused":
            loss, terms = fused(coarse, fine, all_rgb_gt)
            loss.backward()
            terms = terms.tolist()
        else:                                            # the trainer's lines
            rgb_loss = mse(coarse, all_rgb_gt)
            terms = [rgb_loss.item() * lam_c]
            fine_loss = mse(fine, all_rgb_gt)
            rgb_loss = rgb_loss * lam_c + fine_loss * lam_f
            terms.append(fine_loss.item() * lam_f)
            rgb_loss.backward()
            terms.append(rgb_loss.item())
        torch.cuda.synchronize()
        grads = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None and k.startswith("mlp_")}
        return coarse.detach().clone(), fine.detach().clone(), terms, grads

    c_a, f_a, t_a, g_a = step("aten")
    c_b, f_b, t_b, g_b = step("fused")
    assert torch.equal(bits(c_a), bits(c_b)) and torch.equal(bits(f_a), bits(f_b)), "the two steps did not render the same"
    assert c_a.numel() == 192
    assert len(g_a) >= 60 and set(g_a) == set(g_b)
    worst = max(check_grad(g_b[k], g_a[k].cpu(), what=k) for k in g_a)
    e_t = check_terms(torch.tensor(t_b), torch.tensor(t_a), tol=1e-6)
    print("NeRF step: terms %s, max|err| %.2e; worst MLP gradient error %.2e of its max (%d tensors)" % (t_b, e_t, worst, len(g_a)))


def test_yolo_mini_batch_with_yolo_loss_equals_the_restatement():
    """One mini-batch of 32 rays through YoloRenderer, YoloLoss and backward, against the fp64 restatement's terms and its
    gradient sent through the same render.  Terms within 1e-4 absolute, MLP gradients within 1e-4 of each tensor's max."""
    n, K, A = 32, 32, 3
    net, _ = scene_pair(2, 64, 64, 1792, 21, 5, 3, 1700, yolo=True, lat_hw=(8, 8))
    import pnyolo_oracle as orc
    _, tgt_c2w = synth.scene_cameras(2, radius=4.0, phi=-25.0)
    flipyz = np.diag([1.0, -1.0, -1.0, 1.0]).astype(np.float32)
    tgt_w2c = np.linalg.inv(tgt_c2w @ flipyz).astype(np.float32)
    cand = orc.gen_rays_yolo(tgt_w2c[None], 16, 12, [5.0, 5.5], [8.0, 6.0], 1.0, 6.0)[0].reshape(-1, 8)
    rs = np.random.RandomState(8701)
    rays = cand[torch.from_numpy(rs.choice(cand.shape[0], n, replace=False))]
    u = rs.rand(n, K).astype(np.float32)
    _, target, anchors = yolo_inputs(n, A, 2, 8702, f_obj=0.2)
    target, anchors = target.to(DEV), anchors.to(DEV)
    ren = YoloRenderer(K, 128, 1, A)
    ren.bind_parallel(net)
    crit = ploss.YoloLoss(A, *WEIGHTS)

    def step(which):
        net.zero_grad(set_to_none=True)
        ren.draws = dict(u_coarse=u)
        render = ren(rays[None].to(DEV)).reshape(1, n, A, 7)         # YoloTrainer.py:160,181
        if which == "fused":
            out = crit(render, target, anchors)
            out[0].backward(retain_graph=True)                       # :186
            terms = torch.stack([o.detach() for o in out]).cpu()
        else:
            terms, d_pred, _, _ = loss_ref.yolo_with_grads(render, target, anchors, WEIGHTS)
            render.backward(d_pred.to(torch.float32).to(DEV))
        torch.cuda.synchronize()
        grads = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None and k.startswith("mlp_")}
        return render.detach().clone(), terms, grads

    r_a, t_a, g_a = step("ref")
    r_b, t_b, g_b = step("fused")
    assert torch.equal(bits(r_a), bits(r_b)), "the two steps did not render the same"
    assert float(r_a[..., 0].min()) > 0.0 and float(r_a[..., 0].max()) < 1.0
    assert len(g_a) >= 20 and set(g_a) == set(g_b)
    worst = max(check_grad(g_b[k], g_a[k].cpu(), what=k) for k in g_a)
    e_t = check_terms(t_b, t_a)
    print("YOLO mini-batch: terms %s, max|err| %.2e; worst MLP gradient error %.2e of its max (%d tensors)" % (t_b.tolist(), e_t, worst, len(g_a)))


# --------------------------------------------------------------------------- no hidden waiting
def test_the_losses_do_not_wait_for_their_stream():
    """A queue of large matrix products is enqueued first; both losses, forward and backward, must come back with that stream
    still busy -- stream.query(), no timing threshold -- and give the bits of an undisturbed call."""
    pred, target, anchors = yolo_inputs(128, 3, 2, 9000)
    pred, target, anchors = pred.to(DEV), target.to(DEV), anchors.to(DEV)
    rs = np.random.RandomState(9001)
    c, f, g = (torch.from_numpy(rs.uniform(0, 1, size=(4, 128, 3)).astype(np.float32)).to(DEV) for _ in range(3))
    yolo, nerf = ploss.YoloLoss(3, *WEIGHTS), ploss.NerfLoss(cf(0), cf(0), 1.0, 1.0)

    def both():
        p, c1, f1 = pred.clone().requires_grad_(), c.clone().requires_grad_(), f.clone().requires_grad_()
        out = yolo(p, target, anchors)
        out[0].backward()
        loss, terms = nerf(c1, f1, g)
        loss.backward()
        return yolo.terms, p.grad, terms, c1.grad, f1.grad

    quiet = both()                                        # (also loads the kernels and allocates the stream's workspace)
    torch.cuda.synchronize()
    m = torch.randn(8192, 8192, device=DEV)
    out = torch.empty_like(m)
    torch.mm(m, m, out=out)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(DEV)
    for _ in range(60):
        torch.mm(m, m, out=out)
    assert not stream.query(), "the queue of matrix products was too short to test anything"
    busy = both()
    still_busy = not stream.query()
    torch.cuda.synchronize()
    assert still_busy, "a loss call waited for the stream"
    assert all(torch.equal(bits(q), bits(b)) for q, b in zip(quiet, busy))
