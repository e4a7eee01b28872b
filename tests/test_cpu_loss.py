"""
The training losses without a GPU: the fp64 restatement (tests/loss_ref.py) against the reference's recorded results
(tests/golden/losses.npz, tools/make_loss_golden.py), the two new ABI functions in the header and the built library, and
what pixel_nerf_yolo_amd.loss refuses.
"""
import re

import pytest
import torch

import loss_ref
from host_tools import built_lib, c99_program, header_code  # noqa: F401
from pixel_nerf_yolo_amd import conf as pconf
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd import loss as ploss

YOLO_CASES = ("y128", "y37", "ynoobj", "ya1c1", "ya3c5")
RGB_CASES = ("mse_mse", "l1_mse", "coarse_only")
NEW_FUNCTIONS = ("pny_rgb_loss", "pny_yolo_loss")


def rel_to_max(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


# --------------------------------------------------------------------------- the restatement against the reference
@pytest.mark.parametrize("name", YOLO_CASES)
def test_yolo_restatement_equals_the_reference(golden, name):
    """fp64 against the reference's fp32 on O(1) values: terms within 1e-6 absolute, the gradient within 1e-6 of its max.
    Measured: terms 6.3e-7 at the most (the total, a value of 6 to 10, where half an fp32 ulp is 4.8e-7), gradients 9.3e-8."""
    g = golden("losses")
    pred, target, anchors = (torch.from_numpy(g["%s_%s" % (name, k)]) for k in ("pred", "target", "anchors"))
    before = (pred.clone(), target.clone())
    terms, grad, n_obj, n_noobj = loss_ref.yolo_with_grads(pred, target, anchors, g[name + "_weights"])
    assert torch.equal(pred, before[0]) and torch.equal(target, before[1]), "the restatement modified its inputs"
    want = torch.from_numpy(g[name + "_terms"]).to(torch.float64)
    err_t = float((terms - want).abs().max())
    err_g = rel_to_max(grad, torch.from_numpy(g[name + "_d_pred"]).to(torch.float64))
    print("%s: n_obj %d n_noobj %d, terms max|err| %.2e, gradient err / max %.2e" % (name, n_obj, n_noobj, err_t, err_g))
    assert err_t <= 1e-6 and err_g <= 1e-6
    if name == "ynoobj":
        assert n_obj == 0 and float(terms[1]) == 0.0 and float(terms[2]) == 0.0 and float(terms[4]) == 0.0


@pytest.mark.parametrize("name", RGB_CASES)
def test_rgb_restatement_equals_the_reference(golden, name):
    """Terms within 1e-6 absolute, gradients within 1e-6 of each tensor's max (measured: 2.2e-8 and 1.2e-7)."""
    g = golden("losses")
    coarse, gt = torch.from_numpy(g[name + "_coarse"]), torch.from_numpy(g[name + "_gt"])
    fine = torch.from_numpy(g[name + "_fine"]) if name + "_fine" in g else None
    l1, lam = g[name + "_use_l1"], g[name + "_lambdas"]
    terms, d_c, d_f = loss_ref.rgb_with_grads(coarse, fine, gt, use_l1_coarse=bool(l1[0]), use_l1_fine=bool(l1[1]),
                                              lambda_coarse=float(lam[0]), lambda_fine=float(lam[1]))
    err_t = float((terms - torch.from_numpy(g[name + "_terms"]).to(torch.float64)).abs().max())
    err_c = rel_to_max(d_c, torch.from_numpy(g[name + "_d_coarse"]).to(torch.float64))
    err_f = rel_to_max(d_f, torch.from_numpy(g[name + "_d_fine"]).to(torch.float64)) if fine is not None else 0.0
    print("%s: terms max|err| %.2e, gradient err / max %.2e (coarse) %.2e (fine)" % (name, err_t, err_c, err_f))
    assert err_t <= 1e-6 and err_c <= 1e-6 and err_f <= 1e-6
    # the criteria's own values (get_rgb_loss's modules, unscaled)
    raw = loss_ref.rgb_terms(coarse, fine, gt, bool(l1[0]), bool(l1[1]), 1.0, 1.0)
    assert float((raw[:2] - torch.from_numpy(g[name + "_raw"]).to(torch.float64)).abs().max()) <= 1e-6


# --------------------------------------------------------------------------- the ABI
def test_header_declares_and_library_exports_the_loss_functions():
    """Each takes its descriptor first (declared, bound, exported: tests/test_cpu_abi.py)."""
    for name in NEW_FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(\s*const\s+%s_desc\s*\*" % (name, name), header_code()), name + " is not declared"


def test_header_with_the_loss_functions_is_plain_c(built_lib, tmp_path):
    """A C program that names both functions and both descriptors, linked against the shared library: argument errors come
    back before anything touches a device."""
    run = c99_program(tmp_path, '#include "pnyolo.h"\n#include <stdio.h>\n'
                      "int main(void) {\n"
                      "  pny_rgb_loss_desc r = {0, 1, 0.5f, 2.0f}; pny_yolo_loss_desc y = {3, 2, 1.0f, 20.0f, 1.0f, 1.0f};\n"
                      "  float terms[5];\n"
                      "  int a = pny_rgb_loss(&r, NULL, NULL, NULL, 4, terms, NULL, NULL, NULL);\n"
                      "  int b = pny_yolo_loss(&y, NULL, NULL, NULL, 4, terms, NULL, NULL, NULL);\n"
                      '  printf("%d %d %d\\n", a, b, pny_version());\n'
                      "  return a == PNY_ERR_ARG && b == PNY_ERR_ARG && pny_version() == PNY_ABI_VERSION ? 0 : 1; }\n", link=True)()
    assert run.returncode == 0 and run.stdout.split() == ["-1", "-1", "11"], (run.returncode, run.stdout, run.stderr)


def test_argument_errors(built_lib):
    """NULL where not allowed, n <= 0, A < 1, C < 1: PNY_ERR_ARG with a message, checked before any device is touched."""
    import ctypes as C
    L = built_lib
    x = C.c_void_p(256)   # never dereferenced: every call below fails its argument checks
    r = plib.RgbLossDesc(0, 0, 1.0, 1.0)
    y = plib.YoloLossDesc(3, 2, 1.0, 20.0, 1.0, 1.0)
    bad = [L.pny_rgb_loss(None, x, None, x, 4, x, None, None, None), L.pny_rgb_loss(C.byref(r), None, None, x, 4, x, None, None, None),
           L.pny_rgb_loss(C.byref(r), x, None, None, 4, x, None, None, None), L.pny_rgb_loss(C.byref(r), x, None, x, 4, None, None, None, None),
           L.pny_rgb_loss(C.byref(r), x, None, x, 0, x, None, None, None), L.pny_rgb_loss(C.byref(r), x, None, x, -3, x, None, None, None),
           L.pny_rgb_loss(C.byref(r), x, None, x, 4, x, None, x, None),
           L.pny_yolo_loss(None, x, x, x, 4, x, None, None, None), L.pny_yolo_loss(C.byref(y), None, x, x, 4, x, None, None, None),
           L.pny_yolo_loss(C.byref(y), x, None, x, 4, x, None, None, None), L.pny_yolo_loss(C.byref(y), x, x, None, 4, x, None, None, None),
           L.pny_yolo_loss(C.byref(y), x, x, x, 4, None, None, None, None), L.pny_yolo_loss(C.byref(y), x, x, x, 0, x, None, None, None),
           L.pny_yolo_loss(C.byref(plib.YoloLossDesc(0, 2, 1.0, 1.0, 1.0, 1.0)), x, x, x, 4, x, None, None, None),
           L.pny_yolo_loss(C.byref(plib.YoloLossDesc(3, 0, 1.0, 1.0, 1.0, 1.0)), x, x, x, 4, x, None, None, None),
           L.pny_yolo_loss(C.byref(y), x, x, x, 2 ** 31, x, None, None, None)]
    assert bad == [-1] * len(bad), bad
    assert b"pny_yolo_loss" in L.pny_last_error()


# --------------------------------------------------------------------------- the Python module
def test_unsupported_names_raise_not_implemented():
    for make in (lambda: ploss.AlphaLossNV2(1.0, 10.0, 0), lambda: ploss.get_alpha_loss(pconf.Conf({"lambda_alpha": 0.0})),
                 lambda: ploss.RGBWithUncertainty(pconf.Conf({"use_l1": False})),
                 lambda: ploss.RGBWithBackground(pconf.Conf({"use_l1": False}))):
        with pytest.raises(NotImplementedError, match="pixel_nerf_yolo_amd.loss"):
            make()
    with pytest.raises(NotImplementedError, match="use_uncertainty"):
        ploss.get_rgb_loss(pconf.Conf({"use_l1": False, "use_uncertainty": True}), coarse=False)
    with pytest.raises(NotImplementedError, match="reduction"):
        ploss.get_rgb_loss(pconf.Conf({"use_l1": False}), reduction="none")
    # (as in the reference, the coarse criterion ignores use_uncertainty)
    assert ploss.get_rgb_loss(pconf.Conf({"use_l1": True, "use_uncertainty": True}), coarse=True).use_l1


def test_constructors_follow_the_reference():
    c = pconf.Conf({"loss": {"rgb": {"use_l1": False}, "rgb_fine": {"use_l1": True}, "lambda_coarse": 0.5, "lambda_fine": 2.0},
                    "yolo": {"weights": {"box_loss": 1, "object_loss": 20, "no_object_loss": 1, "class_loss": 1}}})
    n = ploss.NerfLoss.from_conf(c["loss"])
    assert (n.use_l1_coarse, n.use_l1_fine, n.lambda_coarse, n.lambda_fine) == (False, True, 0.5, 2.0)
    y = ploss.YoloLoss.from_conf(c, 3)
    assert (y.num_anchors_per_scale, y.box_loss, y.object_loss, y.no_object_loss, y.class_loss) == (3, 1.0, 20.0, 1.0, 1.0)


def test_cpu_tensors_raise():
    x = torch.rand(4, 3)
    with pytest.raises(plib.PnyError, match="no CPU path"):
        ploss.get_rgb_loss(pconf.Conf({"use_l1": False}))(x.clone().requires_grad_(), x)
    with pytest.raises(plib.PnyError, match="no CPU path"):
        ploss.NerfLoss(pconf.Conf({"use_l1": False}), pconf.Conf({"use_l1": False}))(x, x, x)
    with pytest.raises(plib.PnyError, match="no CPU path"):
        ploss.YoloLoss(3, 1, 20, 1, 1)(torch.rand(1, 4, 3, 7), torch.zeros(1, 4, 3, 6), torch.rand(3, 2))
