"""
The losses of all mini-batches of a YOLO training step in one launch (include/pnyolo.h pny_yolo_loss_batches,
loss.YoloLoss.forward_batches), without a GPU: the two ABI functions in the header and the built library, their argument
checks and the mini-batch count, the fp64 restatement of the trainer's loop (tests/loss_batches_ref.py) against autograd of
the summed losses, and what the Python layer refuses.
"""
import ctypes as C
import inspect
import re

import numpy as np
import pytest
import torch

import loss_batches_ref
import loss_ref
from host_tools import built_lib, c99_program, header_code  # noqa: F401
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd import loss as ploss
from pixel_nerf_yolo_amd import util as putil

# (rows per scale, batch_rows, M)
COUNT_CASES = [((1,), 1, 1), ((5,), 2, 3), ((165,), 128, 2), ((7, 3), 4, 3), ((64, 16, 4, 1), 64, 4)]


def batches(rows, batch_rows, n_scales=None):
    rows = list(rows) + [0] * (4 - len(rows))
    return plib.YoloBatchesDesc(len([r for r in rows if r]) if n_scales is None else n_scales, batch_rows, (C.c_int64 * 4)(*rows))


# --------------------------------------------------------------------------- the ABI
def test_header_declares_and_library_exports_the_functions():
    """The types of the descriptors' slots (declared, bound, exported, the mirror's layout: tests/test_cpu_abi.py)."""
    code = header_code()
    assert re.search(r"\bint\s+pny_yolo_loss_batches\s*\(\s*const\s+pny_yolo_loss_desc\s*\*\s*\w+\s*,\s*const\s+pny_yolo_batches_desc\s*\*", code)
    assert re.search(r"\bint\s+pny_yolo_loss_batches_count\s*\(\s*const\s+pny_yolo_batches_desc\s*\*", code)
    assert re.search(r"typedef\s+struct\s+pny_yolo_batches_desc\s*\{[^}]*int32_t\s+n_scales;[^}]*int32_t\s+batch_rows;[^}]*int64_t\s+rows\[4\];[^}]*\}", code)


def test_header_with_the_functions_is_plain_c(built_lib, tmp_path):
    """A C program that names the descriptor and both functions links against the shared library, and a NULL call comes back
    with PNY_ERR_ARG before anything touches a device."""
    run = c99_program(tmp_path, '#include "pnyolo.h"\n#include <stdio.h>\n'
                      "int main(void) {\n"
                      "  pny_yolo_loss_desc y = {3, 2, 1.0f, 20.0f, 1.0f, 1.0f};\n"
                      "  pny_yolo_batches_desc b = {2, 4, {7, 3, 0, 0}};\n"
                      "  float terms[15], step[6];\n"
                      "  int a = pny_yolo_loss_batches(&y, &b, NULL, NULL, NULL, terms, NULL, step, NULL, NULL);\n"
                      "  int m = pny_yolo_loss_batches_count(&b);\n"
                      '  printf("%d %d %d\\n", a, m, pny_version());\n'
                      "  return a == PNY_ERR_ARG && m == 3 && pny_version() == PNY_ABI_VERSION ? 0 : 1; }\n", link=True)()
    assert run.returncode == 0 and run.stdout.split() == ["-1", "3", "11"], (run.returncode, run.stdout, run.stderr)


def test_argument_errors_and_the_mini_batch_count(built_lib):
    """Every refusal is PNY_ERR_ARG with the function's name in pny_last_error(), checked before any device is touched (the
    pointers below are never dereferenced); pny_yolo_loss_batches_count gives M."""
    L = built_lib
    x = C.c_void_p(256)
    y = plib.YoloLossDesc(3, 2, 1.0, 20.0, 1.0, 1.0)
    good = batches((7, 3), 4)

    def call(desc=y, b=good, pred=x, target=x, anchors=x, terms=x, step=x):
        rc = L.pny_yolo_loss_batches(None if desc is None else C.byref(desc), None if b is None else C.byref(b), pred, target, anchors,
                                     terms, None, step, None, None)
        return rc, L.pny_last_error()

    bad = dict(
        null_desc=call(desc=None), null_batches=call(b=None), null_pred=call(pred=None), null_target=call(target=None),
        null_anchors=call(anchors=None), null_terms=call(terms=None), null_step=call(step=None),
        no_scale=call(b=batches((7, 3), 4, n_scales=0)), five_scales=call(b=batches((7, 3, 1, 1), 4, n_scales=5)),
        negative_scales=call(b=batches((7, 3), 4, n_scales=-1)),
        zero_rows=call(b=batches((7, 0), 4, n_scales=2)), negative_rows=call(b=batches((-7,), 4, n_scales=1)),
        zero_batch=call(b=batches((7, 3), 0)), negative_batch=call(b=batches((7, 3), -4)),
        too_many=call(b=batches((4097,), 1)), too_many_over_scales=call(b=batches((2048, 2048, 1), 1)),
        no_anchor=call(desc=plib.YoloLossDesc(0, 2, 1.0, 1.0, 1.0, 1.0)), no_class=call(desc=plib.YoloLossDesc(3, 0, 1.0, 1.0, 1.0, 1.0)),
        items_2_31=call(b=batches((2 ** 31 // 3 + 1,), 2 ** 20)),
        items_2_31_over_scales=call(desc=plib.YoloLossDesc(1, 2, 1.0, 1.0, 1.0, 1.0), b=batches((2 ** 30, 2 ** 30), 2 ** 20)))
    for name, (rc, msg) in bad.items():
        assert rc == -1 and msg.startswith(b"pny_yolo_loss_batches:"), (name, rc, msg)
    # the largest sizes that pass the checks fail later, not here: (2^31 - 1) items, 4096 mini-batches
    assert L.pny_yolo_loss_batches_count(C.byref(batches((4096,), 1))) == 4096
    assert L.pny_yolo_loss_batches_count(C.byref(batches((2 ** 31 - 1,), 2 ** 20))) == 2048
    for rows, b, m in COUNT_CASES:
        assert L.pny_yolo_loss_batches_count(C.byref(batches(rows, b))) == m, (rows, b)
        assert len(loss_batches_ref.segments(rows, b)) == m
    for b in (batches((4097,), 1), batches((2048, 2048, 1), 1), batches((7, 3), 0), batches((7, 0), 4, n_scales=2),
              batches((7,), 4, n_scales=5)):
        assert L.pny_yolo_loss_batches_count(C.byref(b)) == -1
        assert L.pny_last_error().startswith(b"pny_yolo_loss_batches_count:")
    assert L.pny_yolo_loss_batches_count(None) == -1


# --------------------------------------------------------------------------- the restatement
def inputs(rows, A, Cn, seed):
    rs = np.random.RandomState(seed)
    n = sum(rows)
    pred = np.concatenate([rs.uniform(1e-3, 1 - 1e-3, size=(n, A, 1)), rs.randn(n, A, 2), rs.uniform(-2, 2, size=(n, A, 2)),
                           rs.randn(n, A, Cn)], axis=-1).astype(np.float32)
    u = rs.rand(n, A)
    target = np.concatenate([np.where(u < 0.3, 1.0, np.where(u < 0.4, -1.0, 0.0))[..., None], rs.uniform(0, 1, size=(n, A, 2)),
                             rs.uniform(0.02, 0.9, size=(n, A, 2)), rs.randint(0, Cn, size=(n, A, 1))], axis=-1).astype(np.float32)
    anchors = [torch.from_numpy(rs.uniform(0.1, 0.6, size=(A, 2)).astype(np.float32)) for _ in rows]
    return torch.from_numpy(pred), torch.from_numpy(target), anchors


@pytest.mark.parametrize("rows,batch_rows", [((5,), 2), ((165,), 128), ((7, 3), 4), ((64, 16, 4, 1), 64)])
def test_restatement_gradient_is_autograd_of_the_summed_losses(rows, batch_rows):
    """The gradient the trainer's loop accumulates is d (sum_m loss_m) / d pred: the concatenated per-mini-batch gradients
    against ONE fp64 backward through the sum, within 1e-12 of the tensor's max; the step values are the trainer's sums."""
    weights = (1.0, 20.0, 1.0, 1.0)
    pred, target, anchors = inputs(rows, 3, 2, 100 + sum(rows))
    terms, counts, grad, step = loss_batches_ref.yolo_batches(pred, target, anchors, weights, rows, batch_rows)
    segs = loss_batches_ref.segments(rows, batch_rows)
    assert terms.shape == (len(segs), 5) and counts.shape == (len(segs), 2) and grad.shape == pred.shape and step.shape == (6,)
    assert sum(n for _, _, n in segs) == sum(rows) and all(n <= batch_rows for _, _, n in segs)
    p = pred.to(torch.float64).requires_grad_()
    total = sum(loss_ref.yolo_terms(p[r0:r0 + n], target[r0:r0 + n], anchors[s], weights)[0][0] for s, r0, n in segs)
    total.backward()
    err = float((grad - p.grad).abs().max()) / float(p.grad.abs().max())
    print("rows %s, B %d: M %d, gradient err / max %.2e" % (rows, batch_rows, len(segs), err))
    assert err <= 1e-12
    assert int(counts.sum()) == int((target[..., 0] == 1).sum()) + int((target[..., 0] == 0).sum())
    # not YoloLoss over all rows: every mini-batch divides by its own counts
    if len(segs) > 1:
        whole = loss_ref.yolo_with_grads(pred, target, anchors[0], weights)[1]
        assert float((whole - grad).abs().max()) > 1e-3 * float(grad.abs().max())
    f32 = terms.to(torch.float32).to(torch.float64)
    assert abs(float(step[0]) - float(f32[:, 0].sum())) <= 1e-12 * abs(float(step[0]))
    assert float((step[1:] - f32.sum(0) / len(segs)).abs().max()) <= 1e-12 * float(step[1:].abs().max())


# --------------------------------------------------------------------------- the Python layer
def test_forward_batches_refuses_cpu_tensors():
    crit = ploss.YoloLoss(3, 1, 20, 1, 1)
    with pytest.raises(plib.PnyError, match="no CPU path"):
        crit.forward_batches(torch.rand(4, 3, 7), torch.zeros(4, 3, 6), torch.rand(1, 3, 2), [4], 2)
    with pytest.raises(plib.PnyError, match="no CPU path"):
        crit.forward_batches(torch.rand(1, 4, 3, 7), torch.zeros(1, 4, 3, 6), [torch.rand(3, 2)], [4], 2)


def test_yolo_train_batch_has_a_flat_option_that_is_off_by_default():
    p = inspect.signature(putil.yolo_train_batch).parameters
    assert "flat" in p and p["flat"].default is False
    assert list(p)[:10] == ["poses", "view_ids", "focal", "c", "targets", "height", "width", "cell_sizes", "z_near", "z_far"]
