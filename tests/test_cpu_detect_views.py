"""
The batched detection scorer without a GPU (include/pnyolo.h pny_detect_views, util.score_detections / DetectionMeter):
  * the entry's comment cites the reference, its limits are the restatement's (the boundary itself: tests/test_cpu_abi.py);
  * the C entry refuses bad arguments with PNY_ERR_ARG and a message naming the field, before any launch;
  * util.score_detections refuses on the host, by name: wrong ranks, more than 4 scales, anchors that do not divide into the
    scales, offsets that do not start at 0 or do not ascend, CPU tensors;
  * the batched restatement the GPU tests compare against (tests/detect_views_ref.py) equals a per-view loop of the oracle's
    tp_fp_fn on the reference's captured lists (tests/golden/yolo_tail.npz) and on stage_ref.match_cases().
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import detect_views_ref as dr
from host_tools import CSRC, ROOT, built_lib, header_code, header_text  # noqa: F401
import pnyolo_oracle as orc
import stage_ref as sr
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd import util as putil

GOLDEN = os.path.join(ROOT, "tests", "golden")


# --------------------------------------------------------------------------- C ABI
def test_entry_is_declared_bound_and_exported():
    """What is this entry's own (declared, bound, exported, its layout and constants: tests/test_cpu_abi.py)."""
    hdr = header_text()
    assert re.search(r"\bint\s+pny_detect_views\s*\(\s*const\s+pny_detect_views_desc\s*\*", header_code())
    # the comment of the entry names the reference lines it replaces, as every other entry does
    block = hdr[hdr.index("The detection scores of ALL views"):hdr.index("int pny_detect_views")]
    assert "YoloTrainer.py:338-354" in block and "util.py:765-802" in block and "util.py:633-689" in block
    # the limit (the header's, tests/test_cpu_abi.py) lies in the range the LDS allows and is what the restatement assumes
    assert 2048 <= plib.DETECT_MAX_CANDIDATES <= 8192 and plib.DETECT_MAX_CANDIDATES == dr.MAX_CANDIDATES
    assert len(plib.DETECT_RECORD) == 8 and tuple(plib.DETECT_RECORD) == dr.RECORD
    # one copy of the decode and of the IoU: the per-image kernels take them from the shared header
    det, views = (open(os.path.join(CSRC, f)).read() for f in ("detect.hip", "detect_views.hip"))
    shared = open(os.path.join(CSRC, "pny_detect.h")).read()
    assert "float iou_xywh(" in shared and "void cell_to_bbox(" in shared
    for src in (det, views):
        assert '#include "pny_detect.h"' in src and "float iou_xywh(" not in src and "expf(" not in src
    assert "detect_views.hip" in open(os.path.join(CSRC, "Makefile")).read()


def test_bad_arguments_are_refused_before_any_launch(built_lib):
    """PNY_ERR_ARG (-1) with a message naming the field, whether or not a GPU is there (no pointer is dereferenced by the host
    but anchors_host, which is real)."""
    call = built_lib.pny_detect_views
    p = C.c_void_p(4096)
    two = (C.c_void_p * 4)(4096, 4096, 4096, 4096)
    anchors = (C.c_float * 32)(*([0.5] * 32))
    cells = dict(form=plib.DETECT_CELLS, n_views=2, n_scales=2, height=8, width=12, cell_sizes=(C.c_int32 * 4)(1, 2, 0, 0), n_anchors=3,
                 nms_iou=0.5, nms_threshold=0.5, match_iou=0.2)
    boxes = dict(form=plib.DETECT_BOXES, n_views=2, n_pred_rows=5, n_target_rows=5, nms_iou=0.5, nms_threshold=0.5, match_iou=0.2)

    def rc(base, preds=two, targets=two, anc=anchors, prow=p, poff=p, trow=p, toff=p, rec=p, hc=p, tot=p, kt=None, kp=None, **over):
        d = plib.DetectViewsDesc(**dict(base, **over))
        return call(C.byref(d), preds, targets, anc, prow, poff, trow, toff, rec, hc, tot, kt, kp, None)

    def refused(needle, *a, **k):
        assert rc(*a, **k) == -1
        msg = built_lib.pny_last_error().decode()
        assert msg.startswith("pny_detect_views: ") and needle in msg, (needle, msg)

    assert call(None, two, two, anchors, p, p, p, p, p, p, p, None, None, None) == -1
    refused("per_view_dev", cells, rec=None)
    refused("highest_conf_dev", cells, hc=None)
    refused("totals_dev", cells, tot=None)
    refused("form", cells, form=2)
    refused("n_views", cells, n_views=0)
    refused("n_scales", cells, n_scales=5)
    refused("n_scales", cells, n_scales=0)
    refused("n_anchors", cells, n_anchors=5)
    refused("n_anchors", cells, n_anchors=0)
    refused("cell_sizes[1]", cells, cell_sizes=(C.c_int32 * 4)(1, 9, 0, 0))
    refused("cell_sizes[0]", cells, cell_sizes=(C.c_int32 * 4)(0, 2, 0, 0))
    refused("height", cells, height=0)
    refused("anchors_host", cells, anc=None)
    refused("preds_dev", cells, preds=None)
    refused("targets_dev[1]", cells, targets=(C.c_void_p * 4)(4096, 0, 0, 0))
    refused("max_kept", cells, max_kept=-1)
    refused("max_kept", cells, kt=p, max_kept=0)
    refused("finite", cells, nms_iou=float("nan"))
    refused("finite", cells, match_iou=float("inf"))
    refused("2^31", cells, height=30000, width=30000, cell_sizes=(C.c_int32 * 4)(1, 1, 0, 0))
    refused("n_pred_rows", boxes, n_pred_rows=-1)
    refused("offsets", boxes, poff=None)
    refused("offsets", boxes, toff=None)
    refused("rows_dev", boxes, prow=None)
    assert rc(boxes, prow=None, n_pred_rows=0, rec=None) == -1          # an empty list needs no rows (refused for the record only)


# --------------------------------------------------------------------------- host-side refusals of util.score_detections
def cells_inputs(V=2, H=4, W=6, cells=(1, 2), A=3):
    preds = [torch.zeros(V * (H // c) * (W // c), A, 7) for c in cells]
    targets = [torch.zeros(V * (H // c) * (W // c), A, 6) for c in cells]
    return dict(preds=preds, targets=targets, anchors=torch.ones(len(cells) * A, 2), height=H, width=W, cell_sizes=list(cells),
                nms_iou=0.5, nms_t=0.5, match_iou=0.2, n_views=V)


def boxes_inputs(**over):
    k = dict(pred_rows=torch.zeros(5, 6), pred_offsets=[0, 2, 5], target_rows=torch.zeros(4, 6), target_offsets=[0, 1, 4])
    k.update(over)
    return dict(preds=None, targets=None, anchors=None, height=0, width=0, cell_sizes=None, nms_iou=0.5, nms_t=0.5, match_iou=0.2,
                boxes=(k["pred_rows"], k["pred_offsets"], k["target_rows"], k["target_offsets"]))


def test_score_detections_refuses_by_name_on_the_host():
    who = "pixel_nerf_yolo_amd.util.score_detections"
    k = cells_inputs()
    k["preds"][1] = k["preds"][1].reshape(-1, 7)                         # wrong rank
    with pytest.raises(ValueError, match=who + r".*preds\[1\]"):
        putil.score_detections(**k)
    k = cells_inputs()
    k["targets"][0] = k["targets"][0][:-1]                               # wrong row count
    with pytest.raises(ValueError, match=who + r".*targets\[0\]"):
        putil.score_detections(**k)
    k = cells_inputs()
    k["targets"][0] = torch.zeros(2 * 4 * 6, 3, 7)                       # predictions where targets belong
    with pytest.raises(ValueError, match=r"targets\[0\]"):
        putil.score_detections(**k)
    with pytest.raises(ValueError, match="cell_sizes must hold 1 .. 4 scales, got 5"):
        putil.score_detections(**cells_inputs(H=16, W=16, cells=(1, 2, 4, 8, 16), A=1))
    k = cells_inputs()
    k["anchors"] = torch.ones(5, 2)                                      # 5 anchors over 2 scales
    with pytest.raises(ValueError, match="anchors must be"):
        putil.score_detections(**k)
    k = cells_inputs(A=5)
    with pytest.raises(ValueError, match="at most 4 anchors per scale, got 5"):
        putil.score_detections(**k)
    k = cells_inputs()
    k["n_views"] = None
    with pytest.raises(ValueError, match="n_views"):
        putil.score_detections(**k)
    k = cells_inputs()
    k["preds"][0] = k["preds"][0].double()
    with pytest.raises(TypeError, match=r"preds\[0\] must be float32"):
        putil.score_detections(**k)
    with pytest.raises(ValueError, match="pred_offsets must start at 0, got 1"):
        putil.score_detections(**boxes_inputs(pred_offsets=[1, 2, 5]))
    with pytest.raises(ValueError, match="target_offsets must ascend"):
        putil.score_detections(**boxes_inputs(target_offsets=[0, 3, 2]))
    with pytest.raises(ValueError, match="pred_offsets ends at 6, past the 5 rows"):
        putil.score_detections(**boxes_inputs(pred_offsets=[0, 2, 6]))
    with pytest.raises(ValueError, match="target_offsets must hold n_views \\+ 1 = 3 entries, got 4"):
        putil.score_detections(**boxes_inputs(target_offsets=[0, 1, 2, 4]))
    with pytest.raises(ValueError, match=r"pred_rows must be a \(n, 6\) tensor"):
        putil.score_detections(**boxes_inputs(pred_rows=torch.zeros(5, 7)))
    # complete and well-formed, but on the CPU: there is no host path behind this call
    with pytest.raises(plib.PnyError, match=r"preds\[0\] is on cpu"):
        putil.score_detections(**cells_inputs())
    with pytest.raises(plib.PnyError, match="pred_rows is on cpu"):
        putil.score_detections(**boxes_inputs())


# --------------------------------------------------------------------------- the batched restatement is the per-view oracle
def oracle_counts(t, p, nms_iou, nms_t, match_iou):
    return orc.tp_fp_fn(torch.from_numpy(np.ascontiguousarray(t)), torch.from_numpy(np.ascontiguousarray(p)), nms_iou, nms_t, match_iou)


def test_restatement_is_the_per_view_oracle_on_the_reference_captures():
    with np.load(os.path.join(GOLDEN, "yolo_tail.npz")) as f:
        g = {k: f[k] for k in f.files}
    tl = [g["c%d_t_boxes" % c].astype(np.float32) for c in range(3)]
    pl = [g["c%d_p_boxes" % c].astype(np.float32) for c in range(3)]
    for k in range(2):
        iou_t, conf_t = (float(v) for v in g["c0_nms%d_meta" % k][:2])
        assert all(tuple(float(v) for v in g["c%d_nms%d_meta" % (c, k)][:2]) == (iou_t, conf_t) for c in range(3))
        ref = dr.score_views(tl, pl, iou_t, conf_t, 0.2)
        want = [oracle_counts(t, p, iou_t, conf_t, 0.2) for t, p in zip(tl, pl)]
        assert [tuple(r[:3]) for r in ref["per_view"].tolist()] == want
        assert want == [tuple(int(v) for v in g["c%d_tpfpfn%d" % (c, k)]) for c in range(3)]     # the reference's own counts
        assert ref["totals"].tolist() == [sum(w[i] for w in want) for i in range(3)] + [0]
        assert not ref["per_view"][:, 7].any()
        for c in range(3):                                                                       # and its own kept predictions
            assert np.array_equal(ref["kept_preds"][c], g["c%d_nms%d_kept" % (c, k)].astype(np.float32))
            assert ref["per_view"][c, 6] == int(g["c%d_nms%d_meta" % (c, k)][3])
            assert ref["highest_conf"][c, 1] == np.float32(g["c%d_nms%d_meta" % (c, k)][2])


def test_restatement_is_the_per_view_oracle_on_the_match_cases():
    cases = sr.match_cases()
    for group in sorted({c[2:] for c in cases.values()}):                 # one batched call per set of thresholds
        names = sorted(n for n, c in cases.items() if c[2:] == group)
        ref = dr.score_views([cases[n][0] for n in names], [cases[n][1] for n in names], *group)
        want = [oracle_counts(cases[n][0], cases[n][1], *group) for n in names]
        assert [tuple(r[:3]) for r in ref["per_view"].tolist()] == want, names
        assert ref["totals"].tolist() == [sum(w[i] for w in want) for i in range(3)] + [0]
    # the same through the oracle as the per-view counter, and the segment form round-trips
    names = sorted(cases)
    rows, off = dr.segments([cases[n][1] for n in names])
    assert off[0] == 0 and off[-1] == len(rows) and all(np.array_equal(rows[off[i]:off[i + 1]], cases[n][1]) for i, n in enumerate(names))


def test_restatement_orders_scales_then_cells_and_refuses_overflow():
    rs = np.random.RandomState(5)
    a, b = rs.rand(2, 6, 6).astype(np.float32), rs.rand(2, 3, 6).astype(np.float32)
    lists = dr.view_lists([a, b], 2)
    assert np.array_equal(lists[1], np.concatenate([a[1], b[1]]))
    many = sr._boxes(np.random.RandomState(6), 40, conf=0.9)
    few = sr._boxes(np.random.RandomState(7), 10, conf=0.9)
    ref = dr.score_views([few, few, many], [few, many, few], 0.5, 0.5, 0.2, max_candidates=39)
    assert ref["per_view"][:, 7].tolist() == [0, dr.PREDS_OVERFLOW, dr.TARGETS_OVERFLOW] and ref["totals"][3] == 2
    assert ref["per_view"][1:, :5].tolist() == [[0] * 5] * 2 and ref["per_view"][1, 6] == 40 and ref["per_view"][2, 5] == 40
    tp, fp, fn = ref["per_view"][0, :3].tolist()                          # identical lists: every kept prediction is a true positive
    assert tp == ref["per_view"][0, 4] > 0 and (fp, fn) == (0, 0) and ref["totals"][:3].tolist() == [tp, 0, 0]
