"""
The batched detection scorer on the GPU (include/pnyolo.h pny_detect_views, util.score_detections / DetectionMeter): every
count, record, highest confidence and kept row against tests/detect_views_ref.py (stage_ref.nms_fast / tp_fp_fn_fast looped
over the views) and against the per-view path it replaces (util.convert_cells_to_bboxes + util.calculate_tp_fp_fn).  All
comparisons are exact: integers, and float32 rows bit for bit.

  * boxes form: every NMS hard case of stage_ref.nms_cases() of at most 600 boxes as one view's prediction list, all in ONE
    call, under every pair of thresholds the cases name (each case therefore also under its own); uniform4097 passes 3328
    boxes through the filters, more than PNY_DETECT_MAX_CANDIDATES = 2048, and is left to pny_nms' own sweep.  All
    match_cases() the same way;
  * lists of 255, 256, 257 and 513 candidates (the kernel's strides of 256 threads);
  * cells form: 1 and 3 scales, 1 and 3 anchors, 1 .. 16 views, against the boxes the per-image kernel decodes;
  * views without targets, without predictions, without either: their neighbours are unaffected (permutation);
  * accumulation in a DetectionMeter, reset, and identical bits from run to run;
  * a view of PNY_DETECT_MAX_CANDIDATES + 1 candidates is refused alone; one of exactly the limit is scored;
  * a metric step end to end on a rendered scene;
  * a call behind a timed spin returns while the spin runs: nothing is read.
"""
import time
import types

import numpy as np
import pytest
import torch

import detect_views_ref as dr
import stage_ref as sr
from helpers import DEV, scene_pair
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd import util as putil
from pixel_nerf_yolo_amd.render import YoloRenderer

pytestmark = pytest.mark.gpu

NMS_SMALL = {n: c for n, c in sr.nms_cases().items() if c[0].shape[0] <= 600}
NMS_THRESHOLDS = sorted({c[1:] for c in NMS_SMALL.values()})
MATCH_THRESHOLDS = sorted({c[2:] for c in sr.match_cases().values()})
FIXED_TARGETS = sr._boxes(np.random.RandomState(123), 150, size=(0.05, 0.3))
REF = {}                        # key -> detect_views_ref.score_views result: computed once, shared, never changed


def dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)


def ref_of(key, *args, **kw):
    if key not in REF:
        REF[key] = dr.score_views(*args, **kw)
    return REF[key]


def score_boxes(target_lists, pred_lists, nms_iou, nms_t, match_iou, device_offsets=False, **kw):
    pr, po = dr.segments(pred_lists)
    tr, to = dr.segments(target_lists)
    po, to = (dev(o, torch.int32) for o in (po, to)) if device_offsets else (torch.from_numpy(po), torch.from_numpy(to))
    return putil.score_detections(None, None, None, 0, 0, None, nms_iou, nms_t, match_iou, boxes=(dev(pr), po, dev(tr), to), **kw)


# --------------------------------------------------------------------------- boxes form: the hard cases
@pytest.mark.parametrize("thr", NMS_THRESHOLDS, ids=lambda t: "iou%g_conf%g" % t)
def test_boxes_form_nms_hard_cases(thr):
    names = sorted(NMS_SMALL)
    preds = [NMS_SMALL[n][0] for n in names]
    targets = [FIXED_TARGETS] * len(names)
    t0 = time.time()
    ref = ref_of(("nms", thr), targets, preds, thr[0], thr[1], 0.2)
    t_ref = time.time() - t0
    got = dr.read(score_boxes(targets, preds, thr[0], thr[1], 0.2, want_boxes=True))
    print("nms hard cases, %d views in one call, thresholds %s: kept predictions %s, totals %s (reference %.1f s)"
          % (len(names), thr, got["per_view"][:, 4].tolist(), got["totals"].tolist(), t_ref))
    dr.check(got, ref, "thresholds %s" % (thr,))
    # kept rows, counts and highest confidence are nms_fast's, case by case (what check compared, spelt out for the own thresholds)
    for v, n in enumerate(names):
        if NMS_SMALL[n][1:] == thr:
            kept, hi, above = sr.nms_fast(*NMS_SMALL[n])
            assert got["per_view"][v, 4] == len(kept) and got["per_view"][v, 6] == above, n
            assert np.array_equal(got["kept_preds"][v, :len(kept)], kept), n
            assert np.float32(hi).view(np.uint32) == got["highest_conf"][v, 1].view(np.uint32), n
    assert got["totals"][:3].tolist() == got["per_view"][:, :3].sum(0).tolist() and got["totals"][3] == 0


@pytest.mark.parametrize("thr", MATCH_THRESHOLDS, ids=lambda t: "iou%g_conf%g_match%.3g" % t)
def test_boxes_form_match_cases(thr):
    cases = sr.match_cases()
    names = sorted(cases)
    targets, preds = [cases[n][0] for n in names], [cases[n][1] for n in names]
    ref = ref_of(("match", thr), targets, preds, *thr)
    got = dr.read(score_boxes(targets, preds, *thr, want_boxes=True))
    print("match cases %s, thresholds %s: tp fp fn %s" % (names, thr, got["per_view"][:, :3].tolist()))
    dr.check(got, ref, "thresholds %s" % (thr,))
    for v, n in enumerate(names):
        if cases[n][2:] == thr:
            assert tuple(got["per_view"][v, :3].tolist()) == sr.tp_fp_fn_fast(*cases[n]), n
    if thr == cases["iou_equals_match"][2:]:
        v = names.index("iou_equals_match")           # best IoU == match_iou: neither a true positive nor a false negative
        assert got["per_view"][v, :3].tolist() == [0, 1, 0]
    if thr == cases["both_empty"][2:]:
        for n, want in (("targets_empty", lambda r: r[0] == 0 and r[1] == r[4] > 0 and r[2] == 0 and r[3] == 0),
                        ("preds_empty", lambda r: r[0] == 0 and r[1] == 0 and r[2] == r[3] > 0 and r[4] == 0),
                        ("both_empty", lambda r: r[:5] == [0] * 5)):
            assert want(got["per_view"][names.index(n)].tolist()), n


def list_of_candidates(n, seed):
    """n boxes that pass the filters, with boxes that fail them (confidence, width, height) strewn between."""
    rs = np.random.RandomState(seed)
    good = sr.clustered_boxes(n, max(1, n // 6), seed=seed)
    good[:, 1] = 0.3 + 0.7 * rs.rand(n)
    bad = sr._boxes(rs, n // 2 + 3)
    bad[0::3, 1] = 0.1
    bad[1::3, 4] = 5e-4
    bad[2::3, 5] = 2e5
    out = np.concatenate([good, bad])[rs.permutation(n + len(bad))]
    return np.ascontiguousarray(out, np.float32)


def test_candidate_counts_across_thread_strides():
    counts = (255, 256, 257, 513)
    lists = [list_of_candidates(n, 40 + i) for i, n in enumerate(counts)]
    assert [dr.candidates(b, 0.2) for b in lists] == list(counts)
    targets = lists[1:] + lists[:1]                                  # every count also as a target list, against another one
    ref = ref_of("strides", targets, lists, 0.5, 0.2, 0.3)
    got = dr.read(score_boxes(targets, lists, 0.5, 0.2, 0.3, want_boxes=True))
    print("candidates %s: records\n%s" % (counts, got["per_view"]))
    dr.check(got, ref, "strides")
    assert (got["per_view"][:, 3:5] > 1).all() and got["per_view"][:, :2].sum() > 0


# --------------------------------------------------------------------------- cells form against the per-view path
GEOMETRIES = {"one_scale_4x5x3": (4, 5, (1,), 3), "three_scales_A1": (16, 24, (2, 4, 8), 1), "three_scales_A3": (16, 24, (2, 4, 8), 3)}


def scale_anchors(n_scales, A):
    """(n_scales, A, 2): other anchors on every scale."""
    return np.stack([np.roll(sr.ANCHORS, s, axis=0)[:A] for s in range(n_scales)])


def cells_inputs(geometry, V, family, seed=0):
    H, W, cells, A = GEOMETRIES[geometry]
    preds = [sr.cells_case(H // c, W // c, A, True, family, seed=seed, batch=V) for c in cells]
    targets = [sr.cells_case(H // c, W // c, A, False, family, seed=seed, batch=V) for c in cells]
    return H, W, cells, A, preds, targets


def decode_per_view(preds, targets, anchors, H, W, cells, V):
    """The per-image kernel on every scale, concatenated per view in scale order -> (target lists, prediction lists) on the host."""
    out = []
    for arrs, is_pred in ((targets, False), (preds, True)):
        per_scale = [putil.convert_cells_to_bboxes(dev(a), torch.from_numpy(anchors[s]), H // c, W // c, is_pred, as_tensor=True).cpu().numpy()
                     for s, (a, c) in enumerate(zip(arrs, cells))]
        out.append(dr.view_lists(per_scale, V))
    return out


def score_cells(preds, targets, anchors, H, W, cells, V, thr, **kw):
    flat = lambda a: dev(a).reshape(-1, a.shape[-2], a.shape[-1])     # noqa: E731  (V, Hs, Ws, A, C) -> (V * Hs * Ws, A, C)
    return putil.score_detections([flat(a) for a in preds], [flat(a) for a in targets], torch.from_numpy(anchors), H, W, list(cells),
                                  thr[0], thr[1], thr[2], n_views=V, **kw)


@pytest.mark.parametrize("V", (1, 2, 5, 16))
@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
def test_cells_form_equals_the_per_view_path(geometry, V):
    for family in ("random", "class_ties"):
        H, W, cells, A, preds, targets = cells_inputs(geometry, V, family)
        anchors = scale_anchors(len(cells), A)
        nms_t = float(np.median(np.concatenate([p[..., 0].reshape(-1) for p in preds])))      # both lists non-trivial
        thr = (0.45, nms_t, 0.3)
        tl, pl = decode_per_view(preds, targets, anchors, H, W, cells, V)
        ref = dr.score_views(tl, pl, *thr)
        got = dr.read(score_cells(preds, targets, anchors, H, W, cells, V, thr, want_boxes=True))
        print("%s %s V=%d threshold %.4f: tp fp fn %s, kept targets %s, kept predictions %s"
              % (geometry, family, V, nms_t, got["per_view"][:, :3].tolist(), got["per_view"][:, 3].tolist(), got["per_view"][:, 4].tolist()))
        dr.check(got, ref, "%s %s V=%d" % (geometry, family, V))
        assert (got["per_view"][:, 5:7] > 0).all() and got["per_view"][:, 3:5].min() > 0, "a trivial list"
        for v in range(V):                                            # and the parent's own per-view call, reads included
            assert putil.calculate_tp_fp_fn(dev(tl[v]), dev(pl[v]), *thr) == tuple(got["per_view"][v, :3].tolist()), (family, v)


def test_views_that_differ_leave_their_neighbours_alone():
    H, W, cells, A, preds, targets = cells_inputs("three_scales_A3", 6, "random", seed=3)
    anchors = scale_anchors(len(cells), A)
    nms_t = float(np.median(np.concatenate([p[..., 0].reshape(-1) for p in preds])))
    for a in targets:
        a[1, ..., 0] = nms_t - 1.0          # view 1: no target above the threshold
        a[4, ..., 0] = nms_t - 2.0          # view 4: neither
    for a in preds:
        a[2, ..., 0] = nms_t - 1.0          # view 2: no prediction above
        a[4, ..., 0] = nms_t - 2.0
    thr = (0.45, nms_t, 0.3)
    base = dr.read(score_cells(preds, targets, anchors, H, W, cells, 6, thr, want_boxes=True))
    tl, pl = decode_per_view(preds, targets, anchors, H, W, cells, 6)
    dr.check(base, dr.score_views(tl, pl, *thr), "views that differ")
    rec = base["per_view"]
    print("views that differ: records\n%s" % rec)
    assert rec[1, 3] == 0 and rec[1, 5] == 0 and rec[1, :3].tolist() == [0, rec[1, 4], 0] and rec[1, 4] > 0
    assert rec[2, 4] == 0 and rec[2, 6] == 0 and rec[2, :3].tolist() == [0, 0, rec[2, 3]] and rec[2, 3] > 0
    assert rec[4].tolist() == [0] * 8
    assert all(rec[v, 3] > 0 and rec[v, 4] > 0 for v in (0, 3, 5))
    for perm in ([4, 0, 1, 5, 2, 3], [5, 4, 3, 2, 1, 0]):
        got = dr.read(score_cells([a[perm] for a in preds], [a[perm] for a in targets], anchors, H, W, cells, 6, thr, want_boxes=True))
        assert np.array_equal(got["per_view"], rec[perm]), perm
        assert np.array_equal(got["highest_conf"].view(np.uint32), base["highest_conf"][perm].view(np.uint32))
        for name in ("kept_targets", "kept_preds"):
            assert np.array_equal(got[name].view(np.uint32), base[name][perm].view(np.uint32)), (perm, name)
        assert np.array_equal(got["totals"], base["totals"])


# --------------------------------------------------------------------------- the meter
def test_meter_accumulates_resets_and_repeats_bit_for_bit():
    thr = (0.45, 0.0, 0.3)
    calls = []
    for geometry, V, family, seed in (("three_scales_A3", 5, "random", 1), ("one_scale_4x5x3", 2, "class_ties", 2)):
        H, W, cells, A, preds, targets = cells_inputs(geometry, V, family, seed=seed)
        calls.append(([dev(p).reshape(-1, A, 7) for p in preds], [dev(t).reshape(-1, A, 6) for t in targets],
                      torch.from_numpy(scale_anchors(len(cells), A)), H, W, list(cells), V))
    meter = putil.DetectionMeter(DEV)
    assert meter.report() == (0, 0, 0)

    def both():
        return [meter.update(p, t, anc, H, W, cells, *thr, n_views=V, want_boxes=True) for p, t, anc, H, W, cells, V in calls]

    ra, rb = both()
    assert ra.totals is meter.totals and rb.totals is meter.totals
    first = [dr.read(ra), dr.read(rb)]
    want = first[0]["per_view"][:, :3].sum(0) + first[1]["per_view"][:, :3].sum(0)
    assert want.sum() > 0 and meter.report() == tuple(want.tolist())
    p, r, f1 = meter.report(prf=True)
    assert (p, r, f1) == putil.calculate_precision_recall_f1(*want.tolist())
    both()                                                               # a second pass without a reset: twice the sums
    assert meter.report() == tuple((2 * want).tolist())
    meter.reset()
    assert meter.report() == (0, 0, 0)
    again = [dr.read(r) for r in both()]
    assert meter.report() == tuple(want.tolist())
    for x, y in zip(first, again):
        for name in ("per_view", "highest_conf", "kept_targets", "kept_preds"):
            assert np.array_equal(x[name].view(np.uint32), y[name].view(np.uint32)), name


# --------------------------------------------------------------------------- the limit
def test_overflow_is_refused_for_that_view_alone():
    n = plib.DETECT_MAX_CANDIDATES
    over = sr.clustered_boxes(n + 1, 100, seed=11)
    full = sr.clustered_boxes(n, 100, seed=12)
    over[:, 1] = 0.3 + 0.6 * over[:, 1]
    full[:, 1] = 0.3 + 0.6 * full[:, 1]
    assert dr.candidates(over, 0.2) == n + 1 and dr.candidates(full, 0.2) == n
    normal = [sr.clustered_boxes(200, 20, seed=13 + i) for i in range(3)]
    preds = [normal[0], over, normal[1], full, normal[2]]
    targets = [normal[1], normal[2], over, normal[0], full]
    ref = ref_of("overflow", targets, preds, 0.5, 0.2, 0.3)
    meter = putil.DetectionMeter(DEV)
    pr, po = dr.segments(preds)
    tr, to = dr.segments(targets)
    scores = meter.update(None, None, None, 0, 0, None, 0.5, 0.2, 0.3, boxes=(dev(pr), torch.from_numpy(po), dev(tr), torch.from_numpy(to)),
                          want_boxes=True)
    got = dr.read(scores)
    print("overflow: records\n%s\ntotals %s" % (got["per_view"], got["totals"]))
    assert got["per_view"][:, 7].tolist() == [0, plib.DETECT_PREDS_OVERFLOW, plib.DETECT_TARGETS_OVERFLOW, 0, 0]
    assert got["per_view"][1:3, :5].tolist() == [[0] * 5] * 2            # refused: nothing counted, nothing kept
    assert got["per_view"][1, 6] == n + 1 and got["per_view"][2, 5] == n + 1
    dr.check(got, ref, "overflow")                                       # the other views are exact, the full one included
    assert got["totals"].tolist() == got["per_view"][[0, 3, 4], :3].sum(0).tolist() + [1 + 1]
    with pytest.raises(plib.PnyError, match="2 views were refused"):
        meter.report()
    meter.reset()
    # the issue's case: ONE view over the limit among normal ones; the error word is 1
    one = meter.update(None, None, None, 0, 0, None, 0.5, 0.2, 0.3,
                       boxes=(dev(pr), torch.from_numpy(po[:3]), dev(tr), dev(np.array([0, 200, 400], np.int32), torch.int32)))
    got1 = dr.read(one)
    assert got1["per_view"][:, 7].tolist() == [0, plib.DETECT_PREDS_OVERFLOW] and got1["totals"][3] == 1
    assert got1["per_view"][0].tolist() == got["per_view"][0].tolist()
    assert got1["totals"][:3].tolist() == got1["per_view"][0, :3].tolist()
    with pytest.raises(plib.PnyError, match="1 view was refused"):
        meter.report()


def test_segments_given_on_the_device_are_checked_by_the_kernel():
    lists = [sr.clustered_boxes(60, 8, seed=21 + i) for i in range(3)]
    ref = ref_of("segments", lists[::-1], lists, 0.5, 0.2, 0.3)
    got = dr.read(score_boxes(lists[::-1], lists, 0.5, 0.2, 0.3, device_offsets=True, want_boxes=True))
    dr.check(got, ref, "device offsets")
    rows = dev(np.concatenate(lists))
    good = dev(np.array([0, 60, 120, 180], np.int32), torch.int32)
    for bad in ([0, 60, 50, 180], [0, 60, 120, 181], [-1, 60, 120, 180]):
        s = dr.read(putil.score_detections(None, None, None, 0, 0, None, 0.5, 0.2, 0.3,
                                           boxes=(rows, dev(np.array(bad, np.int32), torch.int32), rows, good)))
        want = [plib.DETECT_BAD_SEGMENT if (b0 < 0 or b1 < b0 or b1 > 180) else 0 for b0, b1 in zip(bad, bad[1:])]
        assert s["per_view"][:, 7].tolist() == want and s["totals"][3] == sum(1 for w in want if w), (bad, s["per_view"])
        assert all(s["per_view"][v, :5].tolist() == [0] * 5 for v in range(3) if want[v])


# --------------------------------------------------------------------------- end to end
def test_metric_step_end_to_end_equals_the_per_view_loop(golden):
    import yolo_batch_ref as yb
    k = yb.fixture_case(golden("yolo_train_batch"), "a")                 # 5 cameras of a 40 x 56 image; 3 views, scales 5 x 7 and 2 x 3
    A, K, cells, V = k["A"], 16, k["cells"][:2], len(k["views"])
    H, W = k["H"], k["W"]
    net, _ = scene_pair(2, 64, 64, 1792, 7 * A, 5, 3, 2300, yolo=True, lat_hw=(8, 8))
    net.eval()
    ren = YoloRenderer(K, 128, len(cells), A)
    ren.bind_parallel(net)
    rs = np.random.RandomState(2301)
    grids = []
    for c in cells:
        shape = (k["NV"], H // c, W // c, A)
        t = np.zeros(shape + (6,), np.float32)
        u = rs.rand(*shape)
        t[..., 0] = np.where(u < 0.3, 1.0, np.where(u < 0.4, -1.0, 0.0))
        t[..., 1:3] = rs.uniform(0, 1, size=shape + (2,))
        t[..., 3:5] = rs.uniform(0.3, 2.5, size=shape + (2,))
        t[..., 5] = rs.randint(0, 2, size=shape)
        grids.append(dev(t))
    rays, target_cells = putil.yolo_train_batch(torch.from_numpy(k["poses"]), k["views"], k["focal"], k["c"], grids, H, W, cells, *k["z"])
    n_rays = sum(r.shape[0] for r in rays)
    ren.draws = dict(u_coarse=rs.rand(n_rays, K).astype(np.float32))
    with torch.no_grad():
        render = ren(rays[0]._base).reshape(n_rays, A, 7)                # ONE render of all rays of all scales and views
    off = np.cumsum([0] + [r.shape[0] for r in rays])
    preds = [render[a:b] for a, b in zip(off, off[1:])]
    anchors = rs.uniform(0.5, 3.0, size=(len(cells), A, 2)).astype(np.float32)
    nms_t = float(render[..., 0].median())
    thr = (0.45, nms_t, 0.3)
    scores = putil.score_detections(preds, target_cells, torch.from_numpy(anchors), H, W, cells, *thr, n_views=V, want_boxes=True)
    got = dr.read(scores)
    # the parent's way on the same render: per scale convert_cells_to_bboxes, per view calculate_tp_fp_fn
    boxes = []
    for arrs, is_pred in ((target_cells, False), (preds, True)):
        per_scale = [putil.convert_cells_to_bboxes(a.reshape(V, H // c, W // c, A, -1), torch.from_numpy(anchors[s]), H // c, W // c, is_pred,
                                                   as_tensor=True) for s, (a, c) in enumerate(zip(arrs, cells))]
        boxes.append(torch.cat(per_scale, dim=1))
    want = [putil.calculate_tp_fp_fn(boxes[0][v], boxes[1][v], *thr) for v in range(V)]
    print("end to end: threshold %.4f (median rendered score), per view tp fp fn %s, kept targets %s, kept predictions %s"
          % (nms_t, got["per_view"][:, :3].tolist(), got["per_view"][:, 3].tolist(), got["per_view"][:, 4].tolist()))
    assert [tuple(r) for r in got["per_view"][:, :3].tolist()] == want
    dr.check(got, dr.score_views(list(boxes[0].cpu().numpy()), list(boxes[1].cpu().numpy()), *thr), "end to end")
    assert got["totals"][0] + got["totals"][1] > 0 and got["per_view"][:, 3].sum() > 0, "a vacuous case"
    assert got["totals"][:3].tolist() == np.array(want).sum(0).tolist()


# --------------------------------------------------------------------------- no read
def test_update_returns_while_a_spin_holds_its_stream():
    """The device of tests/test_gpu_streams.py: a timed spin on the stream, the call enqueued behind it, and the spin's event
    still pending when the call has returned -- a call that read a result would have waited for the spin."""
    from test_gpu_streams import Window
    H, W, cells, A, preds, targets = cells_inputs("three_scales_A3", 9, "random", seed=5)
    anchors = torch.from_numpy(scale_anchors(len(cells), A))
    p = [dev(a).reshape(-1, A, 7) for a in preds]
    t = [dev(a).reshape(-1, A, 6) for a in targets]
    side = torch.cuda.Stream(DEV)
    meter = putil.DetectionMeter(DEV)
    with torch.cuda.stream(side):
        warm = dr.read(meter.update(p, t, anchors, H, W, list(cells), 0.45, 0.0, 0.3, n_views=9, want_boxes=True))   # code object, LDS limit, allocator
        meter.reset()
    window = Window(types.SimpleNamespace(s1=side, s2=side, s3=side, s4=side))
    window.spin(side)
    with torch.cuda.stream(side):
        scores = meter.update(p, t, anchors, H, W, list(cells), 0.45, 0.0, 0.3, n_views=9, want_boxes=True)
    window.close("score_detections")                                     # asserts that the spin was still running
    got = dr.read(scores)
    for name in ("per_view", "highest_conf", "kept_targets", "kept_preds", "totals"):
        assert np.array_equal(got[name].view(np.uint32) if got[name].dtype == np.float32 else got[name],
                              warm[name].view(np.uint32) if warm[name].dtype == np.float32 else warm[name]), name
    assert got["totals"][:3].sum() > 0
