"""
The threshold sweep of the detection scorer on the GPU (include/pnyolo.h pny_detect_sweep, util.sweep_detections /
DetectionSweepMeter): every count, kept count, status and total against tests/detect_sweep_ref.py (detect_views_ref.score_views
over the settings, held to the oracle by tests/test_cpu_detect_sweep.py) and, setting by setting, against the one-setting
kernel it shares its device code with (util.score_detections).  All comparisons are of integers: exact.

  * boxes form: the NMS hard cases of stage_ref.nms_cases() of at most 600 boxes, one per view, at 3 x 8 x 3 settings whose cuts
    are unsorted, hold a duplicate, two values EQUAL to a confidence of a list (the strict >) and one at 1.0 (nothing passes);
  * stage_ref.match_cases(), one per view, at their own thresholds and one more of each, 4 match IoUs;
  * cells form: 1 and 3 scales, 1 and 5 views, against the boxes the per-image kernel decodes;
  * 512 workgroups (more than the 256 CUs), and the same bits from a second call;
  * a view over the candidate limit at one cut and under it at another: refused at the one, scored at the other;
  * accumulation in a DetectionSweepMeter, reset, best();
  * a bad segment given on the device: that view alone, at every setting;
  * an update behind a timed spin returns while the spin runs: nothing is read.
"""
import time

import numpy as np
import pytest
import torch

import detect_sweep_ref as ds
import detect_views_ref as dr
import stage_ref as sr
from helpers import DEV
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd import util as putil

pytestmark = pytest.mark.gpu

NMS_SMALL = {n: c for n, c in sr.nms_cases().items() if c[0].shape[0] <= 600}
FIXED_TARGETS = sr._boxes(np.random.RandomState(123), 150, size=(0.05, 0.3))        # the targets of test_gpu_detect_views.py
F32 = lambda x: float(np.float32(x))                                                # noqa: E731
REF = {}                        # key -> detect_sweep_ref.score_sweep result: computed once, shared, never changed
SPIN_CYCLES, SPIN = 20_000_000, 5   # torch.cuda._sleep: ~10 ms of one wave per SPIN_CYCLES (tests/test_gpu_trunk.py, test_gpu_streams.py)


def dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)


def ref_of(key, *args, **kw):
    if key not in REF:
        t0 = time.time()
        REF[key] = ds.score_sweep(*args, **kw)
        print("reference %s: %.1f s on the host" % (key, time.time() - t0))
    return REF[key]


def box_inputs(target_lists, pred_lists, device_offsets=False):
    pr, po = dr.segments(pred_lists)
    tr, to = dr.segments(target_lists)
    po, to = (dev(o, torch.int32) for o in (po, to)) if device_offsets else (torch.from_numpy(po), torch.from_numpy(to))
    return dev(pr), po, dev(tr), to


def sweep_boxes(target_lists, pred_lists, nms_ious, nms_ts, match_ious, **kw):
    return putil.sweep_detections(None, None, None, 0, 0, None, nms_ious, nms_ts, match_ious, boxes=box_inputs(target_lists, pred_lists), **kw)


def equals_the_one_setting_kernel(got, target_lists, pred_lists, nms_ious, nms_ts, match_ious):
    """Setting by setting: util.score_detections on the device at the same three numbers gives the same tp, fp, fn, kept counts
    and status."""
    b = box_inputs(target_lists, pred_lists)
    for i, iou in enumerate(nms_ious):
        for t, cut in enumerate(nms_ts):
            for m, match in enumerate(match_ious):
                one = putil.score_detections(None, None, None, 0, 0, None, iou, cut, match, boxes=b).per_view.cpu().numpy()
                assert np.array_equal(one[:, :3], got["counts"][:, i, t, m]), (iou, cut, match)
                assert np.array_equal(one[:, [3, 4, 7]], got["lists"][:, i, t]), (iou, cut, match)


# --------------------------------------------------------------------------- boxes form: the hard cases
def test_boxes_form_nms_hard_cases():
    names = sorted(NMS_SMALL)
    preds = [NMS_SMALL[n][0] for n in names]
    targets = [FIXED_TARGETS] * len(names)
    eq_a, eq_b = F32(NMS_SMALL["equal_conf600"][0][0, 1]), F32(NMS_SMALL["threshold_edges"][0][0, 1])
    assert eq_a == F32(0.7) and eq_b == F32(0.3) and (NMS_SMALL["threshold_edges"][0][:, 1] == np.float32(0.3)).sum() == 32
    nms_ious, match_ious = (0.3, 0.5, 0.75), (0.2, 0.3, 0.5)
    nms_ts = (0.2, eq_a, 0.5, 0.1, 1.0, eq_b, 0.2, 0.45)              # unsorted, 0.2 twice, two equal to a confidence, one >= 1
    ref = ref_of("nms", targets, preds, nms_ious, nms_ts, match_ious)
    got = ds.read(sweep_boxes(targets, preds, nms_ious, nms_ts, match_ious))
    print("nms hard cases, %d views x 3 x 8 x 3 settings: totals at nms_iou 0.5, match_iou 0.2 per cut\n%s" % (len(names), got["totals"][1, :, 0]))
    ds.check(got, ref, "nms hard cases")
    v = names.index("equal_conf600")                                   # 600 boxes AT the cut: none is above it
    assert (got["lists"][v, :, 1, 1] == 0).all() and (got["lists"][v, :, 2, 1] > 0).all()
    v = names.index("threshold_edges")                                 # the 32 boxes at 0.3f are not above 0.3f; they are above 0.3
    assert (got["lists"][v, :, 5, 1] == 0).all() and (got["lists"][v, :, 0, 1] > 0).all()
    assert not got["lists"][:, :, 4, :2].any() and not got["counts"][:, :, 4].any()        # cut 1.0: nothing passes
    no_t = got["lists"][..., 0] == 0
    assert np.array_equal(got["counts"][no_t][..., 1], np.repeat(got["lists"][no_t][:, 1:2], 3, axis=1)) and not got["counts"][no_t][..., [0, 2]].any()
    assert np.array_equal(got["counts"][:, :, 0], got["counts"][:, :, 6]) and np.array_equal(got["totals"][:, 0], got["totals"][:, 6])
    assert np.array_equal(got["totals"][..., :3], got["counts"].sum(0)) and not got["totals"][..., 3].any()
    assert got["counts"][..., 0].max() > 0 and (got["totals"][0] != got["totals"][2]).any() and (got["totals"][:, :, 0] != got["totals"][:, :, 2]).any()
    equals_the_one_setting_kernel(got, targets, preds, nms_ious, nms_ts, match_ious)


def test_boxes_form_match_cases():
    cases = sr.match_cases()
    names = sorted(cases)
    targets, preds = [cases[n][0] for n in names], [cases[n][1] for n in names]
    own_iou, own_t, own_m = (sorted({c[k] for c in cases.values()}) for k in (2, 3, 4))
    nms_ious, nms_ts = tuple(own_iou) + (0.4,), tuple(own_t) + (0.3,)
    match_ious = tuple(own_m) + (0.5,)
    assert len(match_ious) == 4 and len(nms_ious) == 2 and len(nms_ts) == 3
    ref = ref_of("match", targets, preds, nms_ious, nms_ts, match_ious)
    got = ds.read(sweep_boxes(targets, preds, nms_ious, nms_ts, match_ious))
    ds.check(got, ref, "match cases")
    for v, n in enumerate(names):                                      # each case under its own thresholds: tp_fp_fn_fast's counts
        i, t, m = nms_ious.index(cases[n][2]), nms_ts.index(cases[n][3]), match_ious.index(cases[n][4])
        assert tuple(got["counts"][v, i, t, m].tolist()) == sr.tp_fp_fn_fast(*cases[n]), n
    v, c = names.index("iou_equals_match"), cases["iou_equals_match"]  # best IoU == match_iou: neither a true positive nor a false negative
    assert got["counts"][v, 0, nms_ts.index(c[3]), match_ious.index(c[4])].tolist() == [0, 1, 0]
    assert got["counts"][v, 0, nms_ts.index(c[3]), 0].tolist() == [1, 0, 0]                 # and below it, a true positive
    t5 = nms_ts.index(0.5)
    for n, want in (("targets_empty", lambda r, k: r == [0, k[1], 0] and k[0] == 0 and k[1] > 0),
                    ("preds_empty", lambda r, k: r == [0, 0, k[0]] and k[1] == 0 and k[0] > 0), ("both_empty", lambda r, k: r == [0, 0, 0])):
        v = names.index(n)
        assert all(want(got["counts"][v, 0, t5, m].tolist(), got["lists"][v, 0, t5].tolist()) for m in range(4)), n
    equals_the_one_setting_kernel(got, targets, preds, nms_ious, nms_ts, match_ious)


# --------------------------------------------------------------------------- cells form
GEOMETRIES = {"one_scale_4x5x3": (4, 5, (1,), 3), "three_scales_A3": (16, 24, (2, 4, 8), 3)}


def scale_anchors(n_scales, A):
    """(n_scales, A, 2): other anchors on every scale."""
    return np.stack([np.roll(sr.ANCHORS, s, axis=0)[:A] for s in range(n_scales)])


def cells_inputs(geometry, V, family="random", seed=0):
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


def cells_args(geometry, V, seed=0):
    H, W, cells, A, preds, targets = cells_inputs(geometry, V, seed=seed)
    anchors = scale_anchors(len(cells), A)
    flat = lambda a: dev(a).reshape(-1, a.shape[-2], a.shape[-1])     # noqa: E731  (V, Hs, Ws, A, C) -> (V * Hs * Ws, A, C)
    tl, pl = decode_per_view(preds, targets, anchors, H, W, cells, V)
    scores = np.concatenate([p[..., 0].reshape(-1) for p in preds])
    args = ([flat(a) for a in preds], [flat(a) for a in targets], torch.from_numpy(anchors), H, W, list(cells))
    return args, tl, pl, scores


@pytest.mark.parametrize("V", (1, 5))
@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
def test_cells_form(geometry, V):
    args, tl, pl, scores = cells_args(geometry, V)
    nms_ts = tuple(float(np.quantile(scores, q)) for q in (0.5, 0.25, 0.8, 0.65))       # every list non-trivial at every cut
    nms_ious, match_ious = (0.45, 0.7), (0.3, 0.1)
    ref = ds.score_sweep(tl, pl, nms_ious, nms_ts, match_ious)
    got = ds.read(putil.sweep_detections(*args, nms_ious, nms_ts, match_ious, n_views=V))
    print("%s V=%d: totals per cut at nms_iou 0.45, match_iou 0.3\n%s" % (geometry, V, got["totals"][0, :, 0]))
    ds.check(got, ref, "%s V=%d" % (geometry, V))
    assert got["lists"][..., :2].min() > 0 and not got["lists"][..., 2].any(), "a trivial list"
    one = putil.score_detections(*args, nms_ious[1], nms_ts[2], match_ious[0], n_views=V).per_view.cpu().numpy()
    assert np.array_equal(one[:, :3], got["counts"][:, 1, 2, 0]) and np.array_equal(one[:, [3, 4, 7]], got["lists"][:, 1, 2])


# --------------------------------------------------------------------------- more workgroups than compute units
def test_more_workgroups_than_compute_units_and_the_same_bits_twice():
    V, nms_ious = 16, (0.3, 0.45, 0.6, 0.75)
    nms_ts = (0.05, 0.15, 0.25, 0.35, 0.45, 0.55, 0.65, 0.75)
    match_ious = (0.2, 0.5)
    preds = [sr.clustered_boxes(100 + v, 10 + v, seed=60 + v) for v in range(V)]
    targets = [sr.clustered_boxes(90 + v, 10 + v, seed=80 + v) for v in range(V)]
    assert V * len(nms_ious) * len(nms_ts) == 512 > torch.cuda.get_device_properties(DEV).multi_processor_count
    ref = ref_of("512", targets, preds, nms_ious, nms_ts, match_ious)
    first = sweep_boxes(targets, preds, nms_ious, nms_ts, match_ious)
    got = ds.read(first)
    ds.check(got, ref, "512 workgroups")
    assert got["totals"][..., 0].min() > 0 and got["totals"][..., 2].max() > 0 and (got["lists"][..., :2] > 0).all()
    again = ds.read(sweep_boxes(targets, preds, nms_ious, nms_ts, match_ious))
    for name in ("counts", "lists", "totals"):
        assert np.array_equal(got[name], again[name]), name


# --------------------------------------------------------------------------- the limit, per setting
def test_refusal_is_per_setting():
    n = plib.DETECT_MAX_CANDIDATES
    big = sr.clustered_boxes(2100, 100, seed=11)
    rs = np.random.RandomState(12)
    big[:, 1] = np.where(np.arange(2100) < 1500, 0.15 + 0.4 * rs.rand(2100), 0.65 + 0.3 * rs.rand(2100)).astype(np.float32)
    big = np.ascontiguousarray(big[rs.permutation(2100)])
    assert dr.candidates(big, 0.1) == 2100 > n and dr.candidates(big, 0.6) == 600
    normal = [sr.clustered_boxes(200, 20, seed=13 + i) for i in range(3)]
    preds = [normal[0], big, normal[1]]
    targets = [normal[1], normal[2], normal[0]]
    nms_ious, nms_ts, match_ious = (0.5, 0.7), (0.1, 0.6), (0.2, 0.3, 0.5)
    ref = ref_of("overflow", targets, preds, nms_ious, nms_ts, match_ious)
    got = ds.read(sweep_boxes(targets, preds, nms_ious, nms_ts, match_ious))
    print("refusal per setting: lists of the big view\n%s\ntotals\n%s" % (got["lists"][1], got["totals"]))
    assert got["lists"][:, :, 0, 2].tolist() == [[0, 0], [plib.DETECT_PREDS_OVERFLOW] * 2, [0, 0]]     # at 0.1: that view alone
    assert not got["lists"][:, :, 1, 2].any()                                                            # at 0.6: scored
    assert not got["counts"][1, :, 0].any() and not got["lists"][1, :, 0, :2].any()
    assert (got["totals"][:, 0, :, 3] == 1).all() and (got["totals"][:, 1, :, 3] == 0).all()
    assert (got["lists"][1, :, 1, :2] > 0).all() and got["counts"][1, :, 1].sum() > 0
    assert (got["lists"][[0, 2]][..., :2] > 0).all()                                                     # the neighbours, at both cuts
    assert np.array_equal(got["totals"][..., :3], got["counts"].sum(0))
    ds.check(got, ref, "refusal per setting")
    meter = putil.DetectionSweepMeter(DEV, nms_ious, nms_ts, match_ious)
    meter.update(None, None, None, 0, 0, None, boxes=box_inputs(targets, preds))
    rep = meter.report()
    assert np.isnan(rep.f1[:, 0]).all() and not np.isnan(rep.f1[:, 1]).any() and rep.best()[1] == 0.6


# --------------------------------------------------------------------------- the meter
def test_meter_accumulates_resets_and_picks_the_best():
    nms_ious, nms_ts, match_ious = (0.45, 0.7), (0.3, 0.5, 0.1), (0.2, 0.4)
    calls, refs = [], []
    for seed, V in ((1, 4), (2, 3)):
        preds = [sr.clustered_boxes(120, 12, seed=100 * seed + v) for v in range(V)]
        targets = [sr.clustered_boxes(80, 12, seed=100 * seed + 50 + v, jitter=0.05) for v in range(V)]
        calls.append(box_inputs(targets, preds))
        refs.append(ds.score_sweep(targets, preds, nms_ious, nms_ts, match_ious))
    meter = putil.DetectionSweepMeter(DEV, nms_ious, nms_ts, match_ious)
    assert meter.totals.shape == (2, 3, 2, 4) and not meter.report().tp.any()

    def both():
        return [meter.update(None, None, None, 0, 0, None, boxes=b) for b in calls]

    first = both()
    assert all(s.totals is meter.totals for s in first) and first[0].nms_ts == nms_ts
    want = refs[0]["totals"] + refs[1]["totals"]
    rep = meter.report()
    assert np.array_equal(np.stack([rep.tp, rep.fp, rep.fn, rep.refused], -1), want) and want[..., :3].min() >= 0 and want[..., 0].max() > 0
    for s, r in zip(first, refs):
        ds.check(dict(counts=s.counts.cpu().numpy(), lists=s.lists.cpu().numpy()), r, "meter update")
    p, r, f1 = ds.table(want)
    assert np.array_equal(rep.f1.view(np.uint64), f1.view(np.uint64)) and np.array_equal(rep.precision.view(np.uint64), p.view(np.uint64))
    i, t, m = np.unravel_index(int(np.argmax(f1)), f1.shape)
    assert rep.best() == (nms_ious[i], nms_ts[t], match_ious[m], p[i, t, m], r[i, t, m], f1[i, t, m]) and f1[i, t, m] > 0
    bits = [ds.read(s) for s in first]
    meter.reset()
    assert not meter.report().tp.any() and not meter.report().refused.any()
    again = [ds.read(s) for s in both()]
    assert np.array_equal(again[1]["totals"], want)
    for x, y in zip(bits, again):
        assert np.array_equal(x["counts"], y["counts"]) and np.array_equal(x["lists"], y["lists"])


# --------------------------------------------------------------------------- segments checked by the kernel
def test_bad_segment_on_the_device_refuses_that_view_at_every_setting():
    lists = [sr.clustered_boxes(60, 8, seed=21 + i) for i in range(3)]
    nms_ious, nms_ts, match_ious = (0.5, 0.3), (0.2, 0.5, 0.35), (0.3, 0.2)
    rows = dev(np.concatenate(lists))
    good = dev(np.array([0, 60, 120, 180], np.int32), torch.int32)
    ok = ds.read(putil.sweep_detections(None, None, None, 0, 0, None, nms_ious, nms_ts, match_ious, boxes=(rows, good, rows, good)))
    ds.check(ok, ref_of("segments", lists, lists, nms_ious, nms_ts, match_ious), "device offsets")
    for bad, which in (([0, 60, 50, 180], (1,)), ([0, 60, 120, 181], (2,)), ([-1, 60, 120, 180], (0,))):
        got = ds.read(putil.sweep_detections(None, None, None, 0, 0, None, nms_ious, nms_ts, match_ious,
                                             boxes=(rows, dev(np.array(bad, np.int32), torch.int32), rows, good)))
        v = which[0]
        if bad[1:3] == [60, 50]:                 # view 2 now owns rows [50, 180): its segment is good, its list another one
            others = [0]
        else:
            others = [u for u in range(3) if u != v]
        assert (got["lists"][v, :, :, 2] == plib.DETECT_BAD_SEGMENT).all() and not got["lists"][v, :, :, :2].any() and not got["counts"][v].any(), bad
        assert (got["totals"][..., 3] == 1).all(), bad
        for u in others:
            assert np.array_equal(got["counts"][u], ok["counts"][u]) and np.array_equal(got["lists"][u], ok["lists"][u]), (bad, u)
        assert np.array_equal(got["totals"][..., :3], got["counts"].sum(0))


# --------------------------------------------------------------------------- no read
def test_update_returns_while_a_spin_holds_its_stream():
    """The device of tests/test_gpu_streams.py, restated: a timed spin on the stream, the update enqueued behind it, and the spin's
    event still pending when the update has returned -- a call that read a result, or waited, would have outlasted the spin.
    The spin ends by itself."""
    args, _, _, scores = cells_args("three_scales_A3", 9, seed=5)
    nms_ts = tuple(float(np.quantile(scores, q)) for q in (0.3, 0.6, 0.9))
    side = torch.cuda.Stream(DEV)
    meter = putil.DetectionSweepMeter(DEV, (0.45, 0.7), nms_ts, (0.3, 0.5))
    with torch.cuda.stream(side):
        warm = ds.read(meter.update(*args, n_views=9))                   # code object, LDS limit, allocator
        meter.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.cuda.stream(side):
        torch.cuda._sleep(SPIN * SPIN_CYCLES)
        event = torch.cuda.Event()
        event.record(side)
        sweep = meter.update(*args, n_views=9)
    pending = not event.query()
    host_ms = 1e3 * (time.perf_counter() - t0)
    torch.cuda.synchronize()
    print("sweep update enqueued in %.2f ms of host time, inside a spin of %d x SPIN_CYCLES" % (host_ms, SPIN))
    assert pending, "the spin had ended when update returned (host time %.2f ms): the call waited for the device" % host_ms
    got = ds.read(sweep)
    for name in ("counts", "lists", "totals"):
        assert np.array_equal(got[name], warm[name]), name
    assert got["totals"][..., :3].sum() > 0
