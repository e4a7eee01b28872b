"""
The threshold sweep of the detection scorer (include/pnyolo.h pny_detect_sweep, util.sweep_detections) restated on the host:
tests/detect_views_ref.py score_views -- stage_ref.nms_fast / tp_fp_fn_fast per view, held to the oracle by
tests/test_cpu_stage_refs.py -- looped over the settings and arranged in the sweep's layouts, with the refusal rule per
(view, confidence cut).  Everything is an integer: the comparisons are exact.

score_sweep(..., literal=True) IS that loop: one score_views call per (NMS IoU, cut, match IoU).  The default runs nms_fast once
per (list, NMS IoU, cut) and counts every match IoU on the two kept lists with tp_fp_fn_fast's arithmetic (stage_ref.iou_rows
maxima, > and < in float32); tests/test_cpu_detect_sweep.py holds the two to each other and to the oracle's own nms and tp_fp_fn.
"""
import numpy as np

import detect_views_ref as dr
import stage_ref as sr

MAX_NMS_IOUS, MAX_CUTS, MAX_MATCH_IOUS = 8, 32, 8       # the limits include/pnyolo.h states for pny_detect_sweep
COUNTS = ("tp", "fp", "fn")
LISTS = ("kept_targets", "kept_preds", "status")
TOTALS = ("tp", "fp", "fn", "refused")


def best_ious(kept_t, kept_p):
    """(best IoU of every kept prediction over the kept targets, of every kept target over the kept predictions), float32: the
    maxima of stage_ref.tp_fp_fn_fast.  Both lists non-empty."""
    return (np.array([sr.iou_rows(pb[2:], kept_t[:, 2:]).max() for pb in kept_p], np.float32),
            np.array([sr.iou_rows(tb[2:], kept_p[:, 2:]).max() for tb in kept_t], np.float32))


def counts_of_kept(kept_t, kept_p, match_iou, best=None):
    """(tp, fp, fn) of two SUPPRESSED lists at one match IoU: stage_ref.tp_fp_fn_fast behind its two nms_fast calls.
    best: best_ious(kept_t, kept_p) if the caller has them (they do not depend on the match IoU)."""
    if len(kept_t) == 0:
        return 0, len(kept_p), 0
    if len(kept_p) == 0:
        return 0, 0, len(kept_t)
    m32 = np.float32(match_iou)
    best_p, best_t = best or best_ious(kept_t, kept_p)
    tp = int((best_p > m32).sum())
    return tp, len(kept_p) - tp, int((best_t < m32).sum())


def score_sweep(target_lists, pred_lists, nms_ious, nms_ts, match_ious, max_candidates=dr.MAX_CANDIDATES, bad_views=(), literal=False):
    """-> dict(counts (V, I, T, M, 3) int32, lists (V, I, T, 3) int32, totals (I, T, M, 4) int64).
    bad_views: views whose segment the kernel refuses (BAD_SEGMENT at every setting; their lists are not looked at)."""
    V, I, T, M = len(target_lists), len(nms_ious), len(nms_ts), len(match_ious)
    assert len(pred_lists) == V and 1 <= I <= MAX_NMS_IOUS and 1 <= T <= MAX_CUTS and 1 <= M <= MAX_MATCH_IOUS
    counts = np.zeros((V, I, T, M, 3), np.int32)
    lists = np.zeros((V, I, T, 3), np.int32)
    totals = np.zeros((I, T, M, 4), np.int64)
    live = [v for v in range(V) if v not in bad_views]
    for v in bad_views:
        lists[v, :, :, 2] = dr.BAD_SEGMENT
        totals[..., 3] += 1
    if literal:
        tl, pl = [target_lists[v] for v in live], [pred_lists[v] for v in live]
        for i, iou in enumerate(nms_ious):
            for t, cut in enumerate(nms_ts):
                for m, match in enumerate(match_ious):
                    one = dr.score_views(tl, pl, iou, cut, match, max_candidates=max_candidates)
                    counts[live, i, t, m] = one["per_view"][:, :3]
                    lists[live, i, t] = one["per_view"][:, [3, 4, 7]]
                    totals[i, t, m] += one["totals"]
        return dict(counts=counts, lists=lists, totals=totals)
    done = {}                                            # a list at equal (NMS IoU, cut) -- duplicates, a list shared by views -- once

    def kept_of(b, iou, cut):
        key = (id(b), float(np.float32(iou)), float(cut))
        if key not in done:
            done[key] = dr.nms_or_empty(b, iou, cut)[0]
        return done[key]

    for v in live:
        tb, pb = target_lists[v], pred_lists[v]
        for t, cut in enumerate(nms_ts):
            status = (dr.TARGETS_OVERFLOW if dr.candidates(tb, cut) > max_candidates else 0) | \
                     (dr.PREDS_OVERFLOW if dr.candidates(pb, cut) > max_candidates else 0)
            for i, iou in enumerate(nms_ious):
                lists[v, i, t, 2] = status
                if status:
                    totals[i, t, :, 3] += 1
                    continue
                kt, kp = kept_of(tb, iou, cut), kept_of(pb, iou, cut)
                lists[v, i, t, :2] = len(kt), len(kp)
                key = (id(tb), id(pb), float(np.float32(iou)), float(cut))
                if key not in done and len(kt) and len(kp):
                    done[key] = best_ious(kt, kp)
                for m, match in enumerate(match_ious):
                    counts[v, i, t, m] = counts_of_kept(kt, kp, match, done.get(key))
                    totals[i, t, m, :3] += counts[v, i, t, m]
    return dict(counts=counts, lists=lists, totals=totals)


def table(totals):
    """(precision, recall, f1) float64 (I, T, M) of a totals array, with the reference's arithmetic (util.py:798-803) restated:
    NaN where views were refused."""
    totals = np.asarray(totals, np.int64)
    out = np.full((3,) + totals.shape[:-1], np.nan, np.float64)
    for idx in np.ndindex(*totals.shape[:-1]):
        tp, fp, fn, refused = (int(x) for x in totals[idx])
        if refused:
            continue
        precision = tp / (tp + fp) if tp + fp > 0 else 0
        recall = tp / (tp + fn) if tp + fn > 0 else 0
        f1 = 2 * (precision * recall) / (precision + recall) if precision + recall > 0 else 0
        out[(slice(None),) + idx] = precision, recall, f1
    return out


def check(got, ref, what=""):
    """A DetectionSweep read back (see read) against score_sweep's result: whichever of lists, counts and totals it holds."""
    for name in ("lists", "counts", "totals"):
        if name in got:
            assert got[name].shape == ref[name].shape and got[name].dtype == ref[name].dtype, (what, name, got[name].shape, got[name].dtype)
            bad = np.argwhere(got[name] != ref[name])
            assert len(bad) == 0, "%s: %s differ at %d places, first %s: got %s, expected %s" % (
                what, name, len(bad), bad[0].tolist(), got[name][tuple(bad[0])], ref[name][tuple(bad[0])])


def read(sweep):
    """util.DetectionSweep -> numpy (the test's read; the library never does one)."""
    return dict(counts=sweep.counts.cpu().numpy(), lists=sweep.lists.cpu().numpy(), totals=sweep.totals.cpu().numpy())
