"""
The batched detection scorer (include/pnyolo.h pny_detect_views, util.score_detections) restated on the host: the per-view
reference of tests/stage_ref.py (nms_fast, tp_fp_fn_fast: proven equal to the oracle and to the reference's captured outputs,
tests/test_cpu_stage_refs.py) looped over the views, a view's list being its boxes of every scale in turn.  Everything is an
integer or a copied float32: the comparisons are exact.
"""
import numpy as np

import stage_ref as sr

MAX_CANDIDATES = 2048            # PNY_DETECT_MAX_CANDIDATES
RECORD = ("tp", "fp", "fn", "kept_targets", "kept_preds", "targets_above", "preds_above", "status")
TARGETS_OVERFLOW, PREDS_OVERFLOW, BAD_SEGMENT = 1, 2, 4


def segments(lists):
    """A list of (n_v, 6) arrays -> (rows (sum n_v, 6) float32, offsets (V + 1) int32)."""
    lists = [np.asarray(b, np.float32).reshape(-1, 6) for b in lists]
    off = np.zeros(len(lists) + 1, np.int32)
    off[1:] = np.cumsum([len(b) for b in lists])
    return (np.concatenate(lists) if lists else np.zeros((0, 6), np.float32)), off


def view_lists(boxes_per_scale, n_views):
    """Decoded boxes per scale, each (n_views, Hs * Ws * A, 6) in the (y, x, anchor) order of convert_cells_to_bboxes -> one
    (sum_s Hs Ws A, 6) list per view: scales in order."""
    per_scale = [np.asarray(b, np.float32).reshape(n_views, -1, 6) for b in boxes_per_scale]
    return [np.concatenate([b[v] for b in per_scale]) for v in range(n_views)]


def candidates(boxes, threshold):
    """Boxes that pass nms()'s confidence and size filters (what the kernel holds in LDS)."""
    b = np.asarray(boxes, np.float32).reshape(-1, 6)
    return int(len(sr._filter_sort(b, threshold)[0])) if len(b) else 0


def nms_or_empty(boxes, iou_t, conf_t):
    """nms_fast, and for an empty list what pny_nms gives (n == 0: nothing kept, -inf, 0)."""
    b = np.asarray(boxes, np.float32).reshape(-1, 6)
    if len(b) == 0:
        return b, float("-inf"), 0
    return sr.nms_fast(b, iou_t, conf_t)


def score_views(target_lists, pred_lists, nms_iou, nms_t, match_iou, max_candidates=MAX_CANDIDATES, tp_fp_fn=None):
    """-> dict(per_view (V, 8) int32, highest_conf (V, 2) float32, totals (4,) int64, kept_targets, kept_preds: lists of (k, 6)).
    tp_fp_fn: the per-view counter (default stage_ref.tp_fp_fn_fast; the CPU test passes the oracle's)."""
    tp_fp_fn = tp_fp_fn or sr.tp_fp_fn_fast
    V = len(target_lists)
    assert len(pred_lists) == V
    rec = np.zeros((V, len(RECORD)), np.int32)
    hc = np.zeros((V, 2), np.float32)
    totals = np.zeros(4, np.int64)
    kept_t, kept_p = [], []
    for v, (t, p) in enumerate(zip(target_lists, pred_lists)):
        kt, hc[v, 0], rec[v, 5] = nms_or_empty(t, nms_iou, nms_t)
        kp, hc[v, 1], rec[v, 6] = nms_or_empty(p, nms_iou, nms_t)
        status = (TARGETS_OVERFLOW if candidates(t, nms_t) > max_candidates else 0) | \
                 (PREDS_OVERFLOW if candidates(p, nms_t) > max_candidates else 0)
        rec[v, 7] = status
        if status:
            totals[3] += 1
            kept_t.append(np.zeros((0, 6), np.float32))
            kept_p.append(np.zeros((0, 6), np.float32))
            continue
        if len(t) and len(p):
            rec[v, :3] = tp_fp_fn(t, p, nms_iou, nms_t, match_iou)
        else:                                   # an empty list: nms() of nothing keeps nothing (util.py:779-785 on the rest)
            rec[v, :3] = (0, len(kp), 0) if len(kt) == 0 else (0, 0, len(kt))
        rec[v, 3], rec[v, 4] = len(kt), len(kp)
        totals[:3] += rec[v, :3]
        kept_t.append(kt)
        kept_p.append(kp)
    return dict(per_view=rec, highest_conf=hc, totals=totals, kept_targets=kept_t, kept_preds=kept_p)


def check(got, ref, what=""):
    """A DetectionScores read back (see read) against score_views' result: records, highest confidences (bits), totals, kept rows."""
    assert np.array_equal(got["per_view"], ref["per_view"]), "%s: records\n%s\nexpected\n%s" % (what, got["per_view"], ref["per_view"])
    assert np.array_equal(got["highest_conf"].view(np.uint32), ref["highest_conf"].view(np.uint32)), what + ": highest confidence"
    if "totals" in got:
        assert np.array_equal(got["totals"], ref["totals"]), "%s: totals %s, expected %s" % (what, got["totals"], ref["totals"])
    for name, col in (("kept_targets", 3), ("kept_preds", 4)):
        if got.get(name) is None:
            continue
        for v, want in enumerate(ref[name]):
            have = got[name][v, :len(want)]
            assert have.shape == want.shape and np.array_equal(have.view(np.uint32), want.view(np.uint32)), \
                "%s: %s of view %d" % (what, name, v)


def read(scores):
    """util.DetectionScores -> numpy (the test's read; the library never does one)."""
    out = dict(per_view=scores.per_view.cpu().numpy(), highest_conf=scores.highest_conf.cpu().numpy(),
               totals=scores.totals.cpu().numpy())
    for name in ("kept_targets", "kept_preds"):
        t = getattr(scores, name)
        out[name] = None if t is None else t.cpu().numpy()
    return out
