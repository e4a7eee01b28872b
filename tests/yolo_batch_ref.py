"""
The row order of the YOLO training batch (include/pnyolo.h pny_yolo_train_batch) restated with numpy: scale by scale, inside a
scale (position in view_ids, y, x) -- what train/trainlib/YoloTrainer.py:93-129 of the reference produces with its indexing by
image_ord and its reshapes.  tests/test_cpu_yolo_batch.py holds it to the reference's fixture; the GPU tests use it where the
fixture has no case (repeated views, the documented limit).
"""
import numpy as np

CASES = ("a", "b", "c")


def offsets(n_sel, height, width, cells):
    """off[s] .. off[s + 1]: the rows of scale s; off[-1] = R."""
    return np.cumsum([0] + [n_sel * (height // c) * (width // c) for c in cells]).astype(np.int64)


def gather_targets(grids, view_ids):
    """grids: per scale (NV, Hs, Ws, A, 6) -> per scale (NS * Hs * Ws, A, 6)."""
    ids = np.asarray(view_ids, dtype=np.int64)
    return [np.asarray(g)[ids].reshape(-1, g.shape[3], 6) for g in grids]


def gather_rays(full_rays, view_ids):
    """full_rays: per scale (NV, Hs, Ws, 8), the rays of EVERY view at that scale -> per scale (NS * Hs * Ws, 8)."""
    ids = np.asarray(view_ids, dtype=np.int64)
    return [np.asarray(r)[ids].reshape(-1, 8) for r in full_rays]


def coded_grids(nv, height, width, cells, n_anchors):
    """The fixture's target values (tools/make_yolo_batch_golden.py): every value encodes (view, scale, y, x, anchor, field)."""
    out = []
    for s, cell in enumerate(cells):
        hs, ws = height // cell, width // cell
        v, y, x, a, f = np.meshgrid(np.arange(nv), np.arange(hs), np.arange(ws), np.arange(n_anchors), np.arange(6), indexing="ij")
        out.append((((((v * 4 + s) * 16 + y) * 32 + x) * 4 + a) * 8 + f).astype(np.float32))
    return out


def fixture_case(g, case):
    """(NV, H, W, A, cells, views, poses, focal, c, grids, rays, targets, offsets) of one case of the fixture."""
    nv, h, w, a = (int(v) for v in g[case + "_shape"])
    cells = [int(v) for v in g[case + "_cells"]]
    n = len(cells)
    return dict(NV=nv, H=h, W=w, A=a, cells=cells, views=g[case + "_views"], poses=g[case + "_poses"], focal=g[case + "_focal"],
                c=g[case + "_c"], grids=[g["%s_grid%d" % (case, s)] for s in range(n)],
                rays=[g["%s_rays%d" % (case, s)] for s in range(n)], targets=[g["%s_targets%d" % (case, s)] for s in range(n)],
                offsets=g[case + "_offsets"], z=(float(g["z"][0]), float(g["z"][1])))
