"""
The resident store restated for the tests (tests/test_cpu_resident.py, tests/test_gpu_resident.py), from include/pnyolo.h's
description of pny_resident_train_batch / pny_ingest_views_indexed and on the two restatements that exist: a share of a batch
is a ONE-object training batch (tests/train_batch_ref.py: the pixel choice, with the object's own view count) on the ingest of
that object's views (tests/ingest_ref.py: the fp32 value at the sampled output pixel).
"""
import numpy as np

import ingest_ref as ir
import train_batch_ref as tb

VIEWS = (2, 5, 3, 1)           # views per object of the tests' store
H, W = 12, 10                  # decoded size
# (resize, (OH, OW)): none; area 2:1 and to a size that divides neither axis; bilinear 7 x 9 (shrinking) and 20 x 13 (enlarging)
GEOMS = (("none", (12, 10)), ("area", (6, 5)), ("area", (5, 7)), ("bilinear_u8", (7, 9)), ("bilinear_u8", (20, 13)))


def make_store(channels, seed=0):
    """Four objects of VIEWS views of H x W x channels random bytes with 255s and, in every view, a 2 x 2 block whose 2:1
    bilinear mean is an exact tie; per object poses (NV, 4, 4), focal (2,), c (2,)."""
    rs = np.random.RandomState(100 + seed)
    objs = []
    for k, nv in enumerate(VIEWS):
        u8 = rs.randint(0, 256, size=(nv, H, W, channels)).astype(np.uint8)
        u8[rs.rand(nv, H, W) < 0.1] = 255                                  # whole pixels at 255 (the white background)
        u8[:, :2, :2, :3] = [[[1, 0, 255], [0, 2, 255]], [[0, 0, 254], [1, 1, 255]]]   # sums 2, 3, 1019: 0.5, 0.75, 254.75
        u8[:, -1, -1, :3] = (255, 0, 255)
        poses = np.tile(np.eye(4, dtype=np.float32), (nv, 1, 1))
        for v in range(nv):
            q, _ = np.linalg.qr(rs.randn(3, 3))
            poses[v, :3, :3] = (q * np.sign(np.linalg.det(q))).astype(np.float32)
            poses[v, :3, 3] = rs.uniform(-2, 2, 3).astype(np.float32)
        objs.append(dict(u8=u8, poses=poses, focal=np.array([9.5 + k, 11.25 - k], np.float32),
                         c=np.array([4.75 + 0.5 * k, 5.5 - 0.25 * k], np.float32)))
    return objs


def make_boxes(oh, ow, seed=0):
    """Per object (NV, 4) `cmin rmin cmax rmax` inside an oh x ow image; object 1 holds a one-pixel box and a full-image box."""
    rs = np.random.RandomState(200 + seed)
    out = []
    for k, nv in enumerate(VIEWS):
        lo = np.stack([rs.randint(0, ow, nv), rs.randint(0, oh, nv)], -1)
        hi = np.stack([rs.randint(lo[:, 0], ow), rs.randint(lo[:, 1], oh)], -1)
        b = np.concatenate([lo, hi], -1).astype(np.float32)
        if k == 1:
            b[0] = [3, 2, 3, 2]
            b[1] = [0, 0, ow - 1, oh - 1]
        out.append(b)
    return out


def clamp(v, n):
    return np.clip(np.asarray(v, np.int64), 0, n - 1)


def share_pix(nv, oh, ow, B, boxes=None, seed=None, draw_offset=0, draws=None):
    """(B, 3) [view, y, x] of one share: a one-object pny_sample_train_batch on nv views of oh x ow.  draws: the share's rows of
    a replay, clamped as the header says (a flat index into the grid, an image id into the views, a pixel into the image)."""
    if draws is None:
        return tb.seeded_pix(seed, 1, B, nv, oh, ow, bboxes=None if boxes is None else boxes[None], draw_offset=draw_offset)[0]
    if boxes is None:
        return tb.flat_to_pix(clamp(draws["pix_inds"], nv * oh * ow), oh, ow)
    pix = tb.bbox_to_pix(clamp(draws["image_ids"], nv), draws["u_x"], draws["u_y"], boxes)
    pix[:, 1], pix[:, 2] = clamp(pix[:, 1], oh), clamp(pix[:, 2], ow)
    return pix


def ingest_f64(u8, resize, oh, ow):
    """The ingest's value in float64, (NV, 3, OH, OW), and the bar an fp32 evaluation keeps to it.  none: the byte map, 2^-24.
    area: the window mean, (k + 8) 2^-24 for a window of k pixels (tests/ingest_ref.py area_bar).  bilinear_u8: the byte map
    of the UNROUNDED blend; the kernel rounds to a byte first, so half a byte (1 / 255 after the map) plus its fp32 error."""
    if resize == "none":
        return ir.images_nchw(u8), 2.0 ** -24
    if resize == "area":
        return ir.area(ir.images_nchw(u8), oh, ow), (ir.largest_window(u8.shape[1], u8.shape[2], oh, ow) + 8) * 2.0 ** -24
    return ir.byte_map(np.moveaxis(ir.bilinear(u8, oh, ow), -1, 1)), (0.5 + 1e-4) * 2.0 / 255.0


def gather(objs, obj_of, view_of):
    """(n_out, H, W, C) bytes: view view_of[i] of object obj_of[i]."""
    return np.stack([objs[o]["u8"][v] for o, v in zip(obj_of, view_of)])
