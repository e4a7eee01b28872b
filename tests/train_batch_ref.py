"""
The training batch's pixel choice restated for the tests (tests/test_cpu_train_batch.py, tests/test_gpu_train_batch.py):
numpy on the oracle's Philox (oracle/pnyolo_oracle.py philox4x32_10, philox_uniform), written from include/pnyolo.h's
description of pny_sample_train_batch, not from the kernel's headers.
"""
import numpy as np

import pnyolo_oracle as orc

STREAM_BATCH_PIX, STREAM_BATCH_VIEW, STREAM_BATCH_X, STREAM_BATCH_Y = 5, 6, 7, 8
M32 = 0xFFFFFFFF


def batch_index(seed, stream, idx, n):
    """Integer in [0, n) at position idx of a stream: word idx % 4 of counter idx // 4, times n, shifted right by 32."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    idx = np.asarray(idx, dtype=np.uint64)
    ci = idx >> np.uint64(2)
    w = np.stack(orc.philox4x32_10((ci & np.uint64(M32), ci >> np.uint64(32), int(stream), orc.PHILOX_COUNTER3),
                                   (seed & M32, seed >> 32)), -1)
    w = np.take_along_axis(w, (idx & np.uint64(3)).astype(np.int64)[..., None], -1)[..., 0]
    assert 1 <= n < 2 ** 32
    return ((w * np.uint64(n)) >> np.uint64(32)).astype(np.int64)       # w, n < 2^32: the product is exact in uint64


def flat_to_pix(flat, H, W):
    flat = np.asarray(flat, dtype=np.int64)
    return np.stack([flat // (H * W), (flat % (H * W)) // W, flat % W], -1)


def bbox_to_pix(image_ids, u_x, u_y, boxes):
    """util.bbox_sample's arithmetic (reference src/util/util.py:228-235) in fp32, one rounding per operation; boxes
    (NV, 4) `cmin rmin cmax rmax` of the object."""
    image_ids = np.asarray(image_ids, dtype=np.int64)
    b = np.asarray(boxes, dtype=np.float32)[image_ids]
    u_x, u_y, one = np.asarray(u_x, dtype=np.float32), np.asarray(u_y, dtype=np.float32), np.float32(1)
    x = np.trunc(u_x * (b[..., 2] + one - b[..., 0]) + b[..., 0])
    y = np.trunc(u_y * (b[..., 3] + one - b[..., 1]) + b[..., 1])
    assert x.dtype == np.float32
    return np.stack([image_ids, y.astype(np.int64), x.astype(np.int64)], -1)


def seeded_pix(seed, SB, B, NV, H, W, bboxes=None, draw_offset=0):
    """(SB, B, 3) [view, y, x] of a seeded call: ray r of object s draws at index draw_offset + s * B + r."""
    idx = np.uint64(draw_offset) + np.arange(SB * B, dtype=np.uint64).reshape(SB, B)
    if bboxes is None:
        return flat_to_pix(batch_index(seed, STREAM_BATCH_PIX, idx, NV * H * W), H, W)
    view = batch_index(seed, STREAM_BATCH_VIEW, idx, NV)
    u_x, u_y = orc.philox_uniform(seed, STREAM_BATCH_X, idx), orc.philox_uniform(seed, STREAM_BATCH_Y, idx)
    bboxes = np.asarray(bboxes, dtype=np.float32)
    return np.stack([bbox_to_pix(view[s], u_x[s], u_y[s], bboxes[s]) for s in range(SB)])
