"""
The device ingest on the GPU (csrc/ingest.hip, include/pnyolo.h pny_ingest_views / pny_yolo_build_targets, augment.ingest_views,
util.build_yolo_targets) against data.py's host functions and the float64 restatements of tests/ingest_ref.py:
  * the byte map: every byte value, channels 3 and 4, bit-equal to data.image_to_tensor_balanced;
  * bilinear where every lambda is dyadic (135 x 240 -> 64 x 120 by the shipped scale): byte for byte resize_bilinear_u8 and the
    byte map, exact half-to-even ties included; bilinear at general lambda (27 x 45 -> 13 x 22, 7 x 5 -> 10 x 9 enlarging, a
    1 x 1 source): EVERY output byte within 0.5 + 1e-4 of the unrounded float64 value;
  * area (12 x 18 -> 6 x 9, -> 5 x 7 ragged, 128 x 128 -> 64 x 64) within max(4 e_host, (k + 8) 2^-24) of the float64
    restatement, e_host the host fp32 path's own error on the same inputs, k the largest window (ingest_ref.area_bar);
  * mask and box bit-equal to the restatement of SRNDataset.__getitem__ without resize; with area resize the mask within the
    area bar and the box bit-equal to the host's bbox * scale;
  * bitwise: run to run, a view alone against the view in a batch, (SB, NV, ...) against the flattened call, jitter= against
    ingest_views followed by color_jitter; a byte tensor one byte into a larger buffer;
  * the target grids bit-equal, per scale, to YOLODataset._get_all_bboxes stacked by stage_yolo_targets (distinct IoUs
    asserted), duplicated anchors against the stable-order restatement, the shipped one-scale shape, and the output fed
    unchanged into util.yolo_train_batch.
"""
import numpy as np
import pytest
import torch

import ingest_ref as ir
from helpers import DEV
from pixel_nerf_yolo_amd import augment as paug
from pixel_nerf_yolo_amd import util as putil

pytestmark = pytest.mark.gpu

SCALE = (0.5, 0.47407)                      # conf/exp/yolo.conf image_scale (fx, fy)


def on_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def random_u8(seed, *shape):
    return np.random.RandomState(seed).randint(0, 256, size=shape).astype(np.uint8)


# --------------------------------------------------------------------------- byte map
@pytest.mark.parametrize("channels", [3, 4])
def test_byte_map_is_the_hosts_for_every_byte(channels):
    img = np.zeros((1, 16, 16, channels), np.uint8)
    img[0, :, :, 0] = np.arange(256).reshape(16, 16)
    img[0, :, :, 1] = np.arange(256)[::-1].reshape(16, 16)
    img[0, :, :, 2] = (np.arange(256) * 7 % 256).reshape(16, 16)
    if channels == 4:
        img[..., 3] = random_u8(1, 16, 16)                     # alpha: ignored
    got = paug.ingest_views(on_dev(img)).cpu()
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, 3, 16, 16)
    assert torch.equal(got, ir.host_images(img))
    assert float(got.min()) == -1.0 and float(got.max()) == 1.0


# --------------------------------------------------------------------------- bilinear
def test_bilinear_exact_case_is_the_hosts_byte_for_byte():
    u8 = random_u8(2, 3, 135, 240, 3)
    u8[0, :2, :2] = [[[1, 0, 255], [0, 2, 255]], [[0, 0, 254], [1, 1, 255]]]
    host, res = ir.host_bilinear(u8, *SCALE)
    assert tuple(host.shape) == (3, 3, 64, 120)
    ref = ir.bilinear(u8, 64, 120)
    ties = int((np.abs(ref - np.floor(ref) - 0.5) < 1e-9).sum())
    print("exact case: %d exact ties among %d bytes" % (ties, ref.size))
    assert ties > 50
    got = paug.ingest_views(on_dev(u8), scale=SCALE).cpu()
    assert torch.equal(got, host)
    assert torch.equal(paug.ingest_views(on_dev(u8), size=(64, 120), resize="bilinear_u8").cpu(), host)


@pytest.mark.parametrize("shape,out,kw", [((2, 27, 45), (13, 22), dict(scale=SCALE)),
                                          ((2, 7, 5), (10, 9), dict(size=(10, 9), resize="bilinear_u8")),
                                          ((2, 1, 1), (3, 2), dict(size=(3, 2), resize="bilinear_u8"))])
def test_bilinear_general_lambda_every_byte_within_half(shape, out, kw):
    u8 = random_u8(3, *shape, 3)
    got = paug.ingest_views(on_dev(u8), **kw).cpu().numpy()
    assert got.shape == (shape[0], 3) + out
    # back to bytes: the byte map is injective and the host's table inverts it
    table = ir.host_images(np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1).repeat(3, -1)).numpy()[0, 0].reshape(-1)
    q = np.searchsorted(table, got)
    assert np.array_equal(table[np.clip(q, 0, 255)], got)                       # every output IS a mapped byte
    v = np.moveaxis(ir.bilinear(u8, *out), -1, 1)
    err = np.abs(q - v).max()
    host = torch.nn.functional.interpolate(torch.from_numpy(u8).permute(0, 3, 1, 2).float(), size=out, mode="bilinear",
                                           align_corners=False).round().clamp(0, 255).numpy()
    print("host bytes: worst |q - v| = %.6f, %d of %d bytes differ from the kernel's" % (np.abs(host - v).max(), int((host != q).sum()), q.size))
    print("bilinear %s -> %s: worst |q - v| = %.6f" % (shape[1:], out, err))
    assert err <= 0.5 + 1e-4


# --------------------------------------------------------------------------- area
def check_area(got, u8, size, what):
    h, w = u8.shape[1:3]
    ref = ir.area(ir.images_nchw(u8), *size)
    host = torch.nn.functional.interpolate(ir.host_images(u8), size=size, mode="area").numpy()
    e_host = float(np.abs(host.astype(np.float64) - ref).max())
    k = ir.largest_window(h, w, *size)
    bar = ir.area_bar(e_host, k)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print("%s %dx%d -> %dx%d: kernel %.3g, host %.3g, window %d, bar %.3g" % (what, h, w, size[0], size[1], err, e_host, k, bar))
    assert got.dtype == np.float32 and got.shape == ref.shape and err <= bar
    return bar


@pytest.mark.parametrize("shape,size", [((2, 12, 18), (6, 9)), ((2, 12, 18), (5, 7)), ((2, 128, 128), (64, 64))])
def test_area_against_the_restatement(shape, size):
    u8 = random_u8(4, *shape, 3)
    got = paug.ingest_views(on_dev(u8), size=size, resize="area").cpu().numpy()
    check_area(got, u8, size, "area")
    u8[1] = 77                                                                   # a constant view stays constant
    got = paug.ingest_views(on_dev(u8), size=size, resize="area").cpu().numpy()
    assert np.abs(got[1] - np.float32(ir.byte_map(77))).max() <= 4 * 2.0 ** -24


# --------------------------------------------------------------------------- mask and box
def mask_views(h, w):
    u8 = np.full((3, h, w, 3), 255, np.uint8)
    rs = np.random.RandomState(5)
    u8[0, h - 5:, :4] = rs.randint(0, 255, size=(5, 4, 3))          # a rectangle touching column 0 and the last row
    u8[0, 1, w - 2] = (255, 9, 9)                                   # one byte at 255: outside
    u8[1, h // 2 + 1, w // 2] = (3, 2, 1)                            # a single pixel
    return u8                                                       # view 2: all white


def test_mask_and_box_without_resize_are_the_datasets():
    u8 = mask_views(12, 18)
    img, mask, bbox = (t.cpu() for t in paug.ingest_views(on_dev(u8), white_mask=True))
    m, b = ir.srn_mask_bbox(u8)
    assert torch.equal(img, ir.host_images(u8))
    assert tuple(mask.shape) == (3, 1, 12, 18) and np.array_equal(mask.numpy(), m.astype(np.float32))
    assert np.array_equal(bbox.numpy(), b)
    assert bbox.tolist() == [[0, 7, 3, 11], [9, 7, 9, 7], [18, 12, -1, -1]] and (bbox[:, 2] < 0).tolist() == [False, False, True]


@pytest.mark.parametrize("hw,size", [((12, 18), (6, 9)), ((12, 18), (5, 7)), ((128, 128), (64, 64))])
def test_mask_and_box_with_area_resize(hw, size):
    u8 = mask_views(*hw)
    img, mask, bbox = (t.cpu() for t in paug.ingest_views(on_dev(u8), size=size, resize="area", white_mask=True))
    h_img, h_mask, h_bbox = ir.host_srn(u8, size)
    bar = check_area(img.numpy(), u8, size, "image")
    m, _ = ir.srn_mask_bbox(u8)
    err = float(np.abs(mask.numpy().astype(np.float64) - ir.area(m, *size)).max())
    print("mask: kernel %.3g, host %.3g" % (err, np.abs(h_mask.numpy().astype(np.float64) - ir.area(m, *size)).max()))
    assert tuple(mask.shape) == (3, 1) + size and err <= bar
    assert torch.equal(bbox, h_bbox)                                 # bit for bit the host's bbox * scale; the empty view unscaled
    assert bbox[2].tolist() == [hw[1], hw[0], -1, -1]


# --------------------------------------------------------------------------- reproducibility
def test_bitwise_identities():
    u8 = random_u8(6, 3, 27, 45, 3)
    u8[1, 3:9, 5:20] = 255
    d = on_dev(u8)
    for kw in (dict(), dict(scale=SCALE), dict(size=(13, 22), resize="area", white_mask=True), dict(white_mask=True)):
        a, b = paug.ingest_views(d, **kw), paug.ingest_views(d, **kw)
        one = paug.ingest_views(d[1:2].clone(), **kw)
        five = paug.ingest_views(torch.stack([d, d.flip(0)]), **kw)
        flat = paug.ingest_views(torch.cat([d, d.flip(0)]), **kw)
        for x, y, o, f5, fl in zip(*[(t if isinstance(t, tuple) else (t,)) for t in (a, b, one, five, flat)]):
            assert torch.equal(x, y) and torch.equal(x[1:2], o)
            assert f5.shape[:2] == (2, 3) and torch.equal(f5.reshape(fl.shape), fl) and torch.equal(f5[0], x)
    # one byte into a larger buffer: rows at every alignment
    buf = torch.zeros(u8.size + 8, dtype=torch.uint8, device=DEV)
    for off in (1, 2, 3):
        view = buf[off:off + u8.size].view(3, 27, 45, 3)
        view.copy_(d)
        assert view.data_ptr() % 4 == off
        assert torch.equal(paug.ingest_views(view, scale=SCALE), paug.ingest_views(d, scale=SCALE))
        assert torch.equal(paug.ingest_views(view), paug.ingest_views(d))
    # out=, a side stream, and the chained jitter
    out = torch.empty(3, 3, 27, 45, device=DEV)
    st = torch.cuda.Stream(device=DEV)
    st.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(st):
        assert paug.ingest_views(d, out=out) is out
    st.synchronize()
    assert torch.equal(out, paug.ingest_views(d))
    f = [0.05, 0.9, 1.1, 0.95]
    plain = paug.ingest_views(d, scale=SCALE)
    assert torch.equal(paug.ingest_views(d, scale=SCALE, jitter=f), paug.color_jitter(plain, f))
    two = torch.stack([d, d.flip(0)])
    ff = torch.tensor([f, [-0.1, 1.1, 0.9, 1.05]])
    assert torch.equal(paug.ingest_views(two, jitter=ff), paug.color_jitter(paug.ingest_views(two), ff))


# --------------------------------------------------------------------------- targets
def target_views():
    return [
        [],
        [[0.40, 0.55, 0.12, 0.20, 2.0]],
        [[0.30, 0.40, 0.20, 0.30, 1.0], [0.31, 0.41, 0.21, 0.29, 0.0], [0.80, 0.75, 0.10, 0.12, 3.0], [0.10, 0.90, 0.05, 0.04, 1.0],
         [0.55, 0.15, 0.40, 0.50, 4.0], [0.56, 0.16, 0.39, 0.51, 2.0]],
        [[0.0, 0.0, 0.08, 0.07, 1.0], [0.999, 0.999, 0.3, 0.2, 2.0], [0.5, 0.5, 0.005, 0.004, 3.0]],
    ]


def build(views, height, width, cells, anchors, thresh=ir.YOLO_IGNORE_IOU):
    lab, cnt = ir.pack_labels(views)
    return putil.build_yolo_targets(lab, cnt, height, width, cells, anchors, thresh, DEV)


def test_targets_are_the_datasets_grids_bit_for_bit():
    views, cells, A = target_views(), [32, 16, 8], 3
    assert ir.distinct_ious(views, ir.YOLO_ANCHORS)
    got = build(views, 64, 96, cells, ir.YOLO_ANCHORS)
    host = putil.stage_yolo_targets(ir.host_targets(views, 64, 96, cells, ir.YOLO_ANCHORS, A, ir.YOLO_IGNORE_IOU), "cpu")
    assert [tuple(g.shape) for g in got] == [(4, 2, 3, 3, 6), (4, 4, 6, 3, 6), (4, 8, 12, 3, 6)]
    for s in range(3):
        assert got[s].dtype == torch.float32 and got[s].is_contiguous() and torch.equal(got[s].cpu(), host[s]), s
        assert float(got[s][0].abs().max()) == 0.0                              # view 0: complete, zero-filled grids
        assert int((got[s][1][..., 0] == 1).sum()) == 1
    # view 2: the second box of like size in the same cell took the next anchor and left -1 marks
    assert sum(int((g[2][..., 0] == -1).sum()) for g in got) > 0
    assert [int((g[2][..., 0] == 1).sum()) for g in got] == [6, 6, 6]
    # view 3: corners, and a box below every anchor still gets its best anchor per scale
    assert all(int((g[3][..., 0] == 1).sum()) == 3 for g in got)
    assert all(float(g[3][0, 0, :, 0].max()) == 1.0 and float(g[3][-1, -1, :, 0].max()) == 1.0 for g in got)
    # twice the same bits, and onto buffers that held something else
    again = build(views, 64, 96, cells, ir.YOLO_ANCHORS)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


def test_targets_with_duplicated_anchors_follow_the_stable_order():
    anchors = [[0.1, 0.1], [0.1, 0.1], [0.3, 0.3], [0.1, 0.1], [0.3, 0.3], [0.3, 0.3]]
    views = [[[0.3, 0.3, 0.1, 0.1, 2.0], [0.3, 0.3, 0.1, 0.1, 3.0], [0.7, 0.2, 0.3, 0.3, 1.0]], [[0.3, 0.3, 0.3, 0.3, 1.0]]]
    got = build(views, 32, 32, [16, 8], anchors)
    for v in range(2):
        want = ir.yolo_targets(views[v], 32, 32, [16, 8], anchors, 3, ir.YOLO_IGNORE_IOU)
        for s in range(2):
            assert np.array_equal(got[s][v].cpu().numpy(), want[s]), (v, s)


def test_targets_at_the_shipped_shape_feed_the_train_batch():
    rs = np.random.RandomState(8)
    views = [[[float(rs.uniform(0, 1)), float(rs.uniform(0, 1)), float(rs.uniform(0.05, 0.6)), float(rs.uniform(0.05, 0.6)), float(k % 3)]
              for k in range(8)] for _ in range(2)]
    anchors = ir.YOLO_ANCHORS[:3]
    assert ir.distinct_ious(views, anchors)
    got = build(views, 512, 960, [32], anchors)
    host = putil.stage_yolo_targets(ir.host_targets(views, 512, 960, [32], anchors, 3, ir.YOLO_IGNORE_IOU), "cpu")
    assert len(got) == 1 and tuple(got[0].shape) == (2, 16, 30, 3, 6) and torch.equal(got[0].cpu(), host[0])
    poses = torch.eye(4).repeat(2, 1, 1)
    poses[:, 2, 3] = 3.0
    args = ([1, 0], [480.0, 485.0], [480.0, 256.0])
    rays, tg = putil.yolo_train_batch(poses, args[0], args[1], args[2], got, 512, 960, [32], 1.0, 13.0)
    rays_h, tg_h = putil.yolo_train_batch(poses, args[0], args[1], args[2], [host[0].to(DEV)], 512, 960, [32], 1.0, 13.0)
    assert tuple(tg[0].shape) == (2 * 16 * 30, 3, 6) and torch.equal(tg[0], tg_h[0]) and torch.equal(rays[0], rays_h[0])
    assert torch.equal(tg[0].reshape(2, 16, 30, 3, 6), got[0][[1, 0]])
