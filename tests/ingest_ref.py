"""
Float64 restatements of the device ingest (include/pnyolo.h pny_ingest_views / pny_yolo_build_targets), written from the
definitions rather than from the kernel, for tests/test_cpu_ingest.py and tests/test_gpu_ingest.py:

  byte_map        t = b / 255, (t - 0.5) / 0.5
  bilinear        half-pixel centres, src = max(scale (dst + 0.5) - 0.5, 0), scale = in / out, the four taps, UNROUNDED
  area            the mean over [floor(i in / out), ceil((i + 1) in / out)) per axis
  srn_mask_bbox   SRNDataset.__getitem__'s mask and box (data.py:112-122) with the device path's convention for an empty mask
  yolo_targets    YOLODataset._get_all_bboxes with a stable descending order (ties to the lower anchor index)

and the host fp32 chains of data.py the bars are taken from.
"""
import numpy as np
import torch
import torch.nn.functional as F

from pixel_nerf_yolo_amd import data as pdata

# conf/exp/yolo.conf of the reference: the values conf.yolo() carries
YOLO_ANCHORS = [[0.02, 0.03], [0.04, 0.07], [0.08, 0.06], [0.07, 0.15], [0.15, 0.11], [0.14, 0.29], [0.28, 0.22], [0.38, 0.48],
                [0.9, 0.78]]
YOLO_IGNORE_IOU = 0.5


def byte_map(b):
    return (np.asarray(b, np.float64) / 255.0 - 0.5) / 0.5


def _taps(n_in, n_out):
    dst = np.arange(n_out, dtype=np.float64)
    src = np.maximum((n_in / n_out) * (dst + 0.5) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, src - i0


def bilinear(u8, oh, ow):
    """(NV, H, W, C) bytes -> (NV, oh, ow, 3) float64 in byte units, not rounded."""
    x = np.asarray(u8)[..., :3].astype(np.float64)
    y0, y1, ly = _taps(x.shape[1], oh)
    x0, x1, lx = _taps(x.shape[2], ow)
    ly, lx = ly[None, :, None, None], lx[None, None, :, None]
    top = x[:, y0][:, :, x0] * (1 - lx) + x[:, y0][:, :, x1] * lx
    bot = x[:, y1][:, :, x0] * (1 - lx) + x[:, y1][:, :, x1] * lx
    return top * (1 - ly) + bot * ly


def area_windows(n_in, n_out):
    i = np.arange(n_out, dtype=np.int64)
    return (i * n_in) // n_out, -((-(i + 1) * n_in) // n_out)


def area(x, oh, ow):
    """(..., H, W) float64 -> (..., oh, ow): the mean over each window."""
    x = np.asarray(x, np.float64)
    ys, ye = area_windows(x.shape[-2], oh)
    xs, xe = area_windows(x.shape[-1], ow)
    out = np.empty(x.shape[:-2] + (oh, ow))
    for i in range(oh):
        for j in range(ow):
            out[..., i, j] = x[..., ys[i]:ye[i], xs[j]:xe[j]].mean(axis=(-2, -1))
    return out


def largest_window(h, w, oh, ow):
    ys, ye = area_windows(h, oh)
    xs, xe = area_windows(w, ow)
    return int((ye - ys).max() * (xe - xs).max())


def images_nchw(u8):
    """(NV, H, W, C) bytes -> (NV, 3, H, W) float64 in [-1, 1]."""
    return np.moveaxis(byte_map(np.asarray(u8)[..., :3]), -1, -3)


def srn_mask_bbox(u8):
    """SRNDataset.__getitem__ per view: mask (NV, 1, H, W) float64 in {0, 1}, bbox (NV, 4) float32 [cmin, rmin, cmax, rmax]; a view
    with an empty mask gets [W, H, -1, -1] where the dataset raises."""
    u8 = np.asarray(u8)[..., :3]
    masks, boxes = [], []
    for img in u8:
        mask = (img != 255).all(axis=-1)[..., None].astype(np.uint8) * 255
        rows, cols = np.any(mask, axis=1), np.any(mask, axis=0)
        rnz, cnz = np.where(rows)[0], np.where(cols)[0]
        if len(rnz) == 0:
            box = [img.shape[1], img.shape[0], -1, -1]
        else:
            box = [cnz[0], rnz[0], cnz[-1], rnz[-1]]
        boxes.append(np.array(box, np.float32))
        masks.append(mask[..., 0][None].astype(np.float64) / 255.0)
    return np.stack(masks), np.stack(boxes)


# ---- the host fp32 chains of data.py
def host_images(u8):
    return torch.stack([pdata.image_to_tensor_balanced(v[..., :3]) for v in np.asarray(u8)])


def host_bilinear(u8, fx, fy):
    """YOLODataset's per-view chain: (NV, 3, OH, OW) fp32 and the resized bytes (NV, OH, OW, 3)."""
    res = np.stack([pdata.resize_bilinear_u8(np.ascontiguousarray(v[..., :3]), fx, fy) for v in np.asarray(u8)])
    return host_images(res), res


def host_srn(u8, image_size):
    """SRNDataset's chain after decoding: images, masks, bbox as its item holds them (the empty-mask convention aside)."""
    u8 = np.asarray(u8)[..., :3]
    imgs = host_images(u8)
    m, b = srn_mask_bbox(u8)
    masks, bbox = torch.from_numpy(m).to(torch.float32), torch.from_numpy(b.copy())
    if tuple(imgs.shape[-2:]) != tuple(image_size):
        scale = image_size[0] / imgs.shape[-2]
        empty = bbox[:, 2] < 0
        scaled = bbox * scale
        bbox = torch.where(empty[:, None], bbox, scaled)
        imgs = F.interpolate(imgs, size=tuple(image_size), mode="area")
        masks = F.interpolate(masks, size=tuple(image_size), mode="area")
    return imgs, masks, bbox


def area_bar(e_host, k):
    """max(4 e_host, (k + 8) 2^-24), in output units: k rounded additions on values in [-1, 1] plus the division and the byte map;
    the factor 4 allows another summation order."""
    return max(4.0 * e_host, (k + 8) * 2.0 ** -24)


# ---- targets
def iou_f32(w, h, anchors):
    """data.iou_wh's operations in fp32, one by one."""
    a = np.asarray(anchors, np.float32).reshape(-1, 2)
    w, h = np.float32(w), np.float32(h)
    inter = np.minimum(w, a[:, 0]) * np.minimum(h, a[:, 1])
    union = (w * h + a[:, 0] * a[:, 1]).astype(np.float32) - inter
    return (inter / union).astype(np.float32)


def yolo_targets(boxes, height, width, cell_sizes, anchors, n_anchors, thresh):
    """_get_all_bboxes for one view with a stable order: [(Hs, Ws, A, 6) float32 per scale]."""
    sizes = [(height // c, width // c) for c in cell_sizes]
    out = [np.zeros((h, w, n_anchors, 6), np.float32) for h, w in sizes]
    for x, y, bw, bh, cls in boxes:
        iou = iou_f32(bw, bh, anchors)
        order = np.argsort(-iou.astype(np.float64), kind="stable")
        has = [False] * len(sizes)
        for a in order:
            s, k = int(a) // n_anchors, int(a) % n_anchors
            hs, ws = sizes[s]
            i, j = int(hs * y), int(ws * x)
            if out[s][i, j, k, 0] != 0:
                continue
            if not has[s]:
                out[s][i, j, k] = np.array([1.0, ws * x - j, hs * y - i, bw * ws, bh * hs, int(cls)], np.float64).astype(np.float32)
                has[s] = True
            elif iou[a] > np.float32(thresh):
                out[s][i, j, k, 0] = -1.0
    return out


class _BareYolo(pdata.YOLODataset):
    def __init__(self, cell_sizes, anchors, n_anchors, thresh):           # no directory tree: the attributes alone
        self.cell_sizes, self.num_scales, self.num_anchors_per_scale = list(cell_sizes), len(cell_sizes), n_anchors
        self.anchors = torch.tensor(np.asarray(anchors, np.float64).reshape(-1, 2).tolist(), dtype=torch.float32)
        self.ignore_iou_thresh = thresh


def host_targets(views, height, width, cell_sizes, anchors, n_anchors, thresh):
    """The project's host path: _get_all_bboxes per view on a bare YOLODataset, in the collated form the trainer receives
    (a leading batch axis of 1), for util.stage_yolo_targets."""
    ds = _BareYolo(cell_sizes, anchors, n_anchors, thresh)
    return [tuple(t[None] for t in ds._get_all_bboxes([list(map(float, b)) for b in boxes], height, width)) for boxes in views]


def pack_labels(views):
    """views: per view a list of [cx, cy, w, h, cls] -> labels (NV, MAXB, 5) float64, n_labels (NV,) int32."""
    maxb = max([len(v) for v in views] + [1])
    lab = np.zeros((len(views), maxb, 5), np.float64)
    for i, v in enumerate(views):
        if len(v):
            lab[i, :len(v)] = np.asarray(v, np.float64)
    return lab, np.array([len(v) for v in views], np.int32)


def distinct_ious(views, anchors):
    """Every box's IoUs against the anchors are pairwise distinct: the host's argsort then has one possible order."""
    return all(len(set(iou_f32(b[2], b[3], anchors).tolist())) == len(np.asarray(anchors).reshape(-1, 2)) for v in views for b in v)
