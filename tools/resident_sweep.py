#!/usr/bin/env python3
"""
Time of a training step's inputs drawn from data.ResidentViews against the path it stands in for, taken in the same run, at
the SRN shape (4 objects x 50 views of 128 x 128, boxes from the white background) and the DTU shape (4 x 49 views of
300 x 400, uniform sampling), ray_batch_size 128 and 3 source views per object:

  parent    from the items' bytes ALREADY DECODED in host RAM (pinned, as a DataLoader with pin_memory hands them over): the
            copy to the device, augment.ingest_views (with SRN's mask and boxes), util.sample_train_batch and the source-view
            select (advanced indexing of images and poses).  For DTU also from fp32 images, as the `dvr_dtu` items carry them.
  resident  ResidentViews.batch on a store of STORE_OBJS objects, four random ids per step.
  decode    separately, and nothing more than that: data.imread of one step's files (written by data.imwrite as PNG, synthetic
            smooth images with a textured object) on ONE CPU thread.  The parent path pays it per step in its workers; the
            resident path pays it once, in the fill.
  footprint the store's nbytes and the time of its fill from decoded bytes (copies, and for SRN the box launches and their wait).

Timing: a host clock around blocks of BLOCK steps that end in a device synchronise, after WARMUP steps, the paths alternating
block by block; the median and the spread over the blocks.  Outputs of the two paths on the same ids and seed are compared bit
for bit at these sizes.  Prints one JSON line (profiles/resident_sweep.json is one run of it).  Needs an MI355X.

Usage:  python tools/resident_sweep.py
"""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pnyolo_pkg  # noqa: E402

pnyolo_pkg.load()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pixel_nerf_yolo_amd import augment as paug  # noqa: E402
from pixel_nerf_yolo_amd import data as pdata  # noqa: E402
from pixel_nerf_yolo_amd import util as putil  # noqa: E402

WARMUP, BLOCKS, BLOCK = 10, 10, 20
STORE_OBJS, SB, B, NS = 16, 4, 128, 3


def synthetic_views(rs, n, h, w, white):
    """Smooth backgrounds (white for SRN) with a textured rectangle: bytes a PNG compresses about as it does a rendering."""
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        base = np.full((h, w, 3), 255.0) if white else np.stack([(xx * (0.3 + 0.1 * c) + yy * 0.2 + 17 * i) % 256 for c in range(3)], -1)
        y0, x0 = rs.randint(h // 8, h // 3), rs.randint(w // 8, w // 3)
        tex = rs.randint(0, 255, size=(h - 2 * y0, w - 2 * x0, 3))
        base[y0:h - y0, x0:w - x0] = 0.5 * tex + 0.5 * np.roll(tex, 1, axis=1)
        out[i] = np.clip(base, 0, 254 if white else 255).astype(np.uint8)
        if white:
            out[i][(base == 255.0).all(-1)] = 255
    return out


def blocks_ms(fns):
    """Per path the time per step of each of BLOCKS blocks of BLOCK steps, the paths alternating; every block ends in a synchronise."""
    for fn in fns.values():
        for k in range(WARMUP):
            fn(k)
    torch.cuda.synchronize()
    t = {name: [] for name in fns}
    for blk in range(BLOCKS):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            for k in range(BLOCK):
                fn(blk * BLOCK + k)
            torch.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) * 1e3 / BLOCK)
    return {name: {"min": round(min(v), 4), "median": round(float(np.median(v)), 4), "max": round(max(v), 4)} for name, v in t.items()}


def case(name, dev, nv, h, w, white, z):
    rs = np.random.RandomState(1)
    objs = [synthetic_views(rs, nv, h, w, white) for _ in range(STORE_OBJS)]
    poses = [torch.from_numpy(np.tile(np.eye(4, dtype=np.float32), (nv, 1, 1)) + rs.randn(nv, 4, 4).astype(np.float32) * 0.01) for _ in objs]
    focal, c = torch.tensor([131.25, 131.25]), torch.tensor([w * 0.5, h * 0.5])
    # ---- footprint and fill
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = pdata.ResidentViews(dev, white_bbox=white)
    for u8, p in zip(objs, poses):
        st.add(u8, p, focal, c=c)
    st.tables()
    torch.cuda.synchronize()
    fill_ms = (time.perf_counter() - t0) * 1e3
    # ---- the steps: ids and source views per step, the same for both paths
    steps = WARMUP + BLOCKS * BLOCK
    ids = [rs.choice(STORE_OBJS, SB, replace=False).tolist() for _ in range(steps)]
    src = [rs.randint(0, nv, size=(SB, NS)).tolist() for _ in range(steps)]
    pinned_u8 = [torch.from_numpy(o).pin_memory() for o in objs]
    pinned_f32 = [paug_host_images(o).pin_memory() for o in objs[:SB]] if not white else None

    def parent(k, keep=None):
        u8 = torch.stack([pinned_u8[o].to(dev, non_blocking=True) for o in ids[k]])
        if white:
            images, _, boxes = paug.ingest_views(u8, white_mask=True)
        else:
            images, boxes = paug.ingest_views(u8), None
        p = torch.stack([poses[o] for o in ids[k]]).to(dev, non_blocking=True)
        rays, rgb, pix = putil.sample_train_batch(images, p, focal[None], z[0], z[1], B, c=c[None], bboxes=boxes, seed=k)
        sel = torch.tensor(src[k], device=dev)
        out = (rays, rgb, pix, images[torch.arange(SB, device=dev)[:, None], sel], p[torch.arange(SB, device=dev)[:, None], sel])
        if keep is not None:
            keep.append(out)

    def parent_f32(k):
        images = torch.stack([pinned_f32[s].to(dev, non_blocking=True) for s in range(SB)])
        p = torch.stack([poses[o] for o in ids[k]]).to(dev, non_blocking=True)
        rays, rgb, pix = putil.sample_train_batch(images, p, focal[None], z[0], z[1], B, c=c[None], seed=k)
        sel = torch.tensor(src[k], device=dev)
        return rays, rgb, pix, images[torch.arange(SB, device=dev)[:, None], sel], p[torch.arange(SB, device=dev)[:, None], sel]

    def resident(k, keep=None):
        out = st.batch(ids[k], src[k], B, z[0], z[1], seed=k)
        if keep is not None:
            keep.append(out)

    fns = {"parent_from_bytes_ms": parent, "resident_ms": resident}
    if not white:
        fns["parent_from_fp32_ms"] = parent_f32
    times = blocks_ms(fns)
    # ---- the same bits (all objects have nv views, so a four-object parent call draws what four shares draw)
    a, b = [], []
    parent(3, a)
    resident(3, b)
    torch.cuda.synchronize()
    same = all(torch.equal(x, b[0][key]) for x, key in zip(a[0], ("rays", "rgb_gt", "pix", "src_images", "src_poses")))
    # ---- decode, on its own
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for s in range(SB):
            for v in range(nv):
                paths.append(os.path.join(tmp, "%d_%03d.png" % (s, v)))
                pdata.imwrite(paths[-1], objs[s][v])
        file_bytes = sum(os.path.getsize(p) for p in paths)
        dec = []
        for _ in range(3):
            t0 = time.perf_counter()
            for p in paths:
                pdata.imread(p)
            dec.append((time.perf_counter() - t0) * 1e3)
    step_u8 = SB * nv * h * w * 3
    return {"case": name, "views_per_object": nv, "height": h, "width": w, "objects_per_step": SB, "ray_batch_size": B,
            "source_views": NS, "store_objects": STORE_OBJS, "step_ms": times,
            "parent_over_resident": round(times["parent_from_bytes_ms"]["median"] / times["resident_ms"]["median"], 2),
            "bytes_copied_per_step_parent": step_u8, "bytes_copied_per_step_parent_fp32": step_u8 * 4,
            "outputs_bit_equal_to_parent": bool(same), "store_nbytes": st.nbytes, "fill_ms": round(fill_ms, 2),
            "decode_one_step_one_thread_ms": {"min": round(min(dec), 2), "median": round(float(np.median(dec)), 2), "max": round(max(dec), 2),
                                              "files": len(paths), "file_bytes": file_bytes}}


def paug_host_images(u8):
    """(NV, 3, H, W) fp32 in [-1, 1] of decoded views: data.image_to_tensor_balanced per view."""
    return torch.stack([pdata.image_to_tensor_balanced(v) for v in u8])


def main():
    assert torch.cuda.is_available(), "tools/resident_sweep.py needs an MI355X"
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    out = {"tool": "resident_sweep", "device": torch.cuda.get_device_name(0), "warmup": WARMUP, "blocks": BLOCKS, "steps_per_block": BLOCK,
           "timing": "host clock around a block of steps ending in a device synchronise; paths alternate block by block",
           "cases": [case("srn 4 x 50 x 128 x 128, boxes", dev, 50, 128, 128, True, (0.8, 1.8)),
                     case("dtu 4 x 49 x 300 x 400, uniform", dev, 49, 300, 400, False, (0.1, 5.0))]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
