#!/usr/bin/env python3
"""
tests/golden/train_batch.npz: the ray batch and ground truth that the REFERENCE's trainer prepares
(train/trainlib/PixelNerfTrainer.py:84-123), captured on CPU with the draws that produced them.

Imports the reference the way tools/make_golden.py does (its stubs for the absent third-party modules) and runs, per
object and under a fixed torch.manual_seed, the trainer's own sequence: util.gen_rays of every view, the NHWC copy of
images * 0.5 + 0.5, util.bbox_sample or torch.randint, the two gathers.  The draws are recorded by seeding again and
drawing in the same order -- bbox_sample's randint, rand, rand (src/util/util.py:226-233), or the one randint of :112.

Two cameras x two modes:
  a: one scalar focal for both objects, no principal point given
  b: (fx, fy) and (cx, cy) per object
  *_uni: uniform over all pixels of all views;  *_box: inside per-view boxes `cmin rmin cmax rmax`, among them the whole
  image (touches all four borders), a box one pixel wide and a box one pixel high.
2 objects x 5 views of 24 x 16 (H x W), 64 rays per object.  The file is written with fixed zip timestamps, so a second
run gives the same bytes.

Usage:  python tools/make_train_batch_golden.py     (build container only: needs the reference checkout)
"""
import io
import os
import sys
import zipfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (sets the suite's CPU arithmetic before torch is imported)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pixel_nerf_yolo_amd import synth  # noqa: E402

SB, NV, H, W, B = 2, 5, 24, 16, 64
Z_NEAR, Z_FAR = 0.8, 1.8
SEEDS = {"a_uni": 101, "a_box": 102, "b_uni": 103, "b_box": 104}


def scene(case):
    images = torch.from_numpy(synth.images(900 + ord(case), SB * NV, H, W)).reshape(SB, NV, 3, H, W)
    poses = torch.from_numpy(np.stack([np.stack([synth.pose_spherical(37.0 * v + 11.0 * s, -20.0 - 3.0 * v, 1.3 + 0.1 * s)
                                                 for v in range(NV)]) for s in range(SB)]))
    if case == "a":
        focal, c = torch.tensor(21.5).expand(SB), None           # data["focal"] (SB,), the same scalar for both objects
    else:
        focal = torch.tensor([[19.0, 20.5], [23.25, 22.0]])
        c = torch.tensor([[7.5, 11.25], [8.75, 12.5]])
    # cmin rmin cmax rmax; view 0 of object 0: the whole image; view 1: one pixel wide; view 2: one pixel high
    rs = np.random.RandomState(77)
    bb = np.zeros((SB, NV, 4), dtype=np.float32)
    for s in range(SB):
        for v in range(NV):
            c0, c1 = sorted(rs.randint(0, W, size=2).tolist())
            r0, r1 = sorted(rs.randint(0, H, size=2).tolist())
            bb[s, v] = [c0, r0, c1, r1]
    bb[0, 0] = [0, 0, W - 1, H - 1]
    bb[0, 1] = [7, 3, 7, 20]
    bb[0, 2] = [2, 23, 13, 23]
    bb[1, 3] = [15, 0, 15, 0]                                     # a single pixel in the corner
    return images, poses, focal, c, torch.from_numpy(bb)


def trainer_batch(util, images, poses, focal, c, bboxes, seed):
    """PixelNerfTrainer.calc_losses:84-123 for the ray batch (source-view selection left out: it draws from numpy)."""
    torch.manual_seed(seed)
    all_rays, all_rgb, all_pix = [], [], []
    for obj in range(SB):
        images_0to1 = images[obj] * 0.5 + 0.5
        cam_rays = util.gen_rays(poses[obj], W, H, focal[obj], Z_NEAR, Z_FAR, c=None if c is None else c[obj])
        rgb_gt_all = images_0to1.permute(0, 2, 3, 1).contiguous().reshape(-1, 3)
        if bboxes is not None:
            pix = util.bbox_sample(bboxes[obj], B)
            pix_inds = pix[..., 0] * H * W + pix[..., 1] * W + pix[..., 2]
        else:
            pix_inds = torch.randint(0, NV * H * W, (B,))
            pix = torch.stack((pix_inds // (H * W), (pix_inds % (H * W)) // W, pix_inds % W), dim=-1)
        all_rgb.append(rgb_gt_all[pix_inds])
        all_rays.append(cam_rays.view(-1, cam_rays.shape[-1])[pix_inds])
        all_pix.append(pix)
    return torch.stack(all_rays), torch.stack(all_rgb), torch.stack(all_pix)


def redraw(bbox_mode, seed):
    torch.manual_seed(seed)
    out = {k: [] for k in (("image_ids", "u_x", "u_y") if bbox_mode else ("pix_inds",))}
    for _ in range(SB):
        if bbox_mode:
            out["image_ids"].append(torch.randint(0, NV, (B,)))
            out["u_x"].append(torch.rand(B))
            out["u_y"].append(torch.rand(B))
        else:
            out["pix_inds"].append(torch.randint(0, NV * H * W, (B,)))
    return {k: torch.stack(v) for k, v in out.items()}


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps (numpy stamps the current time)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    mg.install_shims()
    import util

    d = {"shape": np.array([SB, NV, H, W, B], dtype=np.int64), "z": np.array([Z_NEAR, Z_FAR], dtype=np.float32)}
    for case in ("a", "b"):
        images, poses, focal, c, bboxes = scene(case)
        d[case + "_images"], d[case + "_poses"] = mg.np_(images), mg.np_(poses)
        d[case + "_focal"] = mg.np_(focal[0] if case == "a" else focal)      # a: the scalar itself
        if c is not None:
            d[case + "_c"] = mg.np_(c)
        d[case + "_bboxes"] = mg.np_(bboxes)
        for mode in ("uni", "box"):
            key = "%s_%s" % (case, mode)
            bb = bboxes if mode == "box" else None
            rays, rgb, pix = trainer_batch(util, images, poses, focal, c, bb, SEEDS[key])
            draws = redraw(mode == "box", SEEDS[key])
            # the recorded draws are the ones the trainer consumed
            if mode == "uni":
                flat = pix[..., 0] * H * W + pix[..., 1] * W + pix[..., 2]
                assert torch.equal(flat, draws["pix_inds"])
            else:
                assert torch.equal(pix[..., 0], draws["image_ids"])
                inside = (pix[..., 2] >= 0) & (pix[..., 2] < W) & (pix[..., 1] >= 0) & (pix[..., 1] < H)
                assert bool(inside.all())
            d[key + "_rays"], d[key + "_rgb_gt"] = mg.np_(rays), mg.np_(rgb)
            d[key + "_pix"] = pix.numpy().astype(np.int32)
            for k, v in draws.items():
                d["%s_%s" % (key, k)] = v.numpy()
            print("captured", key, tuple(rays.shape), tuple(rgb.shape))
    path = os.path.join(mg.OUT, "train_batch.npz")
    write_npz(path, d)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
