#!/usr/bin/env python3
"""
tests/golden/yolo_train_batch.npz: the rays and target cells that the REFERENCE's YOLO trainer prepares for one object
(train/trainlib/YoloTrainer.py:93-129), captured on the CPU.

Imports the reference the way tools/make_train_batch_golden.py does (tools/make_golden.py's stubs for the absent third-party
modules, cv2 among them) and runs, per scale, the trainer's own sequence on the dataset's nested structure -- an NV-long list
of num_scales-long tuples of (1, Hs, Ws, A, 6) tensors --, restated in this tool's own words around the reference's own
util.gen_rays_yolo: the grids stacked per scale, the rays of the selected views at the scale's grid size with focal / cell
and c / cell, both taken at image_ord and flattened.

Three cases (fx != fy, an off-centre principal point, world->cam extrinsics with a real rotation everywhere):
  a: H = 40, W = 56, cells [8, 16, 32], NV = 5, views [4, 0, 2], A = 3 -- grids 5 x 7, 2 x 3, 1 x 1; 126 rays (not a multiple
     of 64), one ray per view in the last scale
  b: H = 70, W = 100, one scale of cell 32, NV = 2, views [1], A = 3 -- sizes the cell does not divide
  c: H = 64, W = 72, cells [4, 8], NV = 4, views [3, 1, 2], A = 2 -- 864 + 216 rays, several workgroups
Every target value encodes where it came from, ((((view * 4 + scale) * 16 + y) * 32 + x) * 4 + anchor) * 8 + field (exact in
fp32), so a wrong gather index shows.  The file is written with fixed zip timestamps: a second run gives the same bytes.

Usage:  python tools/make_yolo_batch_golden.py     (build container only: needs the reference checkout)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (sets the suite's CPU arithmetic before torch is imported)
from make_train_batch_golden import write_npz  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pixel_nerf_yolo_amd import synth  # noqa: E402

Z_NEAR, Z_FAR = 1.0, 6.0
CASES = {
    "a": dict(H=40, W=56, cells=[8, 16, 32], NV=5, views=[4, 0, 2], A=3, focal=[44.0, 47.5], c=[27.25, 21.5]),
    "b": dict(H=70, W=100, cells=[32], NV=2, views=[1], A=3, focal=[80.5, 77.0], c=[48.5, 36.25]),
    "c": dict(H=64, W=72, cells=[4, 8], NV=4, views=[3, 1, 2], A=2, focal=[60.0, 66.5], c=[37.0, 30.5]),
}


def extrinsics(case, nv):
    """world->cam of cameras on a sphere around the origin, every one at its own azimuth, elevation and distance."""
    flipyz = np.diag([1.0, -1.0, -1.0, 1.0])
    k = ord(case) - ord("a")
    return np.stack([np.linalg.inv(synth.pose_spherical(31.0 * v + 17.0 * k + 9.0, -18.0 - 4.0 * v, 3.6 + 0.2 * v + 0.1 * k).astype(np.float64)
                                   @ flipyz) for v in range(nv)]).astype(np.float32)


def dataset_bboxes(nv, H, W, cells, A):
    """data["bboxes"]: NV-long list of num_scales-long tuples of (1, Hs, Ws, A, 6)."""
    out = []
    for v in range(nv):
        per_scale = []
        for s, cell in enumerate(cells):
            hs, ws = H // cell, W // cell
            y, x, a, f = np.meshgrid(np.arange(hs), np.arange(ws), np.arange(A), np.arange(6), indexing="ij")
            code = ((((v * 4 + s) * 16 + y) * 32 + x) * 4 + a) * 8 + f
            assert hs <= 16 and ws <= 32 and code.max() < 2 ** 24
            per_scale.append(torch.from_numpy(code.astype(np.float32))[None])
        out.append(tuple(per_scale))
    return out


def trainer_batch(util, poses, bboxes, focal, c, image_ord, H, W, cells, A):
    """What YoloTrainer.calc_losses computes for one object on the CPU, per scale (line numbers of train/trainlib/YoloTrainer.py):
    the views' grids of the scale stacked to (NV, Hs, Ws, A, 6) (:97-101), the reference's own util.gen_rays_yolo of the selected
    views at the grid's size with the intrinsics divided by the cell (:104-115), rays and grids taken at image_ord and
    flattened (:120-125)."""
    rays, targets, grids = [], [], []
    for s, cell in enumerate(cells):
        grid = torch.stack([view[s] for view in bboxes]).squeeze(1)
        hs, ws = H // cell, W // cell
        r = util.gen_rays_yolo(poses[image_ord], ws, hs, focal / cell, c / cell, Z_NEAR, Z_FAR)
        assert tuple(r.shape) == (len(image_ord), hs, ws, 8)
        rays.append(r.reshape(-1, 8))
        targets.append(grid[image_ord].reshape(-1, A, 6))
        grids.append(grid)
    return rays, targets, grids


def main():
    mg.install_shims()
    import util

    d = {"z": np.array([Z_NEAR, Z_FAR], dtype=np.float32)}
    for case, k in CASES.items():
        poses = torch.from_numpy(extrinsics(case, k["NV"]))
        assert all(abs(float(torch.det(p[:3, :3])) - 1.0) < 1e-5 and float((p[:3, :3] - torch.eye(3)).abs().max()) > 0.1 for p in poses)
        focal, c = torch.tensor(k["focal"]), torch.tensor(k["c"])
        image_ord = torch.tensor(k["views"], dtype=torch.long)
        bboxes = dataset_bboxes(k["NV"], k["H"], k["W"], k["cells"], k["A"])
        rays, gts, stacked = trainer_batch(util, poses, bboxes, focal, c, image_ord, k["H"], k["W"], k["cells"], k["A"])
        d[case + "_shape"] = np.array([k["NV"], k["H"], k["W"], k["A"]], dtype=np.int64)
        d[case + "_cells"] = np.array(k["cells"], dtype=np.int64)
        d[case + "_views"] = image_ord.numpy()
        d[case + "_poses"], d[case + "_focal"], d[case + "_c"] = mg.np_(poses), mg.np_(focal), mg.np_(c)
        d[case + "_offsets"] = np.cumsum([0] + [r.shape[0] for r in rays]).astype(np.int64)
        for s in range(len(k["cells"])):
            d["%s_grid%d" % (case, s)] = mg.np_(stacked[s])          # the stacked (NV, Hs, Ws, A, 6) tensor of :101
            d["%s_rays%d" % (case, s)] = mg.np_(rays[s])
            d["%s_targets%d" % (case, s)] = mg.np_(gts[s])
        print("captured", case, [tuple(r.shape) for r in rays], [tuple(g.shape) for g in gts])
    path = os.path.join(mg.OUT, "yolo_train_batch.npz")
    write_npz(path, d)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
