"""
Data and image adapters either side of the rendering path: the dataset readers that feed
``PixelNeRFNet.encode`` / ``gen_rays`` and the writers / metrics that consume rendered frames.

Host-side Python mirroring the reference's interface (same class names, constructor arguments, item dictionaries):
  SRNDataset   reference src/data/SRNDataset.py:10-136
  YOLODataset  reference src/data/YOLODataset.py:10-225 (incl. the anchor / cell target assignment)
  DVRDataset   reference src/data/DVRDataset.py:11-275 (ShapeNet / NMR renderings and the DTU sub-format)
  MultiObjectDataset  reference src/data/MultiObjectDataset.py:14-117 (scenes of several ShapeNet objects, NeRF-style transforms.json)
  ColorJitterDataset  reference src/data/data_util.py:13-55 (training-time augmentation of ``dvr_dtu`` and ``yolo``;
                      ``defer=True`` only draws the factors, for ``augment.color_jitter`` to apply on the device)
  get_split_dataset  reference src/data/__init__.py:12-76 (types ``srn``, ``multi_obj``, ``dvr``, ``dvr_gen``, ``dvr_dtu`` and ``yolo``)
  psnr / ssim / write_views  what eval/eval.py:291-359 does with skimage / imageio
  ResidentViews  no counterpart in the reference: the decoded views of a whole split kept on the device as bytes, and a
                      training step (rays, ground truth, source views, cameras) drawn from them without the DataLoader

PARITY UNPINNED against the third-party libraries the reference uses here -- imageio (decoding), cv2 (resize, projection-
matrix decomposition), torchvision (colour jitter), skimage (metrics) are not importable in this environment, so the reference's classes cannot be imported to capture
goldens.  Decoding / encoding goes through Pillow; ``cv2.resize`` (bilinear) is restated with
``F.interpolate(mode="bilinear", align_corners=False)``, which agrees with OpenCV's INTER_LINEAR up to its fixed-point
rounding on uint8; the metrics follow the published definitions (skimage ``structural_similarity`` defaults: 7x7 uniform
window, sample covariance, K1 = 0.01, K2 = 0.03).  Everything is pinned at the tensor-contract level by
tests/test_cpu_data.py on synthetic directory trees.
"""
import glob
import os

import numpy as np
import torch
import torch.nn.functional as F


# ------------------------------------------------------------------ image io
def imread(path):
    """(H, W, C) uint8 array, as ``imageio.imread`` returns for 8-bit images."""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("RGB", "RGBA", "L"):
            im = im.convert("RGBA" if "A" in im.getbands() else "RGB")
        return np.array(im)


def imwrite(path, arr):
    """``imageio.imwrite`` for (H, W[, C]) uint8 arrays (format from the extension)."""
    from PIL import Image
    a = np.asarray(arr)
    assert a.dtype == np.uint8, "imwrite takes uint8 images"
    Image.fromarray(a).save(path)


def image_to_tensor_balanced(img):
    """util.get_image_to_tensor_balanced (reference util.py:70-77): ToTensor + Normalize(0.5, 0.5) -> (C, H, W) in [-1, 1]."""
    t = torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1).to(torch.float32).div(255.0)
    return (t - 0.5) / 0.5


def mask_to_tensor(mask):
    """util.get_mask_to_tensor (reference util.py:80-83): ToTensor + Normalize(0, 1) -> (1, H, W) in [0, 1]."""
    return torch.from_numpy(np.ascontiguousarray(mask)).permute(2, 0, 1).to(torch.float32).div(255.0)


def resize_bilinear_u8(img, fx, fy):
    """cv2.resize(img, (0, 0), fx=fx, fy=fy) (INTER_LINEAR) for uint8 (H, W, C): output size round(W fx) x round(H fy),
    half-pixel centres; rounded back to uint8."""
    h, w = img.shape[:2]
    oh, ow = int(round(h * fy)), int(round(w * fx))
    t = torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1)[None].to(torch.float32)
    out = F.interpolate(t, size=(oh, ow), mode="bilinear", align_corners=False)
    return out[0].permute(1, 2, 0).round().clamp(0, 255).to(torch.uint8).numpy()


# ------------------------------------------------------------------ SRN
class SRNDataset(torch.utils.data.Dataset):
    """reference src/data/SRNDataset.py: <path>_<stage>/<object>/{intrinsics.txt, rgb/*, pose/*}."""

    def __init__(self, path, stage="train", image_size=(128, 128), world_scale=1.0, ingest_on_device=False):
        super().__init__()
        self.ingest_on_device = ingest_on_device
        self.base_path = path + "_" + stage
        self.dataset_name = os.path.basename(path)
        print("Loading SRN dataset", self.base_path, "name:", self.dataset_name)
        self.stage = stage
        assert os.path.exists(self.base_path)
        is_chair = "chair" in self.dataset_name
        if is_chair and stage == "train":
            tmp = os.path.join(self.base_path, "chairs_2.0_train")
            if os.path.exists(tmp):
                self.base_path = tmp
        self.intrins = sorted(glob.glob(os.path.join(self.base_path, "*", "intrinsics.txt")))
        self.image_to_tensor = image_to_tensor_balanced
        self.mask_to_tensor = mask_to_tensor
        self.image_size = image_size
        self.world_scale = world_scale
        self._coord_trans = torch.diag(torch.tensor([1, -1, -1, 1], dtype=torch.float32))
        self.z_near, self.z_far = (1.25, 2.75) if is_chair else (0.8, 1.8)
        self.lindisp = False

    def __len__(self):
        return len(self.intrins)

    def __getitem__(self, index):
        intrin_path = self.intrins[index]
        dir_path = os.path.dirname(intrin_path)
        rgb_paths = sorted(glob.glob(os.path.join(dir_path, "rgb", "*")))
        pose_paths = sorted(glob.glob(os.path.join(dir_path, "pose", "*")))
        assert len(rgb_paths) == len(pose_paths)
        with open(intrin_path, "r") as fh:
            lines = fh.readlines()
            focal, cx, cy, _ = map(float, lines[0].split())
            height, width = map(int, lines[-1].split())
        if self.ingest_on_device:
            return self._item_u8(index, dir_path, rgb_paths, pose_paths, focal, cx, cy)
        all_imgs, all_poses, all_masks, all_bboxes = [], [], [], []
        for rgb_path, pose_path in zip(rgb_paths, pose_paths):
            img = imread(rgb_path)[..., :3]
            img_tensor = self.image_to_tensor(img)
            mask = (img != 255).all(axis=-1)[..., None].astype(np.uint8) * 255      # white background = outside
            mask_tensor = self.mask_to_tensor(mask)
            pose = torch.from_numpy(np.loadtxt(pose_path, dtype=np.float32).reshape(4, 4))
            pose = pose @ self._coord_trans
            rows, cols = np.any(mask, axis=1), np.any(mask, axis=0)
            rnz, cnz = np.where(rows)[0], np.where(cols)[0]
            if len(rnz) == 0:
                raise RuntimeError("ERROR: Bad image at", rgb_path, "please investigate!")
            rmin, rmax = rnz[[0, -1]]
            cmin, cmax = cnz[[0, -1]]
            all_bboxes.append(torch.tensor([cmin, rmin, cmax, rmax], dtype=torch.float32))
            all_imgs.append(img_tensor)
            all_masks.append(mask_tensor)
            all_poses.append(pose)
        all_imgs, all_poses = torch.stack(all_imgs), torch.stack(all_poses)
        all_masks, all_bboxes = torch.stack(all_masks), torch.stack(all_bboxes)
        if tuple(all_imgs.shape[-2:]) != tuple(self.image_size):
            scale = self.image_size[0] / all_imgs.shape[-2]
            focal *= scale
            cx *= scale
            cy *= scale
            all_bboxes *= scale
            all_imgs = F.interpolate(all_imgs, size=self.image_size, mode="area")
            all_masks = F.interpolate(all_masks, size=self.image_size, mode="area")
        if self.world_scale != 1.0:
            focal *= self.world_scale
            all_poses[:, :3, 3] *= self.world_scale
        return {
            "path": dir_path, "img_id": index, "focal": torch.tensor(focal, dtype=torch.float32),
            "c": torch.tensor([cx, cy], dtype=torch.float32), "images": all_imgs, "masks": all_masks, "bbox": all_bboxes,
            "poses": all_poses,
        }

    def _item_u8(self, index, dir_path, rgb_paths, pose_paths, focal, cx, cy):
        """ingest_on_device: the decoded bytes in place of images / masks / bbox, for
        ``augment.ingest_views(images_u8, size=image_size, resize="area", white_mask=True)``; focal and c already scaled."""
        imgs = np.stack([imread(p)[..., :3] for p in rgb_paths])
        poses = torch.stack([torch.from_numpy(np.loadtxt(p, dtype=np.float32).reshape(4, 4)) @ self._coord_trans for p in pose_paths])
        if tuple(imgs.shape[1:3]) != tuple(self.image_size):
            scale = self.image_size[0] / imgs.shape[1]
            focal *= scale
            cx *= scale
            cy *= scale
        if self.world_scale != 1.0:
            focal *= self.world_scale
            poses[:, :3, 3] *= self.world_scale
        return {
            "path": dir_path, "img_id": index, "focal": torch.tensor(focal, dtype=torch.float32),
            "c": torch.tensor([cx, cy], dtype=torch.float32), "images_u8": torch.from_numpy(np.ascontiguousarray(imgs)),
            "image_size": torch.tensor(self.image_size, dtype=torch.int64), "poses": poses,
        }


# ------------------------------------------------------------------ YOLO
def iou_wh(box_wh, anchors_wh):
    """util.iou(..., is_pred=False) (reference util.py:612-630): IoU of (w, h) pairs anchored at a common corner."""
    inter = torch.min(box_wh[..., 0], anchors_wh[..., 0]) * torch.min(box_wh[..., 1], anchors_wh[..., 1])
    union = box_wh[..., 0] * box_wh[..., 1] + anchors_wh[..., 0] * anchors_wh[..., 1] - inter
    return inter / union


class YOLODataset(torch.utils.data.Dataset):
    """reference src/data/YOLODataset.py: <path>/{train,val,test}.lst of scene directories holding image_XXXX.png,
    extrinsic_XXXX.npy, intrinsic_0000.npy and projected_bboxes_XXXX.txt (cls cx cy w h, normalised)."""

    def __init__(self, path, stage="train", z_near=1.2, z_far=4.0, conf=None, ingest_on_device=False):
        super().__init__()
        self.ingest_on_device = ingest_on_device
        self.base_path = path
        assert os.path.exists(self.base_path)
        with open(os.path.join(self.base_path, {"train": "train.lst", "val": "val.lst", "test": "test.lst"}[stage]), "r") as fh:
            self.all_objs = [x.strip() for x in fh.readlines()]
        self.stage = stage
        self.image_to_tensor = image_to_tensor_balanced
        self.mask_to_tensor = mask_to_tensor
        print("Loading YOLO dataset", self.base_path, "stage", stage, len(self.all_objs), "objs")
        self.image_scale = conf["yolo.image_scale"]
        self.z_near, self.z_far = z_near, z_far
        self.num_scales = conf["model.mlp_coarse.num_scales"]
        self.num_anchors_per_scale = conf["model.mlp_coarse.num_anchors_per_scale"]
        self.cell_sizes = conf["yolo.cell_sizes"][:self.num_scales]
        anchors = conf["yolo.anchors"][:self.num_scales]
        self.anchors = torch.tensor([item for sub in anchors for item in sub], dtype=torch.float32)
        self.ignore_iou_thresh = conf["yolo.ignore_iou_thresh"]

    def __len__(self):
        return len(self.all_objs)

    def __getitem__(self, index):
        root_dir = os.path.join(self.base_path, self.all_objs[index])
        all_imgs, all_poses, all_bboxes = [], [], []
        n = 0
        while os.path.exists(os.path.join(root_dir, "image_{:04d}.png".format(n))):   # the reference stops at the first failing read
            img = imread(os.path.join(root_dir, "image_{:04d}.png".format(n)))[..., :3]
            if self.ingest_on_device:
                all_imgs.append(img)
            else:
                img = resize_bilinear_u8(img, self.image_scale[0], self.image_scale[1])
                all_imgs.append(self.image_to_tensor(img))
            n += 1
        for i in range(n):
            pose = np.load(os.path.join(root_dir, "extrinsic_{:04d}.npy".format(i))).copy()
            pose[0] = pose[0] * -1                                                     # YOLODataset.py:112
            all_poses.append(torch.tensor(pose, dtype=torch.float32))
        for i in range(n):
            bb = np.roll(np.loadtxt(os.path.join(root_dir, "projected_bboxes_{:04d}.txt".format(i)), delimiter=" ", ndmin=2),
                         4, axis=1).tolist()                                           # -> cx, cy, w, h, cls
            all_bboxes.append(bb if self.ingest_on_device else self._get_all_bboxes(bb, all_imgs[i].shape[1], all_imgs[i].shape[2]))
        intrinsic = np.load(os.path.join(root_dir, "intrinsic_0000.npy"))
        focal = torch.tensor(intrinsic[0, 0] * np.array(self.image_scale), dtype=torch.float32)
        c = torch.tensor(intrinsic[:2, 2] * self.image_scale, dtype=torch.float32)
        if self.ingest_on_device:
            # the decoded bytes and the label rows in place of images / bboxes, for ``augment.ingest_views(images_u8,
            # scale=image_scale)`` and ``util.build_yolo_targets(labels, n_labels, ...)``
            labels = np.zeros((n, max([len(bb) for bb in all_bboxes] + [1]), 5), np.float64)
            for i, bb in enumerate(all_bboxes):
                if len(bb):
                    labels[i, :len(bb)] = np.asarray(bb, np.float64)
            return {"path": root_dir, "img_id": index, "focal": focal, "images_u8": torch.from_numpy(np.stack(all_imgs)),
                    "labels": torch.from_numpy(labels), "n_labels": torch.tensor([len(bb) for bb in all_bboxes], dtype=torch.int32),
                    "image_scale": torch.tensor(self.image_scale, dtype=torch.float64), "poses": torch.stack(all_poses), "c": c}
        return {"path": root_dir, "img_id": index, "focal": focal, "images": torch.stack(all_imgs), "bboxes": all_bboxes,
                "poses": torch.stack(all_poses), "c": c}

    def _get_all_bboxes(self, bboxes, height, width):
        """Target grids per scale, (s_h, s_w, A, 6) = [objectness, x_cell, y_cell, w_cells, h_cells, class]: each box goes
        to the best free anchor of every scale; other anchors above the IoU threshold are marked -1 (ignored)."""
        grid_sizes = [(height // cs, width // cs) for cs in self.cell_sizes]
        targets = [torch.zeros((s_h, s_w, self.num_anchors_per_scale, 6)) for (s_h, s_w) in grid_sizes]
        for box in bboxes:
            iou_anchors = iou_wh(torch.tensor(box[2:4]), self.anchors)
            anchor_indices = iou_anchors.argsort(descending=True, dim=0)
            x, y, box_width, box_height, class_label = box
            has_anchor = [False] * self.num_scales
            for anchor_idx in anchor_indices:
                scale_idx = int(anchor_idx // self.num_anchors_per_scale)
                anchor_on_scale = int(anchor_idx % self.num_anchors_per_scale)
                s_h, s_w = grid_sizes[scale_idx]
                i, j = int(s_h * y), int(s_w * x)
                anchor_taken = targets[scale_idx][i, j, anchor_on_scale, 0]
                if not anchor_taken and not has_anchor[scale_idx]:
                    targets[scale_idx][i, j, anchor_on_scale, 0] = 1
                    targets[scale_idx][i, j, anchor_on_scale, 1:5] = torch.tensor(
                        [s_w * x - j, s_h * y - i, box_width * s_w, box_height * s_h])
                    targets[scale_idx][i, j, anchor_on_scale, 5] = int(class_label)
                    has_anchor[scale_idx] = True
                elif not anchor_taken and iou_anchors[anchor_idx] > self.ignore_iou_thresh:
                    targets[scale_idx][i, j, anchor_on_scale, 0] = -1
        return tuple(targets)


def get_split_dataset(dataset_type, datadir, want_split="all", training=True, jitter_on_device=False, ingest_on_device=False,
                      **kwargs):
    """reference src/data/__init__.py:12-76: dataset class + flags per type name; the training split of ``dvr_dtu`` and
    ``yolo`` is wrapped in the colour-jitter augmentation.  ``jitter_on_device=True`` defers that augmentation: the items
    carry their factors (``ColorJitterDataset(defer=True)``) and the trainer applies them with ``augment.color_jitter``.
    ``ingest_on_device=True`` (``srn`` and ``yolo``) makes the items carry the decoded bytes (and, for ``yolo``, the label rows)
    for ``augment.ingest_views`` / ``util.build_yolo_targets`` instead of resized, normalised tensors and target grids; with
    ``yolo`` it needs ``jitter_on_device=True`` for the training split, since the host jitter has no images to work on."""
    flags, aug, aug_flags = {}, None, {}
    if ingest_on_device:
        if dataset_type.startswith("dvr") or dataset_type == "multi_obj":
            raise NotImplementedError(
                "ingest_on_device is not implemented for dataset type %r (%s): its masks come from files and it needs no resize "
                "kernel; augment.color_jitter already takes its decoded bytes"
                % (dataset_type, "MultiObjectDataset" if dataset_type == "multi_obj" else "DVRDataset"))
        flags["ingest_on_device"] = True
    if dataset_type == "srn":
        dset_class = SRNDataset
    elif dataset_type == "multi_obj":
        dset_class = MultiObjectDataset
    elif dataset_type.startswith("dvr"):
        dset_class = DVRDataset
        if dataset_type == "dvr_gen":
            flags["list_prefix"] = "gen_"
        elif dataset_type == "dvr_dtu":
            flags.update(list_prefix="new_", sub_format="dtu", scale_focal=False, z_near=0.1, z_far=5.0)
            if training:
                flags["max_imgs"] = 49
            aug, aug_flags = ColorJitterDataset, {"extra_inherit_attrs": ["sub_format"]}
    elif dataset_type == "yolo":
        dset_class = YOLODataset
        flags["z_near"], flags["z_far"] = 1, 13.0
        aug = ColorJitterDataset
    else:
        raise NotImplementedError("dataset type %r is not implemented here (srn, multi_obj, dvr, dvr_gen, dvr_dtu, yolo)" % dataset_type)
    want_train = want_split not in ("val", "test")
    want_val = want_split not in ("train", "test")
    want_test = want_split not in ("train", "val")
    sets = [dset_class(datadir, stage=st, **flags, **kwargs) if want else None
            for st, want in (("train", want_train), ("val", want_val), ("test", want_test))]
    if sets[0] is not None and aug is not None:
        if ingest_on_device and not jitter_on_device:
            raise ValueError("ingest_on_device=True with the training split of %r needs jitter_on_device=True: the items carry "
                             "bytes, which the host jitter cannot work on" % dataset_type)
        sets[0] = aug(sets[0], defer=jitter_on_device, **aug_flags)
    if want_split in ("train", "val", "test"):
        return sets[("train", "val", "test").index(want_split)]
    return tuple(sets)


# ------------------------------------------------------------------ DVR (ShapeNet 64x64 / NMR, DTU)
def decompose_projection(P):
    """cv2.decomposeProjectionMatrix(P)[:3] for a 3x4 projection P = K [R | -R C]: the upper-triangular calibration K with a
    positive diagonal and the rotation R from an RQ factorisation of P[:, :3], and the camera centre C as a homogeneous
    4-vector (the null vector of P, scaled like OpenCV's: unit norm)."""
    import scipy.linalg
    P = np.asarray(P, dtype=np.float64)
    K, R = scipy.linalg.rq(P[:, :3])
    sign = np.diag(np.sign(np.diag(K)))          # RQ is unique up to the signs of K's diagonal
    K, R = K @ sign, sign @ R
    _, _, vt = np.linalg.svd(P)
    c = vt[-1]
    return K, R, c[:, None]


class DVRDataset(torch.utils.data.Dataset):
    """Objects of the DVR release (Niemeyer et al. 2020): <root>/<category>/<object>/{image/*.png|jpg, mask/*.png,
    cameras.npz}, split lists <root>/<category>/<list_prefix><stage>.lst.  Item = {path, img_id, focal, images (NV, 3, H, W)
    in [-1, 1], poses (NV, 4, 4) camera-to-world in the renderer's convention, masks?, and c (DTU) or bbox (ShapeNet)}."""

    def __init__(self, path, stage="train", list_prefix="softras_", image_size=None, sub_format="shapenet", scale_focal=True,
                 max_imgs=100000, z_near=1.2, z_far=4.0, skip_step=None, conf=None):
        super().__init__()
        assert os.path.exists(path), path
        assert stage in ("train", "val", "test")
        self.base_path, self.stage = path, stage
        self.all_objs = []
        for cat_dir in (d for d in glob.glob(os.path.join(path, "*")) if os.path.isdir(d)):
            lst = os.path.join(cat_dir, list_prefix + stage + ".lst")
            if os.path.exists(lst):
                with open(lst) as fh:
                    self.all_objs += [(os.path.basename(cat_dir), os.path.join(cat_dir, ln.strip())) for ln in fh.readlines()]
        self.image_to_tensor, self.mask_to_tensor = image_to_tensor_balanced, mask_to_tensor
        self.image_size = image_size
        flip_yz = torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0]))
        # world frame: DTU keeps its axes up to the y/z flip, ShapeNet's z-up objects are turned to y-up
        self._coord_trans_world = flip_yz if sub_format == "dtu" else torch.tensor(
            [[1.0, 0, 0, 0], [0, 0, -1.0, 0], [0, 1.0, 0, 0], [0, 0, 0, 1.0]])
        self._coord_trans_cam = flip_yz            # OpenCV camera (y down, z forward) -> OpenGL camera
        self.sub_format, self.scale_focal, self.max_imgs = sub_format, scale_focal, max_imgs
        self.z_near, self.z_far, self.lindisp = z_near, z_far, False

    def __len__(self):
        return len(self.all_objs)

    def __getitem__(self, index):
        _, root = self.all_objs[index]
        rgb_paths = sorted(f for f in glob.glob(os.path.join(root, "image", "*")) if f.endswith((".jpg", ".png")))
        mask_paths = sorted(glob.glob(os.path.join(root, "mask", "*.png"))) or [None] * len(rgb_paths)
        sel = np.arange(len(rgb_paths))
        if len(rgb_paths) > self.max_imgs:
            sel = np.random.choice(len(rgb_paths), self.max_imgs, replace=False)
            rgb_paths, mask_paths = [rgb_paths[i] for i in sel], [mask_paths[i] for i in sel]
        cams = np.load(os.path.join(root, "cameras.npz"))
        dtu = self.sub_format != "shapenet"
        imgs, poses, masks, bboxes = [], [], [], []
        focal, intr_sum = None, torch.zeros(4, dtype=torch.float64)     # DTU: fx, fy, cx, cy averaged over the views
        for i, rgb_path, mask_path in zip(sel, rgb_paths, mask_paths):
            img = imread(rgb_path)[..., :3]
            # scale_focal: intrinsics are given for an image spanning [-1, 1]
            xs, ys, delta = (img.shape[1] / 2.0, img.shape[0] / 2.0, 1.0) if self.scale_focal else (1.0, 1.0, 0.0)
            if dtu:
                K, R, t = decompose_projection(cams["world_mat_%d" % i][:3])
                K = K / K[2, 2]
                pose = np.eye(4, dtype=np.float32)
                pose[:3, :3] = R.T
                pose[:3, 3] = (t[:3] / t[3])[:, 0]
                scale = cams.get("scale_mat_%d" % i)
                if scale is not None:                                # normalisation of the scene into the unit sphere
                    pose[:3, 3:] -= scale[:3, 3:]
                    pose[:3, 3:] /= np.diagonal(scale[:3, :3])[..., None]
                intr_sum += torch.tensor([K[0, 0] * xs, K[1, 1] * ys, (K[0, 2] + delta) * xs, (K[1, 2] + delta) * ys])
            else:
                if "world_mat_inv_%d" % i in cams:
                    pose = cams["world_mat_inv_%d" % i]
                else:
                    w = cams["world_mat_%d" % i]
                    if w.shape[0] == 3:
                        w = np.vstack((w, np.array([0, 0, 0, 1])))
                    pose = np.linalg.inv(w)
                intr = cams["camera_mat_%d" % i]
                assert abs(intr[0, 0] - intr[1, 1]) < 1e-9
                f = intr[0, 0] * xs
                assert focal is None or abs(f - focal) < 1e-5, "views of one object must share the focal length"
                focal = f
            poses.append(self._coord_trans_world @ torch.tensor(pose, dtype=torch.float32) @ self._coord_trans_cam)
            imgs.append(self.image_to_tensor(img))
            if mask_path is not None:
                mask = imread(mask_path)
                mask = (mask[..., None] if mask.ndim == 2 else mask)[..., :1]
                rows, cols = np.where(np.any(mask, axis=1))[0], np.where(np.any(mask, axis=0))[0]
                if len(rows) == 0:
                    raise RuntimeError("empty mask for " + rgb_path)
                masks.append(self.mask_to_tensor(mask))
                bboxes.append(torch.tensor([cols[0], rows[0], cols[-1], rows[-1]], dtype=torch.float32))
        images, poses = torch.stack(imgs), torch.stack(poses)
        masks = torch.stack(masks) if masks else None
        if dtu:
            intr = (intr_sum / len(rgb_paths)).to(torch.float32)
            focal, c, bbox = intr[:2].clone(), intr[2:].clone(), None
        else:
            focal, c, bbox = focal, None, (torch.stack(bboxes) if bboxes else [])
        if self.image_size is not None and tuple(images.shape[-2:]) != tuple(self.image_size):
            scale = self.image_size[0] / images.shape[-2]
            focal = focal * scale
            if dtu:
                c = c * scale
            elif len(bbox):
                bbox = bbox * scale
            images = F.interpolate(images, size=tuple(self.image_size), mode="area")
            if masks is not None:
                masks = F.interpolate(masks, size=tuple(self.image_size), mode="area")
        item = {"path": root, "img_id": index, "focal": focal, "images": images, "poses": poses}
        if masks is not None:
            item["masks"] = masks
        if dtu:
            item["c"] = c
        else:
            item["bbox"] = bbox
        return item


# ------------------------------------------------------------------ multi-object scenes
class MultiObjectDataset(torch.utils.data.Dataset):
    """<root>/<stage>/**/transforms.json (camera_angle_x, frames[file_path, transform_matrix]) with <basename>_obj.png RGBA
    renderings beside it.  Item = {path, img_id, focal, images (NV, 3, H, W) composited on white, masks (NV, 1, H, W) = alpha,
    bbox (NV, 4) of the non-empty pixels, poses (NV, 4, 4)}; an instance whose view count differs from ``n_views`` yields {}."""

    def __init__(self, path, stage="train", z_near=4, z_far=9, n_views=None):
        super().__init__()
        self.base_path = os.path.join(path, stage)
        self.trans_files = sorted(os.path.join(root, "transforms.json") for root, _, files in os.walk(self.base_path)
                                  if "transforms.json" in files)
        self.image_to_tensor, self.mask_to_tensor = image_to_tensor_balanced, mask_to_tensor
        self.z_near, self.z_far, self.lindisp, self.n_views = z_near, z_far, False, n_views

    def __len__(self):
        return len(self.trans_files)

    def _check_valid(self, index):
        if self.n_views is None:
            return True
        import json
        trans_file = self.trans_files[index]
        try:
            with open(trans_file) as fh:
                transform = json.load(fh)
        except Exception:
            return False
        return (len(transform["frames"]) == self.n_views and
                len(glob.glob(os.path.join(os.path.dirname(trans_file), "*.png"))) == self.n_views)

    def __getitem__(self, index):
        import json
        if not self._check_valid(index):
            return {}
        trans_file = self.trans_files[index]
        dir_path = os.path.dirname(trans_file)
        with open(trans_file) as fh:
            transform = json.load(fh)
        imgs, masks, bboxes, poses = [], [], [], []
        for frame in transform["frames"]:
            base = os.path.splitext(os.path.basename(frame["file_path"]))[0]
            img = imread(os.path.join(dir_path, base + "_obj.png"))
            mask = self.mask_to_tensor(img[..., 3:4])
            rows, cols = np.where(np.any(img, axis=(1, 2)))[0], np.where(np.any(img, axis=(0, 2)))[0]
            if len(rows) == 0:
                box = [0, 0, mask.shape[-1], mask.shape[-2]]
            else:
                box = [cols[0], rows[0], cols[-1], rows[-1]]
            bboxes.append(torch.tensor(box, dtype=torch.float32))
            imgs.append(self.image_to_tensor(img[..., :3]) * mask + (1.0 - mask))     # white where transparent
            masks.append(mask)
            poses.append(torch.tensor(frame["transform_matrix"]))
        images = torch.stack(imgs)
        focal = 0.5 * images.shape[-1] / np.tan(0.5 * transform.get("camera_angle_x"))
        return {"path": dir_path, "img_id": index, "focal": focal, "images": images, "masks": torch.stack(masks),
                "bbox": torch.stack(bboxes), "poses": torch.stack(poses)}


# ------------------------------------------------------------------ colour jitter (training-time augmentation)
def _gray(img):
    return (0.2989 * img[..., 0, :, :] + 0.587 * img[..., 1, :, :] + 0.114 * img[..., 2, :, :]).unsqueeze(-3)


def _blend(a, b, ratio):
    return (ratio * a + (1.0 - ratio) * b).clamp(0.0, 1.0)


def adjust_brightness(img, factor):
    """torchvision ``adjust_brightness`` on a float (3, H, W) image in [0, 1]: blend with black."""
    return _blend(img, torch.zeros_like(img), factor)


def adjust_contrast(img, factor):
    """blend with the mean grey level of the image."""
    return _blend(img, _gray(img).mean(dim=(-3, -2, -1), keepdim=True), factor)


def adjust_saturation(img, factor):
    """blend with the grey image."""
    return _blend(img, _gray(img), factor)


def adjust_hue(img, factor):
    """rotate the hue by ``factor`` (in turns, |factor| <= 0.5): RGB -> HSV, h <- (h + factor) mod 1, HSV -> RGB."""
    assert -0.5 <= factor <= 0.5
    r, g, b = img.unbind(-3)
    maxc, minc = img.max(-3).values, img.min(-3).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    crd = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / crd, (maxc - g) / crd, (maxc - b) / crd
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = torch.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0)
    h = (h + factor) % 1.0
    i = torch.floor(h * 6.0)
    f = h * 6.0 - i
    i = i.to(torch.int32) % 6
    v = maxc
    p, q, t = (v * (1.0 - s)).clamp(0, 1), (v * (1.0 - s * f)).clamp(0, 1), (v * (1.0 - s * (1.0 - f))).clamp(0, 1)
    sel = i.unsqueeze(-3) == torch.arange(6, device=img.device).view(-1, 1, 1)
    a1 = torch.stack((v, q, p, p, t, v), dim=-3)
    a2 = torch.stack((t, v, v, q, p, p), dim=-3)
    a3 = torch.stack((p, p, t, v, v, q), dim=-3)
    a4 = torch.stack((a1, a2, a3), dim=-4)
    return torch.einsum("...ijk,...xijk->...xjk", sel.to(img.dtype), a4)


class ColorJitterDataset(torch.utils.data.Dataset):
    """Wraps a dataset: ONE random (hue, saturation, brightness, contrast) draw per item, applied to all of its views
    (images are mapped from [-1, 1] to [0, 1] and back; order saturation, hue, contrast, brightness).
    ``defer=True`` makes the same draw but leaves ``images`` as they are and adds ``data["jitter"]``, the (4,) fp32 factors
    {hue, saturation, brightness, contrast} (collated to (SB, 4)), for ``augment.color_jitter`` to apply on the device."""

    def __init__(self, base_dset, hue_range=0.1, saturation_range=0.1, brightness_range=0.1, contrast_range=0.1,
                 extra_inherit_attrs=(), defer=False):
        self.defer = defer
        self.hue_range = [-hue_range, hue_range]
        self.saturation_range = [1 - saturation_range, 1 + saturation_range]
        self.brightness_range = [1 - brightness_range, 1 + brightness_range]
        self.contrast_range = [1 - contrast_range, 1 + contrast_range]
        self.base_dset = base_dset
        for attr in ["z_near", "z_far", "base_path", "image_to_tensor", *extra_inherit_attrs]:
            setattr(self, attr, getattr(base_dset, attr))

    def draw_factors(self):
        """The item's four draws, in the order the reference makes them."""
        hue, sat = np.random.uniform(*self.hue_range), np.random.uniform(*self.saturation_range)
        bri, con = np.random.uniform(*self.brightness_range), np.random.uniform(*self.contrast_range)
        return hue, sat, bri, con

    def apply_color_jitter(self, images):
        hue, sat, bri, con = self.draw_factors()
        for i in range(len(images)):
            t = (images[i] + 1.0) * 0.5
            t = adjust_brightness(adjust_contrast(adjust_hue(adjust_saturation(t, sat), hue), con), bri)
            images[i] = t * 2.0 - 1.0
        return images

    def __len__(self):
        return len(self.base_dset)

    def __getitem__(self, idx):
        data = self.base_dset[idx]
        if self.defer:
            data["jitter"] = torch.tensor(self.draw_factors(), dtype=torch.float32)
        else:
            data["images"] = self.apply_color_jitter(data["images"])
        return data


# ------------------------------------------------------------------ resident views
_WHO_RV = "pixel_nerf_yolo_amd.data.ResidentViews"


def _host_ids(v, name, who, ndim):
    """``v`` as a host int64 array of ``ndim`` dimensions, or None when it is a device tensor (used as it is, clamped by the
    kernels); an error that names the argument otherwise."""
    if isinstance(v, torch.Tensor):
        if v.device.type != "cpu":
            if v.dtype not in (torch.int32, torch.int64) or v.dim() != ndim:
                raise ValueError("%s: %s on the device must be an int32 or int64 tensor of %d dimension%s, got %s %s"
                                 % (who, name, ndim, "" if ndim == 1 else "s", tuple(v.shape), v.dtype))
            return None
        v = v.numpy()
    a = np.asarray(v)
    if a.ndim != ndim or a.size == 0 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("%s: %s must be %d-dimensional, non-empty and of integers, got shape %s %s" % (who, name, ndim, a.shape, a.dtype))
    return a.astype(np.int64)


def _pair_of(v, name, kind, who):
    try:
        a, b = (kind(x) for x in v)
    except (TypeError, ValueError):
        raise ValueError(who + "%s must be a pair, got %r" % (name, v))
    return a, b


class ResidentViews:
    """A dataset's decoded views kept on the device as bytes, once, and a training step drawn straight from them
    (include/pnyolo.h "resident views").  What the DataLoader path does per step -- decode ALL views of every
    object of the super-batch, copy them over, normalise and resize them -- is done for the pixels and source views the step
    keeps: ``batch`` is one launch for the rays and their ground truth, one for the source views, and device-side indexing of
    the small camera tensors; nothing waits for the device.

    One decoded geometry (H, W, C), fixed by the first ``add``, and one output geometry: ``scale=(fx, fy)`` (bilinear_u8, the
    ``yolo`` dataset's rule), ``size=(OH, OW)`` with ``resize="area"`` (``srn``) or ``"bilinear_u8"``, or neither (no resize),
    as ``augment.ingest_views`` takes them.  ``white_bbox=True`` computes SRN's boxes once, when an object is added.
    ``device="cpu"`` holds the store for bookkeeping only: ``batch`` and ``source_views`` then raise PnyError."""

    def __init__(self, device, size=None, scale=None, resize=None, white_bbox=False):
        from . import lib as _lib
        who = _WHO_RV + ": "
        self.device = torch.device(device)
        if resize is not None and resize not in _lib.RESIZE:
            raise ValueError(who + "resize must be None, 'none', 'bilinear_u8' or 'area', got %r" % (resize,))
        if scale is not None and size is not None:
            raise ValueError(who + "scale and size are both given; scale=(fx, fy) or size=(OH, OW)")
        if scale is not None:
            if resize not in (None, "bilinear_u8"):
                raise ValueError(who + "scale goes with resize='bilinear_u8' (cv2's output-size rule), got resize=%r" % (resize,))
            scale, resize = _pair_of(scale, "scale", float, who), "bilinear_u8"
        elif size is not None:
            if resize not in ("area", "bilinear_u8"):
                raise ValueError(who + "size needs resize='area' or resize='bilinear_u8', got resize=%r" % (resize,))
            size = _pair_of(size, "size", int, who)
            if min(size) < 1:
                raise ValueError(who + "size must be positive, got %r" % (size,))
        elif resize not in (None, "none"):
            raise ValueError(who + "resize=%r needs size=(OH, OW)%s" % (resize, " or scale=(fx, fy)" if resize == "bilinear_u8" else ""))
        else:
            resize = "none"
        if white_bbox and resize == "bilinear_u8":
            raise ValueError(who + "white_bbox goes with resize='area' or no resize (no dataset resizes a mask bilinearly)")
        self.resize, self._size, self._scale, self.white_bbox = resize, size, scale, bool(white_bbox)
        self.decoded = None            # (H, W, C) of every view of the store
        self.out_size = None           # (OH, OW)
        self._views, self._poses, self._focal, self._c, self._bbox, self._labels = [], [], [], [], [], []
        self._tab = None               # the device tables of the objects added so far; rebuilt, never rewritten

    # ---- filling
    def add(self, images_u8, poses, focal, c=None, bbox=None, labels=None):
        """One object: ``images_u8`` (NV, H, W, C) uint8 on the host or the device, C = 3 or 4 (alpha ignored); ``poses``
        (NV, 4, 4) cam->world; ``focal`` a scalar or (fx, fy), ``c`` None (the image centre) or (cx, cy) and ``bbox`` None or
        (NV, 4) `cmin rmin cmax rmax`, all at OUTPUT resolution, as the ``ingest_on_device`` items carry them; ``labels`` anything
        (the item's YOLO rows), kept on the host for ``labels(obj)``.  Returns the object's index."""
        who = _WHO_RV + ".add: "
        img = torch.from_numpy(np.ascontiguousarray(images_u8)) if isinstance(images_u8, np.ndarray) else images_u8
        if not isinstance(img, torch.Tensor):
            raise TypeError(who + "images_u8 must be a tensor or an array, got %s" % type(images_u8).__name__)
        if img.dtype != torch.uint8 or img.dim() != 4 or img.shape[-1] not in (3, 4) or img.numel() == 0:
            raise ValueError(who + "images_u8 must be (NV, H, W, C) uint8 with C = 3 or 4, got %s %s" % (tuple(img.shape), img.dtype))
        nv, geom = int(img.shape[0]), tuple(int(v) for v in img.shape[1:])
        if self.decoded is not None and geom != self.decoded:
            raise ValueError(who + "images_u8 is (H, W, C) = %s; the store holds %s (one decoded geometry)" % (geom, self.decoded))
        h, w = geom[:2]
        if self._scale is not None:
            oh, ow = int(round(h * self._scale[1])), int(round(w * self._scale[0]))
            if oh < 1 or ow < 1:
                raise ValueError(who + "scale %r gives an empty %d x %d output" % (self._scale, oh, ow))
        else:
            oh, ow = self._size if self._size is not None else (h, w)
        if nv * oh * ow >= 2 ** 32:
            raise ValueError(who + "images_u8: n_views * OH * OW = %d * %d * %d must be below 2^32 (the draw's limit)" % (nv, oh, ow))
        p = torch.as_tensor(poses).detach().to("cpu", torch.float32)
        if tuple(p.shape) != (nv, 4, 4):
            raise ValueError(who + "poses must be (%d, 4, 4), got %s" % (nv, tuple(p.shape)))
        f = torch.as_tensor(focal).detach().to("cpu", torch.float32).reshape(-1)
        if f.numel() not in (1, 2):
            raise ValueError(who + "focal must be a scalar or (fx, fy), got shape %s" % (tuple(torch.as_tensor(focal).shape),))
        f = f.repeat(2) if f.numel() == 1 else f
        cc = torch.tensor([ow * 0.5, oh * 0.5], dtype=torch.float32) if c is None else \
            torch.as_tensor(c).detach().to("cpu", torch.float32).reshape(-1)
        if cc.numel() != 2:
            raise ValueError(who + "c must be None or (cx, cy), got shape %s" % (tuple(torch.as_tensor(c).shape),))
        img = img.detach().to(self.device).contiguous()
        if self.white_bbox:
            if bbox is not None:
                raise ValueError(who + "bbox is given and the store computes its own (white_bbox=True)")
            from . import augment
            _, _, bb = augment.ingest_views(img, size=self._size, resize=None if self.resize == "none" else self.resize, white_mask=True)
            bb = bb.cpu()                                   # fill time may wait
            empty = (bb[:, 2] < 0).nonzero().reshape(-1)
            if empty.numel():
                raise ValueError(who + "images_u8[%d] has an empty white-background mask (every pixel has a byte at 255): "
                                 "no box to sample from" % int(empty[0]))
        elif bbox is not None:
            bb = torch.as_tensor(bbox).detach().to("cpu", torch.float32)
            if tuple(bb.shape) != (nv, 4):
                raise ValueError(who + "bbox must be (%d, 4) `cmin rmin cmax rmax`, got %s" % (nv, tuple(bb.shape)))
        else:
            bb = None
        if self._views and (bb is None) != (self._bbox[0] is None):
            raise ValueError(who + "bbox is %s, the objects of the store %s boxes: all or none"
                             % ("None" if bb is None else "given", "have no" if self._bbox[0] is None else "have"))
        self.decoded, self.out_size = geom, (oh, ow)
        self._views.append(img)
        self._poses.append(p.contiguous())
        self._focal.append(f)
        self._c.append(cc)
        self._bbox.append(bb)
        self._labels.append(labels)
        self._tab = None
        return len(self._views) - 1

    @classmethod
    def from_dataset(cls, dset, device, indices=None, white_bbox=None):
        """The objects ``indices`` (default: all) of a dataset of this module.  ``ingest_on_device=True`` items (``srn``: area
        resize to the item's ``image_size`` and, unless ``white_bbox=False``, the white-background boxes; ``yolo``: the item's
        ``image_scale`` and label rows) are taken as they are.  Items that carry fp32 ``images`` (``dvr``, ``dvr_gen``,
        ``dvr_dtu``, ``multi_obj``) are re-quantised to bytes; an image that is not the byte map of bytes is refused."""
        who = _WHO_RV + ".from_dataset: "
        store = None
        for i in (range(len(dset)) if indices is None else indices):
            it = dset[int(i)]
            if not it:                                       # MultiObjectDataset's {} for an instance it skips
                continue
            if "images_u8" in it:
                u8 = it["images_u8"]
                if store is None:
                    if "image_scale" in it:
                        store = cls(device, scale=tuple(float(v) for v in it["image_scale"]))
                    else:
                        size = tuple(int(v) for v in it["image_size"])
                        resized = size != tuple(u8.shape[1:3])
                        store = cls(device, size=size if resized else None, resize="area" if resized else None,
                                    white_bbox=True if white_bbox is None else white_bbox)
                labels = (it["labels"], it["n_labels"]) if "labels" in it else None
                store.add(u8, it["poses"], it["focal"], c=it.get("c"), labels=labels)
                continue
            x = it["images"]
            if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
                raise ValueError(who + "item %d: images must be (NV, 3, H, W) fp32, got %s" % (int(i), getattr(x, "shape", type(x))))
            u8 = ((x * 0.5 + 0.5) * 255.0).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
            back = ((u8.permute(0, 3, 1, 2).to(torch.float32).div(255.0)) - 0.5) / 0.5        # image_to_tensor_balanced
            if not torch.equal(back, x):
                v = int((back != x).flatten(1).any(1).nonzero()[0])
                raise ValueError(who + "item %d (%s): images[%d] is not the byte map of 8-bit pixels (resized or jittered on the host?); "
                                 "the store holds bytes" % (int(i), it.get("path"), v))
            if store is None:
                store = cls(device, white_bbox=bool(white_bbox))
            bbox = it.get("bbox")
            store.add(u8, it["poses"], it["focal"], c=it.get("c"), bbox=None if bbox is None or len(bbox) == 0 or store.white_bbox else bbox)
        if store is None:
            raise ValueError(who + "no object to hold")
        return store

    # ---- bookkeeping
    def __len__(self):
        return len(self._views)

    def n_views(self, obj):
        return int(self._views[obj].shape[0])

    def labels(self, obj):
        """What ``add`` was given as ``labels`` for this object (the YOLO rows, for ``util.build_yolo_targets``)."""
        return self._labels[obj]

    @property
    def nbytes(self):
        """Bytes the store holds on its device: the views and the camera tables."""
        n, rows = len(self._views), sum(int(v.shape[0]) for v in self._views)
        per_row = 64 + (16 if n and self._bbox[0] is not None else 0)          # a pose, a box
        return sum(v.numel() for v in self._views) + rows * per_row + n * (16 + 8 + 8 + 16)   # record, focal, c, n_views and first_row

    def epoch(self, batch_size, seed, epoch=0, drop_last=True):
        """The object ids of one epoch in batches of ``batch_size``: a permutation seeded by (seed, epoch), on the host -- what
        the DataLoader's shuffle and batching did."""
        g = torch.Generator()
        g.manual_seed((int(seed) * 1000003 + int(epoch)) % (2 ** 63))
        order = torch.randperm(len(self), generator=g).tolist()
        for k in range(0, len(order), int(batch_size)):
            ids = order[k:k + int(batch_size)]
            if len(ids) == int(batch_size) or (ids and not drop_last):
                yield ids

    def tables(self):
        """The small tables of the objects added so far, on the store's device, built on the host and uploaded once after the
        last ``add`` into FRESH tensors (launches in flight keep the ones they were given): ``objs`` (n, 16) bytes -- the ABI's
        records {views pointer, n_views, first_row} --, ``n_views`` and ``first_row`` (n,) int64, ``poses`` (N_total, 4, 4),
        ``bboxes`` (N_total, 4) or None, ``focal`` and ``c`` (n, 2)."""
        if self._tab is not None:
            return self._tab
        if not self._views:
            raise ValueError(_WHO_RV + ": the store is empty")
        nv = np.array([v.shape[0] for v in self._views], np.int64)
        first = np.concatenate([[0], np.cumsum(nv)[:-1]])
        if int(nv.sum()) >= 2 ** 31:
            raise ValueError(_WHO_RV + ": 2^31 views or more")
        rec = np.zeros(len(nv), np.dtype([("views", np.uint64), ("n_views", np.int32), ("first_row", np.int32)]))
        rec["views"], rec["n_views"], rec["first_row"] = [v.data_ptr() for v in self._views], nv, first
        up = lambda t: t.to(self.device, non_blocking=True)
        self._tab = {
            "objs": up(torch.from_numpy(rec.view(np.uint8).reshape(len(nv), 16).copy())),
            "n_views": up(torch.from_numpy(nv)), "first_row": up(torch.from_numpy(first.astype(np.int64))),
            "poses": up(torch.cat(self._poses)), "focal": up(torch.stack(self._focal)), "c": up(torch.stack(self._c)),
            "bboxes": None if self._bbox[0] is None else up(torch.cat(self._bbox)),
            "max_views": int(nv.max()), "n_rows": int(nv.sum()),
        }
        return self._tab

    # ---- drawing
    def _ids(self, obj_ids, view_ids, who, view_name):
        """(SB,) int32 object ids and (SB, NS) int32 view ids on the device; host lists are validated first."""
        n = len(self)
        o = _host_ids(obj_ids, "obj_ids", who, 1)
        if o is not None and (o.min() < 0 or o.max() >= n):
            raise ValueError("%s: obj_ids holds %d; the store has %d object%s" % (who, int(o[(o < 0) | (o >= n)][0]), n, "" if n == 1 else "s"))
        sb = len(o) if o is not None else int(obj_ids.shape[0])
        o_dev = self._upload_ids(o, obj_ids)
        if view_ids is None:
            return o_dev, None
        v = _host_ids(view_ids, view_name, who, 2)
        shape = v.shape if v is not None else tuple(view_ids.shape)
        if shape[0] != sb:
            raise ValueError("%s: %s must be (%d, NS), one row per entry of obj_ids, got %s" % (who, view_name, sb, tuple(shape)))
        if v is not None and o is not None:
            lim = np.array([self.n_views(int(k)) for k in o])[:, None]
            bad = np.argwhere((v < 0) | (v >= lim))
            if len(bad):
                s, k = (int(t) for t in bad[0])
                raise ValueError("%s: %s[%d][%d] = %d; object %d has %d view%s" % (who, view_name, s, k, int(v[s, k]), int(o[s]), int(lim[s, 0]),
                                                                                   "" if lim[s, 0] == 1 else "s"))
        elif v is not None and v.min() < 0:
            raise ValueError("%s: %s holds %d" % (who, view_name, int(v.min())))
        v_dev = self._upload_ids(v, view_ids)
        return o_dev, v_dev

    def _upload_ids(self, host, given):
        """int32 ids on the store's device: a validated host array goes through pinned memory (a copy from pageable memory may
        wait for the stream), a device tensor is used as it is."""
        if host is None:
            return given.to(self.device, torch.int32).contiguous()
        t = torch.from_numpy(host.astype(np.int32))
        if self.device.type == "cuda":
            t = t.pin_memory()
        return t.to(self.device, non_blocking=True)

    def _need_device(self, who):
        from . import lib as _lib
        if self.device.type != "cuda":
            raise _lib.PnyError("%s: the store is on %s; drawing from it runs on an MI355X only (the host path is the DataLoader over "
                                "data.py's datasets)" % (who, self.device))
        return _lib

    def _source_views(self, _lib, tab, o_dev, v_dev, jitter):
        import ctypes as C
        sb, ns = (int(t) for t in v_dev.shape)
        h, w, ch = self.decoded
        oh, ow = self.out_size
        out = torch.empty(sb, ns, 3, oh, ow, device=self.device, dtype=torch.float32)
        obj_of = o_dev[:, None].expand(sb, ns).contiguous()
        desc = _lib.IngestDesc(n_views=sb * ns, height=h, width=w, channels=ch, out_height=oh, out_width=ow,
                               resize=_lib.RESIZE[self.resize], white_mask=0)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pny_ingest_views_indexed(
                C.byref(desc), C.c_void_p(tab["objs"].data_ptr()), len(self), tab["max_views"], C.c_void_p(obj_of.data_ptr()),
                C.c_void_p(v_dev.data_ptr()), C.c_void_p(out.data_ptr()), _lib.stream_of(self.device)))
        if jitter is not None:
            from . import augment
            augment.color_jitter(out, jitter, out=out)
        return out

    def source_views(self, obj_ids, view_ids, jitter=None):
        """Views ``view_ids`` (SB, NS) of objects ``obj_ids`` (SB,) -- or (NS,) of ONE object given as an int -- as
        ``augment.ingest_views`` gives them: (SB, NS, 3, OH, OW) (or (NS, 3, OH, OW)) fp32 in [-1, 1], in one launch;
        ``jitter`` (SB, 4) applies ``augment.color_jitter`` behind it.  Ids are host lists (validated) or device tensors (clamped)."""
        who = _WHO_RV + ".source_views"
        one = isinstance(obj_ids, (int, np.integer))
        if one:
            obj_ids = [int(obj_ids)]
            view_ids = view_ids[None] if isinstance(view_ids, torch.Tensor) else [list(view_ids)]
        if view_ids is None:
            raise ValueError(who + ": view_ids is None")
        o_dev, v_dev = self._ids(obj_ids, view_ids, who, "view_ids")
        _lib = self._need_device(who)
        out = self._source_views(_lib, self.tables(), o_dev, v_dev, jitter)
        return out[0] if one else out

    def batch(self, obj_ids, src_view_ids, ray_batch_size, z_near, z_far, seed=None, draws=None, draw_offset=0, jitter=None):
        """One training step's inputs for the objects ``obj_ids`` (SB,; repeats allowed), with nothing the size of a view set
        decoded, copied or normalised: a dict of ``rays`` (SB, B, 8), ``rgb_gt`` (SB, B, 3) and ``pix`` (SB, B, 3) int32
        [view, y, x] -- share s bit-equal to ``util.sample_train_batch`` on ``augment.ingest_views`` of that object's views with
        ``draw_offset + s * B`` (bbox mode when the store holds boxes) --, ``src_images`` (SB, NS, 3, OH, OW) of the views
        ``src_view_ids`` (SB, NS) (None: no source views), ``src_poses`` (SB, NS, 4, 4), ``focal`` (SB, 2) and ``c`` (SB, 2).
        ``seed`` / ``draws`` / ``draw_offset`` as ``util.sample_train_batch`` takes them; ``jitter`` (SB, 4) for the source views."""
        import ctypes as C
        who = _WHO_RV + ".batch"
        B = int(ray_batch_size)
        if B < 1:
            raise ValueError(who + ": ray_batch_size must be positive, got %r" % (ray_batch_size,))
        o_dev, v_dev = self._ids(obj_ids, src_view_ids, who, "src_view_ids")
        sb = int(o_dev.shape[0])
        if draws is not None and seed is not None:
            raise ValueError(who + ": draws replay the pixel choice; seed has no effect with them")
        _lib = self._need_device(who)
        tab = self.tables()
        h, w, ch = self.decoded
        oh, ow = self.out_size
        desc = _lib.TrainBatchDesc(n_objs=sb, n_views=tab["max_views"], height=h, width=w, n_rays=B, z_near=float(z_near),
                                   z_far=float(z_far), focal_rows=0, focal_cols=0, c_rows=0, seed=0, draw_offset=int(draw_offset))
        dr, keep = None, []
        if draws is not None:
            names = ("image_ids", "u_x", "u_y") if tab["bboxes"] is not None else ("pix_inds",)
            if set(draws) != set(names):
                raise ValueError(who + ": draws must hold exactly %s (the store has %s boxes), got %s"
                                 % (names, "no" if tab["bboxes"] is None else "its", sorted(draws)))
            keep = [torch.as_tensor(draws[k]).detach().to(self.device, torch.float32 if k.startswith("u_") else torch.int64,
                                                           non_blocking=True).contiguous() for k in names]
            for k, t in zip(names, keep):
                if tuple(t.shape) != (sb, B):
                    raise ValueError(who + ": draws[%r] must be (%d, %d), got %s" % (k, sb, B, tuple(t.shape)))
            dr = _lib.TrainBatchDraws(**{k + "_dev": t.data_ptr() for k, t in zip(names, keep)})
        elif seed is None:
            hi, lo = torch.randint(0, 2 ** 32, (2,), dtype=torch.int64).tolist()   # the CPU generator: nothing to wait for
            desc.seed = (hi << 32) | lo
        else:
            desc.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        rays = torch.empty(sb, B, 8, device=self.device, dtype=torch.float32)
        rgb_gt = torch.empty(sb, B, 3, device=self.device, dtype=torch.float32)
        pix = torch.empty(sb, B, 3, device=self.device, dtype=torch.int32)
        vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pny_resident_train_batch(
                C.byref(desc), ch, oh, ow, _lib.RESIZE[self.resize], vp(tab["objs"]), len(self), vp(o_dev), vp(tab["poses"]),
                tab["n_rows"], vp(tab["focal"]), vp(tab["c"]), vp(tab["bboxes"]), None if dr is None else C.byref(dr), vp(rays),
                vp(rgb_gt), vp(pix), _lib.stream_of(self.device)))
        # the small camera tensors by device-side indexing, with the kernels' clamps
        o = o_dev.to(torch.int64).clamp(0, len(self) - 1)
        out = {"rays": rays, "rgb_gt": rgb_gt, "pix": pix, "focal": tab["focal"][o], "c": tab["c"][o], "src_images": None,
               "src_poses": None}
        if v_dev is not None:
            v = torch.minimum(v_dev.to(torch.int64).clamp(min=0), (tab["n_views"][o] - 1)[:, None])
            out["src_poses"] = tab["poses"][tab["first_row"][o][:, None] + v]
            out["src_images"] = self._source_views(_lib, tab, o_dev, v_dev, jitter)
        elif jitter is not None:
            raise ValueError(who + ": jitter is given without src_view_ids (it applies to the source views)")
        return out


# ------------------------------------------------------------------ metrics / writers (eval/eval.py:291-359)
def psnr(img, gt, data_range=1.0):
    """skimage compare_psnr: 10 log10(data_range^2 / mse), float64."""
    a, b = np.asarray(img, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    return float(10.0 * np.log10(data_range ** 2 / np.mean((a - b) ** 2)))


def ssim(img, gt, data_range=1.0, win_size=7):
    """skimage compare_ssim(multichannel=True, data_range=1) with its defaults: uniform win_size x win_size window, sample
    covariance (n / (n - 1)), K1 = 0.01, K2 = 0.03, mean over the valid (un-padded) region, then over channels.
    img, gt (H, W, C) in [0, data_range]."""
    a = torch.from_numpy(np.asarray(img, dtype=np.float64)).permute(2, 0, 1)[None]
    b = torch.from_numpy(np.asarray(gt, dtype=np.float64)).permute(2, 0, 1)[None]
    n = win_size * win_size
    cov_norm = n / (n - 1.0)
    filt = lambda t: F.avg_pool2d(t, win_size, stride=1)
    ux, uy = filt(a), filt(b)
    uxx, uyy, uxy = filt(a * a), filt(b * b), filt(a * b)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return float(s.mean())


def write_views(out_dir, rgb, view_ids, gt=None, write_compare=False):
    """eval/eval.py:293-340: rgb (NV, H, W, 3) in [0, 1] -> <out_dir>/<id:06>.png (+ _compare.png beside the ground truth);
    returns (mean psnr, mean ssim) when gt is given."""
    os.makedirs(out_dir, exist_ok=True)
    rgb = np.clip(np.asarray(rgb, dtype=np.float32), 0.0, 1.0)
    tot_p = tot_s = 0.0
    for i, vid in enumerate(view_ids):
        imwrite(os.path.join(out_dir, "{:06}.png".format(int(vid))), (rgb[i] * 255).astype(np.uint8))
        if gt is not None:
            tot_s += ssim(rgb[i], gt[i])
            tot_p += psnr(rgb[i], gt[i])
            if write_compare:
                imwrite(os.path.join(out_dir, "{:06}_compare.png".format(int(vid))),
                        (np.hstack((rgb[i], np.asarray(gt[i], dtype=np.float32))) * 255).astype(np.uint8))
    if gt is None:
        return None
    return tot_p / len(view_ids), tot_s / len(view_ids)
