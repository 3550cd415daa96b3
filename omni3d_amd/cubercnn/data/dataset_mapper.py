"""`DatasetMapper3D` (reference cubercnn/data/dataset_mapper.py:17-155): dataset dict -> model input dict.

Same steps and field names as the reference: read the image (BGR uint8), ResizeShortestEdge (+ RandomFlip when training),
transform the annotations (2D box hull, projected 3D centre, keypoints, pose mirroring under a flip, :76-129), build the
`Instances` (gt_classes, gt_boxes, gt_boxes3D = [u, v, z, w, h, l, X, Y, Z], gt_poses, gt_keypoints,
gt_unknown_category_mask, :133-155).

MI355X design: the pixel work -- PIL-bilinear resize and mirror -- runs in csrc/resize.hip (bit-exact
with the PIL call the reference makes) when the mapper is given a device, so the loader hands uint8 images to the GPU at
their ORIGINAL size and the multi-scale augmentation costs no host time; the annotation arithmetic is a few dozen floats
per image and stays on the host.

Beyond the reference: INPUT.CROP (detectron2's RandomCrop in front of the resize) and INPUT.COLOR_JITTER, both off by default and
training-only.  The reference's mapper crops the pixels and the 2D boxes but leaves `K` and `height` alone, so its 3D targets no
longer belong to the image; here the returned dict carries the crop's camera -- `K` with the principal point moved by the crop
origin, `height` / `width` of the crop, `crop` = (x0, y0, cw, ch) -- which is all the model reads (rcnn3d.py, modeling/targets.py).
With a device the window is resized straight out of the uploaded image (csrc/augment.hip, no copy of it), and the jitter runs in
place on the resized image; without one the same bytes come from PIL on the slice and `color_jitter_u8_host`.

INPUT.CAMERA_ROTATION (off by default, training-only) turns the camera about its optical centre by a small random roll, pitch and
yaw Q: the pixels move by the homography K Q K^-1 (csrc/warp.hip, or `warp_homography_u8_host` -- the same bytes), every 3D target
by Q (`rotate_instance_annotations`), and `K`, `height` and `width` stay as they are; the dict gains `camera_rotation` = Q."""
import copy

import numpy as np
import torch

from ...d2.data import (CropTransform, HFlipTransform, NoOpTransform, ResizeTransform, TransformList, camera_rotation, check_crop,
                        random_crop_box, resize_shortest_edge_size, rotation_homography)
from ...d2.structures import Boxes, BoxMode, Instances

_M1 = np.array([[1, 0, 0], [0, -1, 0], [0, 0, -1]])             # dataset_mapper.py:63-72
_M2 = np.array([[-1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, 1.0]])


class Keypoints:
    """detectron2.structures.Keypoints: (N, K, 3) tensor wrapper"""

    def __init__(self, keypoints):
        self.tensor = torch.as_tensor(keypoints, dtype=torch.float32)

    def __len__(self):
        return self.tensor.size(0)

    def to(self, *args, **kwargs):
        return Keypoints(self.tensor.to(*args, **kwargs))

    def __getitem__(self, item):
        return Keypoints(self.tensor[[item]] if isinstance(item, int) else self.tensor[item])


def read_image(dataset_dict, fmt="BGR"):
    """detection_utils.read_image; synthetic datasets carry the pixels in memory (`image_array`, HWC uint8 in `fmt`)"""
    if "image_array" in dataset_dict:
        return np.asarray(dataset_dict["image_array"])
    from PIL import Image
    with Image.open(dataset_dict["file_name"]) as im:
        rgb = np.asarray(im.convert("RGB"))
    return rgb[:, :, ::-1] if fmt == "BGR" else rgb


def color_jitter_u8_host(chw, wb, wc, ws, fmt):
    """include/omni3d_hip.h omni_color_jitter_u8 in numpy: chw (3, H, W) uint8 in channel order `fmt`, integer weights with 12
    fractional bits -> the jittered (3, H, W) uint8 array.  Python's >> on negative integers is arithmetic, like the kernel's."""
    v = chw.astype(np.int64)
    v = np.clip((wb * v + 2048) >> 12, 0, 255)
    n = v.size
    m8 = (256 * int(v.sum()) + n // 2) // n
    v = np.clip((wc * 256 * v + (4096 - wc) * m8 + (1 << 19)) >> 20, 0, 255)
    r, b = (2, 0) if fmt == "BGR" else (0, 2)
    g8 = 77 * v[r] + 150 * v[1] + 29 * v[b]
    v = np.clip((ws * 256 * v + (4096 - ws) * g8[None] + (1 << 19)) >> 20, 0, 255)
    return v.astype(np.uint8)


def warp_homography_u8_host(chw, m, out_h, out_w, fill):
    """include/omni3d_hip.h omni_warp_homography_u8 in numpy: chw (P, H, W) uint8, m 3 x 3 (output pixel -> source pixel), fill P bytes
    -> the warped (P, out_h, out_w) uint8 array.  numpy rounds every float64 product and sum on its own, which is the definition."""
    chw = np.asarray(chw)
    P, H, W = chw.shape
    m = np.asarray(m, dtype=np.float64).reshape(9)
    xd, yd = (np.arange(out_w, dtype=np.float64) + 0.5)[None, :], (np.arange(out_h, dtype=np.float64) + 0.5)[:, None]
    with np.errstate(all="ignore"):
        X = (m[0] * xd + m[1] * yd) + m[2]
        Y = (m[3] * xd + m[4] * yd) + m[5]
        D = (m[6] * xd + m[7] * yd) + m[8]
        r = 1.0 / D
        u, v = X * r, Y * r
        inside = (u >= 0.0) & (u <= float(W)) & (v >= 0.0) & (v <= float(H))
    su, sv = np.where(inside, u, 0.5) - 0.5, np.where(inside, v, 0.5) - 0.5
    fx, fy = np.floor(su), np.floor(sv)
    a, b = ((su - fx) * 256.0 + 0.5).astype(np.int64), ((sv - fy) * 256.0 + 0.5).astype(np.int64)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    x0, y0 = np.maximum(x0, 0), np.maximum(y0, 0)
    s = chw.astype(np.int64)
    top = s[:, y0, x0] * (256 - a) + s[:, y0, x1] * a
    bot = s[:, y1, x0] * (256 - a) + s[:, y1, x1] * a
    out = (top * (256 - b) + bot * b + 32768) >> 16
    border = np.asarray(fill, dtype=np.int64).reshape(P, 1, 1)
    return np.where(inside[None], out, border).astype(np.uint8)


def rotate_instance_annotations(annotation, Q, K, height, width):
    """One annotation under the camera rotation Q (INPUT.CAMERA_ROTATION), before `transform_instance_annotations`: `center_cam` and
    every row of `bbox3D_cam` become Q x, `pose` / `R_cam` become Q pose, `dimensions` stay.  `bbox` becomes the axis-aligned hull of
    its four corners moved by Hm = K Q K^-1, clipped to [0, width] x [0, height] -- detectron2's rule for a rotated box, looser than
    the object.  An annotation one of whose box corners has a non-positive denominator under Hm, or whose centre goes from z > 0 to
    z <= 0, gets an empty box and keeps its other fields: the mapper's empty-box filter drops it."""
    from ...d2.data import homography_apply, rotation_homography
    Q, K = np.asarray(Q, dtype=np.float64), np.asarray(K, dtype=np.float64)
    x0, y0, x1, y1 = BoxMode.convert(annotation["bbox"], annotation["bbox_mode"], BoxMode.XYXY_ABS)
    annotation["bbox_mode"] = BoxMode.XYXY_ABS
    uv, den = homography_apply(rotation_homography(K, Q)[0], [(x0, y0), (x1, y0), (x0, y1), (x1, y1)])
    center = np.asarray(annotation["center_cam"], dtype=np.float64)
    moved = Q @ center
    if not (den > 0).all() or (center[2] > 0 and not moved[2] > 0):
        annotation["bbox"] = [0.0, 0.0, 0.0, 0.0]
        return annotation
    xs, ys = np.clip(uv[:, 0], 0.0, float(width)), np.clip(uv[:, 1], 0.0, float(height))
    annotation["bbox"] = [float(xs.min()), float(ys.min()), float(xs.max()), float(ys.max())]
    annotation["center_cam"] = moved.tolist()
    annotation["bbox3D_cam"] = (np.asarray(annotation["bbox3D_cam"], dtype=np.float64) @ Q.T).tolist()
    pose = (Q @ np.asarray(annotation["pose"], dtype=np.float64)).tolist()
    annotation["pose"] = pose
    annotation["R_cam"] = copy.deepcopy(pose)
    return annotation


class DatasetMapper3D:
    def __init__(self, cfg, is_train=True, device=None, rng=None):
        self.is_train = is_train
        self.image_format = cfg.INPUT.FORMAT
        if is_train:
            self.min_size, self.max_size, self.sample_style = cfg.INPUT.MIN_SIZE_TRAIN, cfg.INPUT.MAX_SIZE_TRAIN, cfg.INPUT.MIN_SIZE_TRAIN_SAMPLING
            self.flip = cfg.INPUT.RANDOM_FLIP
        else:
            self.min_size, self.max_size, self.sample_style, self.flip = cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST, "choice", "none"
        if isinstance(self.min_size, int):
            self.min_size = (self.min_size,)
        if self.sample_style == "range":
            assert len(self.min_size) == 2, "more than 2 ({}) min_size(s) are provided for ranges".format(len(self.min_size))
        self.crop = self.jitter = None          # (type, size) of INPUT.CROP / the three (low, high) of INPUT.COLOR_JITTER: training only
        self.rotation, self.rotation_fill = None, None      # the (low, high) of roll, pitch, yaw in degrees / the border's three bytes
        self.rotation_skipped = 0               # images left unrotated because the warp's denominator was not positive all over them
        if is_train:
            from ..config import camera_rotation_args, color_jitter_args
            rotation = camera_rotation_args(cfg)
            if rotation["enabled"]:
                self.rotation, self.rotation_fill = (rotation["roll"], rotation["pitch"], rotation["yaw"]), rotation["fill"]
            crop = cfg.INPUT.get("CROP")
            if crop is not None and crop.ENABLED:
                self.crop = check_crop(crop.TYPE, crop.SIZE)
            jitter = color_jitter_args(cfg)
            if jitter["enabled"]:
                if self.image_format not in ("BGR", "RGB"):      # the saturation step needs to know which plane is red
                    raise ValueError("INPUT.COLOR_JITTER needs INPUT.FORMAT BGR or RGB, got {!r}".format(self.image_format))
                self.jitter = (jitter["brightness"], jitter["contrast"], jitter["saturation"])
        self.device = device
        self.rng = rng if rng is not None else np.random
        self.dataset_id_to_unknown_cats = {}

    # -- detectron2 build_augmentation(cfg, is_train): ResizeShortestEdge [+ RandomFlip(horizontal)] ----------------------
    def sample_transforms(self, h, w):
        nh, nw = resize_shortest_edge_size(h, w, self.min_size, self.max_size, self.sample_style, self.rng)
        tfm = TransformList([ResizeTransform(h, w, nh, nw)])
        do_flip = self.is_train and self.flip == "horizontal" and self.rng.uniform() < 0.5
        tfm.append(HFlipTransform(nw) if do_flip else NoOpTransform())
        return tfm, (nh, nw), do_flip

    # -- detectron2 puts RandomCrop in front of the resize (DatasetMapper.from_config: augs.insert(0, T.RandomCrop(...))) -------------
    def sample_crop(self, h, w):
        """-> (x0, y0, cw, ch), or None with INPUT.CROP off; drawn before the resize's size"""
        return None if self.crop is None else random_crop_box(h, w, self.crop[0], self.crop[1], self.rng)

    def sample_rotation(self):
        """-> (roll, pitch, yaw) in degrees, or None with INPUT.CAMERA_ROTATION off; drawn first of all, in this order.  An interval of
        [c, c] draws nothing."""
        if self.rotation is None:
            return None
        return tuple(lo if lo == hi else float(self.rng.uniform(lo, hi)) for lo, hi in self.rotation)

    def sample_jitter(self):
        """-> (wb, wc, ws) integer weights (4096 = 1.0), or None with INPUT.COLOR_JITTER off; drawn after the flip, brightness first.
        An interval of [1, 1] draws nothing."""
        if self.jitter is None:
            return None
        return tuple(4096 if lo == hi == 1.0 else int(self.rng.uniform(lo, hi) * 4096 + 0.5) for lo, hi in self.jitter)

    def apply_image(self, image_hwc, out_hw, flip, box=None, jitter=None, warp=None):
        """-> uint8 (3, nh, nw) tensor: the image, or its window `box` = (x0, y0, cw, ch), resized and mirrored, then jittered by the
        weights `jitter`.  `warp` = Hinv (3 x 3, rotated pixel -> source pixel): the image is the rotated one, of which only the
        window is ever produced -- the warp's matrix is Hinv @ T(x0, y0) and its output the window's size -- and the plain resize
        follows.  device set: csrc/resize.hip, csrc/augment.hip, csrc/warp.hip; else PIL on the host (the reference's call) and numpy"""
        nh, nw = out_hw
        if warp is not None:
            ch, cw = image_hwc.shape[:2]
            if box is not None:
                x0, y0, cw, ch = box
                warp = warp @ np.array([[1.0, 0.0, float(x0)], [0.0, 1.0, float(y0)], [0.0, 0.0, 1.0]])
        if self.device is not None:
            from ...kernels import augment, resize
            chw = torch.from_numpy(np.ascontiguousarray(image_hwc.transpose(2, 0, 1))).to(self.device, non_blocking=True)
            if warp is not None:
                out = resize.resize_bilinear_u8(augment.warp_homography_u8(chw, warp, ch, cw, self.rotation_fill), nh, nw, flip)
            else:
                out = resize.resize_bilinear_u8(chw, nh, nw, flip) if box is None else augment.crop_resize_u8(chw, box, nh, nw, flip)
            return out if jitter is None else augment.color_jitter_u8_(out, *jitter, self.image_format)
        from PIL import Image
        if warp is not None:
            chw = warp_homography_u8_host(np.ascontiguousarray(image_hwc.transpose(2, 0, 1)), warp, ch, cw, self.rotation_fill)
            image_hwc = chw.transpose(1, 2, 0)
        elif box is not None:
            image_hwc = image_hwc[box[1]:box[1] + box[3], box[0]:box[0] + box[2]]
        out = np.asarray(Image.fromarray(np.ascontiguousarray(image_hwc)).resize((nw, nh), Image.BILINEAR))
        if flip:
            out = np.flip(out, axis=1)
        out = np.ascontiguousarray(out.transpose(2, 0, 1))
        return torch.as_tensor(out if jitter is None else color_jitter_u8_host(out, *jitter, self.image_format))

    def rotation_of(self, dataset_dict, h, w):
        """-> (Q, Hinv) of this image's drawn camera rotation, (None, None) with INPUT.CAMERA_ROTATION off.  Where the warp's denominator
        is not positive at every corner of the image (no sane camera at these angles) the image stays unrotated: (I, None), counted
        in `rotation_skipped`."""
        angles = self.sample_rotation()
        if angles is None:
            return None, None
        if "K" not in dataset_dict:
            raise ValueError("INPUT.CAMERA_ROTATION needs the camera K of image {}".format(dataset_dict.get("file_name", dataset_dict.get("image_id"))))
        from ...kernels.augment import warp_denominator_positive
        Q = camera_rotation(*angles)
        Hinv = rotation_homography(dataset_dict["K"], Q)[1]
        if not (np.isfinite(Hinv).all() and warp_denominator_positive(Hinv, h, w)):
            self.rotation_skipped += 1
            return np.eye(3), None
        return Q, Hinv

    def __call__(self, dataset_dict):
        dataset_dict = copy.deepcopy(dataset_dict)
        image = read_image(dataset_dict, self.image_format)
        if (image.shape[0], image.shape[1]) != (dataset_dict.get("height", image.shape[0]), dataset_dict.get("width", image.shape[1])):
            raise ValueError("Mismatched image shape for image {}".format(dataset_dict.get("file_name", dataset_dict.get("image_id"))))
        Q, warp = self.rotation_of(dataset_dict, image.shape[0], image.shape[1])
        box = self.sample_crop(image.shape[0], image.shape[1])
        transforms, image_shape, flip = self.sample_transforms(*((image.shape[0], image.shape[1]) if box is None else (box[3], box[2])))
        dataset_dict["image"] = self.apply_image(image, image_shape, flip, box, self.sample_jitter(), warp)
        dataset_dict.pop("image_array", None)
        if not self.is_train:
            return dataset_dict
        camera = {"K": dataset_dict["K"]} if "K" in dataset_dict else {}       # the annotations are projected with the original camera
        if Q is not None:                        # a rotation leaves K and the image size alone
            dataset_dict["camera_rotation"] = Q.tolist()
        if box is not None:
            x0, y0, cw, ch = box
            transforms.insert(0, CropTransform(x0, y0, cw, ch))
            if camera:                           # the crop's camera: same focal length, principal point moved by the origin
                Kc = [list(row) for row in camera["K"]]
                Kc[0][2], Kc[1][2] = Kc[0][2] - x0, Kc[1][2] - y0
                dataset_dict["K"] = Kc
            dataset_dict["height"], dataset_dict["width"], dataset_dict["crop"] = ch, cw, (x0, y0, cw, ch)
        if "annotations" in dataset_dict:
            K = np.array(camera["K"])            # KeyError without a camera, as before
            unknown = self.dataset_id_to_unknown_cats[dataset_dict["dataset_id"]]
            annos = [obj for obj in dataset_dict.pop("annotations") if obj.get("iscrowd", 0) == 0]
            if warp is not None:                 # the rotated targets first; the transform list then moves their projections once
                annos = [rotate_instance_annotations(obj, Q, K, image.shape[0], image.shape[1]) for obj in annos]
            annos = [transform_instance_annotations(obj, transforms, K=K) for obj in annos]
            inst = annotations_to_instances(annos, image_shape, unknown)
            if box is not None and len(inst):
                inst.gt_boxes.clip(image_shape)          # what the crop cut off; boxes wholly outside become empty and are dropped below
            dataset_dict["instances"] = inst[inst.gt_boxes.nonempty()] if len(inst) else inst      # filter_empty_instances
        return dataset_dict


def transform_instance_annotations(annotation, transforms, *, K):
    """dataset_mapper.py:76-129"""
    if isinstance(transforms, (tuple, list)) and not isinstance(transforms, TransformList):
        transforms = TransformList(transforms)
    bbox = BoxMode.convert(annotation["bbox"], annotation["bbox_mode"], BoxMode.XYXY_ABS)
    annotation["bbox"] = transforms.apply_box(np.array([bbox]))[0]
    annotation["bbox_mode"] = BoxMode.XYXY_ABS
    if annotation["center_cam"][2] != 0:
        point2D = K @ np.array(annotation["center_cam"])
        point2D[:2] = point2D[:2] / point2D[-1]
        annotation["center_cam_proj"] = point2D.tolist()
        annotation["center_cam_proj"][0:2] = transforms.apply_coords(point2D[np.newaxis][:, :2])[0].tolist()
        keypoints = (K @ np.array(annotation["bbox3D_cam"]).T).T
        keypoints[:, 0] /= keypoints[:, -1]
        keypoints[:, 1] /= keypoints[:, -1]
        keypoints[:, 2] = 1 if annotation["ignore"] else 2        # 0 unknown, 1 not visible, 2 visible (:103-113)
        transforms.apply_coords(keypoints[:, :2])
        annotation["keypoints"] = keypoints.tolist()
        for t in transforms:
            if isinstance(t, HFlipTransform):                      # manual mirror of the pose (:120-127)
                pose = _M1 @ np.array(annotation["pose"]) @ _M2
                annotation["pose"] = pose.tolist()
                annotation["R_cam"] = pose.tolist()
    return annotation


def annotations_to_instances(annos, image_size, unknown_categories):
    """dataset_mapper.py:133-155"""
    target = Instances(image_size)
    target.gt_classes = torch.tensor([int(obj["category_id"]) for obj in annos], dtype=torch.int64)
    target.gt_boxes = Boxes(torch.tensor(np.asarray([BoxMode.convert(obj["bbox"], obj["bbox_mode"], BoxMode.XYXY_ABS) for obj in annos],
                                                    dtype=np.float32).reshape(-1, 4)))
    target.gt_boxes3D = torch.FloatTensor([a["center_cam_proj"] + a["dimensions"] + a["center_cam"] for a in annos]).reshape(-1, 9)
    target.gt_poses = torch.FloatTensor([a["pose"] for a in annos]).reshape(-1, 3, 3)
    n = len(target.gt_classes)
    target.gt_keypoints = Keypoints(torch.FloatTensor([a["keypoints"] for a in annos]).reshape(-1, 8, 3))
    mask = torch.zeros(max(unknown_categories) + 1 if len(unknown_categories) else 1, dtype=bool)
    if len(unknown_categories):
        mask[torch.tensor(list(unknown_categories))] = True
    target.gt_unknown_category_mask = mask.unsqueeze(0).repeat([n, 1])
    return target
