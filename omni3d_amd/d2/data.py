"""detectron2.data plumbing: DatasetCatalog / MetadataCatalog registries and the two transforms the reference's mapper uses
(ResizeShortestEdge, RandomFlip) with detectron2's parameter sampling and coordinate rules, and RandomCrop (INPUT.CROP), which
detectron2's mapper puts in front of them; the geometry of INPUT.CAMERA_ROTATION (a camera rotation and its pixel homography)."""
import types

import numpy as np


class _DatasetCatalog(dict):
    def register(self, name, func):
        assert callable(func), "You must register a function with `DatasetCatalog.register`!"
        assert name not in self, "Dataset '{}' is already registered!".format(name)
        self[name] = func

    def get(self, name):
        try:
            f = self[name]
        except KeyError as e:
            raise KeyError("Dataset '{}' is not registered! Available datasets are: {}".format(name, ", ".join(self.keys()))) from e
        return f()

    def list(self):
        return list(self.keys())

    def remove(self, name):
        self.pop(name)


class Metadata(types.SimpleNamespace):
    """detectron2.data.catalog.Metadata: attribute bag with `.set(**kw)` / `.get(key, default)`; unknown attributes raise."""

    def set(self, **kwargs):
        for k, v in kwargs.items():
            setattr(self, k, v)
        return self

    def get(self, key, default=None):
        return getattr(self, key, default)

    def as_dict(self):
        return dict(vars(self))


class _MetadataCatalog(dict):
    def get(self, name):
        if name not in self:
            self[name] = Metadata(name=name)
        return self[name]

    def list(self):
        return list(self.keys())


DatasetCatalog = _DatasetCatalog()
MetadataCatalog = _MetadataCatalog()


# ---- transforms (detectron2.data.transforms) ---------------------------------------------------------------------------
class ResizeTransform:
    def __init__(self, h, w, new_h, new_w):
        self.h, self.w, self.new_h, self.new_w = h, w, new_h, new_w

    def apply_coords(self, coords):
        coords[:, 0] = coords[:, 0] * (self.new_w * 1.0 / self.w)
        coords[:, 1] = coords[:, 1] * (self.new_h * 1.0 / self.h)
        return coords


class HFlipTransform:
    def __init__(self, width):
        self.width = width

    def apply_coords(self, coords):
        coords[:, 0] = self.width - coords[:, 0]
        return coords


class CropTransform:
    """detectron2 CropTransform: the window [x0, x0 + w) x [y0, y0 + h) becomes the image"""

    def __init__(self, x0, y0, w, h):
        self.x0, self.y0, self.w, self.h = x0, y0, w, h

    def apply_coords(self, coords):
        coords[:, 0] -= self.x0
        coords[:, 1] -= self.y0
        return coords


class NoOpTransform:
    def apply_coords(self, coords):
        return coords


class TransformList(list):
    def apply_coords(self, coords):
        for t in self:
            coords = t.apply_coords(coords)
        return coords

    def apply_box(self, box):
        """detectron2 Transform.apply_box: transform the four corners, take the axis-aligned hull"""
        idxs = np.array([(0, 1), (2, 1), (0, 3), (2, 3)]).flatten()
        coords = np.asarray(box, dtype=np.float64).reshape(-1, 4)[:, idxs].reshape(-1, 2)
        coords = self.apply_coords(coords).reshape((-1, 4, 2))
        minxy, maxxy = coords.min(axis=1), coords.max(axis=1)
        return np.concatenate((minxy, maxxy), axis=1)


def resize_shortest_edge_size(h, w, short_edge_length, max_size, sample_style="range", rng=np.random):
    """detectron2 ResizeShortestEdge.get_transform / get_output_shape -> (new_h, new_w)"""
    if sample_style == "range":
        size = rng.randint(short_edge_length[0], short_edge_length[1] + 1)
    else:
        size = rng.choice(short_edge_length)
    if size == 0:
        return h, w
    scale = size * 1.0 / min(h, w)
    newh, neww = (size, scale * w) if h < w else (scale * h, size)
    if max(newh, neww) > max_size:
        scale = max_size * 1.0 / max(newh, neww)
        newh, neww = newh * scale, neww * scale
    return int(newh + 0.5), int(neww + 0.5)


def camera_rotation(roll, pitch, yaw):
    """A rotation of the camera about its optical centre, angles in degrees, camera frame x right, y down, z forward:
    Q = Rz(roll) @ Ry(yaw) @ Rx(pitch) as float64 (3, 3).  A point of the scene moves as X' = Q X."""
    r, p, y = (np.deg2rad(float(a)) for a in (roll, pitch, yaw))
    rz = np.array([[np.cos(r), -np.sin(r), 0.0], [np.sin(r), np.cos(r), 0.0], [0.0, 0.0, 1.0]])
    ry = np.array([[np.cos(y), 0.0, np.sin(y)], [0.0, 1.0, 0.0], [-np.sin(y), 0.0, np.cos(y)]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(p), -np.sin(p)], [0.0, np.sin(p), np.cos(p)]])
    return rz @ ry @ rx


def rotation_homography(K, Q):
    """-> (Hm, Hinv) float64: Hm = K Q K^-1 moves a pixel of the image to its place under the camera rotation Q, Hinv = K Q^T K^-1
    moves it back (the map a warp samples through)"""
    K, Q = np.asarray(K, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    Kinv = np.linalg.inv(K)
    return K @ Q @ Kinv, K @ Q.T @ Kinv


def homography_apply(Hm, pts):
    """pts (n, 2) pixels through the 3 x 3 map Hm -> ((n, 2) pixels, (n,) denominators), float64"""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    xyw = np.concatenate([pts, np.ones((len(pts), 1))], axis=1) @ np.asarray(Hm, dtype=np.float64).T
    with np.errstate(divide="ignore", invalid="ignore"):
        return xyw[:, :2] / xyw[:, 2:3], xyw[:, 2]


CROP_TYPES = ("relative_range", "relative", "absolute", "absolute_range")


def check_crop(crop_type, crop_size):
    """INPUT.CROP.TYPE / SIZE as detectron2's RandomCrop takes them -> (crop_type, (s0, s1)); ValueError otherwise"""
    if crop_type not in CROP_TYPES:
        raise ValueError("INPUT.CROP.TYPE must be one of {}, got {!r}".format(", ".join(CROP_TYPES), crop_type))
    if isinstance(crop_size, (str, bytes)) or not hasattr(crop_size, "__len__") or len(crop_size) != 2:
        raise ValueError("INPUT.CROP.SIZE must hold two numbers, got {!r}".format(crop_size))
    if any(isinstance(v, bool) or not isinstance(v, (int, float)) for v in crop_size):
        raise ValueError("INPUT.CROP.SIZE must hold two numbers, got {!r}".format(crop_size))
    s0, s1 = crop_size
    if crop_type.startswith("relative"):
        if not (0 < s0 <= 1 and 0 < s1 <= 1):
            raise ValueError("INPUT.CROP.SIZE of a relative crop must lie in (0, 1], got {!r}".format(crop_size))
    else:
        if int(s0) != s0 or int(s1) != s1 or s0 < 1 or s1 < 1:
            raise ValueError("INPUT.CROP.SIZE of an absolute crop must hold integers > 0, got {!r}".format(crop_size))
        s0, s1 = int(s0), int(s1)
        if crop_type == "absolute_range" and s0 > s1:
            raise ValueError("INPUT.CROP.SIZE of an absolute_range crop must be (low, high) with low <= high, got {!r}".format(crop_size))
    return crop_type, (s0, s1)


def random_crop_box(h, w, crop_type, crop_size, rng=np.random):
    """detectron2 RandomCrop.get_crop_size + get_transform -> (x0, y0, cropw, croph) inside the h x w image.  This is a reading of
    detectron2's code written down from memory, not checked against an installed detectron2: crop_size is (height, width) for
    "relative" (fractions) and "absolute" (pixels); "relative_range" draws each fraction uniformly from [size, 1] (size in float32,
    one rng.rand(2)); "absolute_range" draws the height, then the width, from [min(edge, s0), min(edge, s1)].  The origin is drawn
    last: y0, then x0."""
    if crop_type == "relative":
        ch, cw = crop_size
        croph, cropw = int(h * ch + 0.5), int(w * cw + 0.5)
    elif crop_type == "relative_range":
        size = np.asarray(crop_size, dtype=np.float32)
        ch, cw = size + rng.rand(2) * (1 - size)
        croph, cropw = int(h * ch + 0.5), int(w * cw + 0.5)
    elif crop_type == "absolute":
        croph, cropw = min(crop_size[0], h), min(crop_size[1], w)
    elif crop_type == "absolute_range":
        croph = rng.randint(min(h, crop_size[0]), min(h, crop_size[1]) + 1)
        cropw = rng.randint(min(w, crop_size[0]), min(w, crop_size[1]) + 1)
    else:
        raise ValueError("Unknown crop type {}".format(crop_type))
    y0 = rng.randint(h - croph + 1)
    x0 = rng.randint(w - cropw + 1)
    return int(x0), int(y0), int(cropw), int(croph)
