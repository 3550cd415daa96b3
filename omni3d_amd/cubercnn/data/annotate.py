"""From a user's own 3D boxes to Omni3D annotations: the six derived fields that `cubercnn.data.datasets` reads (`bbox3D_cam`,
`bbox2D_proj`, `bbox2D_trunc`, `truncation`, `behind_camera`, `visibility`) computed from `center_cam`, `dimensions`, `R_cam`, the
image's `K` and its size, for a whole dataset in two launches of csrc/annotate.hip (`kernels.annotate`).  The reference ships the
per-box / per-image building blocks only (cubercnn/util/math_util.py: `convert_3d_box_to_2d`, `estimate_truncation`,
`estimate_visibility`)."""
import numpy as np
import torch

from ...kernels import annotate as _k
from ...kernels import render

FIELDS = ("bbox3D_cam", "bbox2D_proj", "bbox2D_trunc", "truncation", "behind_camera", "visibility")
SOURCES = ("center_cam", "dimensions", "R_cam")


def _unavailable(anno, key):
    """missing, -1, or a (nested) list of nothing but -1: the file format's way of saying "not there" """
    if key not in anno or anno[key] is None:
        return True
    v = anno[key]
    if isinstance(v, bool):
        return False
    if isinstance(v, (list, tuple)):
        flat = np.asarray(v, np.float64).reshape(-1)
        return len(flat) == 0 or bool((flat == -1).all())
    return v == -1


def _pack(dataset):
    """the annotations to derive (valid3D and all three source fields there), grouped by image in the order of dataset['images'],
    as the flat arrays of `kernels.annotate` -> (annotations, box3d (N,6), R (N,9), box_off (I+1,), K (I,9), size (I,2))"""
    images = dataset["images"]
    row = {im["id"]: i for i, im in enumerate(images)}
    per_image = [[] for _ in images]
    for a in dataset["annotations"]:
        if bool(a.get("valid3D", False)) and not any(_unavailable(a, s) for s in SOURCES) and a["image_id"] in row:
            per_image[row[a["image_id"]]].append(a)
    annos = [a for group in per_image for a in group]
    N, I = len(annos), len(images)
    box3d, R = np.zeros((N, 6), np.float32), np.zeros((N, 9), np.float32)
    for n, a in enumerate(annos):
        box3d[n, :3], box3d[n, 3:] = a["center_cam"], a["dimensions"][:3]
        R[n] = np.asarray(a["R_cam"], np.float64).reshape(9)
    K, size = np.zeros((I, 9), np.float32), np.zeros((I, 2), np.int32)
    for i, im in enumerate(images):
        K[i], size[i] = np.asarray(im["K"], np.float64).reshape(9), (im["width"], im["height"])
    off = np.concatenate(([0], np.cumsum([len(g) for g in per_image], dtype=np.int64))).astype(np.int32)
    return annos, box3d, R, off, K, size


def annotate_dataset(dataset, device=None, overwrite=False, min_z=0.20, zplane=0.05):
    """Fills, in place, the derived fields of every annotation of an Omni3D dict (`images` with id / width / height / K,
    `annotations` with image_id / valid3D / center_cam / dimensions [w, h, l] / R_cam) that has `valid3D` and the three source fields:
      bbox3D_cam     8 x 3 vertices in the order of get_cuboid_verts_faces
      bbox2D_proj    XYXY of the projected vertices (`convert_3d_box_to_2d(..., XYWH=False)` with the image size as clip)
      bbox2D_trunc   bbox2D_proj cut to [0, W - 1] x [0, H - 1]; [-1, -1, -1, -1] where nothing with an area is left
      truncation     `estimate_truncation`; -1 where the projection has no area (the reference's division gives NaN there)
      behind_camera  any vertex at z <= min_z
      visibility     visible / area of `estimate_visibility`; -1 for a box that covers no pixel (NaN in the reference; -1 is the
                     file format's "unavailable")
    A field is written only where it is missing or unavailable (-1, or a list of -1), every field when `overwrite` is set.
    Occlusion is judged among the boxes of the same image only -- and only among those derived here: an annotation without valid3D
    or without a source field hides nothing.  Everything is packed once on the host, copied once, computed by one launch of each of
    the two kernels and copied back once.  -> {field: number of annotations it was written to}."""
    annos, box3d, R, off, K, size = _pack(dataset)
    counts = {f: 0 for f in FIELDS}
    if not annos:
        return counts
    dev = render.default_device() if device is None else torch.device(device)
    args = [torch.from_numpy(a).to(dev) for a in (box3d, R, off, K, size)]
    verts3d, _, proj, trunc, truncation, behind, _ = _k.box_annotate(*args, min_z=min_z)
    area, visible = _k.visibility_ragged(*args, zplane=zplane)
    verts3d, proj, trunc = verts3d.cpu().numpy().astype(np.float64), proj.cpu().numpy().astype(np.float64), trunc.cpu().numpy().astype(np.float64)
    truncation, behind, area, visible = truncation.cpu().numpy(), behind.cpu().numpy(), area.cpu().numpy(), visible.cpu().numpy()
    for n, a in enumerate(annos):
        values = {"bbox3D_cam": verts3d[n].tolist(), "bbox2D_proj": proj[n].tolist(), "bbox2D_trunc": trunc[n].tolist(),
                  "truncation": -1 if np.isnan(truncation[n]) else float(truncation[n]), "behind_camera": bool(behind[n]),
                  "visibility": float(visible[n]) / float(area[n]) if area[n] > 0 else -1}
        for f in FIELDS:
            if overwrite or _unavailable(a, f):
                a[f] = values[f]
                counts[f] += 1
    return counts
