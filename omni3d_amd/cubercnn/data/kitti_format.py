"""KITTI object label files (`<stem>.txt`, one object per line) to and from the records this project evaluates: host code around
`kernels.kitti.box_params` (corners -> h, w, l, location, rotation_y, alpha) and `det.cuboid_corners` (the way back), one launch per
call, not one per file.  The reference has no counterpart.

A line is `type truncated occluded alpha x1 y1 x2 y2 h w l x y z rotation_y [score]`.  The heading convention is the one of
`box_params`: the corner order puts the length along v1 - v0, whose angle in the ground plane is rotation_y, and `location` is the
centre of the bottom face.

CAMERA FRAME.  All coordinates are those of the records' camera frame.  No calibration file is read, and the shift by the `P2`
baseline that separates raw KITTI labels (reference camera 0) from the frame of colour camera 2 is NOT applied: files written here
are in the frame of the records, and files read here are taken to be in the frame the detections live in.  Nobody could check this
module against the real data; the data are not at hand.

Types are written capitalised (`car` -> `Car`, `dontcare` -> `DontCare`) and read back in lower case, the spelling of Omni3D's
category names."""
import os

import numpy as np
import torch

from ...kernels import det
from ...kernels import kitti as K

_SPELLING = {"dontcare": "DontCare"}
# what a line says where there is no cuboid
NO_ALPHA, NO_DIMS, NO_LOCATION, NO_ROTATION = -10.0, (-1.0, -1.0, -1.0), (-1000.0, -1000.0, -1000.0), -10.0


def _device():
    from ... import lib
    return torch.device("cpu") if lib.get().emulated else torch.device("cuda")


def _type_of(rec, names):
    n = rec.get("category_name")
    if n is None and names is not None:
        n = names[rec["category_id"]] if isinstance(names, (list, tuple)) else names.get(rec["category_id"])
    if n is None:
        raise ValueError("a record needs `category_name`, or `names` must map its category_id")
    n = str(n).lower()
    return _SPELLING.get(n, n.capitalize()).replace(" ", "_")


def _corners_of(rec):
    b = rec.get("bbox3D", rec.get("bbox3D_cam"))
    ok = b is not None and bool(rec.get("valid3D", True)) and np.asarray(b).shape == (8, 3)
    return np.asarray(b, dtype=np.float32) if ok else np.full((8, 3), np.nan, dtype=np.float32)


def write_kitti_results(records, out_dir, names=None, stems=None, decimals=2, image_ids=None, up=K.UP):
    """Writes one `<stem>.txt` per image id of `records` (`image_id`, `category_id` or `category_name`, `score`, `bbox` XYWH,
    `bbox3D` 8 x 3) into `out_dir` -> {image id: path}.  names: category id -> name (dict or list) for records without
    `category_name`; stems: image id -> stem, default "%06d" % image_id; image_ids: images that get a file even without detections (an
    empty one).  `truncated` and `occluded` are written as -1 -1; x1 y1 x2 y2 come from `bbox`; h w l, the location, rotation_y and
    alpha from `box_params` of `bbox3D` under `up`, all records in one launch.  A record without a valid cuboid writes KITTI's
    placeholders (-10, -1 -1 -1, -1000 -1000 -1000, -10).  See the module docstring for the camera frame."""
    records = list(records)
    up = K.check_up(up)
    corners = np.stack([_corners_of(r) for r in records]) if records else np.zeros((0, 8, 3), np.float32)
    params = K.box_params(torch.from_numpy(corners).to(_device()).contiguous(), up).cpu().numpy()
    os.makedirs(out_dir, exist_ok=True)
    by_img = {i: [] for i in (image_ids if image_ids is not None else [])}
    for k, r in enumerate(records):
        by_img.setdefault(r["image_id"], []).append(k)
    num = "%%.%df" % int(decimals)
    fmt = lambda vals: " ".join(num % float(v) for v in vals)      # noqa: E731
    paths = {}
    for img, idx in by_img.items():
        stem = stems[img] if stems is not None and img in stems else "%06d" % int(img)
        lines = []
        for k in idx:
            r, q = records[k], params[k]
            x, y, w, h = (float(v) for v in list(r["bbox"])[:4])
            if q[8] == 1.0:
                alpha, dims, loc, ry = q[7], q[0:3], q[3:6], q[6]
            else:
                alpha, dims, loc, ry = NO_ALPHA, NO_DIMS, NO_LOCATION, NO_ROTATION
            lines.append("%s -1 -1 %s %s %s %s %s %s" % (_type_of(r, names), num % alpha, fmt((x, y, x + w, y + h)), fmt(dims), fmt(loc), num % ry,
                                                         num % float(r["score"])))
        paths[img] = os.path.join(out_dir, stem + ".txt")
        with open(paths[img], "w") as f:
            f.write("".join(ln + "\n" for ln in lines))
    return paths


def _basis(up):
    u = np.asarray(K.check_up(up), dtype=np.float64)
    u = u / np.linalg.norm(u)
    a = np.array([1.0, 0.0, 0.0]) - u[0] * u
    a = a / np.linalg.norm(a)
    return u, a, np.cross(u, a)


def read_kitti_labels(label_dir, with_score=None, up=K.UP):
    """Reads every `*.txt` of `label_dir` (sorted by name).  Without a score column -> the list of dataset dicts {image_id, stem,
    annotations} that `KittiEval` takes as `gt`; with one (with_score=True, or None and the first non-empty line has 16 fields) -> the
    flat record list it takes as `dt`.  image_id is int(stem) when the stem is a number, else the file's index in sorted order.

    Fields: `category_name` (the type in lower case), `truncation`, integer `occlusion`, `alpha`, `bbox` (XYWH), `dimensions`
    [w, h, l], `center_cam` = location + (h / 2) up, `R_cam` (Ry(rotation_y) for the default up: the length axis is cos(ry) a -
    sin(ry) b, the height axis -up), `bbox3D_cam` = `bbox3D` (from `det.cuboid_corners`, all objects in one launch), `valid3D` (False
    for DontCare and for a line of placeholders: dimensions not all > 0 or location -1000), and `score` when present.  See the module
    docstring for the camera frame: no calibration is read and no `P2` shift is applied."""
    u, a, b = _basis(up)
    files = sorted(f for f in os.listdir(label_dir) if f.endswith(".txt"))
    rows, per_file = [], []
    for k, name in enumerate(files):
        stem = name[:-4]
        with open(os.path.join(label_dir, name)) as f:
            lines = [ln.split() for ln in f if ln.strip()]
        if with_score is None and lines:
            with_score = len(lines[0]) >= 16
        recs = []
        for t in lines:
            if len(t) < (16 if with_score else 15):
                raise ValueError("%s: a line needs %d fields, got %d" % (name, 16 if with_score else 15, len(t)))
            v = [float(x) for x in t[1:16 if with_score else 15]]
            h, w, l = v[7:10]
            loc, ry = np.array(v[10:13]), v[13]
            cname = t[0].lower()
            valid = cname != "dontcare" and min(h, w, l) > 0 and not (loc == -1000.0).any() and np.isfinite(v[7:14]).all()
            rec = {"category_name": cname, "truncation": v[0], "occlusion": int(v[1]), "alpha": v[2],
                   "bbox": [v[3], v[4], v[5] - v[3], v[6] - v[4]], "valid3D": bool(valid)}
            if with_score:
                rec["score"] = v[14]
            if valid:
                x_l = np.cos(ry) * a - np.sin(ry) * b
                y_l = -u
                rec["dimensions"] = [w, h, l]
                rec["center_cam"] = (loc + 0.5 * h * u).tolist()
                rec["R_cam"] = np.stack([x_l, y_l, np.cross(x_l, y_l)], axis=1).tolist()
                rows.append(rec)
            else:
                rec["dimensions"], rec["center_cam"], rec["R_cam"] = [-1.0] * 3, [-1.0] * 3, np.eye(3).tolist()
                rec["bbox3D_cam"] = rec["bbox3D"] = np.full((8, 3), -1.0).tolist()
            recs.append(rec)
        per_file.append((int(stem) if stem.isdigit() else k, stem, recs))
    if rows:
        dev = _device()
        box = torch.tensor([r["center_cam"] + r["dimensions"] for r in rows], dtype=torch.float32, device=dev)
        R = torch.tensor([r["R_cam"] for r in rows], dtype=torch.float32, device=dev).reshape(-1, 9)
        verts = det.cuboid_corners(box, R).cpu().numpy().astype(np.float64)
        for r, c in zip(rows, verts):
            r["bbox3D_cam"] = c.tolist()
            r["bbox3D"] = c.tolist()
    if with_score:
        return [dict(r, image_id=img, stem=stem) for img, stem, recs in per_file for r in recs]
    return [{"image_id": img, "stem": stem, "annotations": [dict(r, image_id=img) for r in recs]} for img, stem, recs in per_file]
