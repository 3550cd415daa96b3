"""`cubercnn.vis.visualize_from_instances` / `match_errors_from_instances` end to end on a synthetic in-memory dataset, and the small
drawing helpers `draw_line` / `draw_2d_box` / `draw_bev`.  The kernel behind the error line is pinned in test_vis_errors.py; here the
packing of the prediction records and dataset dicts, the log line, the sample files and the geometry handed to
`omni_draw_segments` are checked against float64 evaluations written in this file."""
import os

import numpy as np
import pytest

N_IMAGES, H, W = 101, 64, 80                       # 101: the samples are the images 0, 50 and 100
CATS = ["chair", "table", "sofa", "bed"]
THRES = np.sqrt(1 / len(CATS))                     # 0.5
EDGES = [[0, 1], [1, 2], [2, 3], [3, 0], [1, 5], [5, 6], [6, 2], [4, 5], [4, 7], [6, 7], [0, 4], [3, 7]]


def _image(seed):
    """smooth, so that a JPEG round trip stays close"""
    ys, xs = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    rs = np.random.RandomState(seed)
    ch = [90 + 60 * np.sin(2 * np.pi * (rs.uniform(0.3, 1.2) * xs + rs.uniform(0.3, 1.2) * ys) + rs.uniform(0, 6)) for _ in range(3)]
    return np.clip(np.rint(np.stack(ch, axis=-1)), 0, 255).astype(np.uint8)


def _rot_y(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def _dataset(seed=0, empty=(), low_scores=False, no_match=False):
    """-> (dataset dicts, prediction records).  `empty`: images without annotations; `low_scores`: every score below the drawing
    threshold; `no_match`: every prediction carries a category no ground truth of its image has"""
    from omni3d_amd.d2.structures import BoxMode
    rs = np.random.RandomState(seed)
    K = np.array([[70.0, 0.0, 40.5], [0.0, 72.0, 31.0], [0.0, 0.0, 1.0]])
    dicts, dets = [], []
    for i in range(N_IMAGES):
        annos, recs = [], []
        n_gt = 0 if i in empty else (2 if i % 50 == 0 else int(rs.randint(0, 4)))
        for j in range(n_gt):
            z = rs.uniform(3.0, 8.0)
            c = np.array([rs.uniform(-0.3, 0.3) * z, rs.uniform(-0.25, 0.25) * z, z])
            u, v = (K @ c)[:2] / z
            w, h = rs.uniform(14, 30), rs.uniform(12, 26)
            box = [u - w / 2, v - h / 2, w, h]
            xyxy = j % 2 == 1                                               # every other box is stored as XYXY
            annos.append({"bbox": [box[0], box[1], box[0] + w, box[1] + h] if xyxy else box, "bbox_mode": BoxMode.XYXY_ABS if xyxy else BoxMode.XYWH_ABS,
                          "category_id": int(rs.randint(len(CATS) - 1)), "center_cam": c.tolist(), "dimensions": rs.uniform(0.5, 1.5, 3).tolist(),
                          "pose": _rot_y(rs.uniform(-3, 3)).tolist()})
            if not xyxy and i % 3 == 0:
                del annos[-1]["bbox_mode"]                                  # the Omni3D default
            # a prediction near this ground truth (IoU well above or well below 0.5) and sometimes an unrelated one
            shift = rs.choice([0.05, 0.6]) * w
            score = rs.uniform(0.05, 0.45) if low_scores else rs.choice([0.9, 0.75, 0.3])
            recs.append({"image_id": 1000 + i, "category_id": len(CATS) - 1 if no_match else annos[-1]["category_id"],
                         "bbox": [box[0] + shift, box[1] + 1.0, w, h], "score": float(score), "depth": float(z + 0.3),
                         "center_cam": [float(c[0]), float(c[1]), float(z + rs.uniform(-0.5, 0.5))],
                         "center_2D": [float(u + rs.uniform(-3, 3)), float(v + rs.uniform(-3, 3))],
                         "dimensions": (np.asarray(annos[-1]["dimensions"]) + rs.uniform(-0.2, 0.2, 3)).tolist(),
                         "pose": (_rot_y(rs.uniform(-0.5, 0.5)) @ np.asarray(annos[-1]["pose"])).tolist()})
        if rs.rand() < 0.4:
            recs.append({"image_id": 1000 + i, "category_id": int(rs.randint(len(CATS) - 1)), "bbox": [2.0, 3.0, 9.0, 8.0],
                         "score": 0.2, "depth": 4.0, "center_cam": [0.0, 0.0, 4.0], "center_2D": [6.0, 7.0], "dimensions": [1.0, 1.0, 1.0],
                         "pose": np.eye(3).tolist()})
        dicts.append({"image_array": _image(i), "height": H, "width": W, "K": K.tolist(), "image_id": 1000 + i, "annotations": annos,
                      "file_name": "memory://%d" % i})
        dets.append({"image_id": 1000 + i, "K": K.tolist(), "width": W, "height": H, "instances": recs})
    return dicts, dets


def _reference_means(dicts, dets):
    """float64, the loop of the definition -> ({name: mean}, matched pairs, per-image lists of the matched ground-truth index)"""
    from omni3d_amd.d2.structures import BoxMode
    errs, matches = {n: [] for n in ("xy", "z", "w", "h", "l", "dim", "ry")}, []
    for entry, o in zip(dicts, dets):
        K = np.asarray(o["K"], np.float64)
        per = []
        for r in o["instances"]:
            x1, y1, w, h = r["bbox"]
            best, bj = -1.0, -1
            for j, a in enumerate(entry["annotations"]):
                if a["category_id"] != r["category_id"]:
                    continue
                g = a["bbox"]
                if a.get("bbox_mode", BoxMode.XYWH_ABS) == BoxMode.XYXY_ABS:
                    g = [g[0], g[1], g[2] - g[0], g[3] - g[1]]
                # the float32 values the launcher receives
                bx = [float(np.float32(t)) for t in (x1, y1, w, h)]
                gx = [float(np.float32(t)) for t in g]
                iw = max(min(bx[0] + bx[2], gx[0] + gx[2]) - max(bx[0], gx[0]), 0.0)
                ih = max(min(bx[1] + bx[3], gx[1] + gx[3]) - max(bx[1], gx[1]), 0.0)
                union = bx[2] * bx[3] + gx[2] * gx[3] - iw * ih
                iou = iw * ih / union if union > 0 else 0.0
                if iou > best:
                    best, bj = iou, j
            assert abs(best - 0.5) > 1e-3                                   # a condition on the data: no match near the threshold
            per.append(bj if best >= 0.5 else -1)
            if best < 0.5:
                continue
            a = entry["annotations"][bj]
            c = np.asarray(a["center_cam"], np.float64)
            errs["xy"].append(np.linalg.norm(np.asarray(r["center_2D"]) - (K @ c / c[2])[:2]))
            errs["z"].append(abs(r["center_cam"][2] - c[2]))
            dd = np.asarray(r["dimensions"]) - np.asarray(a["dimensions"])
            for n, v in zip("whl", np.abs(dd)):
                errs[n].append(v)
            errs["dim"].append(np.linalg.norm(dd))
            tr = np.trace(np.asarray(r["pose"]) @ np.asarray(a["pose"]).T)
            if -1 - 1e-4 <= tr <= 3 + 1e-4:
                errs["ry"].append(np.pi / 2 - (tr - 1) / 2)
        matches.append(per)
    return {n: (float(np.mean(v)) if v else float("nan")) for n, v in errs.items()}, len(errs["xy"]), matches


def _line(name, iteration, m):
    ry = m["ry"] if m["ry"] == m["ry"] else 1000.0
    return name + "iter={}, xy({:.2f}), z({:.2f}), whl({:.2f}, {:.2f}, {:.2f}), ry({:.2f})\n".format(iteration, m["xy"], m["z"], m["w"], m["h"],
                                                                                                   m["l"], ry)


def _segment_distance(segs):
    ys, xs = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    best = np.full((H, W), np.inf)
    for a, b in segs:
        e = b - a
        l2 = float(e @ e)
        s = np.clip(((xs - a[0]) * e[0] + (ys - a[1]) * e[1]) / l2, 0, 1) if l2 > 0 else np.zeros_like(xs)
        best = np.minimum(best, np.hypot(xs - a[0] - s * e[0], ys - a[1] - s * e[1]))
    return best


def _drawn_geometry(o):
    """float64: the projected edges of the predictions above the threshold and the rectangles of their labels"""
    from PIL import ImageFont
    from omni3d_amd.cubercnn.util import mesh_cuboid
    K = np.asarray(o["K"], np.float64)
    segs, rects = [], []
    for r in o["instances"]:
        if not r["score"] > THRES:
            continue
        z = r["center_cam"][2]
        c = np.linalg.inv(K) @ (z * np.array(r["center_2D"] + [1.0]))
        verts = mesh_cuboid(list(c) + list(r["dimensions"]), np.asarray(r["pose"])).verts_padded()[0].double().numpy()
        assert verts[:, 2].min() > 0.5
        p = (K @ verts.T / verts[:, 2]).T[:, :2]
        segs += [(p[i], p[j]) for i, j in EDGES]
        text = "{}, z={:.1f}, s={:.2f}".format(CATS[r["category_id"]], c[2], r["score"])
        x0, y0, x1, y1 = ImageFont.load_default().getbbox(text)
        xs, ye = int(np.clip(r["bbox"][0], 0, W)), int(np.clip(r["bbox"][1], 0, H))
        rects.append((xs, int(np.clip(ye - (y1 - y0) - 4, 0, H)), int(np.clip(xs + (x1 - x0) + 4, 0, W)), ye))
    return segs, rects


def _read_bgr(path):
    from PIL import Image
    with Image.open(path) as im:
        assert im.size == (W, H)
        return np.asarray(im.convert("RGB"))[:, :, ::-1].astype(np.float64)


def _run_end_to_end(tmp_path):
    from omni3d_amd.cubercnn import vis
    dicts, dets = _dataset()
    want, pairs, matches = _reference_means(dicts, dets)
    assert pairs > 20 and all(abs(v * 100 - np.floor(v * 100) - 0.5) > 0.01 for v in want.values())    # conditions on the data
    out = tmp_path / "plain"
    line = vis.visualize_from_instances(dets, dicts, "SyntheticSet", 64, str(out), CATS, iteration=1234)
    assert line == _line("SyntheticSet", 1234, want)
    assert sorted(os.listdir(str(out))) == ["vis"]
    assert sorted(os.listdir(str(out / "vis"))) == ["000000.jpg", "000050.jpg", "000100.jpg"]
    thickness = int(np.round(3 * H / 500))
    for imind in (0, 50, 100):
        got, src = _read_bgr(str(out / "vis" / ("%06d.jpg" % imind))), dicts[imind]["image_array"].astype(np.float64)
        segs, rects = _drawn_geometry(dets[imind])
        far = _segment_distance(segs) > thickness / 2 + 1 if segs else np.ones((H, W), bool)
        for x0, y0, x1, y1 in rects:
            far[y0:y1, x0:x1] = False
        assert far.sum() > 0.3 * H * W
        diff = np.abs(got - src)[far]
        print("sample %d: %d boxes drawn, |jpeg - source| away from the drawing: mean %.2f max %.1f" % (imind, len(rects), diff.mean(), diff.max()))
        assert diff.mean() < 2.0 and diff.max() < 16.0
        if segs:                                                            # ... and something was drawn where the edges are
            near = _segment_distance(segs) <= 0.5
            assert np.abs(got - src)[near].max() > 40
    assert any(_drawn_geometry(dets[i])[0] for i in (0, 50, 100))
    # the numbers behind the line
    res = vis.match_errors_from_instances(dets, dicts)
    flat = [m for per in matches for m in per]
    gt_off = np.concatenate(([0], np.cumsum([len(d["annotations"]) for d in dicts])))
    img = np.repeat(np.arange(N_IMAGES), [len(o["instances"]) for o in dets])
    assert res["match"].tolist() == [-1 if m < 0 else int(gt_off[i] + m) for m, i in zip(flat, img)]
    assert res["counts"][0] == pairs and set(res["means"]) == {"xy", "z", "w", "h", "l", "dim", "ry"}
    for n, v in want.items():
        assert abs(res["means"][n] - v) <= 1e-5 * (1 + abs(v)), (n, res["means"][n], v)
    assert res["err"].shape == (len(flat), 7) and bool(np.isnan(res["err"].numpy()[np.asarray(flat) < 0]).all())

    # an object exposing the dicts as `._dataset` (detectron2's MapDataset) gives the same line
    class Mapped:
        def __init__(self, d):
            self._dataset = d

    assert vis.visualize_from_instances(dets, Mapped(dicts), "SyntheticSet", 64, str(tmp_path / "mapped"), CATS, iteration=1234) == line
    # a sample whose image has no ground truth is not written
    d2, p2 = _dataset(empty=(50,))
    out = tmp_path / "gap"
    vis.visualize_from_instances(p2, d2, "SyntheticSet", 64, str(out), CATS)
    assert sorted(os.listdir(str(out / "vis"))) == ["000000.jpg", "000100.jpg"]
    # all scores below the threshold: the samples are the unmodified images
    d3, p3 = _dataset(low_scores=True)
    out = tmp_path / "low"
    vis.visualize_from_instances(p3, d3, "SyntheticSet", 64, str(out), CATS)
    for imind in (0, 50, 100):
        diff = np.abs(_read_bgr(str(out / "vis" / ("%06d.jpg" % imind))) - d3[imind]["image_array"].astype(np.float64))
        assert diff.mean() < 2.0 and diff.max() < 16.0
    # no prediction matches: nan, and the reference's stand-in for ry
    d4, p4 = _dataset(no_match=True)
    line = vis.visualize_from_instances(p4, d4, "SyntheticSet", 64, str(tmp_path / "none"), CATS, iteration="final")
    assert line == "SyntheticSetiter=final, xy(nan), z(nan), whl(nan, nan, nan), ry(1000.00)\n"


def test_visualize_from_instances_emulated(emu_lib, tmp_path):
    _run_end_to_end(tmp_path)


@pytest.mark.gpu
def test_visualize_from_instances_gpu(hip_lib, tmp_path):
    _run_end_to_end(tmp_path)


# ---- draw_line / draw_2d_box / draw_bev --------------------------------------------------------------------------------------------

def _bev_reference(width, z3d, l3d, w3d, x3d, ry3d, scale):
    """float64 evaluation of the reference's bird's-eye corners, with its swap of w and l"""
    w, l, x, z, r = l3d * scale, w3d * scale, x3d * scale, z3d * scale, -ry3d
    out = []
    for cx, cy in ((-w / 2, -l / 2), (w / 2, -l / 2), (w / 2, l / 2), (-w / 2, l / 2)):
        out.append([np.cos(r) * cx - np.sin(r) * cy + w / 2 + x + width / 2, np.sin(r) * cx + np.cos(r) * cy + l / 2 + z])
    return np.asarray(out)


def _check_painted(before, after, segs, thickness, color):
    """painted pixels lie within thickness / 2 + 1 px of the float64 segments; the pixels whose centre is within thickness / 2 of the
    segment between the truncated end points (the pixels cv2.line is handed) are all painted"""
    changed = (after != before).any(-1)
    segs = [(np.asarray(a, np.float64), np.asarray(b, np.float64)) for a, b in segs]
    assert changed.any() and (_segment_distance(segs)[changed] <= thickness / 2 + 1).all()
    drawn = [(np.trunc(a) + 0.5, np.trunc(b) + 0.5) for a, b in segs]
    core = _segment_distance(drawn) <= thickness / 2 - 1e-3
    assert core.any() and changed[core].all()
    assert (after[changed] == np.asarray(color, np.uint8)).all()


def _run_helpers():
    from omni3d_amd.cubercnn import vis
    color = (10, 200, 250)
    for thickness in (1, 2, 5):
        im = _image(7)
        before = im.copy()
        vis.draw_line(im, (5.7, 9.2), (70.9, 50.6), color=color, thickness=thickness)
        _check_painted(before, im, [((5.7, 9.2), (70.9, 50.6))], thickness, color)
        im = _image(8)
        before = im.copy()
        box = [12.6, 8.3, 40.8, 30.9]
        vis.draw_2d_box(im, box, color=color, thickness=thickness)
        x1, y1, x2, y2 = box[0], box[1], box[0] + box[2] - 1, box[1] + box[3] - 1
        _check_painted(before, im, [((x1, y1), (x2, y1)), ((x2, y1), (x2, y2)), ((x2, y2), (x1, y2)), ((x1, y2), (x1, y1))], thickness, color)
    for yaw in (0.0, 0.7):
        im = _image(9)
        before = im.copy()
        args = dict(z3d=2.1, l3d=2.4, w3d=1.3, x3d=-0.6, ry3d=yaw, scale=10)
        corners = vis.draw_bev(im, color=color, thickness=2, **args)
        want = _bev_reference(W, **args)
        assert corners.shape == (4, 2) and np.abs(corners - want).max() < 1e-12
        assert want.min() > 0 and (want[:, 0] < W).all() and (want[:, 1] < H).all()
        _check_painted(before, im, [(want[k], want[(k + 1) % 4]) for k in range(4)], 2, color)


def test_draw_helpers_emulated(emu_lib):
    _run_helpers()


@pytest.mark.gpu
def test_draw_helpers_gpu(hip_lib):
    _run_helpers()
