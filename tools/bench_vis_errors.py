"""Time of the 3D error report of `visualize_from_instances` on one synthetic dataset: `match_errors_from_instances` (packing the
prediction records and dataset dicts on the host, one copy, one launch of csrc/vis_errors.hip, the results back) against a host loop
written here from the same definitions, the way the reference walks its predictions (one numpy IoU call per prediction).  Device
events around `reps` back-to-back launches after a warm-up for the kernel alone; a host clock around calls that end in a
device-to-host copy for the whole function and around the host loop.  Information only: no ratio is required of these numbers.
    python tools/bench_vis_errors.py [images] [output file]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from omni3d_amd.cubercnn import vis  # noqa: E402
from omni3d_amd.cubercnn.vis import vis as V  # noqa: E402
from omni3d_amd.kernels import render, viserr  # noqa: E402

DETS, GTS, CATS = 100, 15, 50


def make_dataset(images, seed=0):
    """`images` images of DETS predictions and GTS ground truths over CATS categories; half of the predictions sit on a ground truth"""
    rs = np.random.RandomState(seed)
    K = [[500.0, 0.0, 320.0], [0.0, 500.0, 240.0], [0.0, 0.0, 1.0]]
    dicts, dets = [], []
    for i in range(images):
        annos = [{"bbox": [rs.uniform(0, 500), rs.uniform(0, 380), rs.uniform(20, 140), rs.uniform(20, 100)], "category_id": int(rs.randint(CATS)),
                  "center_cam": [rs.uniform(-2, 2), rs.uniform(-1, 1), rs.uniform(2, 20)], "dimensions": rs.uniform(0.3, 3, 3).tolist(),
                  "pose": np.eye(3).tolist()} for _ in range(GTS)]
        recs = []
        for k in range(DETS):
            a = annos[k % GTS]
            near = k % 2 == 0
            x, y, w, h = a["bbox"]
            recs.append({"image_id": i, "category_id": a["category_id"] if near else int(rs.randint(CATS)), "score": float(rs.rand()),
                         "bbox": [x + rs.uniform(-0.2, 0.2) * w, y + rs.uniform(-0.2, 0.2) * h, w, h] if near else
                         [rs.uniform(0, 500), rs.uniform(0, 380), rs.uniform(20, 140), rs.uniform(20, 100)],
                         "center_2D": [rs.uniform(0, 640), rs.uniform(0, 480)], "center_cam": [0.0, 0.0, rs.uniform(2, 20)],
                         "dimensions": rs.uniform(0.3, 3, 3).tolist(), "pose": np.eye(3).tolist()})
        dicts.append({"image_id": i, "height": 480, "width": 640, "annotations": annos, "file_name": "none"})
        dets.append({"image_id": i, "K": K, "height": 480, "width": 640, "instances": recs})
    return dicts, dets


def host_loop(dicts, dets):
    """the definitions of kernels/viserr.py in float64, one numpy IoU call per prediction -> ({name: mean}, matched pairs)"""
    errs = {n: [] for n in viserr.ERR_NAMES}
    for entry, o in zip(dicts, dets):
        annos = entry["annotations"]
        if not annos:
            continue
        gt = np.array([a["bbox"] for a in annos])
        gt[:, 2:] += gt[:, :2]
        gt_cat = np.array([a["category_id"] for a in annos])
        gt_area = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
        K = np.array(o["K"])
        for r in o["instances"]:
            idx = np.flatnonzero(gt_cat == r["category_id"])
            if len(idx) == 0:
                continue
            x1, y1, w, h = r["bbox"]
            g = gt[idx]
            iw = np.clip(np.minimum(x1 + w, g[:, 2]) - np.maximum(x1, g[:, 0]), 0, None)
            ih = np.clip(np.minimum(y1 + h, g[:, 3]) - np.maximum(y1, g[:, 1]), 0, None)
            union = w * h + gt_area[idx] - iw * ih
            iou = np.where(union > 0, iw * ih / np.where(union > 0, union, 1.0), 0.0)
            j = int(iou.argmax())
            if iou[j] < 0.5:
                continue
            a = annos[idx[j]]
            c = np.array(a["center_cam"])
            errs["xy"].append(np.sqrt((((K @ c / c[2])[:2] - np.array(r["center_2D"])) ** 2).sum()))
            errs["z"].append(abs(r["center_cam"][2] - c[2]))
            dd = np.array(r["dimensions"]) - np.array(a["dimensions"])
            for n, v in zip("whl", np.abs(dd)):
                errs[n].append(v)
            errs["dim"].append(np.sqrt((dd ** 2).sum()))
            tr = (np.array(r["pose"]) * np.array(a["pose"])).sum()
            if -1 - 1e-4 <= tr <= 3 + 1e-4:
                errs["ry"].append(np.pi / 2 - (tr - 1) / 2)
    return {n: float(np.mean(v)) if v else float("nan") for n, v in errs.items()}, len(errs["xy"])


def main(images=1000, out=None, reps=50):
    assert torch.cuda.is_available(), "needs the GPU"
    dicts, dets = make_dataset(images)
    lines = ["csrc/vis_errors.hip -- times on one synthetic dataset: %d images x %d predictions (%d in all) x %d ground truths, %d categories"
             % (images, DETS, images * DETS, GTS, CATS)]
    for _ in range(2):
        res = vis.match_errors_from_instances(dets, dicts)
    n = 5
    t0 = time.perf_counter()
    for _ in range(n):
        res = vis.match_errors_from_instances(dets, dicts)
    t_all = (time.perf_counter() - t0) / n
    t0 = time.perf_counter()
    packed = V._pack_instances(dets, dicts)
    t_pack = time.perf_counter() - t0
    dev = render.default_device()
    args = [torch.from_numpy(a).to(dev) for a in packed]
    for _ in range(5):
        viserr.match_errors(*args)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        viserr.match_errors(*args)
    e1.record()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want, pairs = host_loop(dicts, dets)
    t_host = time.perf_counter() - t0
    lines.append("match_errors_from_instances (host packing + copy + launch + results back): %.1f ms per call, host clock, %d calls" % (1e3 * t_all, n))
    lines.append("    of which packing the records into flat arrays on the host: %.1f ms" % (1e3 * t_pack))
    lines.append("viserr.match_errors on device tensors (launcher with its offset check + two kernels): %.1f us per call, device events, %d calls"
                 % (1e3 * e0.elapsed_time(e1) / reps, reps))
    lines.append("host loop from the same definitions (float64, one numpy IoU per prediction): %.1f ms, one pass" % (1e3 * t_host))
    lines.append("matched pairs: device %d, host %d" % (res["counts"][0], pairs))
    lines.append("means device | host: " + ", ".join("%s %.4f | %.4f" % (k, res["means"][k], want[k]) for k in viserr.ERR_NAMES))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 1000, sys.argv[2] if len(sys.argv) > 2 else None)
