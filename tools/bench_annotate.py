"""Time of deriving the box fields of a synthetic dataset: the two ragged launches of csrc/annotate.hip (`kernels.annotate.box_annotate`
+ `visibility_ragged`, all images at once) against the per-image loop a user of the reference's building blocks writes
(`math_util.estimate_visibility` + `convert_3d_box_to_2d` once per image: uploads, one launch each and a device-to-host copy per
image).  Device events around `reps` back-to-back ragged launches after a warm-up; a host clock around the whole `annotate_dataset`
and around the loop, both of which end in device-to-host copies.  Information only: no ratio is required of these numbers.
    python tools/bench_annotate.py [images] [boxes per image] [output file]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from omni3d_amd.cubercnn.data import annotate as A  # noqa: E402
from omni3d_amd.cubercnn.util import math_util as M  # noqa: E402
from omni3d_amd.kernels import annotate as KA  # noqa: E402
from omni3d_amd.kernels import render  # noqa: E402

WIDTH, HEIGHT = 640, 480
K = [[500.0, 0.0, 320.0], [0.0, 500.0, 240.0], [0.0, 0.0, 1.0]]


def make_dataset(images, boxes, seed=0):
    rs = np.random.RandomState(seed)
    ims = [{"id": i, "width": WIDTH, "height": HEIGHT, "K": K} for i in range(images)]
    annos = []
    for i in range(images):
        for _ in range(boxes):
            z = rs.uniform(2.0, 20.0)
            t = rs.uniform(-np.pi, np.pi)
            annos.append({"id": len(annos), "image_id": i, "valid3D": True, "center_cam": [rs.uniform(-0.7, 0.7) * z, rs.uniform(-0.5, 0.5) * z, z],
                          "dimensions": rs.uniform(0.3, 3.0, 3).tolist(),
                          "R_cam": [[np.cos(t), 0.0, np.sin(t)], [0.0, 1.0, 0.0], [-np.sin(t), 0.0, np.cos(t)]]})
    return {"images": ims, "annotations": annos}


def per_image_loop(dataset):
    """the reference's way: one estimate_visibility and one convert_3d_box_to_2d per image -> number of boxes handled"""
    by_image = {}
    for a in dataset["annotations"]:
        by_image.setdefault(a["image_id"], []).append(a)
    done = 0
    for im in dataset["images"]:
        annos = by_image.get(im["id"], [])
        if not annos:
            continue
        box3d = [a["center_cam"] + a["dimensions"] for a in annos]
        R = [a["R_cam"] for a in annos]
        M.estimate_visibility(im["K"], box3d, R, im["width"], im["height"])
        M.convert_3d_box_to_2d(im["K"], box3d, R, im["width"], im["height"], XYWH=False)[0].tolist()
        done += len(annos)
    return done


def main(images=200, boxes=13, out=None, reps=20):
    assert torch.cuda.is_available(), "needs the GPU"
    dataset = make_dataset(images, boxes)
    lines = ["csrc/annotate.hip -- times on one synthetic dataset: %d images of %d x %d with %d boxes each (%d in all)"
             % (images, WIDTH, HEIGHT, boxes, images * boxes)]
    for _ in range(2):
        A.annotate_dataset(dataset, overwrite=True)
    n = 3
    t0 = time.perf_counter()
    for _ in range(n):
        A.annotate_dataset(dataset, overwrite=True)
    t_all = (time.perf_counter() - t0) / n
    t0 = time.perf_counter()
    packed = A._pack(make_dataset(images, boxes))
    t_pack = time.perf_counter() - t0
    dev = render.default_device()
    args = [torch.from_numpy(a).to(dev) for a in packed[1:]]
    for _ in range(3):
        KA.box_annotate(*args)
        KA.visibility_ragged(*args)
    torch.cuda.synchronize()
    times = []
    for fn in (KA.box_annotate, KA.visibility_ragged):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn(*args)
        e1.record()
        torch.cuda.synchronize()
        times.append(1e3 * e0.elapsed_time(e1) / reps)
    per_image_loop(make_dataset(min(images, 5), boxes))
    t0 = time.perf_counter()
    done = per_image_loop(dataset)
    t_loop = time.perf_counter() - t0
    lines.append("annotate_dataset (host packing + one copy + two launches + results back + writing the fields): %.1f ms per call, host clock, %d calls"
                 % (1e3 * t_all, n))
    lines.append("    of which packing the annotations into flat arrays on the host: %.1f ms" % (1e3 * t_pack))
    lines.append("kernels.annotate.box_annotate on device tensors (launcher with its offset check + one kernel): %.1f us per call, device events, %d calls"
                 % (times[0], reps))
    lines.append("kernels.annotate.visibility_ragged on device tensors (launcher, tile offsets, one kernel): %.1f us per call, device events, %d calls"
                 % (times[1], reps))
    lines.append("per-image loop (estimate_visibility + convert_3d_box_to_2d once per image, %d boxes): %.1f ms, host clock, one pass" % (done, 1e3 * t_loop))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200, int(sys.argv[2]) if len(sys.argv) > 2 else 13, sys.argv[3] if len(sys.argv) > 3 else None)
