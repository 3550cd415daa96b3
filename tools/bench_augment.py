"""Time of one training-mapper call per image with the augmentations of csrc/augment.hip: `DatasetMapper3D(cfg, True, device)` from
configs/Base.yaml (MIN_SIZE_TRAIN 256..640, random flip) on a 375 x 1242 and a 1080 x 1920 source with eight cuboids, in five
variants -- plain (the parent's path: csrc/resize.hip with host-built tables, reported as context only), INPUT.CROP, INPUT.CROP +
INPUT.COLOR_JITTER, INPUT.CAMERA_ROTATION (csrc/warp.hip: the warp of the full frame, then the plain resize, timed with the resize's
tables cached like the plain call it is compared with) and INPUT.CAMERA_ROTATION + INPUT.CROP (the warp of the window only, then the
plain resize, whose tables are new for every crop and built on the host).  The plain path is timed twice: "cold", the table cache emptied before the first call, so that each of the 25
output sizes of MIN_SIZE_TRAIN builds its tables on the host when it first appears, and "tables cached", every table of this source
built before the first call -- its steady state on a dataset with a handful of source sizes.  Each figure is the median over 20
calls, after 5 warm-up calls, of the time between two device events recorded around the whole call (host work, the upload and the
launches); every crop draws a new size pair.  Next to them the host time of
`pil_bilinear_coeffs` on a cache miss against `device_coeffs` for the same pair.  Information only: no ratio is required.
    python tools/bench_augment.py [output file]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from omni3d_amd.cubercnn.config import add_camera_rotation_config, add_color_jitter_config, get_cfg_defaults  # noqa: E402
from omni3d_amd.cubercnn.data import DatasetMapper3D  # noqa: E402
from omni3d_amd.d2.config import get_cfg  # noqa: E402
from omni3d_amd.d2.data import resize_shortest_edge_size  # noqa: E402
from omni3d_amd.d2.structures import BoxMode  # noqa: E402
from omni3d_amd.kernels import augment, resize  # noqa: E402

SOURCES = [(375, 1242), (1080, 1920)]
VARIANTS = [("plain", []), ("crop", ["INPUT.CROP.ENABLED", True]), ("crop + jitter", ["INPUT.CROP.ENABLED", True, "INPUT.COLOR_JITTER.ENABLED", True]),
            ("rotate", ["INPUT.CAMERA_ROTATION.ENABLED", True]), ("rotate + crop", ["INPUT.CAMERA_ROTATION.ENABLED", True, "INPUT.CROP.ENABLED", True])]
CACHED = {"plain": (False, True), "rotate": (True,)}      # variants whose resize tables depend on the source alone: timed with them built
WARMUP, CALLS = 5, 20


def make_record(h, w, boxes=8, seed=0):
    rs = np.random.RandomState(seed)
    f = 0.8 * w
    K = [[f, 0.0, w / 2.0], [0.0, f, h / 2.0], [0.0, 0.0, 1.0]]
    annos = []
    for _ in range(boxes):
        z = rs.uniform(5.0, 30.0)
        c = np.array([rs.uniform(-0.4, 0.4) * z * w / f, rs.uniform(-0.3, 0.3) * z * h / f, z])
        d = rs.uniform(0.5, 2.5, 3)
        corners = np.array([[c[0] + sx * d[0] / 2, c[1] + sy * d[1] / 2, c[2] + sz * d[2] / 2] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
        uv = corners @ np.array(K).T
        uv = uv[:, :2] / uv[:, 2:3]
        eye = np.eye(3).tolist()
        annos.append({"bbox": [uv[:, 0].min(), uv[:, 1].min(), uv[:, 0].max(), uv[:, 1].max()], "bbox_mode": BoxMode.XYXY_ABS, "category_id": 0,
                      "center_cam": c.tolist(), "dimensions": d.tolist(), "pose": eye, "R_cam": eye, "bbox3D_cam": corners.tolist(),
                      "ignore": False, "iscrowd": 0})
    return {"image_array": rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8), "height": h, "width": w, "K": K, "image_id": seed,
            "dataset_id": 0, "annotations": annos}


def make_cfg(opts):
    cfg = get_cfg()
    get_cfg_defaults(cfg)
    add_color_jitter_config(cfg)
    add_camera_rotation_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "Base.yaml"))
    cfg.merge_from_list(list(opts))
    return cfg


def time_mapper(mapper, record):
    """-> median ms of CALLS calls between device events, after WARMUP calls"""
    times = []
    for k in range(WARMUP + CALLS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        mapper(record)
        e1.record()
        torch.cuda.synchronize()
        if k >= WARMUP:
            times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def time_coeffs(in_size, out_size, device):
    """-> (host ms of pil_bilinear_coeffs on a cache miss, ms of device_coeffs between device events), medians of CALLS after WARMUP"""
    host, dev = [], []
    for k in range(WARMUP + CALLS):
        resize.pil_bilinear_coeffs.cache_clear()
        t0 = time.perf_counter()
        resize.pil_bilinear_coeffs(in_size, out_size)
        t1 = time.perf_counter()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        augment.device_coeffs(in_size, out_size, device)
        e1.record()
        torch.cuda.synchronize()
        if k >= WARMUP:
            host.append(1e3 * (t1 - t0))
            dev.append(e0.elapsed_time(e1))
    resize.pil_bilinear_coeffs.cache_clear()
    return statistics.median(host), statistics.median(dev)


def main(out=None):
    assert torch.cuda.is_available(), "needs the GPU"
    device = torch.device("cuda")
    lines = ["csrc/augment.hip -- one DatasetMapper3D training call per image (configs/Base.yaml sizes, 8 cuboids), median of %d calls after %d, "
             "device events around the call" % (CALLS, WARMUP)]
    for h, w in SOURCES:
        record = make_record(h, w)
        for name, opts in VARIANTS:
            for cached in CACHED.get(name, (None,)):
                cfg = make_cfg(opts)
                mapper = DatasetMapper3D(cfg, True, device=device, rng=np.random.RandomState(0))
                mapper.dataset_id_to_unknown_cats = {0: set()}
                resize.pil_bilinear_coeffs.cache_clear()
                if cached:
                    for size in cfg.INPUT.MIN_SIZE_TRAIN:
                        nh, nw = resize_shortest_edge_size(h, w, (size,), cfg.INPUT.MAX_SIZE_TRAIN, "choice")
                        resize.pil_bilinear_coeffs(w, nw), resize.pil_bilinear_coeffs(h, nh)
                label = name if cached is None else name + (", tables cached" if cached else ", cold")
                lines.append("%4d x %4d  %-22s %7.3f ms%s" % (h, w, label, time_mapper(mapper, record),
                                                              "   (the parent's path, context only)" if name == "plain" else ""))
    lines.append("coefficient tables for one size pair: host pil_bilinear_coeffs on a cache miss (host clock) | device_coeffs (allocation + one "
                 "launch, device events)")
    for in_size, out_size in ((1242, 640), (1118, 1067), (1920, 1138), (1080, 640)):
        th, td = time_coeffs(in_size, out_size, device)
        lines.append("%5d -> %4d   host %7.3f ms | device %7.3f ms" % (in_size, out_size, th, td))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
