"""Time of the KITTI-protocol evaluation (`KittiEval`, csrc/eval_kitti.hip), run by hand on an MI355X; not part of bench.py.
A KITTI-val-sized synthetic set: 3769 images, about 8 ground truths and 20 detections per image over car / pedestrian / cyclist (plus
vans, persons and DontCare regions), yaw-only cuboids, detections = jittered ground truths and clutter.  `KittiEval.evaluate()`
(packing, three similarity passes, the four launches, one synchronisation) between device events: the median of 5 blocks after one
warm-up call.  Beside it, on the same records, `Omni3Deval(mode="3D")` `evaluate()` + `accumulate()`: the existing thing a reader can
relate the number to, not a bar.  Information only: there is no earlier figure and no speed bar.
    python tools/bench_kitti_eval.py [output file]
    python tools/bench_kitti_eval.py --aos [output file]     # evaluate() without and with AOS in one run, both figures APPENDED to the file
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_kitti_eval.py --once      # one evaluate() for the per-launch times"""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from omni3d_amd import boxgen  # noqa: E402
from omni3d_amd.cubercnn.evaluation import AnnotationIndex, KittiEval, Omni3Deval  # noqa: E402

IMAGES, BLOCKS = 3769, 5
NAMES = {1: "car", 2: "pedestrian", 3: "cyclist", 4: "van", 5: "person", 6: "dontcare"}
DIMS = {1: (3.9, 1.5, 1.6), 2: (0.8, 1.75, 0.6), 3: (1.8, 1.7, 0.6), 4: (5.0, 2.2, 1.9), 5: (0.8, 1.3, 0.8)}
# the compiler's report for gfx950: VGPR / LDS bytes per workgroup / waves per SIMD / scratch
RESOURCES = (("kitti_match_tp_kernel", 20, 0, 8, 0), ("kitti_thresholds_kernel", 24, 1304, 8, 0), ("kitti_match_counts_kernel", 28, 0, 8, 0),
             ("kitti_finalize_kernel", 34, 0, 8, 0))
RESOURCES_AOS = (("kitti_match_counts_kernel<true>", 70, 0, 7, 0), ("kitti_finalize_kernel<true>", 24, 0, 8, 0), ("kitti_box_params_kernel", 72, 0, 7, 0))


def _ry(a):
    c, s = np.cos(a), np.sin(a)
    z, o = np.zeros_like(a), np.ones_like(a)
    return np.stack([c, z, s, z, o, z, -s, z, c], -1).reshape(-1, 3, 3)


def _bbox(boxes):
    u, v = 620.0 + 700.0 * boxes[:, :, 0] / boxes[:, :, 2], 190.0 + 700.0 * boxes[:, :, 1] / boxes[:, :, 2]
    return np.stack([u.min(1), v.min(1), u.max(1) - u.min(1), v.max(1) - v.min(1)], 1)


def make_records(images=IMAGES, seed=0):
    rng = np.random.default_rng(seed)
    n = 7 * images
    img = np.repeat(np.arange(1, images + 1), 7)
    cat = rng.choice([1, 2, 3, 4, 5], n, p=[0.55, 0.2, 0.1, 0.1, 0.05])
    z = rng.uniform(6, 60, n)
    c = np.stack([rng.uniform(-0.45, 0.45, n) * z, rng.uniform(0.9, 1.3, n), z], 1)
    d = np.array([DIMS[k] for k in cat]) * rng.uniform(0.85, 1.15, (n, 3))
    yaw = rng.uniform(-np.pi, np.pi, n)
    b3 = boxgen.corners(c, d, _ry(yaw))
    b2 = _bbox(b3)
    trunc, vis = rng.choice([0.0, 0.0, 0.1, 0.2, 0.4, 0.6], n), rng.choice([1.0, 1.0, 0.8, 0.6, 0.3, 0.1], n)
    gts = [{"id": k + 1, "image_id": int(img[k]), "category_id": int(cat[k]), "category_name": NAMES[int(cat[k])], "bbox3D": b3[k].tolist(),
            "bbox": b2[k].tolist(), "valid3D": True, "ignore": False, "ignore2D": False, "ignore3D": False, "iscrowd": 0, "area": float(b2[k, 2] * b2[k, 3]),
            "depth": float(z[k]), "truncation": float(trunc[k]), "visibility": float(vis[k])} for k in range(n)]
    for i in range(1, images + 1):                         # one DontCare region per image
        x, y, w, h = rng.uniform(0, 1000), rng.uniform(100, 200), rng.uniform(60, 200), rng.uniform(40, 90)
        gts.append({"id": len(gts) + 1, "image_id": i, "category_id": 6, "category_name": "dontcare", "bbox": [x, y, w, h], "valid3D": False,
                    "bbox3D": np.full((8, 3), -1.0).tolist(), "ignore": True, "ignore2D": True, "ignore3D": True, "iscrowd": 0, "area": w * h,
                    "depth": 1.0, "truncation": -1.0, "visibility": -1.0})
    # detections: ~85 % of the objects found (jittered), each found one twice more often than not, plus clutter: about 20 per image
    dts = []
    found = np.nonzero(rng.uniform(size=n) < 0.85)[0]
    for rep in range(2):
        idx = found if rep == 0 else found[rng.uniform(size=len(found)) < 0.6]
        amount = rng.choice([0.02, 0.05, 0.1, 0.2, 0.35], len(idx))[:, None]
        c2 = c[idx] + rng.normal(size=(len(idx), 3)) * amount * d[idx] * np.array([1.0, 0.3, 1.0])
        d2 = d[idx] * rng.uniform(1 - amount, 1 + amount, (len(idx), 3))
        p3 = boxgen.corners(c2, d2, _ry(yaw[idx] + rng.normal(size=len(idx)) * amount[:, 0]))
        p2, sc = _bbox(p3), rng.uniform(0.05, 0.99, len(idx)) * (1.0 if rep == 0 else 0.6)
        dts += [{"image_id": int(img[g]), "category_id": int(min(cat[g], 3) if cat[g] < 4 else cat[g] - 3), "score": float(sc[k]), "bbox": p2[k].tolist(),
                 "bbox3D": p3[k].tolist(), "depth": float(c2[k, 2])} for k, g in enumerate(idx)]
    m = 10 * images
    zc = rng.uniform(6, 60, m)
    cc = np.stack([rng.uniform(-0.45, 0.45, m) * zc, np.full(m, 1.1), zc], 1)
    kc = rng.choice([1, 2, 3], m)
    q3 = boxgen.corners(cc, np.array([DIMS[k] for k in kc]) * rng.uniform(0.8, 1.2, (m, 3)), _ry(rng.uniform(-3, 3, m)))
    q2, sc = _bbox(q3), rng.uniform(0.05, 0.7, m)
    dts += [{"image_id": int(rng.integers(1, images + 1)), "category_id": int(kc[k]), "score": float(sc[k]), "bbox": q2[k].tolist(), "bbox3D": q3[k].tolist(),
             "depth": float(zc[k])} for k in range(m)]
    return gts, dts


def timed(call):
    call()
    torch.cuda.synchronize()
    out = []
    for _ in range(BLOCKS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main(argv):
    assert torch.cuda.is_available(), "needs the GPU"
    gts, dts = make_records()
    imgs, cats = list(range(1, IMAGES + 1)), [1, 2, 3, 4, 5]
    names = {k: v for k, v in NAMES.items()}
    gt_index = AnnotationIndex(gts, imgs, list(NAMES))
    ev = KittiEval(gt_index, dts, names=names)
    if "--once" in argv:
        ev.evaluate()
        return
    if "--aos" in argv:
        # the same evaluator without and with `aos`, one after the other in this run: the comparison is between these two figures
        t_off = timed(ev.evaluate)
        ev.params.aos = True
        t_on = timed(ev.evaluate)
        e = ev.eval
        lines = ["AOS (--aos), the same set and run: KittiEval.evaluate() without AOS median %.1f ms (min %.1f, max %.1f), with AOS median %.1f ms "
                 "(min %.1f, max %.1f); device events around each of %d calls after one warm-up call"
                 % (statistics.median(t_off), min(t_off), max(t_off), statistics.median(t_on), min(t_on), max(t_on), BLOCKS),
                 "AOS|R40 car easy / moderate / hard at the strict overlaps: %s (AP2D|R40: %s); ground-truth rows without a heading: %d"
                 % (", ".join("%.2f" % v for v in e["aos_r40"][0, :, 0, 0]), ", ".join("%.2f" % v for v in e["ap_r40"][0, :, 0, 0]), e["n_unoriented"]),
                 "gfx950 resources of the AOS kernels from the compiler's report (VGPR / LDS bytes per workgroup / waves per SIMD / scratch):"]
        lines += ["  %-32s %3d / %4d / %d / %d" % r for r in RESOURCES_AOS]
        text = "\n".join(lines) + "\n"
        print(text, end="")
        out = [a for a in argv if not a.startswith("--")]
        if out:
            with open(out[0], "a") as f:
                f.write(text)
        return
    t_kitti = timed(ev.evaluate)
    plain = [g for g in gts if g["category_id"] != 6]

    def omni():
        o = Omni3Deval(AnnotationIndex([dict(g) for g in plain], imgs, cats), AnnotationIndex([dict(d) for d in dts], imgs, cats), mode="3D")
        o.evaluate()
        o.accumulate()

    t_omni = timed(omni)
    e = ev.eval
    lines = ["KittiEval on a KITTI-val-sized synthetic set: %d images, %d ground-truth rows, %d DontCare regions, %d detections; %d slots "
             "(3 classes x 3 difficulties x 3 metrics x 2 overlap sets), K between %d and %d"
             % (IMAGES, ev.problem.sumG, int(ev.problem.dc_off[-1]), ev.problem.sumD, ev.problem.S, int(e["K"].min()), int(e["K"].max())),
             "KittiEval.evaluate(): median %.1f ms (device events around each of %d calls after one warm-up call; min %.1f, max %.1f)"
             % (statistics.median(t_kitti), BLOCKS, min(t_kitti), max(t_kitti)),
             "Omni3Deval(mode='3D') evaluate() + accumulate() on the same records (no DontCare rows): median %.1f ms (min %.1f, max %.1f)"
             % (statistics.median(t_omni), min(t_omni), max(t_omni)),
             "AP3D|R40 car easy / moderate / hard at the strict overlaps: %s" % ", ".join("%.2f" % v for v in e["ap_r40"][0, :, 2, 0]),
             "gfx950 resources from the compiler's report (VGPR / LDS bytes per workgroup / waves per SIMD / scratch):"]
    lines += ["  %-28s %3d / %4d / %d / %d" % r for r in RESOURCES]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = [a for a in argv if not a.startswith("--")]
    if out:
        with open(out[0], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main(sys.argv[1:])
