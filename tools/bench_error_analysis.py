"""Time of the error decomposition (`Omni3Deval.errors`, csrc/eval_errors.hip) against the evaluation it explains, run by hand on an
MI355X; not part of bench.py.  One synthetic split in mode 3D: 300 images x 10 categories, 8 ground truths and 40 detections per image
(good copies, duplicates, copies slid along the line of sight, copies filed under another category, boxes elsewhere).
 1. evaluate() + accumulate() of the split (host wall clock around a device synchronisation: both are host loops around a few launches);
 2. errors() on the evaluated split (the same clock): the image-level similarity pass, omni_eval_error_types, nine omni_eval_accumulate
    calls with T = A = M = 1, one omni_pair_errors;
 3. omni_eval_error_types alone on the tensors errors() hands it (device events around 20 calls).
Alternating blocks in one process, median of five, after one warm-up of each; the clocks the device reported right after the loops are
noted.  Nobody has set a speed bar: the file says what the analysis costs next to the evaluation.
    python tools/bench_error_analysis.py [output file]"""
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from omni3d_amd import boxgen  # noqa: E402
from omni3d_amd.cubercnn.evaluation import omni3d_evaluation as E  # noqa: E402
from omni3d_amd.kernels import errtypes  # noqa: E402

IMAGES, CATS, GT_PER_IMAGE, BLOCKS, CALLS = 300, 10, 8, 5, 20


def split(rng):
    gts, dts = [], []

    def rec(img, cat, c, d, R, score=None):
        box = boxgen.corners(np.asarray(c)[None], np.asarray(d)[None], R[None])[0].astype(np.float32)
        r = {"image_id": img, "category_id": cat, "bbox3D": box.tolist(), "depth": float(box[:, 2].mean()), "bbox": [0.0, 0.0, 10.0, 10.0], "area": 100.0}
        if score is None:
            r.update(ignore3D=int(rng.uniform() < 0.1), ignore2D=0, iscrowd=0)
            gts.append(r)
        else:
            r["score"] = float(score)
            dts.append(r)

    for img in range(1, IMAGES + 1):
        for _ in range(GT_PER_IMAGE):
            cat = int(rng.integers(1, CATS + 1))
            c = np.array([rng.uniform(-8, 8), rng.uniform(-2, 2), rng.uniform(3, 60)])
            d, R = rng.uniform(0.6, 4.0, 3), boxgen.rand_rot(rng, 1)[0]
            rec(img, cat, c, d, R)
            for kind in rng.choice(5, size=int(rng.integers(3, 8))):      # 0 / 1 good copy, 2 slid, 3 other category, 4 elsewhere
                c2 = c + R @ (rng.normal(0, 0.08, 3) * d)
                if kind == 2:
                    c2 = c2 + rng.uniform(0.45, 0.8) * d.min() * c / np.linalg.norm(c)
                if kind == 4:
                    c2 = np.array([rng.uniform(-8, 8), rng.uniform(-2, 2), rng.uniform(3, 60)])
                rec(img, cat if kind != 3 else 1 + cat % CATS, c2, d * rng.uniform(0.9, 1.1, 3), boxgen.rand_rot(rng, 1)[0] if kind == 4 else R,
                    score=rng.uniform(0.05, 0.99))
    for k, r in enumerate(gts + dts):
        r["id"] = k + 1
    return gts, dts


def clocks():
    """the sclk / mclk lines of `rocm-smi --showclocks` (read only), or a note that they could not be read"""
    try:
        text = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        rows = [" ".join(ln.split()) for ln in text.splitlines() if "sclk" in ln or "mclk" in ln]
        return "; ".join(rows[:2]) if rows else "clocks not reported"
    except Exception as exc:      # noqa: BLE001
        return "clocks not read (%s)" % type(exc).__name__


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def main(out=None):
    assert torch.cuda.is_available(), "needs the GPU"
    gts, dts = split(np.random.default_rng(0))
    imgs, cats = list(range(1, IMAGES + 1)), list(range(1, CATS + 1))
    ev = E.Omni3Deval(E.AnnotationIndex(gts, imgs, cats), E.AnnotationIndex(dts, imgs, cats), mode="3D")

    def evaluation():
        ev.evaluate()
        ev.accumulate()

    seen = {}
    launch = errtypes.error_types

    def spy(*args):
        seen["args"] = args
        return launch(*args)

    evaluation()
    errtypes.error_types = spy                    # the tensors errors() hands the kernel, for (3)
    try:
        res = ev.errors()
    finally:
        errtypes.error_types = launch
    t_eval, t_err, t_kernel = [], [], []
    for _ in range(BLOCKS):                        # alternating: all see the same clocks and neighbours
        t_eval.append(wall(evaluation)[0])
        t_err.append(wall(ev.errors)[0])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            launch(*seen["args"])
        e1.record()
        torch.cuda.synchronize()
        t_kernel.append(1e3 * e0.elapsed_time(e1) / CALLS)
    during = clocks()
    fmt = lambda t, unit: "median %.1f %s (min %.1f, max %.1f)" % (statistics.median(t), unit, min(t), max(t))      # noqa: E731
    lines = ["csrc/eval_errors.hip -- mode 3D, %d images x %d categories, %d ground truths, %d detections; types %s, missed %d"
             % (IMAGES, CATS, len(gts), len(dts), dict(zip(E.ERROR_TYPES[:5], res["counts_total"][:5].tolist())), int(res["counts_total"][5])),
             "evaluate() + accumulate(): %s per call, host clock" % fmt(t_eval, "ms"),
             "errors(): %s per call, host clock = %.2f x the evaluation" % (fmt(t_err, "ms"), statistics.median(t_err) / statistics.median(t_eval)),
             "omni_eval_error_types alone (launcher with its argument checks): %s per call, device events around %d calls" % (fmt(t_kernel, "us"), CALLS),
             "%d alternating blocks in one process after one warm-up of each; clocks right after the loops: %s" % (BLOCKS, during)]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
