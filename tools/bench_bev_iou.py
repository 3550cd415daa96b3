"""Time of the bird's-eye-view IoU (csrc/bev_iou.hip), run by hand on an MI355X; not part of bench.py.
100 000 Omni3D-like pairs (`boxgen.omni3d_like_pairs`: half of the second boxes are jittered copies of the first, so half of the
pairs go through the clipping) through `omni_bev_iou_pairs`, footprints taken once beforehand, outputs allocated once; device events
around 2000 calls after 20 warm-up calls, repeated 5 times, the median reported with the spread, next to the two footprint launches
timed the same way and the clocks the device reported during the run.
Information only: there is no earlier figure and no speed bar.
    python tools/bench_bev_iou.py [output file]"""
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from omni3d_amd import boxgen, lib  # noqa: E402
from omni3d_amd.kernels import bev  # noqa: E402

PAIRS, WARMUP, CALLS, REPEATS = 100_000, 20, 2000, 5


def timed(call):
    for _ in range(WARMUP):
        call()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            call()
        e1.record()
        torch.cuda.synchronize()
        out.append(1e3 * e0.elapsed_time(e1) / CALLS)
    return out


def clocks():
    """the sclk / mclk lines of `rocm-smi --showclocks` (read only), or a note that they could not be read"""
    try:
        text = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        rows = [" ".join(ln.split()) for ln in text.splitlines() if "sclk" in ln or "mclk" in ln]
        return "; ".join(rows[:2]) if rows else "clocks not reported"
    except Exception as exc:      # noqa: BLE001
        return "clocks not read (%s)" % type(exc).__name__


def main(out=None):
    assert torch.cuda.is_available(), "needs the GPU"
    dt, gt, _ = boxgen.omni3d_like_pairs(np.random.default_rng(0), PAIRS)
    dt, gt = torch.from_numpy(dt).cuda(), torch.from_numpy(gt).cuda()
    fp1, fp2 = bev.bev_footprints(dt), bev.bev_footprints(gt)
    idx = torch.arange(PAIRS, dtype=torch.int32, device="cuda")
    iou = torch.empty(PAIRS, dtype=torch.float32, device="cuda")
    L, st = lib.get(), lib.stream_of(dt)
    e1, e2 = bev.plane_basis()

    def pairs():
        L.call("omni_bev_iou_pairs", *[t.data_ptr() for t in fp1], PAIRS, *[t.data_ptr() for t in fp2], PAIRS, idx.data_ptr(), idx.data_ptr(),
               PAIRS, iou.data_ptr(), st)

    def footprints():
        for boxes, fp in ((dt, fp1), (gt, fp2)):
            L.call("omni_bev_footprint", boxes.data_ptr(), PAIRS, *map(float, e1), *map(float, e2), 1e-8, *[t.data_ptr() for t in fp], None, st)

    t_pairs, t_foot = timed(pairs), timed(footprints)
    during = clocks()
    med = statistics.median(t_pairs)
    lines = ["csrc/bev_iou.hip -- %d Omni3D-like pairs, %d with overlapping footprints, mean IoU of those %.3f"
             % (PAIRS, int((iou > 0).sum()), float(iou[iou > 0].mean())),
             "omni_bev_iou_pairs: median %.1f us per call (%d x %d calls between device events after %d warm-up calls; min %.1f, max %.1f) "
             "= %.2f G pairs/s" % (med, REPEATS, CALLS, WARMUP, min(t_pairs), max(t_pairs), PAIRS / med / 1e3),
             "omni_bev_footprint, both sets (2 x %d boxes, two launches): median %.1f us (min %.1f, max %.1f)"
             % (PAIRS, statistics.median(t_foot), min(t_foot), max(t_foot)),
             "clocks right after the timed loops: %s" % during]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
