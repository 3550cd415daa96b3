"""Times of the exact IoU3D (csrc/cuboid_exact.h, csrc/iou3d_exact.hip, omni_nms3d_exact) next to the evaluator's pair algorithm it
stands beside, run by hand on an MI355X; not part of bench.py.  Everything between device events, outputs allocated once, the median
of repeated blocks reported with the spread.
 1. omni_iou3d_exact_pairs (fits taken once beforehand, and timed on their own) against omni_iou_box3d_pairs on the same 100 000
    `boxgen.omni3d_like_pairs`.
 2. omni_nms3d_exact against omni_nms3d on the clustered and the sparse scene of tools/bench_nms3d.py at B = 4, S = 100.
 3. the replayed inference pass of bench.py's inference workload with TEST.NMS_3D on, deciding by either type: alternating blocks of
    passes on ONE model, host clock around each block with a device synchronisation at both ends.
Information only: nobody measured a double-precision kernel of this shape on this device before, so no speed bar is set; the
partners above are what the numbers are read against.
    python tools/bench_iou3d_exact.py [output file]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench_nms3d  # noqa: E402
from bench_bev_iou import clocks  # noqa: E402
from omni3d_amd import boxgen, lib  # noqa: E402
from omni3d_amd.kernels import iou3d  # noqa: E402

PAIRS, WARMUP, CALLS, REPEATS = 100_000, 5, 40, 5
B, S, THR = bench_nms3d.B, bench_nms3d.S, bench_nms3d.THR


def timed(call, calls=CALLS):
    for _ in range(WARMUP):
        call()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            call()
        e1.record()
        torch.cuda.synchronize()
        out.append(1e3 * e0.elapsed_time(e1) / calls)
    return out


def fmt(t):
    return "median %.1f us (min %.1f, max %.1f)" % (statistics.median(t), min(t), max(t))


def time_pairs(lines):
    dt, gt, _ = boxgen.omni3d_like_pairs(np.random.default_rng(0), PAIRS)
    dt, gt = torch.from_numpy(dt).cuda(), torch.from_numpy(gt).cuda()
    fit1, fit2 = iou3d.cuboid_fit(dt), iou3d.cuboid_fit(gt)
    idx = torch.arange(PAIRS, dtype=torch.int32, device="cuda")
    vol, iou, ref = (torch.empty(PAIRS, dtype=torch.float32, device="cuda") for _ in range(3))
    overflow = torch.zeros(1, dtype=torch.int32, device="cuda")
    valid = iou3d.box3d_validity(dt)[0]                 # the evaluator's mask of degenerate detections, as box3d_overlap passes it
    L, st = lib.get(), lib.stream_of(dt)

    def exact():
        L.call("omni_iou3d_exact_pairs", *[t.data_ptr() for t in fit1], PAIRS, *[t.data_ptr() for t in fit2], PAIRS, idx.data_ptr(),
               idx.data_ptr(), PAIRS, vol.data_ptr(), iou.data_ptr(), st)

    def fits():
        for boxes, fit in ((dt, fit1), (gt, fit2)):
            L.call("omni_cuboid_fit", boxes.data_ptr(), PAIRS, 1e-8, 1e-3, *[t.data_ptr() for t in fit], None, st)

    def evaluator():
        L.call("omni_iou_box3d_pairs", dt.data_ptr(), gt.data_ptr(), idx.data_ptr(), idx.data_ptr(), PAIRS, valid.data_ptr(), None, ref.data_ptr(),
               overflow.data_ptr(), st)

    t_exact, t_fit, t_eval = timed(exact), timed(fits), timed(evaluator)
    both = (iou > 0) | (ref > 0)
    lines += ["%d Omni3D-like pairs, %d overlapping; |exact - evaluator's algorithm| on them: max %.3f, %d above 1e-2"
              % (PAIRS, int((iou > 0).sum()), float((iou - ref).abs().max()), int(((iou - ref).abs()[both] > 1e-2).sum())),
              "omni_iou3d_exact_pairs: %s per call = %.1f M pairs/s" % (fmt(t_exact), PAIRS / statistics.median(t_exact)),
              "omni_cuboid_fit, both sets (2 x %d boxes, two launches): %s" % (PAIRS, fmt(t_fit)),
              "omni_iou_box3d_pairs on the same pairs: %s per call = %.1f M pairs/s; exact / evaluator = %.2f"
              % (fmt(t_eval), PAIRS / statistics.median(t_eval), statistics.median(t_exact) / statistics.median(t_eval)),
              "clocks right after the timed loops: %s" % clocks()]


def time_nms(lines):
    for clustered in (True, False):
        verts, score, cls = (torch.from_numpy(a).cuda() for a in bench_nms3d.boxes(clustered))
        count = torch.full((B,), S, dtype=torch.int32, device="cuda")
        iou = torch.empty((B, S, S), dtype=torch.float32, device="cuda")
        keep, order = torch.empty((B, S), dtype=torch.int32, device="cuda"), torch.empty((B, S), dtype=torch.int32, device="cuda")
        new_count, extra = torch.empty(B, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        L, st = lib.get(), lib.stream_of(verts)
        res = {}
        for name in ("omni_nms3d_exact", "omni_nms3d"):
            def call():
                L.call(name, verts.data_ptr(), score.data_ptr(), cls.data_ptr(), count.data_ptr(), B, S, THR, 1, 1e-4, 1e-8, iou.data_ptr(),
                       keep.data_ptr(), order.data_ptr(), new_count.data_ptr(), extra.data_ptr(), st)
            extra.zero_()
            t = timed(call, 100)
            res[name] = statistics.median(t)
            lines.append("%s, %s boxes, B = %d, S = %d: %s per call (two launches); %d pairs above the threshold, kept per image %s"
                         % (name, "clustered" if clustered else "sparse", B, S, fmt(t), int((iou > THR).sum()) // 2, new_count.tolist()))
        lines.append("    exact / evaluator = %.2f" % (res["omni_nms3d_exact"] / res["omni_nms3d"]))


def time_passes(lines, blocks=6, per_block=20):
    from omni3d_amd import bench_train as BT
    _, model, _, priors = BT.build(1)
    batch, _ = BT.stage_batch(model, priors, 0)
    model.eval()
    heads, kinds = model.roi_heads, ("evaluator", "exact")
    times, kept = {k: [] for k in kinds}, {}
    heads.nms3d_thresh = THR
    with torch.no_grad():
        for kind in kinds:                               # per type: the eager pass of the bucket, the capture, replays
            heads.nms3d_iou_type = kind
            for _ in range(4):
                out = model(batch)
            kept[kind] = [len(o["instances"]) for o in out]
        for _ in range(blocks):
            for kind in kinds:
                heads.nms3d_iou_type = kind
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(per_block):
                    model(batch)
                torch.cuda.synchronize()
                times[kind].append(1e3 * (time.perf_counter() - t0) / per_block)
    heads.nms3d_thresh, heads.nms3d_iou_type = None, "evaluator"
    rep = model.__dict__.get("_omni_infer")
    a, b = statistics.median(times["evaluator"]), statistics.median(times["exact"])
    lines.append("replayed inference pass, cubercnn_DLA34_FPN 4 x 512 x 512 (bench.py --workload infer), TEST.NMS_3D at %.2f, host clock, "
                 "median of %d alternating blocks of %d passes:" % (THR, blocks, per_block))
    for kind in kinds:
        lines.append("    IOU_TYPE %-9s: %.3f ms per pass (blocks %s), detections per image %s"
                     % (kind, statistics.median(times[kind]), " ".join("%.3f" % t for t in times[kind]), kept[kind]))
    lines.append("    exact / evaluator = %.4f (%+.1f us per pass); captures, replays, failure: %s"
                 % (b / a, 1e3 * (b - a), (rep.captures, rep.replays, rep.failed) if rep is not None else None))


def main(out=None):
    assert torch.cuda.is_available(), "needs the GPU"
    lines = ["csrc/cuboid_exact.h -- exact IoU3D in double, one thread per pair"]
    time_pairs(lines)
    time_nms(lines)
    time_passes(lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
