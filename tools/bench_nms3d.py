"""Times of the duplicate-cuboid suppression (csrc/nms3d.hip, omni_nms3d), run by hand on an MI355X; not part of bench.py.
 1. omni_nms3d alone (its two launches, outputs allocated once) between device events at B = 4, S = 100: with clustered boxes (60 of
    the 100 slots of every image jittered around 4 centres: ~400 overlapping pairs per image go through the pair algorithm) and with
    sparse boxes (almost every pair ends at the bounding-sphere screen).
 2. the replayed inference pass of bench.py's inference workload (cubercnn_DLA34_FPN, 4 x 512 x 512, random-init weights, ~100
    detections per image) with the feature off and on (TEST.NMS_3D.IOU_THRESH 0.25, class-agnostic), alternating blocks of passes on
    ONE model, host clock around each block with a device synchronisation at both ends; the median block of each setting is reported
    and the figure that matters is their ratio in the same run.
Information only: no speed bar is set.
    python tools/bench_nms3d.py [output file]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from omni3d_amd import boxgen, lib  # noqa: E402

B, S, THR = 4, 100, 0.25


def boxes(clustered, seed=0):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-22.0, 22.0, size=(B * S, 3)) + np.array([0.0, 0.0, 30.0])
    d = rng.uniform(0.5, 2.0, size=(B * S, 3))
    R = boxgen.rand_rot(rng, B * S)
    if clustered:
        for b in range(B):
            o = b * S
            src = o + np.arange(60) % 4
            c[o:o + 60] = c[src] + rng.normal(scale=0.15, size=(60, 3)) * d[src]
            d[o:o + 60] = d[src] * rng.uniform(0.85, 1.15, size=(60, 3))
            R[o:o + 60] = R[src]
    return boxgen.corners(c, d, R), rng.uniform(0.05, 0.98, B * S).astype(np.float32), rng.integers(5, size=B * S).astype(np.int32)


def time_kernels(clustered, reps=200):
    verts, score, cls = (torch.from_numpy(a).cuda() for a in boxes(clustered))
    count = torch.full((B,), S, dtype=torch.int32, device="cuda")
    iou = torch.empty((B, S, S), dtype=torch.float32, device="cuda")
    keep, order = torch.empty((B, S), dtype=torch.int32, device="cuda"), torch.empty((B, S), dtype=torch.int32, device="cuda")
    new_count, overflow = torch.empty(B, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    L, st = lib.get(), lib.stream_of(verts)

    def call():
        L.call("omni_nms3d", verts.data_ptr(), score.data_ptr(), cls.data_ptr(), count.data_ptr(), B, S, THR, 1, 1e-4, 1e-8, iou.data_ptr(),
               keep.data_ptr(), order.data_ptr(), new_count.data_ptr(), overflow.data_ptr(), st)
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps, int((iou > THR).sum()) // 2, new_count.tolist(), int(overflow)


def time_passes(blocks=6, per_block=20):
    from omni3d_amd import bench_train as BT
    _, model, _, priors = BT.build(1)
    batch, _ = BT.stage_batch(model, priors, 0)
    model.eval()
    heads, times, kept = model.roi_heads, {None: [], THR: []}, {}
    with torch.no_grad():
        for thr in (None, THR):                      # per setting: the eager pass of the bucket, the capture, replays
            heads.nms3d_thresh = thr
            for _ in range(4):
                out = model(batch)
            kept[thr] = [len(o["instances"]) for o in out]
        for _ in range(blocks):
            for thr in (None, THR):
                heads.nms3d_thresh = thr
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(per_block):
                    model(batch)
                torch.cuda.synchronize()
                times[thr].append(1e3 * (time.perf_counter() - t0) / per_block)
    heads.nms3d_thresh = None
    rep = model.__dict__.get("_omni_infer")
    return times, kept, (rep.captures, rep.replays, rep.failed) if rep is not None else None


def main(out=None):
    assert torch.cuda.is_available(), "needs the GPU"
    lines = ["csrc/nms3d.hip omni_nms3d -- B = %d images, S = %d slots, threshold %.2f, class-agnostic" % (B, S, THR)]
    for clustered in (True, False):
        us, pairs, counts, over = time_kernels(clustered)
        lines.append("omni_nms3d alone, %s boxes: %.1f us per call (two launches; device events, 200 calls); %d pairs above the threshold, "
                     "kept per image %s, overflow %d" % ("clustered" if clustered else "sparse", us, pairs, counts, over))
    times, kept, rep = time_passes()
    off, on = statistics.median(times[None]), statistics.median(times[THR])
    lines.append("replayed inference pass, cubercnn_DLA34_FPN 4 x 512 x 512 (bench.py --workload infer), host clock, median of %d alternating "
                 "blocks of 20 passes:" % len(times[None]))
    lines.append("    feature off: %.3f ms per pass (blocks %s), detections per image %s" % (off, " ".join("%.3f" % t for t in times[None]), kept[None]))
    lines.append("    feature on : %.3f ms per pass (blocks %s), detections per image %s" % (on, " ".join("%.3f" % t for t in times[THR]), kept[THR]))
    lines.append("    on / off = %.4f (+%.1f us per pass); captures, replays, failure: %s" % (on / off, 1e3 * (on - off), rep))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
