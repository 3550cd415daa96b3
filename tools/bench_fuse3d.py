"""Times of the cuboid fusion of test-time augmentation (csrc/nms3d.hip, omni_fuse3d), run by hand on an MI355X; not part of bench.py.
 1. omni_fuse3d alone (its two launches, outputs allocated once, A = 54 aux columns as the wrapper passes for 50 classes) between
    device events at B = 4, S = 200 -- two views of 100 slots -- next to omni_nms3d_exact on the same slots as the yardstick (they
    share launch 1): clustered (the second view's 100 cuboids are jittered copies of the first view's, so nearly every cuboid has a
    partner) and sparse (200 unrelated cuboids, almost every pair ends at the bounding-sphere test).
 2. images/s of bench.py's inference workload (cubercnn_DLA34_FPN, 4 x 512 x 512, random-init weights) through the model alone (one
    view) and through RCNN3DWithTTA with the defaults of TEST.AUG (the image and its mirror image): alternating blocks of passes on
    ONE model, host clock around each block with a device synchronisation at both ends, the median block of each.
Information only: no speed bar is set, and nothing here says anything about accuracy.
    python tools/bench_fuse3d.py [output file]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from omni3d_amd import boxgen, lib  # noqa: E402

B, PER_VIEW, VIEWS, A, THR = 4, 100, 2, 54, 0.5
S = PER_VIEW * VIEWS


def boxes(clustered, seed=0):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-22.0, 22.0, size=(B, S, 3)) + np.array([0.0, 0.0, 30.0])
    d = rng.uniform(0.5, 2.0, size=(B, S, 3))
    R = boxgen.rand_rot(rng, B * S).reshape(B, S, 3, 3)
    if clustered:                                        # the second view sees the first view's cuboids again, a little off
        c[:, PER_VIEW:] = c[:, :PER_VIEW] + rng.normal(scale=0.05, size=(B, PER_VIEW, 3)) * d[:, :PER_VIEW]
        d[:, PER_VIEW:] = d[:, :PER_VIEW] * rng.uniform(0.95, 1.05, size=(B, PER_VIEW, 3))
        R[:, PER_VIEW:] = R[:, :PER_VIEW]
    return (boxgen.corners(c.reshape(-1, 3), d.reshape(-1, 3), R.reshape(-1, 3, 3)), rng.uniform(0.05, 0.98, B * S).astype(np.float32),
            np.tile(rng.integers(5, size=(B, PER_VIEW)), (1, VIEWS)).reshape(-1).astype(np.int32), rng.uniform(0, 500, size=(B * S, A)).astype(np.float32))


def _timed(call, reps=200):
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def time_kernels(clustered):
    verts, score, cls, aux = (torch.from_numpy(a).cuda() for a in boxes(clustered))
    count = torch.full((B,), S, dtype=torch.int32, device="cuda")
    new = lambda shape, dt=torch.float32: torch.empty(shape, dtype=dt, device="cuda")          # noqa: E731
    i32 = torch.int32
    iou, cluster, bad = new((B, S, S)), new((B, S), i32), torch.zeros(1, dtype=i32, device="cuda")
    o = [new((B * S, 8, 3)), new((B * S, 3)), new((B * S, 3, 3)), new((B * S, 3)), new((B * S,)), new((B * S,), i32), new((B * S, A)),
         new((B * S,), i32), new((B * S,), i32), new((B,), i32)]
    keep, order, new_count = new((B, S), i32), new((B, S), i32), new((B,), i32)
    L, st = lib.get(), lib.stream_of(verts)
    ins = (verts.data_ptr(), score.data_ptr(), cls.data_ptr(), count.data_ptr())

    def fuse():
        L.call("omni_fuse3d", *ins, aux.data_ptr(), B, S, A, VIEWS, THR, 0, 1e-4, 1e-8, iou.data_ptr(), cluster.data_ptr(), *[t.data_ptr() for t in o],
               bad.data_ptr(), st)

    def nms():
        L.call("omni_nms3d_exact", *ins, B, S, THR, 0, 1e-4, 1e-8, iou.data_ptr(), keep.data_ptr(), order.data_ptr(), new_count.data_ptr(), bad.data_ptr(), st)
    t_fuse, t_nms = _timed(fuse), _timed(nms)
    return t_fuse, t_nms, o[9].tolist(), new_count.tolist(), int((o[7] > 1).sum())


def time_passes(blocks=6, per_block=20):
    from omni3d_amd import bench_train as BT
    from omni3d_amd.cubercnn.config import add_tta_config
    from omni3d_amd.cubercnn.modeling.meta_arch.tta import RCNN3DWithTTA
    cfg, model, _, priors = BT.build(1)
    batch, _ = BT.stage_batch(model, priors, 0)
    model.eval()
    add_tta_config(cfg)
    cfg.merge_from_list(["TEST.AUG.ENABLED", True])
    runners = {"one view": model, "two views": RCNN3DWithTTA(cfg, model).eval()}
    times, kept = {k: [] for k in runners}, {}
    with torch.no_grad():
        for name, run in runners.items():                # the eager pass of every bucket, the captures, replays
            for _ in range(4):
                out = run(batch)
            kept[name] = [len(o["instances"]) for o in out]
        for _ in range(blocks):
            for name, run in runners.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(per_block):
                    run(batch)
                torch.cuda.synchronize()
                times[name].append(1e3 * (time.perf_counter() - t0) / per_block)
    rep = model.__dict__.get("_omni_infer")
    return times, kept, len(batch), (rep.captures, rep.replays, rep.failed) if rep is not None else None


def main(out=None):
    assert torch.cuda.is_available(), "needs the GPU"
    lines = ["csrc/nms3d.hip omni_fuse3d -- B = %d images, S = %d slots (%d views of %d), A = %d aux columns, threshold %.2f, class-specific"
             % (B, S, VIEWS, PER_VIEW, A, THR)]
    for clustered in (True, False):
        t_fuse, t_nms, clusters, kept, merged = time_kernels(clustered)
        lines.append("%s cuboids: omni_fuse3d %.1f us per call, omni_nms3d_exact %.1f us per call (two launches each; device events, 200 calls); "
                     "clusters per image %s (%d of more than one member), kept by the suppression %s"
                     % ("clustered" if clustered else "sparse", t_fuse, t_nms, clusters, merged, kept))
    times, kept, n, rep = time_passes()
    lines.append("inference, cubercnn_DLA34_FPN %d x 512 x 512 (bench.py --workload infer), host clock, median of %d alternating blocks of 20 passes:"
                 % (n, len(times["one view"])))
    for name, ts in times.items():
        ms = statistics.median(ts)
        lines.append("    %-9s: %.3f ms per pass = %.1f images/s (blocks %s), detections per image %s"
                     % (name, ms, 1e3 * n / ms, " ".join("%.3f" % t for t in ts), kept[name]))
    lines.append("    captures, replays, failure of the replayed passes: %s" % (rep,))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
