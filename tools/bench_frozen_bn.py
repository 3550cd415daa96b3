#!/usr/bin/env python
"""ms per training step with every BatchNorm frozen (freeze_bn after .train(): MODEL.USE_BN False) against the default step
(BatchNorm in training mode) on the benchmarked shape -- DLA-34, 4 x 512 x 512, one GPU -- both as the staged hipGraph step that
bench.py times (cubercnn/solver/graphed.py GraphedPipelined) followed by the eager SGD update.  Each mode builds its own model from
the same seed; the two modes alternate over --rounds timed windows so that clock drift hits both.

    python tools/bench_frozen_bn.py [--steps 20] [--warmup 5] [--rounds 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def make(frozen):
    from omni3d_amd import bench_train as BT
    from omni3d_amd.cubercnn.solver.build import freeze_bn
    from omni3d_amd.cubercnn.solver.graphed import GraphedPipelined
    cfg, model, opt, priors = BT.build(1)
    if frozen:
        freeze_bn(model)
    batch, packed = BT.stage_batch(model, priors, 0)
    graphed = GraphedPipelined(model, opt, batch, packed, graphs=True)

    def step():
        losses, total, pending = graphed()
        opt.all_reduce_finish(pending, defer_scale=True)
        opt.step()
    return step, opt


def timed(step, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    modes = {"default": make(False), "frozen_bn": make(True)}
    for step, _ in modes.values():
        for _ in range(args.warmup):
            step()
    ms = {k: [] for k in modes}
    for _ in range(args.rounds):
        for k, (step, _) in modes.items():
            ms[k].append(round(timed(step, args.steps), 3))
    out = {"shape": "dla34 4x512x512", "steps": args.steps, "rounds": args.rounds, "ms_per_step": ms,
           "median_ms": {k: sorted(v)[len(v) // 2] for k, v in ms.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
