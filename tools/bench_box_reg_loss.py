"""Forward + backward times of the box regression losses of both detector stages (csrc/box_reg_loss.h behind omni_box_reg_loss_* and
omni_rpn_reg_loss_*) beside the L1 entry points of the default configuration, at the shapes of bench.py's training step, run by hand
on an MI355X; not part of bench.py.
  box head: R = 2048 sampled ROIs (a quarter foreground), K = 50, ldp = 256
  RPN:      B = 4 images, A = 65 472 anchors (levels 128^2 .. 8^2, 3 anchors each), 256 sampled anchors per image, half positive
Each variant's pair of launches (forward with its memset of the sums, backward) is captured 20 times into one graph on buffers
allocated once, so the host's launch cost is not in the figure; device events around 20 replays after 3 warm-up replays.  One JSON line
per variant: microseconds per forward + backward, and its ratio to the L1 pair of the same stage in the same run.
    python tools/bench_box_reg_loss.py [output file]"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from omni3d_amd import lib  # noqa: E402
from omni3d_amd.kernels import det  # noqa: E402

VARIANTS = [("smooth_l1", 0.0), ("smooth_l1", 0.5), ("giou", 0.0), ("diou", 0.0), ("ciou", 0.0)]     # beta 0: the L1 entry points
PAIRS, REPLAYS, WARM = 20, 20, 3


def time_pair(call):
    """call(): enqueue one forward + backward on the current stream -> microseconds per pair"""
    call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(PAIRS):
            call()
    for _ in range(WARM):
        graph.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPLAYS):
        graph.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / (REPLAYS * PAIRS) * 1e3


def jitter(box, g, shift=0.2, scale=0.3):
    w, h = box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]
    u = torch.rand(box.shape[0], 4, generator=g) - 0.5
    cx, cy = (box[:, 0] + box[:, 2]) / 2 + u[:, 0] * 2 * shift * w, (box[:, 1] + box[:, 3]) / 2 + u[:, 1] * 2 * shift * h
    w, h = w * torch.exp(u[:, 2] * 2 * scale), h * torch.exp(u[:, 3] * 2 * scale)
    return torch.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], dim=1)


def box_head_calls(g, R=2048, K=50, G=40):
    ldp = (5 * K + 1 + 15) // 16 * 16
    pred = torch.randn(R, ldp, generator=g) * 0.5
    xy = torch.rand(G, 2, generator=g) * 400
    gt = torch.cat([xy, xy + 20 + torch.rand(G, 2, generator=g) * 100], dim=1)
    gt_row = torch.randint(0, G, (R,), generator=g)
    prop = jitter(gt[gt_row], g)
    cls = torch.where(torch.arange(R) % 4 == 0, torch.randint(0, K, (R,), generator=g), torch.full((R,), K))
    pred, gt, prop, cls, gt_row = pred.cuda(), gt.cuda(), prop.cuda(), cls.int().cuda(), gt_row.int().cuda()
    sums, dpred = torch.zeros(7, dtype=torch.float64).cuda(), torch.empty_like(pred)
    one = torch.ones(1).cuda()
    L = lib.get()
    head = (pred.data_ptr(), ldp, R, K, cls.data_ptr(), prop.data_ptr(), gt.data_ptr(), gt_row.data_ptr(), 10.0, 10.0, 5.0, 5.0)

    def make(kind, beta):
        reg = det.box_reg_args(kind, beta, det.SCALE_CLAMP)
        name, extra = ("omni_box_loss", ()) if reg is None else ("omni_box_reg_loss", reg)

        def call():
            st = lib.stream_of(pred)
            L.call(name + "_fwd", *head, *extra, sums.data_ptr(), st)
            L.call(name + "_bwd", *head, *extra, sums.data_ptr(), one.data_ptr(), one.data_ptr(), dpred.data_ptr(), st)
        return call
    make.keep = (pred, cls, prop, gt, gt_row)          # `head` holds raw pointers
    return make


def rpn_calls(g, plain, B=4, sampled=256):
    hw = [(128, 128), (64, 64), (32, 32), (16, 16), (8, 8)]
    anchors = []
    for (h, w), stride, size in zip(hw, (4, 8, 16, 32, 64), (32, 64, 128, 256, 512)):
        cy, cx = torch.meshgrid(torch.arange(h, dtype=torch.float32) * stride, torch.arange(w, dtype=torch.float32) * stride, indexing="ij")
        per = []
        for r in (0.5, 1.0, 2.0):
            aw, ah = size / r ** 0.5, size * r ** 0.5
            per.append(torch.stack([cx - aw / 2, cy - ah / 2, cx + aw / 2, cy + ah / 2], dim=-1))
        anchors.append(torch.stack(per, dim=2).reshape(-1, 4))
    anchors = torch.cat(anchors)
    A = anchors.shape[0]
    levels = [(torch.randn(B, h, w, 16, generator=g) * 0.5).cuda() for h, w in hw]
    grads = [torch.empty_like(t) for t in levels]
    labels = torch.full((B, A), -1, dtype=torch.int8)
    midx = torch.zeros(B, A, dtype=torch.int32)
    gts = []
    for n in range(B):
        perm = torch.randperm(A, generator=g)[:sampled]
        pos = perm[:sampled // 2]
        labels[n, pos], labels[n, perm[sampled // 2:]] = 1, 0
        midx[n, pos] = torch.arange(pos.shape[0], dtype=torch.int32)
        gts.append(jitter(anchors[pos], g))
    gt_off = torch.arange(B + 1, dtype=torch.int32) * (sampled // 2)
    anchors, labels, midx, gt, gt_off = anchors.cuda(), labels.cuda(), midx.cuda(), torch.cat(gts).cuda(), gt_off.cuda()
    pack, dpack = det.LevelPack(levels), det.LevelPack(grads)
    sums, one = torch.zeros(6, dtype=torch.float64).cuda(), torch.ones(1).cuda()
    L = lib.get()
    a, da = pack.args(), dpack.args()
    tail = (B, anchors.data_ptr(), labels.data_ptr(), midx.data_ptr(), gt.data_ptr(), gt_off.data_ptr())

    def make(kind, beta):
        reg = det.box_reg_args(kind, beta, det.SCALE_CLAMP)
        name, extra = ("omni_rpn_loss_plain" if plain else "omni_rpn_loss", ()) if reg is None else ("omni_rpn_reg_loss", (int(plain),) + reg)

        def call():
            st = lib.stream_of(anchors)
            L.call(name + "_fwd", *a, *tail, *extra, sums.data_ptr(), st)
            L.call(name + "_bwd", a[0], da[0], a[1], a[2], *tail, *extra, one.data_ptr(), one.data_ptr(), 1.0 / (sampled * B), st)
        return call
    make.keep = (pack, dpack, levels, grads, anchors, labels, midx, gt, gt_off)          # `a`, `da`, `tail` hold raw pointers
    return make


def main(out=None):
    assert torch.cuda.is_available(), "needs the GPU"
    g = torch.Generator().manual_seed(0)
    lines = []
    stages = [("box_head", box_head_calls(g), VARIANTS), ("rpn_none", rpn_calls(g, True), VARIANTS),
              ("rpn_iouness", rpn_calls(g, False), VARIANTS[:2])]
    for stage, make, variants in stages:
        base = None
        for kind, beta in variants:
            us = time_pair(make(kind, beta))
            base = us if base is None else base
            lines.append({"stage": stage, "loss": kind, "beta": beta, "entry": "L1" if (kind, beta) == ("smooth_l1", 0.0) else "reg",
                          "fwd_bwd_us": round(us, 2), "ratio_to_l1": round(us / base, 2)})
    text = "".join(json.dumps(l) + "\n" for l in lines)
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
