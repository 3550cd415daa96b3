"""Times of the proposal path's selection launches (csrc/select_nms.hip) at the shapes of bench.py's training step and inference
pass (cubercnn_DLA34_FPN, 4 x 512 x 512), run by hand on an MI355X; not part of bench.py.  Device events around 200 calls after
20 warm-up calls, outputs and scratch allocated once; one JSON line per launch group:
  train: topk_segments 4 x [49152, 12288, 3072, 768, 192] -> 2000 on stride-1 logits; nms_sorted 20 x 2000 at 0.7 (mask + scan: the
         two kernels of one call -- run the tool under `rocprofv3 --kernel-trace --stats` for the split); topk_rows 4 x 10000 -> 1000
         on the masked scores the NMS call wrote (about half of them -inf)
  infer: the same chain at PRE_NMS_TOPK_TEST 1000, and the detection pair of kernels/det.py fast_rcnn_inference: topk_rows
         4 x 50000 -> 8192 and nms_sorted 4 x 8192 at 0.5
The NMS boxes are anchors of the real grid (strides 4 .. 64, sizes 32 .. 512, ratios 0.5 / 1 / 2) decoded with N(0, 0.1) deltas and
clipped, so their overlap statistics resemble proposals, not uniform random boxes.
    python tools/bench_select.py [output file]"""
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from omni3d_amd import lib  # noqa: E402
from omni3d_amd.kernels import select  # noqa: E402

B, IMG = 4, 512
STRIDES, SIZES, RATIOS = (4, 8, 16, 32, 64), (32, 64, 128, 256, 512), (0.5, 1.0, 2.0)
SEG_N = [(IMG // s) ** 2 * len(RATIOS) for s in STRIDES]
SEG_OFF = [sum(SEG_N[:i]) for i in range(len(SEG_N))]


def timeit(fn, iters=200, warm=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def level_anchors(stride, size):
    n = IMG // stride
    c = (torch.arange(n, dtype=torch.float32) * stride)
    cy, cx = torch.meshgrid(c, c, indexing="ij")
    out = []
    for r in RATIOS:
        w, h = size / math.sqrt(r), size * math.sqrt(r)
        out.append(torch.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], dim=-1))
    return torch.stack(out, dim=2).reshape(-1, 4)                     # (H * W * 3, 4)


def proposal_problems(k, g):
    """(B * L, k, 4) decoded boxes of k random anchors per (image, level), in score order = random order; valid (B * L, k)"""
    boxes = torch.zeros(B * len(STRIDES), k, 4)
    valid = torch.zeros(B * len(STRIDES), k, dtype=torch.int32)
    for b in range(B):
        for l, (s, z) in enumerate(zip(STRIDES, SIZES)):
            a = level_anchors(s, z)
            m = min(k, a.shape[0])
            a = a[torch.randperm(a.shape[0], generator=g)[:m]]
            d = torch.randn(m, 4, generator=g) * 0.1
            w, h = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
            cx, cy = a[:, 0] + 0.5 * w + d[:, 0] * w, a[:, 1] + 0.5 * h + d[:, 1] * h
            w, h = w * torch.exp(d[:, 2]), h * torch.exp(d[:, 3])
            box = torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], dim=1).clamp(0, IMG)
            boxes[b * len(STRIDES) + l, :m] = box
            valid[b * len(STRIDES) + l, :m] = ((box[:, 2] - box[:, 0] > 0) & (box[:, 3] - box[:, 1] > 0)).int()
    return boxes, valid


def nms_call(boxes, valid, thr, scores=None, counts=None):
    """the raw entry point on buffers allocated once -> (callable, keep, masked).  With scores, and where the library has it, the
    call is the proposal path's: omni_nms_sorted_masked with the per-problem counts of real candidates."""
    L, st = lib.get(), lib.stream_of(boxes)
    Q, nmax, _ = boxes.shape
    ws = torch.empty(Q * nmax * ((nmax + 63) // 64), dtype=torch.int64, device="cuda")
    keep = torch.empty((Q, nmax), dtype=torch.int32, device="cuda")
    masked = torch.empty((Q, nmax), dtype=torch.float32, device="cuda")
    folded = scores is not None and "omni_nms_sorted_masked" in lib.SIGNATURES

    def call():
        if folded:
            L.call("omni_nms_sorted_masked", boxes.data_ptr(), counts.data_ptr(), valid.data_ptr(), Q, nmax, thr, ws.data_ptr(), keep.data_ptr(),
                   scores.data_ptr(), masked.data_ptr(), st)
        else:
            L.call("omni_nms_sorted", boxes.data_ptr(), None, valid.data_ptr(), Q, nmax, thr, ws.data_ptr(), keep.data_ptr(), st)
    return call, keep, masked


def proposal_chain(tag, k, post, g, lines):
    logits = torch.randn(B, sum(SEG_N), generator=g).cuda()
    us = timeit(lambda: select.topk_segments(logits, SEG_OFF, SEG_N, k))
    lines.append({"kernel": "topk_segments", "leg": tag, "rows": B, "segments": SEG_N, "k": k, "us": round(us, 2)})
    scores, _ = select.topk_segments(logits, SEG_OFF, SEG_N, k)
    boxes, valid = proposal_problems(k, g)
    boxes, valid = boxes.cuda(), valid.cuda()
    counts = torch.tensor([min(k, n) for n in SEG_N] * B, dtype=torch.int32).cuda()
    call, keep, masked = nms_call(boxes, valid, 0.7, scores.view(B * len(STRIDES), k).contiguous(), counts)
    us = timeit(call)
    torch.cuda.synchronize()
    kept = int(keep.sum())
    lines.append({"kernel": "nms_sorted (mask + scan)", "leg": tag, "problems": B * len(STRIDES), "boxes": k, "thr": 0.7, "us": round(us, 2),
                  "valid": int(valid.sum()), "kept": kept})
    masked = torch.where(keep != 0, scores.view(B * len(STRIDES), k), torch.full_like(masked, float("-inf"))).view(B, -1).contiguous()
    us = timeit(lambda: select.topk_rows(masked, post))
    lines.append({"kernel": "topk_rows", "leg": tag, "rows": B, "n": masked.shape[1], "k": post, "us": round(us, 2),
                  "minus_inf_share": round(float((masked == float("-inf")).float().mean()), 3)})


def detection_pair(g, lines, n=50000, cap=8192):
    scores = torch.randn(B, n, generator=g)
    scores[torch.rand(B, n, generator=g) < 0.9] = float("-inf")        # below SCORE_THRESH_TEST
    scores = scores.cuda()
    us = timeit(lambda: select.topk_rows(scores, cap), iters=100)
    lines.append({"kernel": "topk_rows", "leg": "infer-det", "rows": B, "n": n, "k": cap, "us": round(us, 2)})
    vals, _ = select.topk_rows(scores, cap)
    # class-offset boxes of ~100 objects per image: clusters of near-duplicates far apart, like the per-class candidates of one image
    centre = torch.rand(B, 100, 2, generator=g) * IMG
    pick = torch.randint(100, (B, cap), generator=g)
    c = torch.gather(centre, 1, pick.unsqueeze(-1).expand(-1, -1, 2)) + torch.randn(B, cap, 2, generator=g) * 4.0
    wh = torch.rand(B, cap, 2, generator=g) * 60.0 + 20.0
    boxes = torch.cat([c - 0.5 * wh, c + 0.5 * wh], dim=2).cuda()
    valid = torch.isfinite(vals).int().contiguous()
    call, keep, _ = nms_call(boxes, valid, 0.5)
    us = timeit(call, iters=100)
    torch.cuda.synchronize()
    lines.append({"kernel": "nms_sorted (mask + scan)", "leg": "infer-det", "problems": B, "boxes": cap, "thr": 0.5, "us": round(us, 2),
                  "valid": int(valid.sum()), "kept": int(keep.sum())})


def main(out=None):
    assert torch.cuda.is_available(), "needs the GPU"
    g = torch.Generator().manual_seed(0)
    lines = []
    proposal_chain("train", 2000, 1000, g, lines)
    proposal_chain("infer", 1000, 1000, g, lines)
    detection_pair(g, lines)
    text = "".join(json.dumps(l) + "\n" for l in lines)
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
