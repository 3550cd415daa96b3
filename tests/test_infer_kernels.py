"""csrc/infer.hip (det_score / det_nms_boxes / det_compact, through the shipped `det.fast_rcnn_inference`), `det.box_decode_gt_class`
and `det.pairwise_iou` (IoU and IoA) against plain float64 references written here from the algorithm.

Integer outputs (counts, classes, ROI indices, dummy slots) are compared exactly.  Floating outputs are compared against the float64
reference with the rule of `bounded()` in test_inference_parity.py: the same reference is evaluated once more in float32 on the CPU and
the bar is max(3 x that run's own distance to float64, one fp32 ulp of the largest compared magnitude).  Scores and probabilities are
measured as |a - b| / (1 + |b|), boxes relative to the image extent.

Measured distances to float64, largest over the cases (kernel | fp32 reference); the host emulator and the MI355X gave the same figures:
    fast_rcnn_inference   scores, probabilities 2.2e-08 | 2.9e-08      boxes 9.1e-08 | 9.1e-08 of the image extent
    box_decode_gt_class   2.0e-06 | 2.0e-06        pairwise IoU 5.5e-08 | 5.5e-08        pairwise IoA 4.5e-08 | 4.5e-08
Share of the would-be candidates altered by the input conditions (`_offenders`): 0 % (K = 50), 0.04 % (K = 80), 0.30 % (K = 130).
"""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import upstream as U
from omni3d_amd.d2 import structures as S
from omni3d_amd.d2.structures import Boxes

WEIGHTS = (10.0, 10.0, 5.0, 5.0)
NMS_THRESH = 0.5
B, P = 3, 40
COUNT = (P, 0, 17)
IMAGE_HW = ((96, 128), (80, 112), (120, 72))              # (H, W): all different, none square
SCORE_THRESH = {50: 0.002, 80: 0.00125, 130: 0.00075}     # ~0.1 / (K + 1): most (roi, class) pairs of a plain row are candidates

# image 0, rows with a purpose (everything else is a plain clustered row)
R_DUP_A, R_DUP_B = 3, 11          # identical logits, deltas and ROIs
R_NAN, R_PINF, R_BGNAN, R_INFDELTA, R_OVERFLOW = 5, 8, 13, 17, 21      # must be dropped whole
R_NEGINF, R_CLAMP, R_LEFT, R_RIGHT, R_TOP, R_BOTTOM, R_OUTSIDE, R_TWOCLS = 22, 25, 28, 29, 30, 31, 34, 37
R_SMALL = 19                      # a 1 x 1 px proposal: its clamped box stays inside the image
DROPPED = (R_NAN, R_PINF, R_BGNAN, R_INFDELTA, R_OVERFLOW)
EDGE_ROWS = DROPPED + (R_DUP_A, R_DUP_B, R_NEGINF, R_CLAMP, R_SMALL, R_LEFT, R_RIGHT, R_TOP, R_BOTTOM, R_OUTSIDE, R_TWOCLS)


def _decode(deltas, boxes, weights, scale_clamp=math.log(1000.0 / 16)):
    """Box2BoxTransform.apply_deltas in the dtype of its arguments (oracle/upstream.py's computes in float32 whatever it is given;
    `test_decode_matches_oracle` pins the two to each other bit for bit in float32)"""
    w, h = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    cx, cy = boxes[:, 0] + 0.5 * w, boxes[:, 1] + 0.5 * h
    dx, dy = deltas[:, 0::4] / weights[0], deltas[:, 1::4] / weights[1]
    dw, dh = (deltas[:, 2::4] / weights[2]).clamp(max=scale_clamp), (deltas[:, 3::4] / weights[3]).clamp(max=scale_clamp)
    pcx, pcy = dx * w[:, None] + cx[:, None], dy * h[:, None] + cy[:, None]
    pw, ph = torch.exp(dw) * w[:, None], torch.exp(dh) * h[:, None]
    return torch.stack((pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph), dim=-1).reshape(deltas.shape)


def _ld(K):
    return (5 * K + 1 + 15) // 16 * 16          # 256 / 416 / 656: never 5K + 1


def _cluster_rows(g, n, H, W):
    """n proposals in four well separated groups, each split in two halves shifted by half a width: IoU ~0.8 inside a half (suppressed),
    ~1/3 between the halves (kept), 0 across groups"""
    centres = [(0.24 * W, 0.30 * H), (0.72 * W, 0.28 * H), (0.26 * W, 0.74 * H), (0.70 * W, 0.72 * H)]
    out = []
    for i in range(n):
        cx, cy = centres[i % 4]
        w, h = 0.22 * W + 2.0 * (i % 4), 0.26 * H - 1.5 * (i % 4)
        if (i // 4) % 2:
            cx += 0.5 * w
        j = (torch.rand(4, generator=g, dtype=torch.float64) - 0.5) * 2.0
        out.append([cx - w / 2 + j[0], cy - h / 2 + j[1], cx + w / 2 + j[2], cy + h / 2 + j[3]])
    return torch.tensor(out, dtype=torch.float64)


def _build(K, seed, quiet):
    """-> pred (B*P, ld), rois (B*P, 4) float32.  quiet: every row of image 0 scores below the threshold."""
    g = torch.Generator().manual_seed(seed)
    ld = _ld(K)
    pred = torch.full((B * P, ld), float("nan"), dtype=torch.float64)          # the pad is never to be read
    pred[:, :K + 1] = torch.randn(B * P, K + 1, generator=g, dtype=torch.float64)
    pred[:, K + 1:5 * K + 1] = 0.3 * torch.randn(B * P, 4 * K, generator=g, dtype=torch.float64)
    rois = torch.zeros(B * P, 4, dtype=torch.float64)
    for b in range(B):
        H, W = IMAGE_HW[b]
        rois[b * P:(b + 1) * P] = _cluster_rows(g, P, H, W)
    logit, delta = pred[:, :K + 1], pred[:, K + 1:5 * K + 1].view(B * P, K, 4)          # views
    # rows past count[b] (all of image 1): well-formed, confident rows -- they would lead the detections if they were looked at
    for b in range(B):
        logit[b * P + COUNT[b]:(b + 1) * P, 1] += 9.0
    # image 2: background dominates, a few dozen candidates, fewer survivors than any topk used
    logit[2 * P:2 * P + COUNT[2], K] = math.log(6.0 * math.sqrt(K) * (K + 1))
    H, W = IMAGE_HW[0]
    pred[R_DUP_B], rois[R_DUP_B] = pred[R_DUP_A], rois[R_DUP_A]
    logit[R_DUP_A, 5] = logit[R_DUP_B, 5] = 3.5
    for r in DROPPED:                                       # confident rows: kept, they would lead the detections
        logit[r, 7] = 5.0
    c_hi = (7 * K) // 8                                     # 43 / 70 / 113: past the first wave of classes for K >= 80
    logit[R_NAN, c_hi] = float("nan")
    logit[R_PINF, 2] = float("inf")
    logit[R_BGNAN, K] = float("nan")
    logit[R_INFDELTA, K - 1] = -10.0                        # class K-1 (the last pass of the class loop) is far below the threshold ...
    delta[R_INFDELTA, K - 1, 0] = float("inf")              # ... and its box is not finite: the whole row goes
    delta[R_OVERFLOW, 1, 0] = 3.0e38                        # dx / wx * w ~ 9e38: finite in float64, +inf in the fp32 the pipeline computes in
    logit[R_NEGINF, 4] = float("-inf")                      # probability 0, nothing non-finite: the row stays
    logit[R_NEGINF, 7] = 4.0
    delta[R_CLAMP, 0::7, 2:] = 40.0                         # dw / ww = dh / wh = 8 > log(1000 / 16)
    logit[R_CLAMP, 0] = 4.0
    rois[R_SMALL] = torch.tensor([W / 2 - 0.5, H / 2 - 0.5, W / 2 + 0.5, H / 2 + 0.5])
    for c in (2, K - 2):                                    # clamped to 1000 / 16 = 62.5 px a side, nothing for the clip to hide
        delta[R_SMALL, c, 2:] = 40.0
        logit[R_SMALL, c] = 4.0
    rois[R_LEFT] = torch.tensor([-14.0, 20.0, 18.0, 50.0])
    rois[R_RIGHT] = torch.tensor([W - 17.0, 30.0, W + 13.0, 62.0])
    rois[R_TOP] = torch.tensor([50.0, -15.0, 84.0, 16.0])
    rois[R_BOTTOM] = torch.tensor([40.0, H - 18.0, 70.0, H + 12.0])
    rois[R_OUTSIDE] = torch.tensor([W + 10.0, 30.0, W + 40.0, 60.0])           # clips to the empty box (W, y1, W, y2); still a candidate
    for r in (R_LEFT, R_RIGHT, R_TOP, R_BOTTOM, R_OUTSIDE):
        logit[r, 3] = 4.0
    delta[R_TWOCLS, 9] = delta[R_TWOCLS, 6]                 # one box under two classes: both survive
    logit[R_TWOCLS, 6] = 4.0
    logit[R_TWOCLS, 9] = 3.9
    if quiet:
        logit[:P, K] += 30.0
    return pred.float(), rois.float()


def _iou_matrix(b):
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    wh = (torch.min(b[:, None, 2:], b[:, 2:]) - torch.max(b[:, None, :2], b[:, :2])).clamp(min=0)
    inter = wh.prod(dim=2)
    return torch.where(inter > 0, inter / (area[:, None] + area - inter), torch.zeros((), dtype=b.dtype))


def _candidates(pred, rois, b, K, dtype):
    """steps 1-5 for image b: softmax, decode of every class, drop the non-finite rows, clip, threshold -> row-major (roi, class) list"""
    n, thr = COUNT[b], SCORE_THRESH[K]
    rows = slice(b * P, b * P + n)
    probs = torch.softmax(pred[rows, :K + 1].to(dtype), dim=1)
    boxes = _decode(pred[rows, K + 1:5 * K + 1].to(dtype), rois[rows].to(dtype), WEIGHTS).view(n, K, 4)
    # the pipeline's numbers are fp32: "finite" means finite as an fp32 value
    ok = torch.isfinite(probs.float()).all(dim=1) & torch.isfinite(boxes.float()).view(n, 4 * K).all(dim=1)
    H, W = IMAGE_HW[b]
    boxes = torch.stack((boxes[..., 0].clamp(0, W), boxes[..., 1].clamp(0, H), boxes[..., 2].clamp(0, W), boxes[..., 3].clamp(0, H)), dim=-1)
    roi, cls = torch.nonzero(ok[:, None] & (probs[:, :K] > thr), as_tuple=True)
    return {"probs": probs[:, :K], "ok": ok, "roi": roi, "cls": cls, "score": probs[roi, cls], "box": boxes[roi, cls]}


def _survivors(c, cap):
    """steps 6-7 on the `cap` best candidates in stable order: per-class NMS -> indices into the candidate list, stable descending score"""
    first = torch.sort(c["score"], descending=True, stable=True)[1][:cap]
    first = torch.sort(first)[0]                                         # the row-major list again
    return first[U.batched_nms(c["box"][first], c["score"][first], c["cls"][first], NMS_THRESH)]


def _detect(c, keep, topk):
    """step 8: the first topk survivors; rank = place of the last one in the sorted candidate list"""
    keep = keep[:topk]
    return {"box": c["box"][keep], "score": c["score"][keep], "cls": c["cls"][keep], "roi": c["roi"][keep], "full": c["probs"][c["roi"][keep]],
            "rank": int((c["score"] >= c["score"][keep[-1]]).sum()) if len(keep) else 0}


def _offenders(c, thr):
    """(roi, class) pairs of image candidates that make the comparison ill defined (float64 only):
    a score within 1e-5 (relative) of the threshold; a same-class pair whose IoU is within 1e-2 of the NMS threshold (the kernel runs
    NMS on coordinates shifted by class x (max + 1), rounded by up to 2^-9 px: ~2e-3 of IoU for the 8 px boxes here); two unequal
    scores within 1e-6 (relative), whose order fp32 may legitimately swap -- the order decides NMS, the cap and the topk cut."""
    roi, cls, score, box = c["roi"], c["cls"], c["score"], c["box"]
    bad = set(torch.nonzero((score - thr).abs() <= 1e-5 * thr).flatten().tolist())
    pairs = []
    for k in torch.unique(cls).tolist():
        sel = torch.nonzero(cls == k).flatten()
        near = torch.triu((_iou_matrix(box[sel]) - NMS_THRESH).abs() <= 1e-2, diagonal=1)
        pairs += [(int(sel[i]), int(sel[j])) for i, j in torch.nonzero(near).tolist()]
    s, order = torch.sort(score, descending=True, stable=True)
    close = torch.nonzero((s[:-1] != s[1:]) & ((s[:-1] - s[1:]) <= 1e-6 * s[:-1])).flatten().tolist()
    pairs += [(int(order[i]), int(order[i + 1])) for i in close]
    for i, j in pairs:
        lo, hi = (i, j) if score[i] <= score[j] else (j, i)
        bad.add(hi if int(roi[lo]) in EDGE_ROWS and int(roi[hi]) not in EDGE_ROWS else lo)
    return [(int(roi[i]), int(cls[i])) for i in sorted(bad)]


@functools.lru_cache(maxsize=None)
def _case(K, quiet=False):
    """inputs that satisfy the conditions of `_offenders` (an offending candidate's logit is lowered until it is no candidate), with
    their float64 and float32 candidate lists.  Nothing here looks at the code under test."""
    pred, rois = _build(K, seed=K, quiet=quiet)
    thr = SCORE_THRESH[K]
    total = sum(len(_candidates(pred, rois, b, K, torch.float64)["score"]) for b in range(B))
    altered = []
    for _ in range(8):
        found = []
        for b in range(B):
            found += [(b * P + r, c) for r, c in _offenders(_candidates(pred, rois, b, K, torch.float64), thr)]
        if not found:
            break
        for r, c in found:
            pred[r, c] = -12.0
        altered += found
    else:
        raise AssertionError("input conditions not met after 8 rounds")
    assert not any(b == 0 and r in EDGE_ROWS for b, r in ((row // P, row % P) for row, _ in altered)), altered
    share = len(altered) / max(total, 1)
    assert share <= 0.05, "%.1f %% of the candidates altered" % (100 * share)
    c64 = [_candidates(pred, rois, b, K, torch.float64) for b in range(B)]
    c32 = [_candidates(pred, rois, b, K, torch.float32) for b in range(B)]
    for b in range(B):          # the fp32 evaluation of the reference sees the same candidates
        assert torch.equal(c64[b]["roi"], c32[b]["roi"]) and torch.equal(c64[b]["cls"], c32[b]["cls"]) and torch.equal(c64[b]["ok"], c32[b]["ok"])
    return {"K": K, "pred": pred, "rois": rois, "c64": c64, "c32": c32, "share": share, "candidates": [len(c["score"]) for c in c64]}


@functools.lru_cache(maxsize=None)
def _kept(K, quiet, cap):
    case = _case(K, quiet)
    return [(_survivors(case["c64"][b], cap), _survivors(case["c32"][b], cap)) for b in range(B)]


def _expected(K, quiet, cap, topk):
    """per image (float64 result, float32 result) of the reference"""
    case, kept = _case(K, quiet), _kept(K, quiet, cap)
    return [(_detect(case["c64"][b], kept[b][0], topk), _detect(case["c32"][b], kept[b][1], topk)) for b in range(B)]


class _Dist:
    """|got - fp64| against max(3 x |fp32 reference - fp64|, one fp32 ulp of the largest compared magnitude); `scale` None: 1 + |fp64|"""

    def __init__(self):
        self.rows = {}

    def add(self, name, got, r32, r64, scale=None):
        got, r32, r64 = got.double().cpu(), r32.double(), r64.double()
        if r64.numel() == 0:
            assert got.numel() == 0 and r32.numel() == 0
            return
        den = (1.0 + r64.abs()) if scale is None else torch.full_like(r64, float(scale))
        e_got, e_ref = float(((got - r64).abs() / den).max()), float(((r32 - r64).abs() / den).max())
        k = int(r64.abs().argmax())
        ulp = float(np.spacing(np.float32(r64.abs().flatten()[k]))) / float(den.flatten()[k])
        row = self.rows.setdefault(name, [0.0, 0.0, 0.0])
        row[0], row[1], row[2] = max(row[0], e_got), max(row[1], e_ref), max(row[2], e_got / max(3.0 * e_ref, ulp))
        assert e_got <= max(3.0 * e_ref, ulp), "%s: |kernel - fp64| %.3e, |fp32 ref - fp64| %.3e, ulp %.3e" % (name, e_got, e_ref, ulp)

    def report(self, title):
        for name, (e_got, e_ref, used) in sorted(self.rows.items()):
            print("%s %-8s |kernel-fp64| %.2e  |ref32-fp64| %.2e  (%.2f of the bound)" % (title, name, e_got, e_ref, used))


def _check(dev, K, quiet, cap, topk, dist):
    from omni3d_amd.kernels import det
    case = _case(K, quiet)
    pred, rois = case["pred"], case["rois"]
    count = torch.tensor(COUNT, dtype=torch.int32)
    hw = torch.tensor(IMAGE_HW, dtype=torch.int32)
    out = det.fast_rcnn_inference(pred.to(dev), rois.to(dev), count.to(dev), hw.to(dev), B, P, K, WEIGHTS, SCORE_THRESH[K], NMS_THRESH, topk,
                                  cap)
    dbox, dscore, dcls, droi, dcount, probs = [t.cpu() for t in out]
    assert dbox.shape == (B, topk, 4) and dscore.shape == dcls.shape == droi.shape == (B, topk) and probs.shape == (B * P, K)
    # the kept rows' probabilities of every class, gathered as roi_heads/inference.py gathers them
    full = torch.gather(probs.view(B, P, K), 1, droi.long()[:, :, None].expand(-1, -1, K))
    eff_cap = min(det.DET_MAX_CANDIDATES, P * K) if cap is None else cap
    exp = _expected(K, quiet, eff_cap, topk)
    for b in range(B):
        e64, e32 = exp[b]
        n = len(e64["cls"])
        tag = "K=%d quiet=%d cap=%s topk=%d image %d" % (K, quiet, cap, topk, b)
        assert torch.equal(e64["cls"], e32["cls"]) and torch.equal(e64["roi"], e32["roi"]), tag + ": fp32 and fp64 references disagree"
        assert int(dcount[b]) == n, "%s: dcount %d, reference %d" % (tag, int(dcount[b]), n)
        assert torch.equal(dcls[b, :n].long(), e64["cls"]), tag
        assert torch.equal(droi[b, :n].long(), e64["roi"]), tag
        # unused slots: exactly the dummy box (0, 0, 1, 1), score 0, class 0, roi 0
        assert torch.equal(dbox[b, n:], torch.tensor([0.0, 0.0, 1.0, 1.0]).expand(topk - n, 4)), tag
        assert not dscore[b, n:].any() and not dcls[b, n:].any() and not droi[b, n:].any(), tag
        ext = float(max(IMAGE_HW[b]))
        dist.add("scores", dscore[b, :n], e32["score"], e64["score"])
        dist.add("boxes", dbox[b, :n], e32["box"], e64["box"], scale=ext)
        dist.add("full", full[b, :n], e32["full"], e64["full"])
        # probabilities: rows that exist and were not dropped against the softmax; rows past count exactly 0; no class of a dropped row
        # among the detections
        c64, c32 = case["c64"][b], case["c32"][b]
        mine = probs.view(B, P, K)[b]
        ok = c64["ok"]
        dist.add("probs", mine[:COUNT[b]][ok], c32["probs"][ok], c64["probs"][ok])
        assert not mine[COUNT[b]:].any(), tag + ": probabilities of rows past count"
        dropped = torch.nonzero(~ok).flatten()
        assert not torch.isin(droi[b, :n].long(), dropped).any(), tag + ": a dropped row among the detections"
    return exp, (dcount, dcls, droi, dscore, dbox)


def _run_infer(dev, K):
    dist = _Dist()
    case = _case(K)
    assert case["candidates"][1] == 0 and 0 < case["candidates"][2] < 150 and case["candidates"][0] > 1500
    dropped = torch.nonzero(~case["c64"][0]["ok"]).flatten().tolist()
    assert dropped == sorted(DROPPED), dropped                                     # exactly the rows meant to go, -inf logit row kept
    full_cap = P * K
    if K == 50:
        runs = [(full_cap, 100), (None, 10), (64, 10), (1500, 100)]
    elif K == 80:
        runs = [(full_cap, 10), (64, 10), (64, 100)]          # the last: more slots than the capped list leaves survivors
    else:                                                     # uncapped: six trips of the 1024-thread gather, 82 NMS words
        runs = [(full_cap, 10), (full_cap, 100), (64, 10), (1500, 100)]
    cap_changes_nothing = [(64, 10), (1500, 100)]
    res = {(cap, topk): _check(dev, K, False, cap, topk, dist) for cap, topk in runs}
    exp = {k: v[0] for k, v in res.items()}
    # the edges are really there (float64 reference only)
    top = _expected(K, False, full_cap, 100)[0][0]
    det_pairs = list(zip(top["roi"].tolist(), top["cls"].tolist()))
    assert (R_DUP_A, 5) in det_pairs and (R_DUP_B, 5) not in det_pairs             # tie, IoU 1: the lower ROI index survives
    assert (R_TWOCLS, 6) in det_pairs and (R_TWOCLS, 9) in det_pairs               # one box, two classes: both survive
    H, W = IMAGE_HW[0]
    box_of = {rc: top["box"][i] for i, rc in enumerate(det_pairs)}
    assert box_of[(R_CLAMP, 0)].tolist() == [0.0, 0.0, W, H]                       # clipped on all four sides
    for c in (2, K - 2):                                                           # dw, dh clamped: 1 px x 1000 / 16, and not clipped
        x1, y1, x2, y2 = box_of[(R_SMALL, c)].tolist()
        assert 0 < x1 and 0 < y1 and x2 < W and y2 < H
        sw, sh = float(case["rois"][R_SMALL, 2] - case["rois"][R_SMALL, 0]), float(case["rois"][R_SMALL, 3] - case["rois"][R_SMALL, 1])
        assert abs(x2 - x1 - sw * 1000.0 / 16) < 1e-9 and abs(y2 - y1 - sh * 1000.0 / 16) < 1e-9
    assert box_of[(R_LEFT, 3)][0] == 0 and box_of[(R_RIGHT, 3)][2] == W and box_of[(R_TOP, 3)][1] == 0 and box_of[(R_BOTTOM, 3)][3] == H
    assert box_of[(R_OUTSIDE, 3)][0] == W and box_of[(R_OUTSIDE, 3)][2] == W       # empty after clipping, a detection all the same
    assert any(r == R_NEGINF for r, _ in det_pairs)                                # a -inf logit drops nothing
    assert len(top["cls"]) == 100 and len(_expected(K, False, full_cap, 100)[2][0]["cls"]) < 100
    # documented property of the cap: if the uncapped topk-th detection ranks inside the first `cap` candidates, the cap changes nothing
    for (cap, topk), got in exp.items():
        if (cap, topk) not in cap_changes_nothing:
            continue
        for b in range(B):
            free, capped = _expected(K, False, full_cap, topk)[b][0], got[b][0]
            assert free["rank"] <= cap, "case does not exercise the property: rank %d, cap %d" % (free["rank"], cap)
            for k in ("cls", "roi", "score", "box"):
                assert torch.equal(free[k], capped[k]), (cap, topk, b, k)
        # ... and the same of the kernels themselves: every output at `cap` equals the output without a cap, bit for bit
        uncapped = res[(full_cap, topk)] if (full_cap, topk) in res else res[(None, topk)]
        for a, c in zip(uncapped[1], res[(cap, topk)][1]):
            assert torch.equal(a, c), (cap, topk)
    # an image with P rows that all score below the threshold: no detection, every slot a dummy
    quiet = _case(K, True)
    assert quiet["candidates"][0] == 0 and quiet["candidates"][2] > 0
    _check(dev, K, True, 64, 10, dist)
    print("K=%d candidates %s, altered by the input conditions: %.2f %% (quiet variant %.2f %%)"
          % (K, case["candidates"], 100 * case["share"], 100 * quiet["share"]))
    dist.report("infer K=%d %s" % (K, dev))


def test_decode_matches_oracle():
    """the dtype-generic decode of this file is oracle/upstream.py's Box2BoxTransform.apply_deltas, bit for bit in float32"""
    g = torch.Generator().manual_seed(3)
    deltas = torch.randn(33, 4 * 7, generator=g) * 3.0
    deltas[0, 2::4] = 40.0
    boxes = torch.tensor([[3.0, 4.0, 40.0, 60.0]]).repeat(33, 1) + torch.rand(33, 4, generator=g)
    for w in (WEIGHTS, (1.0, 2.0, 3.0, 4.0)):
        assert torch.equal(_decode(deltas, boxes, w), U.Box2BoxTransform(w).apply_deltas(deltas, boxes))


@pytest.mark.parametrize("K", [50, 80, 130])
def test_fast_rcnn_inference_emulated(emu_lib, K):
    _run_infer("cpu", K)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [50, 80, 130])
def test_fast_rcnn_inference_gpu(hip_lib, K):
    _run_infer("cuda", K)


def _run_score_equal_to_threshold(dev):
    """`score > thresh` is strict.  Four equal logits give 1/4 in every precision (exp(0) = 1, the sum 4 and the quotient are exact), so with
    thresh = 0.25 that row has no candidate; two classes of the other row pass and share one box: both survive, the rest is dummy slots."""
    from omni3d_amd.kernels import det
    K, ld = 3, 32
    pred = torch.zeros(2, ld)
    pred[1, 0] = 1.0                                        # e / (e + 3) = 0.475, 1 / (e + 3) = 0.175 < 0.25
    pred[1, 1] = 0.5                                        # 0.30 for class 1, 0.18 for class 2 and the background
    rois = torch.tensor([[4.0, 6.0, 20.0, 30.0], [8.0, 2.0, 28.0, 22.0]])
    out = det.fast_rcnn_inference(pred.to(dev), rois.to(dev), torch.tensor([2], dtype=torch.int32).to(dev),
                                  torch.tensor([[40, 50]], dtype=torch.int32).to(dev), 1, 2, K, WEIGHTS, 0.25, NMS_THRESH, 4)
    dbox, dscore, dcls, droi, dcount, probs = [t.cpu() for t in out]
    assert probs[0].tolist() == [0.25, 0.25, 0.25]
    assert int(dcount[0]) == 2 and dcls[0].tolist() == [0, 1, 0, 0] and droi[0].tolist() == [1, 1, 0, 0]
    assert torch.equal(dbox[0], torch.tensor([[8.0, 2.0, 28.0, 22.0], [8.0, 2.0, 28.0, 22.0], [0.0, 0.0, 1.0, 1.0], [0.0, 0.0, 1.0, 1.0]]))
    assert dscore[0, 2:].tolist() == [0.0, 0.0] and float(dscore[0, 0]) > float(dscore[0, 1]) > 0.25


def test_score_equal_to_threshold_emulated(emu_lib):
    _run_score_equal_to_threshold("cpu")


@pytest.mark.gpu
def test_score_equal_to_threshold_gpu(hip_lib):
    _run_score_equal_to_threshold("cuda")


# ---- det.box_decode_gt_class (csrc/box_loss.hip, the TRAIN_ON_PRED_BOXES path) -----------------------------------------------------
def _run_box_decode_gt_class(dev):
    from omni3d_amd.kernels import det
    R, K = 300, 50                      # one full block of 256 rows and a partial one
    ldp = _ld(K)
    g = torch.Generator().manual_seed(5)
    pred = torch.full((R, ldp), float("nan"))
    pred[:, :5 * K + 1] = torch.randn(R, 5 * K + 1, generator=g)
    prop = torch.rand(R, 4, generator=g) * 60.0
    prop[:, 2:] += prop[:, :2] + 4.0
    cls = torch.randint(0, K + 1, (R,), generator=g).int()
    cls[[0, 17, 255, 256, 299]] = torch.tensor([-1, -1, K, -1, K], dtype=torch.int32)          # ignored / background rows on both blocks
    cls[[1, 257]] = torch.tensor([0, K - 1], dtype=torch.int32)
    assert int((cls == K).sum()) >= 2 and int((cls < 0).sum()) == 3
    dist = _Dist()
    for weights in (WEIGHTS, (1.5, 2.5, 0.75, 3.0)):
        c = cls.long().clamp(0, K - 1)                                                          # background rows use class K - 1
        own = torch.gather(pred[:, K + 1:5 * K + 1].view(R, K, 4), 1, c[:, None, None].expand(-1, 1, 4)).reshape(R, 4).clone()
        big = [2, 258]
        own[big, 2] = 30.0 * weights[2]                                                         # dw, dh above the clamp
        own[big, 3] = 25.0 * weights[3]
        p = pred.clone()
        p[:, K + 1:5 * K + 1].view(R, K, 4)[torch.arange(R), c] = own
        r64 = _decode(own.double(), prop.double(), weights)
        r32 = U.Box2BoxTransform(weights).apply_deltas(own, prop)
        r64[cls < 0], r32[cls < 0] = prop[cls < 0].double(), prop[cls < 0]
        out = det.box_decode_gt_class(p.to(dev), K, cls.to(dev), prop.to(dev), weights=weights).cpu()
        assert out.shape == (R, 4)
        assert torch.equal(out[cls < 0], prop[cls < 0])                                         # copied, not recomputed
        w64 = r64[big, 2] - r64[big, 0]
        assert torch.allclose(w64, (prop[big, 2] - prop[big, 0]).double() * 1000.0 / 16, rtol=1e-12)      # the clamp took effect, nothing is clipped
        dist.add("decode", out, r32, r64)
    dist.report("box_decode_gt_class %s" % dev)


def test_box_decode_gt_class_emulated(emu_lib):
    _run_box_decode_gt_class("cpu")


@pytest.mark.gpu
def test_box_decode_gt_class_gpu(hip_lib):
    _run_box_decode_gt_class("cuda")


# ---- det.pairwise_iou, both modes (csrc/rpn_roi.hip) ---------------------------------------------------------------------------
class _Boxes64:
    """what oracle/upstream.py's pairwise functions need of a Boxes, in float64 (d2.structures.Boxes is float32 by construction)"""

    def __init__(self, tensor):
        self.tensor = tensor.double()

    def area(self):
        return (self.tensor[:, 2] - self.tensor[:, 0]) * (self.tensor[:, 3] - self.tensor[:, 1])


def _run_pairwise(dev):
    from omni3d_amd.kernels import det
    g = torch.Generator().manual_seed(9)

    def rand(n):
        b = torch.rand(n, 4, generator=g) * 50.0
        b[:, 2:] += b[:, :2] + 1.0
        return b

    dist = _Dist()
    for N, M in ((7, 37), (13, 41)):              # 259 and 533 pairs: two and three blocks of 256, the last one partial
        b1, b2 = rand(N), rand(M)
        b1[0] = torch.tensor([10.0, 10.0, 30.0, 40.0])
        b2[0] = torch.tensor([40.0, 50.0, 60.0, 70.0])                  # disjoint
        b2[1] = torch.tensor([30.0, 10.0, 50.0, 40.0])                  # shares an edge
        b2[2] = torch.tensor([30.0, 40.0, 50.0, 60.0])                  # shares a corner
        b2[3] = b1[0]                                                   # identical
        b2[4] = torch.tensor([15.0, 15.0, 20.0, 25.0])                  # nested in b1[0]
        b2[5] = torch.tensor([5.0, 5.0, 35.0, 45.0])                    # b1[0] nested in it
        b2[6] = torch.tensor([20.0, 20.0, 20.0, 30.0])                  # zero area, inside b1[0]
        b2[M - 1] = torch.tensor([12.0, 12.0, 12.0, 12.0])              # a point, in the last column
        b1[N - 1] = torch.tensor([25.0, 25.0, 25.0, 35.0])              # zero-area boxes1 row, the last row
        for mode, ref, public in (("iou", U.pairwise_iou, S.pairwise_iou), ("ioa", U.pairwise_ioa, S.pairwise_ioa)):
            out = det.pairwise_iou(b1.to(dev), b2.to(dev), mode=mode).cpu()
            r64, r32 = ref(_Boxes64(b1), _Boxes64(b2)), ref(Boxes(b1), Boxes(b2))
            assert out.shape == (N, M) and bool(torch.isfinite(out).all())
            assert torch.equal(out == 0, r64 == 0)                      # inter == 0 is exactly 0 in both modes, never NaN
            assert not out[0, [0, 1, 2, 6, M - 1]].any() and not out[N - 1, [0, 6, M - 1]].any()
            assert float(out[0, 3]) == 1.0
            assert float(out[0, 5]) == 0.5 and (mode == "iou" or float(out[0, 4]) == 1.0)          # nested either way round
            dist.add(mode, out, r32, r64)
            assert torch.equal(public(Boxes(b1.to(dev)), Boxes(b2.to(dev))).cpu(), out)          # the public route: same kernel, same result
    for mode in ("iou", "ioa"):
        some = rand(3)
        for a, b in ((some[:0], some), (some, some[:0]), (some[:0], some[:0])):
            out = det.pairwise_iou(a.to(dev), b.to(dev), mode=mode)
            assert out.shape == (a.shape[0], b.shape[0]) and out.dtype == torch.float32
    dist.report("pairwise %s" % dev)


def test_pairwise_iou_ioa_emulated(emu_lib):
    _run_pairwise("cpu")


@pytest.mark.gpu
def test_pairwise_iou_ioa_gpu(hip_lib):
    _run_pairwise("cuda")
