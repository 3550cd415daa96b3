"""The box regression losses of both detector stages -- smooth-L1 with beta, GIoU, DIoU, CIoU (csrc/box_reg_loss.h, reached through
omni_box_reg_loss_* in csrc/box_loss.hip and omni_rpn_reg_loss_* in csrc/rpn_roi.hip) -- against float64 references written here in
plain torch with autograd, straight from the formulas (fvcore's smooth_l1_loss / giou_loss / diou_loss / ciou_loss on
Box2BoxTransform.apply_deltas).

Tolerance: the rule of `_Dist` (test_infer_kernels.py) / test_train_roi_kernels.py.  The reference is evaluated once in float64 and once
in float32 on the CPU, and |kernel - fp64| <= max(3 x |fp32 reference - fp64|, one fp32 ulp of the largest compared magnitude).  Losses
and logged sums are measured as |a - b| / (1 + |b|), gradients relative to the largest magnitude of the compared tensor.  Counts and
everything specified as exactly zero (pad columns / channels, ignored rows, the gradient of a clamped delta, smooth-L1 at x == y) are
compared exactly.  Every case first asserts, on the CPU, that the float32 and the float64 reference take the same discrete decisions
for EVERY row -- intersection mask, the operand every min / max picked, clamp active or not, smooth-L1 branch, signs -- and that no
min / max operands tie.  Share of rows left out of a comparison: 0.

Measured distances to float64, largest over the cases (kernel | fp32 reference).  'all': the whole gradient tensor, where the
cross-entropy / objectness gradients set the scale; 'reg': the regression gradients alone, on their own scale.  Host emulator:
    box head   smooth_l1   loss 1.0e-08 | 8.4e-08      dpred all 2.6e-06 | 2.6e-06      reg 1.6e-05 | 1.6e-05
               giou        loss 4.8e-09 | 8.4e-08      dpred all 1.4e-07 | 1.7e-07      reg 2.5e-07 | 2.5e-07
               diou        loss 4.8e-09 | 8.4e-08      dpred all 1.4e-07 | 1.7e-07      reg 2.9e-07 | 2.3e-07
               ciou        loss 4.8e-09 | 8.4e-08      dpred all 1.4e-07 | 1.7e-07      reg 2.9e-07 | 2.3e-07
    RPN        IoUness smooth_l1   loss 4.5e-09 | 2.9e-08      levels all 5.2e-07 | 5.2e-07      reg 3.9e-07 | 3.9e-07
               none smooth_l1      loss 8.7e-09 | 4.6e-08      levels all 1.9e-07 | 1.9e-07      reg 6.5e-07 | 6.5e-07
               none giou           loss 1.9e-08 | 3.2e-08      levels all 5.5e-07 | 5.5e-07      reg 1.0e-06 | 1.0e-06
               none diou           loss 2.0e-08 | 2.0e-08      levels all 5.5e-07 | 5.7e-07      reg 9.6e-07 | 9.9e-07
               none ciou           loss 1.9e-08 | 2.4e-08      levels all 5.5e-07 | 5.7e-07      reg 9.6e-07 | 9.9e-07
               sums of sigmoid (all variants)   2.0e-08 | 4.3e-08
MI355X: the gradient columns are the same to both digits; the losses are
    box head   smooth_l1 1.2e-08 | 8.4e-08      giou, diou, ciou 1.0e-08 | 8.4e-08
    RPN        IoUness smooth_l1 3.4e-09 | 1.3e-08      none: smooth_l1 8.7e-09 | 4.7e-08, giou 1.7e-08 | 3.2e-08, diou 2.0e-08 | 2.0e-08,
               ciou 1.9e-08 | 2.4e-08
(smooth_l1 'reg': the quadratic branch divides x - y, which carries the float32 rounding of the target delta, by beta; both columns.)
On both, smooth_l1 with beta 1e-6 returns the bits of the L1 entry points, sums and gradients.
"""
import functools
import math

import pytest
import torch

from oracle import upstream as U
from test_det import _anchors
from test_infer_kernels import _Dist
from test_train_roi_kernels import BOX_R, G_CLS, G_REG, WEIGHTS, _box_inputs, _scale

NAN = float("nan")
CLAMP = math.log(1000.0 / 16)
IOU_KINDS = ("giou", "diou", "ciou")
VARIANTS = [("smooth_l1", 0.5), ("smooth_l1", 1e-6), ("giou", 0.0), ("diou", 0.0), ("ciou", 0.0)]
VARIANT_IDS = ["smooth_l1-0.5", "smooth_l1-1e-6", "giou", "diou", "ciou"]


# ---- the reference: one (predicted deltas, source box, ground-truth box) triple per row, any dtype ------------------------------------
def _smooth_l1(x, y, beta):
    n = (x - y).abs()
    if beta < 1e-5:
        return n, torch.zeros_like(n, dtype=torch.bool)
    quad = n < beta
    return torch.where(quad, 0.5 * n ** 2 / beta, n - 0.5 * beta), quad


def _apply_deltas(d, src, weights):
    """Box2BoxTransform.apply_deltas; -> boxes XYXY, (n, 2) whether the clamp on dw / dh is active"""
    wx, wy, ww, wh = weights
    w, h = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]
    cx, cy = src[:, 0] + 0.5 * w, src[:, 1] + 0.5 * h
    dx, dy, dw, dh = d[:, 0] / wx, d[:, 1] / wy, d[:, 2] / ww, d[:, 3] / wh
    active = torch.stack([dw > CLAMP, dh > CLAMP], dim=1).detach()
    dw, dh = torch.clamp(dw, max=CLAMP), torch.clamp(dh, max=CLAMP)
    pcx, pcy, pw, ph = dx * w + cx, dy * h + cy, torch.exp(dw) * w, torch.exp(dh) * h
    return torch.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], dim=1), active


def _iou_loss(kind, p, g):
    eps = 1e-7
    px1, py1, px2, py2 = p.unbind(1)
    gx1, gy1, gx2, gy2 = g.unbind(1)
    xk1, yk1, xk2, yk2 = torch.max(px1, gx1), torch.max(py1, gy1), torch.min(px2, gx2), torch.min(py2, gy2)
    mask = (yk2 > yk1) & (xk2 > xk1)
    inter = torch.where(mask, (xk2 - xk1) * (yk2 - yk1), torch.zeros_like(xk1))
    xc1, yc1, xc2, yc2 = torch.min(px1, gx1), torch.min(py1, gy1), torch.max(px2, gx2), torch.max(py2, gy2)
    area_p, area_g = (px2 - px1) * (py2 - py1), (gx2 - gx1) * (gy2 - gy1)
    dec = {"mask": mask.detach(), "side": torch.sign(p.detach() - g).long(), "tie": bool((p.detach() == g).any())}
    if kind == "giou":
        union = area_p + area_g - inter
        iou = inter / (union + eps)
        area_c = (xc2 - xc1) * (yc2 - yc1)
        return 1 - iou + (area_c - union) / (area_c + eps), dec
    union = area_p + area_g - inter + eps
    iou = inter / union
    diag = (xc2 - xc1) ** 2 + (yc2 - yc1) ** 2 + eps
    dist = ((px1 + px2) / 2 - (gx1 + gx2) / 2) ** 2 + ((py1 + py2) / 2 - (gy1 + gy2) / 2) ** 2
    loss = 1 - iou + dist / diag
    if kind == "ciou":
        da = torch.atan((gx2 - gx1) / (gy2 - gy1)) - torch.atan((px2 - px1) / (py2 - py1))
        v = (4 / math.pi ** 2) * da ** 2
        with torch.no_grad():
            alpha = v / (1 - iou + v + eps)
        loss = loss + alpha * v
        dec["aspect"] = torch.sign(da.detach()).long()
    return loss, dec


def _reg_loss(kind, beta, d, src, gt, weights):
    """-> per-row loss (n,), the discrete decisions taken on the way"""
    if kind == "smooth_l1":
        tgt = U.Box2BoxTransform(weights).get_deltas(src, gt) if d.shape[0] else d.detach()
        v, quad = _smooth_l1(d, tgt, beta)
        return v.sum(dim=1), {"sign": torch.sign(d.detach() - tgt).long(), "quad": quad.detach(), "tie": False}
    p, active = _apply_deltas(d, src, weights)
    loss, dec = _iou_loss(kind, p, gt)
    dec["clamp"] = active
    return loss, dec


def _same_decisions(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], "float32 and float64 references decide differently: " + k
    assert not a["tie"], "min / max operands tie"


# ---- 1. box head (omni_box_reg_loss_fwd / _bwd) -------------------------------------------------------------------------------------------
BOX_KS = [7, 80]                   # K = 80: the softmax uses both slots of a lane; R = 300: waves 0 .. 43 take a second row


@functools.lru_cache(maxsize=None)
def _box_case(K, variant, iou):
    """the rows of test_train_roi_kernels._box_inputs (ldp padded to 16; NaN in the pad columns and in ignored rows), plus planted
    foreground rows with ground-truth boxes of their own ('mixed' only).  iou: the case serves giou / diou / ciou"""
    inp = {k: (v.clone() if torch.is_tensor(v) else dict(v) if isinstance(v, dict) else v) for k, v in _box_inputs(K, variant).items()}
    if variant != "mixed":
        return inp
    g = torch.Generator().manual_seed(500 + K)
    pred, cls, prop, gt_row, planted = inp["pred"], inp["cls"], inp["prop"], inp["gt_row"], inp["planted"]
    extra = []

    def plant(name, r, box, gt, deltas):
        c = (3 * r) % K
        pred[r, :K + 1] = torch.randn(K + 1, generator=g) * 2.0
        pred[r, K + 1:5 * K + 1] = torch.randn(4 * K, generator=g) * 0.5
        pred[r, K + 1 + 4 * c:K + 5 + 4 * c] = torch.tensor(deltas)
        cls[r], prop[r], gt_row[r] = c, torch.tensor(box), inp["gtb"].shape[0] + len(extra)
        extra.append(gt)
        planted[name] = r

    # dw above the scale clamp (weights 5): the box uses the clamp, the gradient of that delta is exactly 0
    plant("clamp", 100, [40.0, 40.0, 60.0, 70.0], [30.0, 20.0, 90.0, 100.0], [0.3, -0.2, 5.0 * (CLAMP + 0.5), 0.4])
    plant("disjoint", 101, [10.0, 10.0, 30.0, 30.0], [100.0, 120.0, 150.0, 160.0], [0.5, -0.5, 0.2, 0.1])
    plant("pred_in_gt", 102, [50.0, 50.0, 90.0, 100.0], [40.0, 35.0, 110.0, 120.0], [0.1, 0.1, -0.2, -0.2])
    plant("gt_in_pred", 285, [30.0, 30.0, 120.0, 130.0], [50.0, 60.0, 80.0, 90.0], [0.1, -0.1, 0.1, 0.1])
    # targets 10 * 2 / 20 = 1, 10 * 8 / 40 = 2, 5 * log(20 / 20) = 0 in any precision: |x - y| == beta = 0.5 in dx and dw (the
    # linear branch), x == y in dy
    plant("beta", 286, [100.0, 100.0, 120.0, 140.0], [102.0, 104.0, 122.0, 152.0], [1.5, 2.0, -0.5, 1.0])
    plant("elongated", 287, [20.0, 100.0, 220.0, 104.0], [100.0, 20.0, 106.0, 230.0], [0.1, 0.2, 0.1, -0.1])
    if iou:
        # the 'exact' row of _box_inputs decodes onto its ground-truth box in x: min / max would tie
        r = planted["exact"]
        c = int(cls[r])
        pred[r, K + 1 + 4 * c], pred[r, K + 1 + 4 * c + 2] = 0.7, 0.3
    inp["gtb"] = torch.cat([inp["gtb"], torch.tensor(extra)])
    return inp


def _box_ref(inp, kind, beta, dtype):
    """log_softmax cross-entropy over the rows with cls >= 0 + the regression loss summed over the rows with cls < K, both
    / max(#rows, 1); the gradient of G_CLS * loss_cls + G_REG * loss_box_reg by autograd"""
    K, pred, cls = inp["K"], inp["pred"], inp["cls"].long()
    val = cls >= 0
    fg = val & (cls < K)
    n = max(int(val.sum()), 1)
    grad = torch.zeros(pred.shape, dtype=dtype)
    x = pred[val][:, :5 * K + 1].to(dtype).requires_grad_(True)
    c, fgv = cls[val], fg[val]
    ce = -torch.log_softmax(x[:, :K + 1], dim=1).gather(1, c[:, None]).sum()
    own = x[fgv][:, K + 1:].reshape(-1, K, 4)[torch.arange(int(fgv.sum())), c[fgv]]
    per, dec = _reg_loss(kind, beta, own, inp["prop"][fg].to(dtype), inp["gtb"][inp["gt_row"][fg].long()].to(dtype), WEIGHTS)
    loss_cls, loss_reg = ce / n, per.sum() / n
    if x.shape[0]:
        (G_CLS * loss_cls + G_REG * loss_reg).backward()
        grad[val, :5 * K + 1] = x.grad
    return {"loss": torch.stack([loss_cls.detach(), loss_reg.detach()]), "grad": grad, "dec": dec, "per": per.detach(),
            "fg_rows": torch.nonzero(fg).flatten().tolist()}


def _run_box(dev, K, variant, kind, beta, dist):
    from omni3d_amd.kernels import det
    inp = _box_case(K, variant, kind in IOU_KINDS)
    r64, r32 = _box_ref(inp, kind, beta, torch.float64), _box_ref(inp, kind, beta, torch.float32)
    _same_decisions(r64["dec"], r32["dec"])
    cls = inp["cls"]
    val = cls >= 0
    args = [inp["pred"].to(dev), K] + [inp[k].to(dev) for k in ("cls", "prop", "gtb", "gt_row")]
    sums = det.box_loss_fwd(*args, WEIGHTS, kind, beta)
    s = sums.cpu()
    assert s.dtype == torch.float64 and bool(torch.isfinite(s).all())
    assert s[2] == int(val.sum()) and s[3] == len(r64["fg_rows"])
    dist.add("loss", s[:2] / max(float(s[2]), 1.0), r32["loss"], r64["loss"])
    gc, gr = torch.tensor([G_CLS]).to(dev), torch.tensor([G_REG]).to(dev)
    dpred = det.box_loss_bwd(*args, sums, gc, gr, WEIGHTS, kind, beta).cpu()
    assert bool(torch.isfinite(dpred).all())
    assert not dpred[~val].any() and not dpred[:, 5 * K + 1:].any()                              # ignored rows, pad columns: exactly 0
    own = torch.zeros(dpred.shape, dtype=torch.bool)                                             # the GT-class deltas of the foreground rows
    for r in r64["fg_rows"]:
        own[r, K + 1 + 4 * int(cls[r]):K + 5 + 4 * int(cls[r])] = True
    assert not dpred[:, K + 1:][~own[:, K + 1:]].any()                                           # every other delta: exactly 0
    if kind == "smooth_l1":
        # the exact-zero pattern of the GT-class deltas too.  (Not asserted for the IoU losses: where a box encloses the other along an
        # axis, the gradient of a centre is a sum of two corner gradients that cancel, exactly or to the last bits)
        assert torch.equal(dpred[own] == 0, r64["grad"][own] == 0)
    if own.any():
        # the regression gradients on their own scale (in 'grad' the larger cross-entropy gradients set it)
        dist.add("dreg", dpred[own], r32["grad"][own], r64["grad"][own], scale=_scale(r64["grad"][own]))
    if val.any():
        dist.add("grad", dpred[val], r32["grad"][val], r64["grad"][val], scale=_scale(r64["grad"]))
    if kind == "smooth_l1" and beta < 1e-5:
        # the L1 branch of the new kernels against the L1 kernels of the default configuration: the same values
        s0 = det.box_loss_fwd(*args)
        assert torch.equal(s0.cpu(), s)
        assert torch.equal(det.box_loss_bwd(*args, s0, gc, gr).cpu(), dpred)
    return inp, s, dpred, r64


def _run_box_mixed(dev, K, kind, beta):
    dist = _Dist()
    inp, s, dpred, r64 = _run_box(dev, K, "mixed", kind, beta, dist)
    cls, pl, dec = inp["cls"], inp["planted"], r64["dec"]
    at = {r: i for i, r in enumerate(r64["fg_rows"])}
    assert 0 < s[3] < s[2] < BOX_R and int((cls < 0).sum()) > 20

    def own(name):
        r = pl[name]
        c = int(cls[r])
        return dpred[r, K + 1 + 4 * c:K + 5 + 4 * c]

    if kind == "smooth_l1":
        g = own("exact")
        assert g[0] == 0 and g[2] == 0 and g[1] != 0 and g[3] != 0                               # x == y: gradient exactly 0
        g, i = own("beta"), at[pl["beta"]]
        assert g[1] == 0 and dec["sign"][i].tolist()[1] == 0
        if beta >= 1e-5:
            assert dec["quad"][i].tolist() == [False, True, False, True]                         # |x - y| == beta: the linear branch
            assert g[0] > 0 and g[2] == -g[0]                                                    # sign(x - y) * g_reg / n
            assert 0 < int(dec["quad"].sum()) < dec["quad"].numel()
    else:
        i = at[pl["clamp"]]
        assert dec["clamp"][i].tolist() == [True, False] and int(dec["clamp"].sum()) == 1
        g = own("clamp")
        assert g[2] == 0 and g[3] != 0                                                         # the clamped delta: gradient exactly 0
        i = at[pl["disjoint"]]
        assert not dec["mask"][i] and 0 < int(dec["mask"].sum())
        if kind in ("giou", "diou"):
            assert bool((own("disjoint") != 0).all())                                            # I = 0: the enclosing-box terms still pull
        assert dec["side"][at[pl["pred_in_gt"]]].tolist() == [1, 1, -1, -1]
        assert dec["side"][at[pl["gt_in_pred"]]].tolist() == [-1, -1, 1, 1]
        assert float(r64["per"].min()) >= 0 and float(r64["per"].max()) < (3.0 if kind == "ciou" else 2.0)
    dist.report("box_reg %s beta %g K=%d %s" % (kind, beta, K, dev))


def _run_box_degenerate(dev, kind, beta):
    dist = _Dist()
    for K in BOX_KS:
        inp, s, dpred, r64 = _run_box(dev, K, "no_fg", kind, beta, dist)
        assert s[1] == 0 and s[3] == 0 and s[2] > 0 and not dpred[:, K + 1:].any()               # no foreground row: no delta gradient
        inp, s, dpred, r64 = _run_box(dev, K, "ignored", kind, beta, dist)
        assert not s.any() and not dpred.any()                                                   # max(n, 1): nothing non-finite, all 0
    dist.report("box_reg %s beta %g degenerate %s" % (kind, beta, dev))


@pytest.mark.parametrize("kind,beta", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("K", BOX_KS)
def test_box_reg_loss_emulated(emu_lib, K, kind, beta):
    _run_box_mixed("cpu", K, kind, beta)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,beta", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("K", BOX_KS)
def test_box_reg_loss_gpu(hip_lib, K, kind, beta):
    _run_box_mixed("cuda", K, kind, beta)


@pytest.mark.parametrize("kind,beta", VARIANTS, ids=VARIANT_IDS)
def test_box_reg_loss_degenerate_emulated(emu_lib, kind, beta):
    _run_box_degenerate("cpu", kind, beta)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,beta", VARIANTS, ids=VARIANT_IDS)
def test_box_reg_loss_degenerate_gpu(hip_lib, kind, beta):
    _run_box_degenerate("cuda", kind, beta)


# ---- 2. RPN (omni_rpn_reg_loss_fwd / _bwd) ----------------------------------------------------------------------------------------------
# 'big': B * A = 2 * 66 510 = 133 020 > 256 * 512 threads of the capped forward grid: its first workgroups take a second trip
RPN_CASES = {"big": (2, [(104, 160), (52, 80), (26, 40), (13, 20), (7, 10)], [32, 64, 128, 256, 512], [4, 8, 16, 32, 64]),
             "tiny": (2, [(4, 4), (2, 2), (1, 1)], [16, 32, 64], [4, 8, 16])}
RPN_G_CLS, RPN_G_LOC = 2.0, 0.5
RPN_VARIANTS = [(False, "smooth_l1", 0.5)] + [(True, k, b) for k, b in VARIANTS]
RPN_IDS = ["IoUness-smooth_l1-0.5"] + ["none-" + i for i in VARIANT_IDS]


@functools.lru_cache(maxsize=None)
def _rpn_case(name):
    """level tensors (B, H, W, 16) = [3 logits | 12 deltas | NaN pad], labels in {-1, 0, 1}, one jittered ground-truth box per positive
    anchor (every 7th positive is matched to its neighbour's box instead: mostly disjoint), planted rows in image 0 of 'big'"""
    B, hw, sizes, strides = RPN_CASES[name]
    g = torch.Generator().manual_seed(900 + len(hw))
    anchors = _anchors(sizes, strides, hw)
    A = anchors.shape[0]
    a_off = [0]
    for h, w in hw:
        a_off.append(a_off[-1] + 3 * h * w)
    levels = [torch.randn(B, h, w, 16, generator=g) * 0.5 for h, w in hw]
    for t in levels:
        t[..., 15] = NAN
    labels = torch.full((B, A), -1, dtype=torch.int8)
    midx = torch.zeros(B, A, dtype=torch.int32)
    npos = min(48, A // 4)
    gts, planted = [], {}

    def jitter(box):
        w, h = box[2] - box[0], box[3] - box[1]
        u = torch.rand(4, generator=g)
        cx, cy = (box[0] + box[2]) / 2 + (u[0] - 0.5) * 0.4 * w, (box[1] + box[3]) / 2 + (u[1] - 0.5) * 0.4 * h
        w, h = w * torch.exp((u[2] - 0.5) * 0.6), h * torch.exp((u[3] - 0.5) * 0.6)
        return torch.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2])

    def set_deltas(n, a, deltas):
        l = max(i for i in range(len(hw)) if a_off[i] <= a)
        loc, k = divmod(a - a_off[l], 3)
        y, x = divmod(loc, hw[l][1])
        levels[l][n, y, x, 3 + 4 * k:7 + 4 * k] = torch.tensor(deltas)

    for n in range(B):
        perm = torch.randperm(A, generator=g)
        pos, neg = perm[:npos], perm[npos:3 * npos]
        labels[n, pos], labels[n, neg] = 1, 0
        boxes = [jitter(anchors[a]) for a in pos.tolist()]
        for j, a in enumerate(pos.tolist()):
            midx[n, a] = j + 1 if (j % 7 == 6 and j + 1 < npos) else j
        if name == "big" and n == 0:
            def plant(tag, a, gt, deltas):
                labels[0, a], midx[0, a] = 1, len(boxes)
                boxes.append(gt)
                set_deltas(0, a, deltas)
                planted[tag] = a

            def ab(a):
                x1, y1, x2, y2 = anchors[a].tolist()
                return x1, y1, x2, y2, x2 - x1, y2 - y1, (x1 + x2) / 2, (y1 + y2) / 2

            base = a_off[2]                                                   # the 128 px anchors
            x1, y1, x2, y2, w, h, cx, cy = ab(base + 31)
            plant("clamp", base + 31, jitter(anchors[base + 31]), [0.1, -0.1, CLAMP + 0.5, 0.2])
            x1, y1, x2, y2, w, h, cx, cy = ab(base + 602)
            plant("disjoint", base + 602, torch.tensor([x1 + 3 * w, y1, x2 + 3 * w, y2]), [0.2, 0.1, 0.1, -0.1])
            x1, y1, x2, y2, w, h, cx, cy = ab(base + 1500)
            plant("pred_in_gt", base + 1500, torch.tensor([x1 - 0.3 * w, y1 - 0.3 * h, x2 + 0.3 * w, y2 + 0.3 * h]), [0.02, -0.03, -0.1, -0.1])
            x1, y1, x2, y2, w, h, cx, cy = ab(base + 2411)
            plant("gt_in_pred", base + 2411, torch.tensor([cx - 0.2 * w, cy - 0.3 * h, cx + 0.3 * w, cy + 0.2 * h]), [0.01, 0.02, 0.1, 0.1])
            # ground truth == anchor: every target delta is exactly 0; x == y in dx, |x - y| == beta = 0.5 in dy and dw
            plant("beta", base + 2900, anchors[base + 2900].clone(), [0.0, 0.5, -0.5, 0.25])
            x1, y1, x2, y2, w, h, cx, cy = ab(base + 3052)
            plant("elongated", base + 3052, torch.tensor([cx - 2 * w, cy - 0.02 * h, cx + 2 * w, cy + 0.02 * h]), [0.1, 0.1, 0.2, -0.2])
        gts.append(torch.stack(boxes))
    gt_off = torch.tensor([0] + [int(x) for x in torch.tensor([len(b) for b in gts]).cumsum(0)], dtype=torch.int32)
    return {"B": B, "hw": hw, "anchors": anchors, "levels": levels, "labels": labels, "midx": midx, "gt": torch.cat(gts), "gt_off": gt_off,
            "planted": planted, "inv_norm": 1.0 / (64 * B)}


def _rpn_ref(case, plain, kind, beta, dtype):
    B, anchors, labels = case["B"], case["anchors"], case["labels"]
    lv = [t.to(dtype).clone().requires_grad_(True) for t in case["levels"]]
    x = torch.cat([t[..., :3].reshape(B, -1) for t in lv], dim=1)
    deltas = torch.cat([t[..., 3:15].reshape(B, -1, 4) for t in lv], dim=1)
    pos = labels == 1
    n_i, a_i = torch.nonzero(pos, as_tuple=True)
    src = anchors[a_i].to(dtype)
    gt = case["gt"][(case["gt_off"][n_i] + case["midx"][n_i, a_i]).long()].to(dtype)
    per, dec = _reg_loss(kind, beta, deltas[n_i, a_i], src, gt, (1.0, 1.0, 1.0, 1.0))
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    if plain:
        valid = labels >= 0
        cls, loc = bce(x[valid], pos[valid].to(dtype), reduction="sum"), per.sum()
    else:
        iw = (torch.min(src[:, 2], gt[:, 2]) - torch.max(src[:, 0], gt[:, 0])).clamp(min=0)
        ih = (torch.min(src[:, 3], gt[:, 3]) - torch.max(src[:, 1], gt[:, 1])).clamp(min=0)
        area = lambda b: (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        t = iw * ih / (area(src) + area(gt) - iw * ih)
        cls, loc = (bce(x[pos], t, reduction="none") * t).sum(), (per * t).sum()
        dec["overlap"] = t > 0
    ((RPN_G_CLS * cls + RPN_G_LOC * loc) * case["inv_norm"]).backward()
    sg = torch.sigmoid(x.detach())
    return {"loss": torch.stack([cls.detach(), loc.detach()]) * case["inv_norm"], "grads": [t.grad for t in lv], "dec": dec,
            "counts": [int(pos.sum()), int((labels == 0).sum())], "conf": torch.stack([sg[pos].sum(), sg[~pos].sum()]),
            "rows": list(zip(n_i.tolist(), a_i.tolist()))}


def _run_rpn(dev, name, plain, kind, beta):
    from omni3d_amd.kernels import det
    case = _rpn_case(name)
    r64, r32 = _rpn_ref(case, plain, kind, beta, torch.float64), _rpn_ref(case, plain, kind, beta, torch.float32)
    _same_decisions(r64["dec"], r32["dec"])
    dist = _Dist()
    pack = det.LevelPack([t.to(dev) for t in case["levels"]])
    args = [pack] + [case[k].to(dev) for k in ("anchors", "labels", "midx", "gt", "gt_off")]
    s = det.rpn_loss_fwd(*args, plain, kind, beta).cpu()
    assert s.dtype == torch.float64 and bool(torch.isfinite(s).all())
    assert s[2:4].tolist() == [float(c) for c in r64["counts"]]
    dist.add("loss", s[:2] * case["inv_norm"], r32["loss"], r64["loss"])
    dist.add("conf", s[4:6], r32["conf"], r64["conf"])
    gc, gl = torch.tensor([RPN_G_CLS]).to(dev), torch.tensor([RPN_G_LOC]).to(dev)
    grads = [t.cpu() for t in det.rpn_loss_bwd(*args, gc, gl, case["inv_norm"], plain, kind, beta)]
    for got, g32, g64 in zip(grads, r32["grads"], r64["grads"]):
        # every element of every level gradient; the pad channel and everything the reference leaves at 0: exactly 0
        assert got.shape == g64.shape and bool(torch.isfinite(got).all()) and not got[..., 15].any()
        assert torch.equal(got[..., :3] == 0, g64[..., :3] == 0)
        dist.add("grad", got, g32, g64, scale=_scale(g64))
    pos = case["labels"] == 1
    ddel, rdel = [torch.cat([t[..., 3:15].reshape(case["B"], -1, 4) for t in gs], dim=1) for gs in (grads, r64["grads"])]
    assert not ddel[~pos].any()                                                                  # deltas of anchors that are not positive
    r32del = torch.cat([t[..., 3:15].reshape(case["B"], -1, 4) for t in r32["grads"]], dim=1)
    dist.add("ddel", ddel[pos], r32del[pos], rdel[pos], scale=_scale(rdel[pos]))                 # the delta gradients on their own scale
    if kind == "smooth_l1":
        assert torch.equal(ddel[pos] == 0, rdel[pos] == 0)       # (IoU losses: centre gradients may cancel exactly or to the last bits)
    if kind == "smooth_l1" and beta < 1e-5:
        # the L1 branch of the new kernels against the L1 kernels of the default configuration: the same values
        assert torch.equal(det.rpn_loss_fwd(*args, plain).cpu(), s)
        for a, b in zip(det.rpn_loss_bwd(*args, gc, gl, case["inv_norm"], plain), grads):
            assert torch.equal(a.cpu(), b)
    dec, pl = r64["dec"], case["planted"]
    at = {(n, a): i for i, (n, a) in enumerate(r64["rows"])}
    deltas = ddel
    if name == "big":
        assert case["B"] * case["anchors"].shape[0] > 256 * 512
        if kind == "smooth_l1":
            i, g = at[(0, pl["beta"])], deltas[0, pl["beta"]]
            assert dec["sign"][i].tolist() == [0, 1, -1, 1] and g[0] == 0 and bool((g[1:] != 0).all())
            if beta >= 1e-5:
                assert dec["quad"][i].tolist() == [True, False, False, True] and g[2] == -g[1]   # |x - y| == beta: the linear branch
                assert 0 < int(dec["quad"].sum()) < dec["quad"].numel()
            if not plain:
                assert 0 < int(dec["overlap"].sum()) < dec["overlap"].numel()                    # t == 0 rows and weighted rows
        else:
            i, g = at[(0, pl["clamp"])], deltas[0, pl["clamp"]]
            assert dec["clamp"][i].tolist() == [True, False] and int(dec["clamp"].sum()) == 1
            assert g[2] == 0 and g[3] != 0                                                         # the clamped delta: gradient exactly 0
            assert not dec["mask"][at[(0, pl["disjoint"])]] and 0 < int(dec["mask"].sum()) < dec["mask"].numel()
            if kind in ("giou", "diou"):
                assert bool((deltas[0, pl["disjoint"]] != 0).all())
            assert dec["side"][at[(0, pl["pred_in_gt"])]].tolist() == [1, 1, -1, -1]
            assert dec["side"][at[(0, pl["gt_in_pred"])]].tolist() == [-1, -1, 1, 1]
    dist.report("rpn_reg %s %s beta %g %s %s" % ("none" if plain else "IoUness", kind, beta, name, dev))


@pytest.mark.parametrize("plain,kind,beta", RPN_VARIANTS, ids=RPN_IDS)
@pytest.mark.parametrize("name", ["big", "tiny"])
def test_rpn_reg_loss_emulated(emu_lib, name, plain, kind, beta):
    _run_rpn("cpu", name, plain, kind, beta)


@pytest.mark.gpu
@pytest.mark.parametrize("plain,kind,beta", RPN_VARIANTS, ids=RPN_IDS)
@pytest.mark.parametrize("name", ["big", "tiny"])
def test_rpn_reg_loss_gpu(hip_lib, name, plain, kind, beta):
    _run_rpn("cuda", name, plain, kind, beta)


# ---- 3. the default configuration: the same entry points, the same bits -----------------------------------------------------------------
def test_default_arguments_reach_the_l1_entry_points(emu_lib, monkeypatch):
    """`box_loss` / `rpn_loss` with default arguments call the C entry points they called before the regression options existed and
    return bit-identical sums and gradients to the wrappers called as before"""
    import omni3d_amd.functional as HF
    from omni3d_amd.kernels import det
    called = []
    real = emu_lib.call
    monkeypatch.setattr(emu_lib, "call", lambda name, *a: (called.append(name), real(name, *a))[1])
    loss_calls = lambda: [n for n in called if "loss" in n]

    inp = _box_case(7, "mixed", False)
    K = inp["K"]
    args = [K] + [inp[k] for k in ("cls", "prop", "gtb", "gt_row")]
    pred = inp["pred"].clone().requires_grad_(True)
    vec, sums = HF.box_loss(pred, *args)
    (G_CLS * vec[0] + G_REG * vec[1]).backward()
    assert loss_calls() == ["omni_box_loss_fwd", "omni_box_loss_bwd"]
    s0 = det.box_loss_fwd(inp["pred"], *args)
    assert torch.equal(sums, s0)
    assert torch.equal(pred.grad, det.box_loss_bwd(inp["pred"], *args, s0, torch.tensor([G_CLS]), torch.tensor([G_REG])))

    case = _rpn_case("tiny")
    targs = [case[k] for k in ("anchors", "labels", "midx", "gt", "gt_off")]
    for plain, names in ((False, ["omni_rpn_loss_fwd", "omni_rpn_loss_bwd"]), (True, ["omni_rpn_loss_plain_fwd", "omni_rpn_loss_plain_bwd"])):
        del called[:]
        lv = [t.clone().permute(0, 3, 1, 2).requires_grad_(True) for t in case["levels"]]           # (B, 16, H, W), channels last
        vec, sums = HF.rpn_loss(lv, *targs, case["inv_norm"], plain=plain)
        (RPN_G_CLS * vec[0] + RPN_G_LOC * vec[1]).backward()
        assert loss_calls() == names
        pack = det.LevelPack(list(case["levels"]))
        assert torch.equal(sums, det.rpn_loss_fwd(pack, *targs, plain))
        old = det.rpn_loss_bwd(pack, *targs, torch.tensor([RPN_G_CLS]), torch.tensor([RPN_G_LOC]), case["inv_norm"], plain)
        for t, o in zip(lv, old):
            assert torch.equal(t.grad.permute(0, 2, 3, 1), o)
    # and a non-default value reaches the new ones
    del called[:]
    vec, _ = HF.box_loss(inp["pred"].clone().requires_grad_(True), *args, reg_type="giou")
    vec.sum().backward()
    assert loss_calls() == ["omni_box_reg_loss_fwd", "omni_box_reg_loss_bwd"]


# ---- 4. construction ------------------------------------------------------------------------------------------------------------------------
def _rpn_module(**kw):
    from omni3d_amd.cubercnn.modeling.proposal_generator.rpn import RPNWithIgnore
    return RPNWithIgnore(in_features=["p2"], head=torch.nn.Identity(), anchor_generator=None, anchor_thresholds=[0.05, 0.05],
                         anchor_labels=[0, -1, 1], batch_size_per_image=64, positive_fraction=0.5, pre_nms_topk=(10, 10),
                         post_nms_topk=(10, 10), **kw)


def _box_module(**kw):
    from omni3d_amd.cubercnn.modeling.roi_heads.fast_rcnn import FastRCNNOutputs
    return FastRCNNOutputs(16, box2box_weights=WEIGHTS, num_classes=5, **kw)


def test_accepted_configurations_build():
    for kind, beta in VARIANTS + [("smooth_l1", 0.0)]:
        m = _box_module(box_reg_loss_type=kind, smooth_l1_beta=beta)
        assert (m.box_reg_loss_type, m.smooth_l1_beta) == (kind, beta)
        m = _rpn_module(box_reg_loss_type=kind, smooth_l1_beta=beta, objectness_uncertainty="none")
        assert (m.box_reg_loss_type, m.smooth_l1_beta, m.plain_objectness) == (kind, beta, True)
    for beta in (0.0, 1e-6, 0.5):
        m = _rpn_module(box_reg_loss_type="smooth_l1", smooth_l1_beta=beta, objectness_uncertainty="IoUness")
        assert (m.box_reg_loss_type, m.smooth_l1_beta, m.plain_objectness) == ("smooth_l1", beta, False)


def test_refused_configurations_raise():
    for kind in IOU_KINDS:
        with pytest.raises(ValueError, match="Invalid dense box regression loss type '%s'" % kind):
            _rpn_module(box_reg_loss_type=kind, objectness_uncertainty="IoUness")
    with pytest.raises(ValueError, match="Invalid dense box regression loss type 'l2'"):
        _rpn_module(box_reg_loss_type="l2", objectness_uncertainty="none")
    with pytest.raises(ValueError, match="Invalid bbox reg loss type 'l2'"):
        _box_module(box_reg_loss_type="l2")
    with pytest.raises(NotImplementedError, match="CLS_AGNOSTIC_BBOX_REG"):
        _box_module(cls_agnostic_bbox_reg=True)
    with pytest.raises(NotImplementedError, match="CLS_AGNOSTIC_BBOX_REG"):
        _box_module(cls_agnostic_bbox_reg=True, box_reg_loss_type="giou")
