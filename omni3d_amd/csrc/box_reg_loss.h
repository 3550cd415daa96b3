// box_reg_loss.h -- the box regression losses of both detector stages for one (source box, predicted deltas, ground-truth box)
// triple: value and gradient wrt the four deltas.  One definition shared by csrc/box_loss.hip (MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_TYPE /
// SMOOTH_L1_BETA; source box = proposal) and csrc/rpn_roi.hip (MODEL.RPN.*; source box = anchor).
//
// Reference: smooth-L1 with beta -- fast_rcnn.py:245-252 (box head), rpn.py:258-268 (RPN, IoUness), detectron2
// _dense_box_regression_loss (RPN, OBJECTNESS_UNCERTAINTY none); giou / diou / ciou -- fvcore giou_loss, diou_loss, ciou_loss on
// Box2BoxTransform.apply_deltas of the predicted deltas, as _dense_box_regression_loss (RPN) and detectron2's
// FastRCNNOutputLayers.box_reg_loss (box head: an extension over the reference, whose box head only evaluates smooth_l1) call them.
#pragma once
#include <device_rt.h>
#include "box_decode.h"

enum { OMNI_BOX_REG_SMOOTH_L1 = 0, OMNI_BOX_REG_GIOU = 1, OMNI_BOX_REG_DIOU = 2, OMNI_BOX_REG_CIOU = 3 };

// Box2BoxTransform.get_deltas
__device__ __forceinline__ void omni_get_deltas(const float* pb, const float* gb, float wx, float wy, float ww, float wh, float (&d)[4]) {
    const float sw = pb[2] - pb[0], sh = pb[3] - pb[1], scx = pb[0] + 0.5f * sw, scy = pb[1] + 0.5f * sh;
    const float tw = gb[2] - gb[0], th = gb[3] - gb[1], tcx = gb[0] + 0.5f * tw, tcy = gb[1] + 0.5f * th;
    d[0] = wx * (tcx - scx) / sw; d[1] = wy * (tcy - scy) / sh; d[2] = ww * logf(tw / sw); d[3] = wh * logf(th / sh);
}

// fvcore smooth_l1_loss: beta < 1e-5 is L1; the quadratic branch holds for |x - y| < beta (strict).  g = d/dx (0 at x == y).
template <bool GRAD>
__device__ __forceinline__ float omni_smooth_l1(float x, float y, float beta, float& g) {
    const float df = x - y, n = fabsf(df);
    const bool quad = beta >= 1e-5f && n < beta;
    if (GRAD) g = quad ? df / beta : (df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f));
    return quad ? 0.5f * n * n / beta : (beta >= 1e-5f ? n - 0.5f * beta : n);
}

// torch's subgradient of maximum(a, b) wrt a (minimum(a, b): swap the operands): 1 where a wins, 1/2 on a tie
__device__ __forceinline__ float omni_wins(float a, float b) { return a > b ? 1.f : (a == b ? 0.5f : 0.f); }

// fvcore giou_loss / diou_loss / ciou_loss (eps 1e-7) of the box p against g, both XYXY; gb = gradient wrt the corners of p
template <bool GRAD>
__device__ __forceinline__ float omni_iou_loss(int type, const float (&p)[4], const float* g, float (&gb)[4]) {
    const float eps = 1e-7f;
    const float wp = p[2] - p[0], hp = p[3] - p[1], wg = g[2] - g[0], hg = g[3] - g[1];
    const float xk1 = fmaxf(p[0], g[0]), yk1 = fmaxf(p[1], g[1]), xk2 = fminf(p[2], g[2]), yk2 = fminf(p[3], g[3]);
    const float iw = xk2 - xk1, ih = yk2 - yk1;
    const bool hit = xk2 > xk1 && yk2 > yk1;
    const float I = hit ? iw * ih : 0.f;
    const float cw = fmaxf(p[2], g[2]) - fminf(p[0], g[0]), ch = fmaxf(p[3], g[3]) - fminf(p[1], g[1]);
    const float S = wp * hp + wg * hg - I;                       // union without its eps
    // derivatives wrt (x1, y1, x2, y2) of p: intersection, own area, enclosing width and height
    float dI[4] = {0.f, 0.f, 0.f, 0.f}, dA[4], dcw[4], dch[4];
    if (GRAD) {
        if (hit) {
            dI[0] = -ih * omni_wins(p[0], g[0]); dI[1] = -iw * omni_wins(p[1], g[1]);
            dI[2] = ih * omni_wins(g[2], p[2]);  dI[3] = iw * omni_wins(g[3], p[3]);
        }
        dA[0] = -hp; dA[1] = -wp; dA[2] = hp; dA[3] = wp;
        dcw[0] = -omni_wins(g[0], p[0]); dcw[1] = 0.f; dcw[2] = omni_wins(p[2], g[2]); dcw[3] = 0.f;
        dch[0] = 0.f; dch[1] = -omni_wins(g[1], p[1]); dch[2] = 0.f; dch[3] = omni_wins(p[3], g[3]);
    }
    if (type == OMNI_BOX_REG_GIOU) {
        const float U = S + eps, iou = I / U, C = cw * ch, Ce = C + eps;
        if (GRAD) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float dU = dA[q] - dI[q], dC = dcw[q] * ch + cw * dch[q];
                gb[q] = (dC * U - dU * Ce) / (Ce * Ce) - (dI[q] * U - I * dU) / (U * U);
            }
        }
        return 1.f - iou + (C - S) / Ce;
    }
    const float U = S + eps, iou = I / U;
    const float diag = cw * cw + ch * ch + eps;
    const float ex = (p[0] + p[2]) / 2.f - (g[0] + g[2]) / 2.f, ey = (p[1] + p[3]) / 2.f - (g[1] + g[3]) / 2.f;
    const float dist = ex * ex + ey * ey;
    float loss = 1.f - iou + dist / diag;
    if (GRAD) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float dU = dA[q] - dI[q], ddiag = 2.f * (cw * dcw[q] + ch * dch[q]), ddist = (q & 1) ? ey : ex;
            gb[q] = (ddist * diag - dist * ddiag) / (diag * diag) - (dI[q] * U - I * dU) / (U * U);
        }
    }
    if (type == OMNI_BOX_REG_CIOU) {
        const float k = 0.405284734569351086f;                   // 4 / pi^2
        const float da = atanf(wg / hg) - atanf(wp / hp);
        const float v = k * (da * da);
        const float alpha = v / (1.f - iou + v + eps);           // a constant of the backward pass (no_grad)
        loss += alpha * v;
        if (GRAD) {
            const float s = alpha * 2.f * k * da / (wp * wp + hp * hp);      // -d(alpha v)/d atan(wp/hp) / (wp^2 + hp^2)
            gb[0] += s * hp; gb[1] -= s * wp; gb[2] -= s * hp; gb[3] += s * wp;
        }
    }
    return loss;
}

// One pair.  type, beta: the configured loss; d: the four predicted deltas; src: proposal / anchor; gt: its ground-truth box;
// scale_clamp: Box2BoxTransform's bound on dw, dh (IoU types).  v: the loss as four terms -- smooth-L1 per delta, IoU types
// (loss, 0, 0, 0) -- so the caller adds them in the order of the L1 kernel it stands beside.  g: gradient wrt d.
template <bool GRAD>
__device__ __forceinline__ void omni_box_reg_pair(int type, float beta, float scale_clamp, const float* d, const float* src,
                                                  const float* gt, float wx, float wy, float ww, float wh, float (&v)[4], float (&g)[4]) {
    // (scalars, not v / g, are written under the branch: stores to different elements of one array from two branches get merged into
    //  one store at a variable index, which puts the array into scratch)
    float v0, v1 = 0.f, v2 = 0.f, v3 = 0.f, g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f;
    if (type == OMNI_BOX_REG_SMOOTH_L1) {
        float gd[4];
        omni_get_deltas(src, gt, wx, wy, ww, wh, gd);
        v0 = omni_smooth_l1<GRAD>(d[0], gd[0], beta, g0);
        v1 = omni_smooth_l1<GRAD>(d[1], gd[1], beta, g1);
        v2 = omni_smooth_l1<GRAD>(d[2], gd[2], beta, g2);
        v3 = omni_smooth_l1<GRAD>(d[3], gd[3], beta, g3);
    } else {
        float p[4], gb[4], pw, ph;
        omni_apply_deltas(d, src, wx, wy, ww, wh, scale_clamp, p, pw, ph);
        v0 = omni_iou_loss<GRAD>(type, p, gt, gb);
        if (GRAD) {
            // through apply_deltas; torch.clamp passes the gradient where d / w <= clamp
            g0 = (gb[0] + gb[2]) * (src[2] - src[0]) / wx;
            g1 = (gb[1] + gb[3]) * (src[3] - src[1]) / wy;
            g2 = d[2] / ww <= scale_clamp ? 0.5f * (gb[2] - gb[0]) * pw / ww : 0.f;
            g3 = d[3] / wh <= scale_clamp ? 0.5f * (gb[3] - gb[1]) * ph / wh : 0.f;
        }
    }
    v[0] = v0; v[1] = v1; v[2] = v2; v[3] = v3;
    if (GRAD) { g[0] = g0; g[1] = g1; g[2] = g2; g[3] = g3; }
}
