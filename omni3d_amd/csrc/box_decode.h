// box_decode.h -- Box2BoxTransform.apply_deltas of one row's GT-class deltas on its proposal box (detectron2
// FastRCNNOutputLayers.predict_boxes_for_gt_classes; reference roi_heads.py:276-289), unclipped.  One definition shared by
// csrc/box_loss.hip (TRAIN_ON_PRED_BOXES), csrc/train_vis.hip (the training-time drawings) and csrc/box_reg_loss.h (the IoU
// regression losses of both stages), so all give the same bits.
#pragma once
#include <device_rt.h>

// d: the four deltas (dx, dy, dw, dh); pb: the source box XYXY; o: the predicted box XYXY; pw, ph: its width and height before the
// corners are rounded (the factors of the gradient wrt dw, dh)
__device__ __forceinline__ void omni_apply_deltas(const float* __restrict__ d, const float* __restrict__ pb, float wx, float wy, float ww,
                                                  float wh, float scale_clamp, float* __restrict__ o, float& pw, float& ph) {
    const float w = pb[2] - pb[0], h = pb[3] - pb[1], cx = pb[0] + 0.5f * w, cy = pb[1] + 0.5f * h;
    const float dx = d[0] / wx, dy = d[1] / wy, dw = fminf(d[2] / ww, scale_clamp), dh = fminf(d[3] / wh, scale_clamp);
    const float pcx = dx * w + cx, pcy = dy * h + cy;
    pw = expf(dw) * w;
    ph = expf(dh) * h;
    o[0] = pcx - 0.5f * pw; o[1] = pcy - 0.5f * ph; o[2] = pcx + 0.5f * pw; o[3] = pcy + 0.5f * ph;
}

// pred_row: one row of pred (R, ldp) = [K+1 logits | 4K deltas]; pb: the proposal box XYXY; c: the row's class, clamped here to
// [0, K-1] (gt_classes.clamp_(0, K - 1): background rows use the last class); o: the predicted box XYXY
__device__ __forceinline__ void omni_decode_gt_class_box(const float* __restrict__ pred_row, int K, int c, const float* __restrict__ pb,
                                                         float wx, float wy, float ww, float wh, float scale_clamp, float* __restrict__ o) {
    c = c > K - 1 ? K - 1 : c;
    float pw, ph;
    omni_apply_deltas(pred_row + (K + 1) + 4 * c, pb, wx, wy, ww, wh, scale_clamp, o, pw, ph);
}
