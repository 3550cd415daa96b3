// train_vis.hip -- the selection behind the training-time drawings (`RCNN3D.visualize_training`, every VIS_PERIOD iterations): which
// of an image's foreground rows the reference would draw as predicted cuboids.  One launch replaces, for the training-mode rows,
//   predict_boxes_for_gt_classes                                  (reference roi_heads.py:276-281)
//   scores = exp(-uncertainty of the GT class)                    (roi_heads.py:782-805)
//   batched_nms(pred_boxes, scores, zeros, test_nms_thresh)[:20]  (rcnn3d.py:207-214)
//
//   train_vis_pick_kernel  one 256-thread workgroup per image.  (1) every foreground row's GT-class box (csrc/box_decode.h, the
//                          arithmetic of omni_box_decode_gt_class, unclipped) and score expf(-uncert) go to LDS; (2) a bitonic
//                          network sorts 64-bit keys [~score bits | row], padded to a power of two, so the order is descending score
//                          with ties to the lower row; (3) greedy NMS over the sorted list: the next live row is kept, the threads
//                          stride over the rows behind it and mark those with IoU > iou_thr (float32, torchvision's box_iou: areas
//                          (x2 - x1) * (y2 - y1), no +1); it stops once max_keep rows are kept; (4) the unused slots are filled.
// No atomics, no scratch, no arrival order: every key is distinct, so the network's result and with it every output is a function
// of the inputs alone.  A row whose box or score is not finite (or whose class lies outside [0, K)) sorts behind every other row, is
// never kept and never suppresses.
#include <device_rt.h>
#include "box_decode.h"

namespace {

constexpr int TV_MAXF = 1024;                     // rows per image the LDS arrays hold
constexpr unsigned TV_INVALID = 0xFFFFFFFFu;      // high key word of padding and of rows that are never kept

struct TrainVisP {
    const float* pred;        // (B*S, ldp) = [K+1 logits | 4K deltas]
    const float* head;        // (B*Fc, ldh)
    const float* rois;        // (B, Fc, 4)
    const int* cls;           // (B, Fc)
    const int* nfg;           // (B)
    int ldp, ldh, uncert_off, S, Fc, K, max_keep;
    float wx, wy, ww, wh, scale_clamp, iou_thr;
    int* keep_row;            // (B, max_keep)
    int* keep_count;          // (B)
    float* keep_box;          // (B, max_keep, 4)
    float* keep_score;        // (B, max_keep)
};

__device__ __forceinline__ bool tv_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__global__ void __launch_bounds__(256) train_vis_pick_kernel(TrainVisP p) {
    __shared__ unsigned long long s_key[TV_MAXF];     // sorted: [~score bits | row]
    __shared__ float s_box[TV_MAXF * 4];              // by row
    __shared__ unsigned char s_dead[TV_MAXF];         // by sorted position
    const int t = threadIdx.x, b = blockIdx.x;
    int n = p.nfg[b];
    n = n < 0 ? 0 : n;
    n = n > p.Fc ? p.Fc : n;
    n = n > p.S ? p.S : n;
    int NP = 1;
    while (NP < n) NP <<= 1;
    // ---- 1. decode + score ----
    for (int j = t; j < NP; j += 256) {
        unsigned hi = TV_INVALID;
        if (j < n) {
            const int c = p.cls[(long)b * p.Fc + j];
            if (c >= 0 && c < p.K) {
                float* o = s_box + 4 * j;
                omni_decode_gt_class_box(p.pred + ((long)b * p.S + j) * p.ldp, p.K, c, p.rois + 4 * ((long)b * p.Fc + j), p.wx, p.wy,
                                         p.ww, p.wh, p.scale_clamp, o);
                const float score = p.uncert_off >= 0 ? expf(-p.head[((long)b * p.Fc + j) * p.ldh + p.uncert_off + c]) : 1.0f;
                // a finite score is >= 0 here, so its bit pattern grows with its value
                if (tv_finite(o[0]) && tv_finite(o[1]) && tv_finite(o[2]) && tv_finite(o[3]) && tv_finite(score) && score >= 0.0f)
                    hi = ~__float_as_uint(score);
            }
        }
        s_key[j] = ((unsigned long long)hi << 32) | (unsigned)j;
        s_dead[j] = 0;
    }
    __syncthreads();
    // ---- 2. bitonic sort, ascending keys = descending score, ties to the lower row ----
    for (int k = 2; k <= NP; k <<= 1) {
        for (int jj = k >> 1; jj > 0; jj >>= 1) {
            for (int i = t; i < NP; i += 256) {
                const int l = i ^ jj;
                if (l > i) {
                    const unsigned long long a = s_key[i], c = s_key[l];
                    if ((a > c) == ((i & k) == 0)) { s_key[i] = c; s_key[l] = a; }
                }
            }
            __syncthreads();
        }
    }
    // ---- 3. greedy NMS over the sorted list (every thread walks the same `cur`, so the barriers are uniform) ----
    int cur = 0, kept = 0;
    while (kept < p.max_keep) {
        while (cur < n && (unsigned)(s_key[cur] >> 32) != TV_INVALID && s_dead[cur]) ++cur;
        if (cur >= n || (unsigned)(s_key[cur] >> 32) == TV_INVALID) break;            // the rows that are never kept sort last
        const unsigned long long key = s_key[cur];
        const int row = (int)(unsigned)key;
        const float x1 = s_box[4 * row], y1 = s_box[4 * row + 1], x2 = s_box[4 * row + 2], y2 = s_box[4 * row + 3];
        if (t == 0) {
            const long o = (long)b * p.max_keep + kept;
            p.keep_row[o] = row;
            p.keep_score[o] = __uint_as_float(~(unsigned)(key >> 32));
            p.keep_box[4 * o] = x1; p.keep_box[4 * o + 1] = y1; p.keep_box[4 * o + 2] = x2; p.keep_box[4 * o + 3] = y2;
        }
        ++kept;
        if (kept == p.max_keep) break;
        const float area = (x2 - x1) * (y2 - y1);
        for (int j = cur + 1 + t; j < n; j += 256) {
            const unsigned long long kj = s_key[j];
            if ((unsigned)(kj >> 32) == TV_INVALID || s_dead[j]) continue;
            const float* q = s_box + 4 * (int)(unsigned)kj;
            const float iw = fmaxf(fminf(x2, q[2]) - fmaxf(x1, q[0]), 0.0f), ih = fmaxf(fminf(y2, q[3]) - fmaxf(y1, q[1]), 0.0f);
            const float inter = iw * ih;
            const float iou = inter / (area + (q[2] - q[0]) * (q[3] - q[1]) - inter);
            if (iou > p.iou_thr) s_dead[j] = 1;
        }
        __syncthreads();
        ++cur;
    }
    // ---- 4. the unused slots ----
    for (int s = kept + t; s < p.max_keep; s += 256) {
        const long o = (long)b * p.max_keep + s;
        p.keep_row[o] = -1;
        p.keep_score[o] = 0.0f;
        p.keep_box[4 * o] = 0.0f; p.keep_box[4 * o + 1] = 0.0f; p.keep_box[4 * o + 2] = 0.0f; p.keep_box[4 * o + 3] = 0.0f;
    }
    if (t == 0) p.keep_count[b] = kept;
}

}  // namespace

extern "C" {

// pred (B*S, ldp), head (B*Fc, ldh), rois (B, Fc, 4), cls (B, Fc), nfg (B): image b uses pred rows b*S + j and head rows b*Fc + j for
// j < nfg[b] (clamped to [0, min(Fc, S)]).  uncert_off: column of the uncertainty block in a head row, -1 = no confidence (score 1).
// keep_row (B, max_keep) row j of the kept boxes in score order, -1 beyond keep_count (B); keep_box (B, max_keep, 4), keep_score
// (B, max_keep), zero beyond the count.
int omni_train_vis_pick(const float* pred, int ldp, const float* head, int ldh, int uncert_off, const float* rois, const int* cls,
                        const int* nfg, int B, int S, int Fc, int K, float wx, float wy, float ww, float wh, float scale_clamp,
                        float iou_thr, int max_keep, int* keep_row, int* keep_count, float* keep_box, float* keep_score, void* stream) {
    if (B < 0 || S <= 0 || Fc <= 0 || Fc > TV_MAXF || K <= 0 || ldp < 5 * K + 1 || max_keep <= 0 || uncert_off < -1
        || (uncert_off >= 0 && ldh < uncert_off + K))
        return OMNI_ERR_ARG;
    if (B == 0) return OMNI_OK;
    TrainVisP p{pred, head, rois, cls, nfg, ldp, ldh, uncert_off, S, Fc, K, max_keep, wx, wy, ww, wh, scale_clamp, iou_thr,
                keep_row, keep_count, keep_box, keep_score};
    hipLaunchKernelGGL(train_vis_pick_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, p);
    return omni_launch_status();
}

}  // extern "C"
