// vis_errors.hip -- the 3D error report of `visualize_from_instances` (reference cubercnn/vis/vis.py:95-171) for a whole dataset in
// one launch: every prediction of every image is matched to the same-category ground-truth box of its image with the largest 2D
// IoU (valid at IoU >= 0.5), and seven errors of the matched pairs are summed: projected centre (xy), depth (z), the three
// dimensions (w, h, l), their Euclidean norm (dim) and the relative rotation angle (ry).  The reference walks the predictions in
// a Python loop with one numpy IoU call each.
//
//   match_errors_kernel    one 256-thread workgroup per image; the image's ground-truth boxes (XYXY) and categories are staged
//                          through LDS in chunks of 64, the threads stride over the image's detections.  The two decisions (IoU
//                          against 0.5 and against the best so far; the trace against its bounds) are taken in float64, so they
//                          agree with a float64 evaluation of the float32 inputs; error terms in float32, per-thread sums in
//                          float64, reduced over the workgroup in a fixed tree (wave butterfly, then the four waves in order) into
//                          one row of 9 doubles per image: 7 sums, matched pairs, pairs with a valid ry.
//   match_errors_finalize  one workgroup of 9 waves, wave q adds column q of the per-image rows: lane l takes the images
//                          l, l + 64, ... in ascending order, then the same butterfly.
// No floating-point atomics and no arrival order anywhere: the order of every addition is a function of the indices alone, so two
// runs give the same bits.  Definitions (stated departures from the reference where noted):
//   IoU   plain XYXY intersection over union, no +1; a pair whose union is not positive has IoU 0 (the reference divides 0 by 0).
//   match the candidate with the largest IoU, the lowest row among equal ones (numpy argmax); -1 without candidates or below 0.5.
//   ry    so3_relative_angle(R_dt, R_gt, cos_bound=1) as read from pytorch3d's source: with that bound acos is replaced by its
//         tangent at 0 on both sides, ry = pi / 2 - (trace(R_dt R_gt^T) - 1) / 2; a trace outside [-1 - 1e-4, 3 + 1e-4] raises there
//         and the reference then leaves the pair out of ry alone: here ry = NaN and the pair is not counted for ry.
#include <device_rt.h>

namespace {

constexpr int CHUNK = 64;      // ground-truth boxes staged in LDS at a time
constexpr int NQ = 9;          // 7 error sums + matched pairs + pairs with a valid ry

struct MatchP {
    const float* dt_box;       // (D,4) XYWH
    const int* dt_cat;         // (D)
    const float* dt_c2d;       // (D,2)
    const float* dt_z;         // (D)
    const float* dt_dims;      // (D,3)
    const float* dt_pose;      // (D,9)
    const int* dt_off;         // (I+1)
    const float* gt_box;       // (G,4) XYWH
    const int* gt_cat;         // (G)
    const float* gt_center;    // (G,3)
    const float* gt_dims;      // (G,3)
    const float* gt_pose;      // (G,9)
    const int* gt_off;         // (I+1)
    const float* K;            // (I,9)
    int* match;                // (D)
    float* err;                // (D,7)
    double* partial;           // (I,NQ)
};

// the same sum in every lane; which lanes meet at which step depends on the lane numbers only
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__global__ void __launch_bounds__(256) match_errors_kernel(MatchP p) {
    __shared__ double s_box[CHUNK * 4];
    __shared__ int s_cat[CHUNK];
    __shared__ double s_red[4 * NQ];
    const int t = threadIdx.x, img = blockIdx.x;
    const int d0 = p.dt_off[img], d1 = p.dt_off[img + 1], g0 = p.gt_off[img], g1 = p.gt_off[img + 1];
    const float* K = p.K + 9L * img;
    const float nan = __int_as_float(0x7fc00000);
    double acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
    for (int base = d0; base < d1; base += 256) {          // the same trip count in every thread: the barriers below are uniform
        const int d = base + t;
        const bool active = d < d1;
        double x1 = 0.0, y1 = 0.0, x2 = 0.0, y2 = 0.0, area = 0.0;
        int cat = 0;
        if (active) {
            const float4 b = *reinterpret_cast<const float4*>(p.dt_box + 4L * d);
            x1 = b.x; y1 = b.y; x2 = x1 + (double)b.z; y2 = y1 + (double)b.w;
            area = (x2 - x1) * (y2 - y1);
            cat = p.dt_cat[d];
        }
        double best = -1.0;
        int bj = -1;
        for (int c0 = g0; c0 < g1; c0 += CHUNK) {
            const int n = min(CHUNK, g1 - c0);
            __syncthreads();                               // the previous chunk has been read by everyone
            if (t < n) {
                const float4 g = *reinterpret_cast<const float4*>(p.gt_box + 4L * (c0 + t));
                s_box[4 * t] = g.x; s_box[4 * t + 1] = g.y; s_box[4 * t + 2] = (double)g.x + (double)g.z; s_box[4 * t + 3] = (double)g.y + (double)g.w;
                s_cat[t] = p.gt_cat[c0 + t];
            }
            __syncthreads();
            if (active) {
                for (int j = 0; j < n; ++j) {
                    if (s_cat[j] != cat) continue;
                    const double gx1 = s_box[4 * j], gy1 = s_box[4 * j + 1], gx2 = s_box[4 * j + 2], gy2 = s_box[4 * j + 3];
                    const double iw = fmax(fmin(x2, gx2) - fmax(x1, gx1), 0.0), ih = fmax(fmin(y2, gy2) - fmax(y1, gy1), 0.0);
                    const double inter = iw * ih;
                    const double uni = area + (gx2 - gx1) * (gy2 - gy1) - inter;
                    const double iou = uni > 0.0 ? inter / uni : 0.0;
                    if (iou > best) { best = iou; bj = c0 + j; }          // ascending rows: the lowest row keeps a tie
                }
            }
        }
        if (!active) continue;
        const int m = best >= 0.5 ? bj : -1;
        p.match[d] = m;
        float e[7];
        if (m >= 0) {
            const float* c = p.gt_center + 3L * m;
            const float cx = c[0], cy = c[1], cz = c[2];
            const float u = (K[0] * cx + K[1] * cy + K[2] * cz) / cz, v = (K[3] * cx + K[4] * cy + K[5] * cz) / cz;
            const float du = p.dt_c2d[2L * d] - u, dv = p.dt_c2d[2L * d + 1] - v;
            e[0] = sqrtf(du * du + dv * dv);
            e[1] = fabsf(p.dt_z[d] - cz);
            const float dw = p.dt_dims[3L * d] - p.gt_dims[3L * m], dh = p.dt_dims[3L * d + 1] - p.gt_dims[3L * m + 1],
                        dl = p.dt_dims[3L * d + 2] - p.gt_dims[3L * m + 2];
            e[2] = fabsf(dw); e[3] = fabsf(dh); e[4] = fabsf(dl);
            e[5] = sqrtf(dw * dw + dh * dh + dl * dl);
            double tr = 0.0;                               // trace(R_dt R_gt^T) = sum of the element-wise products
#pragma unroll
            for (int k = 0; k < 9; ++k) tr += (double)p.dt_pose[9L * d + k] * (double)p.gt_pose[9L * m + k];
            const bool ok = tr >= -1.0 - 1e-4 && tr <= 3.0 + 1e-4;
            e[6] = ok ? 1.57079632679489662f - 0.5f * ((float)tr - 1.0f) : nan;
#pragma unroll
            for (int q = 0; q < 6; ++q) acc[q] += (double)e[q];
            if (ok) { acc[6] += (double)e[6]; acc[8] += 1.0; }
            acc[7] += 1.0;
        } else {
#pragma unroll
            for (int q = 0; q < 7; ++q) e[q] = nan;
        }
#pragma unroll
        for (int q = 0; q < 7; ++q) p.err[7L * d + q] = e[q];
    }
    // workgroup sum: butterfly inside each wave, then the four waves in order
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const double s = wave_sum_d(acc[q]);
        if ((t & 63) == 0) s_red[(t >> 6) * NQ + q] = s;
    }
    __syncthreads();
    if (t < NQ) p.partial[(long)img * NQ + t] = ((s_red[t] + s_red[NQ + t]) + s_red[2 * NQ + t]) + s_red[3 * NQ + t];
}

__global__ void __launch_bounds__(64 * NQ) match_errors_finalize(const double* __restrict__ partial, int I, double* __restrict__ sums,
                                                                 long long* __restrict__ counts) {
    const int q = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double s = 0.0;
    for (int i = lane; i < I; i += 64) s += partial[(long)i * NQ + q];
    s = wave_sum_d(s);
    if (lane == 0) {
        if (q < 7) sums[q] = s;
        else counts[q - 7] = (long long)s;                 // whole numbers far below 2^53: exact
    }
}

}  // namespace

extern "C" {

int omni_match_errors(const float* dt_box, const int* dt_cat, const float* dt_c2d, const float* dt_z, const float* dt_dims,
                      const float* dt_pose, const int* dt_off, const float* gt_box, const int* gt_cat, const float* gt_center,
                      const float* gt_dims, const float* gt_pose, const int* gt_off, const float* K, int I, int D, int G, int* match,
                      float* err, double* sums, long long* counts, double* workspace, void* stream) {
    if (I < 0 || D < 0 || G < 0 || (I == 0 && (D > 0 || G > 0))) return OMNI_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (I > 0) {
        MatchP p{dt_box, dt_cat, dt_c2d, dt_z, dt_dims, dt_pose, dt_off, gt_box, gt_cat, gt_center, gt_dims, gt_pose, gt_off, K,
                 match, err, workspace};
        hipLaunchKernelGGL(match_errors_kernel, dim3((unsigned)I), dim3(256), 0, st, p);
    }
    hipLaunchKernelGGL(match_errors_finalize, dim3(1), dim3(64 * NQ), 0, st, workspace, I, sums, counts);   // I == 0: writes the zeros
    return omni_launch_status();
}

}  // extern "C"
