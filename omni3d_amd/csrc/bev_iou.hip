// bev_iou.hip -- IoU of cuboids in the bird's-eye view: the overlap of their footprints on the ground plane, the matching criterion
// of AP-BEV (KITTI, nuScenes).  The reference has no such step: its evaluator matches by 2D IoU or IoU3D only
// (cubercnn/evaluation/omni3d_evaluation.py:1359-1431).
//
//   bev_footprint_kernel   one thread per box: the eight corners are projected on the plane orthogonal to `up` (coordinates along
//                          e1, e2, which the host derives from `up`), sorted by a 19-comparator network in registers (constant
//                          indices only) and turned into their convex hull by Andrew's monotone chain (pop while cross <= 0: duplicate
//                          and collinear points go).  The chain's stack is indexed by a run-time depth, so it lives in a per-thread
//                          LDS slice laid out [slot][thread], not in a private array (which would go to scratch).  Out: the hull
//                          counter-clockwise, its size and its area (fan from its first vertex).  A box with a non-finite vertex or
//                          an area <= eps_area is invalid: count 0, area 0, counted into `invalid`.
//   bev_iou_pairs_kernel   one thread per pair: bounding rectangles (exact 0 when disjoint), then BOTH polygons minus the first
//                          vertex of the first one -- every product below is formed on such local coordinates; in absolute ones the
//                          float32 cancellation at z = 80 costs 2.7e-4 of IoU instead of 5.8e-7 -- then Sutherland-Hodgman: the first
//                          polygon clipped by every edge of the second, ping-pong between two 16-vertex lists in per-thread LDS
//                          slices [vertex][thread] (a wave's 32-lane groups fall on 32 distinct banks; 256 B per thread), the fan
//                          area of the result and inter / (a1 + a2 - inter) clamped to [0, 1].  No atomics, no barrier, no
//                          dependence on another thread: two launches give the same bits.
//
// No fused multiply-add in this file: the turn test p * q - r * s of a point against a segment that ENDS in a bit-equal copy of it
// (the top and bottom corners of an upright box) is exactly 0 only when both products are rounded; contracted to fma(p, q, -(r * s))
// it is the rounding residual of one product, of either sign, and the copy stays in the hull as a fifth vertex.
#include <device_rt.h>

#pragma clang fp contract(off)

namespace {

constexpr int BEV_T = 64;          // threads per workgroup: one wave
constexpr int BEV_HULL = 16;       // chain stack: every point is pushed at most twice (8 + 7 pushes)
constexpr int BEV_CAP = 16;        // clipped polygon: 8 vertices + at most one per clipping edge

__device__ __forceinline__ bool bev_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// z of (a - o) x (b - o): > 0 when o -> a -> b turns left
__device__ __forceinline__ float bev_cross(float ox, float oy, float ax, float ay, float bx, float by) {
    return (ax - ox) * (by - oy) - (ay - oy) * (bx - ox);
}

// compare-exchange by (x, then y), ascending
__device__ __forceinline__ void bev_cswap(float& ax, float& ay, float& bx, float& by) {
    const bool sw = bx < ax || (bx == ax && by < ay);
    const float tx = sw ? bx : ax, ty = sw ? by : ay;
    bx = sw ? ax : bx; by = sw ? ay : by;
    ax = tx; ay = ty;
}

__global__ void __launch_bounds__(BEV_T) bev_footprint_kernel(const float* __restrict__ verts, int N, float e1x, float e1y, float e1z,
                                                              float e2x, float e2y, float e2z, float eps_area,
                                                              float* __restrict__ poly, int* __restrict__ count,
                                                              float* __restrict__ area, int* __restrict__ invalid) {
    __shared__ float s_h[2 * BEV_HULL * BEV_T];                   // chain stack [slot][x | y][thread]
    const int t = threadIdx.x;
    const long n = (long)blockIdx.x * BEV_T + t;
    if (n >= N) return;
    const float* v = verts + 24L * n;
    float* hx = s_h + t;
    float* hy = s_h + BEV_T + t;
#define BEV_HX(i) hx[(i) * (2 * BEV_T)]
#define BEV_HY(i) hy[(i) * (2 * BEV_T)]
    float px[8], py[8];
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float x = v[3 * k], y = v[3 * k + 1], z = v[3 * k + 2];
        px[k] = x * e1x + y * e1y + z * e1z;
        py[k] = x * e2x + y * e2y + z * e2z;
        finite = finite && bev_finite(x) && bev_finite(y) && bev_finite(z) && bev_finite(px[k]) && bev_finite(py[k]);
    }
    int k = 0;
    float a = 0.0f;
    if (finite) {
        // optimal sorting network for 8 keys: 19 comparators in 6 layers
#define BEV_CS(i, j) bev_cswap(px[i], py[i], px[j], py[j])
        BEV_CS(0, 2); BEV_CS(1, 3); BEV_CS(4, 6); BEV_CS(5, 7);
        BEV_CS(0, 4); BEV_CS(1, 5); BEV_CS(2, 6); BEV_CS(3, 7);
        BEV_CS(0, 1); BEV_CS(2, 3); BEV_CS(4, 5); BEV_CS(6, 7);
        BEV_CS(2, 4); BEV_CS(3, 5);
        BEV_CS(1, 4); BEV_CS(3, 6);
        BEV_CS(1, 2); BEV_CS(3, 4); BEV_CS(5, 6);
#undef BEV_CS
        // lower chain left to right, upper chain back; the input index is a constant of the unrolled loop
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            while (k >= 2 && bev_cross(BEV_HX(k - 2), BEV_HY(k - 2), BEV_HX(k - 1), BEV_HY(k - 1), px[i], py[i]) <= 0.0f) --k;
            BEV_HX(k) = px[i]; BEV_HY(k) = py[i];
            ++k;
        }
        const int lo = k + 1;
#pragma unroll
        for (int i = 6; i >= 0; --i) {
            while (k >= lo && bev_cross(BEV_HX(k - 2), BEV_HY(k - 2), BEV_HX(k - 1), BEV_HY(k - 1), px[i], py[i]) <= 0.0f) --k;
            BEV_HX(k) = px[i]; BEV_HY(k) = py[i];
            ++k;
        }
        --k;                                                       // the last point is the first again
        if (k > 8) k = 0;                                          // cannot happen in exact arithmetic: such a box takes no part
        const float ox = BEV_HX(0), oy = BEV_HY(0);
        for (int i = 1; i + 1 < k; ++i) a += bev_cross(ox, oy, BEV_HX(i), BEV_HY(i), BEV_HX(i + 1), BEV_HY(i + 1));
        a *= 0.5f;
    }
    const bool ok = k >= 3 && a > eps_area && bev_finite(a);
    if (!ok) {
        k = 0;
        a = 0.0f;
        if (invalid) atomicAdd(invalid, 1);
    }
    float* o = poly + 16L * n;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const bool used = i < k;
        o[2 * i] = used ? BEV_HX(i) : 0.0f;
        o[2 * i + 1] = used ? BEV_HY(i) : 0.0f;
    }
    count[n] = k;
    area[n] = a;
#undef BEV_HX
#undef BEV_HY
}

__global__ void __launch_bounds__(BEV_T) bev_iou_pairs_kernel(const float* __restrict__ poly1, const int* __restrict__ count1,
                                                              const float* __restrict__ area1, int n1,
                                                              const float* __restrict__ poly2, const int* __restrict__ count2,
                                                              const float* __restrict__ area2, int n2, const int* __restrict__ idx1,
                                                              const int* __restrict__ idx2, long P, float* __restrict__ iou) {
    __shared__ float s_v[2 * 2 * BEV_CAP * BEV_T];                // two lists [vertex][x | y][thread]: 16 KB
    const int t = threadIdx.x;
    const long p = (long)blockIdx.x * BEV_T + t;
    if (p >= P) return;
    const int i1 = idx1[p], i2 = idx2[p];
    float out = 0.0f;
    int c1 = 0, c2 = 0;
    if ((unsigned)i1 < (unsigned)n1 && (unsigned)i2 < (unsigned)n2) {          // an index outside its set: IoU 0, nothing is read
        c1 = count1[i1];
        c2 = count2[i2];
    }
    if (c1 >= 3 && c1 <= 8 && c2 >= 3 && c2 <= 8) {
        const float* A = poly1 + 16L * i1;
        const float* B = poly2 + 16L * i2;
        const float ox = A[0], oy = A[1];                          // the local origin of this pair
        const float inf = __int_as_float(0x7f800000);
        float ax0 = inf, ay0 = inf, ax1 = -inf, ay1 = -inf, bx0 = inf, by0 = inf, bx1 = -inf, by1 = -inf;
        float* L0 = s_v + t;
        float* L1 = s_v + 2 * BEV_CAP * BEV_T + t;
        for (int i = 0; i < c1; ++i) {
            const float x = A[2 * i], y = A[2 * i + 1];
            ax0 = fminf(ax0, x); ax1 = fmaxf(ax1, x); ay0 = fminf(ay0, y); ay1 = fmaxf(ay1, y);
            L0[(2 * i) * BEV_T] = x - ox;
            L0[(2 * i + 1) * BEV_T] = y - oy;
        }
        for (int j = 0; j < c2; ++j) {
            const float x = B[2 * j], y = B[2 * j + 1];
            bx0 = fminf(bx0, x); bx1 = fmaxf(bx1, x); by0 = fminf(by0, y); by1 = fmaxf(by1, y);
        }
        const bool apart = ax1 < bx0 || bx1 < ax0 || ay1 < by0 || by1 < ay0;
        if (!apart) {
            int n = c1;
            float* src = L0;
            float* dst = L1;
            float ex0 = B[2 * (c2 - 1)] - ox, ey0 = B[2 * (c2 - 1) + 1] - oy;      // edge j runs from vertex j - 1 to vertex j
            for (int j = 0; j < c2 && n > 0; ++j) {
                const float ex1 = B[2 * j] - ox, ey1 = B[2 * j + 1] - oy;
                const float dx = ex1 - ex0, dy = ey1 - ey0;
                float qx = src[(2 * (n - 1)) * BEV_T], qy = src[(2 * (n - 1) + 1) * BEV_T];
                float dq = dx * (qy - ey0) - dy * (qx - ex0);      // >= 0: on the inner (left) side of the edge
                int m = 0;
                for (int i = 0; i < n; ++i) {
                    const float cx = src[(2 * i) * BEV_T], cy = src[(2 * i + 1) * BEV_T];
                    const float dc = dx * (cy - ey0) - dy * (cx - ex0);
                    if ((dc >= 0.0f) != (dq >= 0.0f) && m < BEV_CAP) {
                        const float s = dq / (dq - dc);
                        dst[(2 * m) * BEV_T] = qx + s * (cx - qx);
                        dst[(2 * m + 1) * BEV_T] = qy + s * (cy - qy);
                        ++m;
                    }
                    if (dc >= 0.0f && m < BEV_CAP) {
                        dst[(2 * m) * BEV_T] = cx;
                        dst[(2 * m + 1) * BEV_T] = cy;
                        ++m;
                    }
                    qx = cx; qy = cy; dq = dc;
                }
                n = m;
                float* sw = src; src = dst; dst = sw;
                ex0 = ex1; ey0 = ey1;
            }
            float inter = 0.0f;
            if (n >= 3) {
                const float rx = src[0], ry = src[BEV_T];
                for (int i = 1; i + 1 < n; ++i)
                    inter += bev_cross(rx, ry, src[(2 * i) * BEV_T], src[(2 * i + 1) * BEV_T], src[(2 * i + 2) * BEV_T],
                                       src[(2 * i + 3) * BEV_T]);
                inter = fmaxf(0.5f * inter, 0.0f);
            }
            const float uni = area1[i1] + area2[i2] - inter;
            const float r = uni > 0.0f ? inter / uni : 0.0f;
            out = fminf(fmaxf(r, 0.0f), 1.0f);                     // fmaxf drops a NaN
        }
    }
    iou[p] = out;
}

}  // namespace

extern "C" {

int omni_bev_footprint(const float* verts, int N, float e1x, float e1y, float e1z, float e2x, float e2y, float e2z, float eps_area,
                       float* poly, int* count, float* area, int* invalid, void* stream) {
    const float e[6] = {e1x, e1y, e1z, e2x, e2y, e2z};
    for (int i = 0; i < 6; ++i)
        if (!(fabsf(e[i]) <= 2.0f)) return OMNI_ERR_ARG;           // a unit vector's component (also refuses a NaN)
    if (N < 0 || !(eps_area >= 0.0f)) return OMNI_ERR_ARG;
    if (N == 0) return OMNI_OK;
    if (!verts || !poly || !count || !area) return OMNI_ERR_ARG;
    hipLaunchKernelGGL(bev_footprint_kernel, dim3((unsigned)((N + BEV_T - 1) / BEV_T)), dim3(BEV_T), 0, (hipStream_t)stream, verts, N,
                       e1x, e1y, e1z, e2x, e2y, e2z, eps_area, poly, count, area, invalid);
    return omni_launch_status();
}

int omni_bev_iou_pairs(const float* poly1, const int* count1, const float* area1, int n1, const float* poly2, const int* count2,
                       const float* area2, int n2, const int* idx1, const int* idx2, long long npairs, float* iou, void* stream) {
    if (n1 < 0 || n2 < 0 || npairs < 0 || npairs > (long long)BEV_T * 0x7fffffffLL) return OMNI_ERR_ARG;
    if (npairs == 0) return OMNI_OK;
    if (!idx1 || !idx2 || !iou) return OMNI_ERR_ARG;
    if ((n1 > 0 && (!poly1 || !count1 || !area1)) || (n2 > 0 && (!poly2 || !count2 || !area2))) return OMNI_ERR_ARG;
    hipLaunchKernelGGL(bev_iou_pairs_kernel, dim3((unsigned)((npairs + BEV_T - 1) / BEV_T)), dim3(BEV_T), 0, (hipStream_t)stream,
                       poly1, count1, area1, n1, poly2, count2, area2, n2, idx1, idx2, (long)npairs, iou);
    return omni_launch_status();
}

}  // extern "C"
