// iou3d_exact.hip -- IoU3D of two cuboids that is right whatever their relative pose.  The evaluator's pair algorithm (csrc/box3d_pair.h,
// the float32 restatement of pytorch3d's iou_box3d) treats a triangle within 2.56 degrees of a face plane, and close to it, as lying in
// that plane; on near-aligned duplicates it is up to 0.3 away from exact geometry.  AP3D keeps it to stay comparable with the reference;
// this file is for the callers that want the geometry itself (kernels/iou3d.py: cuboid_fit, iou_box3d_exact*; TEST.NMS_3D.IOU_TYPE
// "exact" goes through omni_nms3d_exact in csrc/nms3d.hip, which shares the device functions of cuboid_exact.h).
//
//   cuboid_fit_kernel         one thread per box: cuboid_fit, the result stored as doubles; an invalid box is counted into `invalid`.
//   iou3d_exact_pairs_kernel  one thread per pair: cuboid_pair_iou on two fitted boxes; exactly 0 for an invalid box or an index outside
//                             its set.  No atomics, no barrier: two launches give the same bits.
// One wave per workgroup: the clip lists take 320 B of LDS per thread, 20 KB per workgroup, so eight workgroups fit a CU's 160 KB --
// two waves per SIMD, which is what the double-precision registers of the pair loop leave room for anyway.
//
// No fused multiply-add in this file: the emulator and the device then take the same clip decisions on the same bits.
#include <device_rt.h>

#pragma clang fp contract(off)

#include "cuboid_exact.h"

namespace {

constexpr int CXK_T = 64;          // threads per workgroup: one wave

__global__ void __launch_bounds__(CXK_T) cuboid_fit_kernel(const float* __restrict__ verts, int N, double eps_dim, double fit_tol,
                                                           double* __restrict__ centre, double* __restrict__ axes,
                                                           double* __restrict__ dims, int* __restrict__ valid, int* __restrict__ invalid) {
    const long n = (long)blockIdx.x * CXK_T + threadIdx.x;
    if (n >= N) return;
    CxBox b;
    const bool ok = cuboid_fit(verts + 24L * n, eps_dim, fit_tol, b);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        centre[3L * n + a] = b.c[a];
        dims[3L * n + a] = b.d[a];
#pragma unroll
        for (int k = 0; k < 3; ++k) axes[9L * n + 3 * k + a] = b.x[k][a];
    }
    valid[n] = ok ? 1 : 0;
    if (!ok && invalid) atomicAdd(invalid, 1);
}

__device__ __forceinline__ void cxk_load(CxBox& b, const double* __restrict__ centre, const double* __restrict__ axes,
                                         const double* __restrict__ dims, long i) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        b.c[a] = centre[3 * i + a];
        b.d[a] = dims[3 * i + a];
#pragma unroll
        for (int k = 0; k < 3; ++k) b.x[k][a] = axes[9 * i + 3 * k + a];
    }
}

__global__ void __launch_bounds__(CXK_T) iou3d_exact_pairs_kernel(const double* __restrict__ centre1, const double* __restrict__ axes1,
                                                                  const double* __restrict__ dims1, const int* __restrict__ valid1, int n1,
                                                                  const double* __restrict__ centre2, const double* __restrict__ axes2,
                                                                  const double* __restrict__ dims2, const int* __restrict__ valid2, int n2,
                                                                  const int* __restrict__ idx1, const int* __restrict__ idx2, long P,
                                                                  float* __restrict__ vol, float* __restrict__ iou) {
    __shared__ double s_v[2 * 2 * CX_CAP * CXK_T];                // two lists [vertex][x | y][thread]: 20 KB
    const int t = threadIdx.x;
    const long p = (long)blockIdx.x * CXK_T + t;
    if (p >= P) return;
    const int i1 = idx1[p], i2 = idx2[p];
    float v = 0.0f, r = 0.0f;
    if ((unsigned)i1 < (unsigned)n1 && (unsigned)i2 < (unsigned)n2 && valid1[i1] != 0 && valid2[i2] != 0) {
        CxBox A, B;
        cxk_load(A, centre1, axes1, dims1, i1);
        cxk_load(B, centre2, axes2, dims2, i2);
        // a set that did not come from omni_cuboid_fit: nothing is divided by these, but a NaN would travel
        if (A.d[0] > 0.0 && A.d[1] > 0.0 && A.d[2] > 0.0 && B.d[0] > 0.0 && B.d[1] > 0.0 && B.d[2] > 0.0)
            cuboid_pair_iou<CXK_T>(A, B, s_v + t, s_v + 2 * CX_CAP * CXK_T + t, v, r);
    }
    vol[p] = v == v ? v : 0.0f;
    iou[p] = r == r ? r : 0.0f;
}

}  // namespace

extern "C" {

int omni_cuboid_fit(const float* verts, int N, double eps_dim, double fit_tol, double* centre, double* axes, double* dims, int* valid,
                    int* invalid, void* stream) {
    if (N < 0 || !(eps_dim >= 0.0) || !(fit_tol >= 0.0) || !(eps_dim < 1e300) || !(fit_tol < 1e300)) return OMNI_ERR_ARG;
    if (N == 0) return OMNI_OK;
    if (!verts || !centre || !axes || !dims || !valid) return OMNI_ERR_ARG;
    hipLaunchKernelGGL(cuboid_fit_kernel, dim3((unsigned)((N + CXK_T - 1) / CXK_T)), dim3(CXK_T), 0, (hipStream_t)stream, verts, N, eps_dim,
                       fit_tol, centre, axes, dims, valid, invalid);
    return omni_launch_status();
}

int omni_iou3d_exact_pairs(const double* centre1, const double* axes1, const double* dims1, const int* valid1, int n1,
                           const double* centre2, const double* axes2, const double* dims2, const int* valid2, int n2, const int* idx1,
                           const int* idx2, long long npairs, float* vol, float* iou, void* stream) {
    if (n1 < 0 || n2 < 0 || npairs < 0 || npairs > (long long)CXK_T * 0x7fffffffLL) return OMNI_ERR_ARG;
    if (npairs == 0) return OMNI_OK;
    if (!idx1 || !idx2 || !vol || !iou) return OMNI_ERR_ARG;
    if ((n1 > 0 && (!centre1 || !axes1 || !dims1 || !valid1)) || (n2 > 0 && (!centre2 || !axes2 || !dims2 || !valid2))) return OMNI_ERR_ARG;
    hipLaunchKernelGGL(iou3d_exact_pairs_kernel, dim3((unsigned)((npairs + CXK_T - 1) / CXK_T)), dim3(CXK_T), 0, (hipStream_t)stream,
                       centre1, axes1, dims1, valid1, n1, centre2, axes2, dims2, valid2, n2, idx1, idx2, (long)npairs, vol, iou);
    return omni_launch_status();
}

}  // extern "C"
