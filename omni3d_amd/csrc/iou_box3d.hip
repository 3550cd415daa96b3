// iou_box3d.hip -- exact oriented-box IoU3D for gfx950 (CDNA4).
//
// Replaces pytorch3d._C.iou_box3d as called by the reference evaluator
//   /root/reference/cubercnn/evaluation/omni3d_evaluation.py:155  (box3d_overlap, :106-166)
// and the validity masks _check_coplanar (:65-86) / _check_nonzero (:89-104).
//
// MI355X mapping (NOT the upstream CUDA thread-per-pair + per-thread scratch design):
//   * a 32-lane half of a wavefront owns one (dt, gt) pair (two pairs per wave; 64 / 16 lanes per pair selectable);
//     workgroup = one wave, so the LDS region is private to the wave and __syncthreads() is a wave-local fence
//   * both clip directions (tris(box1) vs planes(box2) and tris(box2) vs planes(box1)) live in one
//     LDS triangle list, lanes = triangles; every plane pass is clip -> ballot prefix -> stable
//     compaction into the other LDS buffer, so triangle order equals the sequential algorithm
//   * the O(n1*n2) coplanar-duplicate removal is spread over the 64 lanes with per-triangle
//     normals/areas cached in LDS
//   * I/O is 192 B in + 4 B out per pair: the kernel is VALU/latency bound, HBM
//     traffic is negligible.
// fp contraction is disabled so the epsilon-threshold branches take exactly the decisions of the
// CPU oracle (oracle/iou_box3d_oracle.c), which the parity tests compare against.
// The pair algorithm itself (iou_pair_body and what it needs) is in box3d_pair.h, which csrc/nms3d.hip shares; this file holds the
// evaluator's kernels and entry points.
#include <device_rt.h>
#pragma clang fp contract(off)
#include "box3d_pair.h"

#if defined(OMNI_HIPEMU) && defined(IOU_DEBUG_HIST)
extern "C" long* omni_debug_iou_phase() { return &g_iou_phase[0][0]; }
extern "C" int* omni_debug_iou_hist() { return &g_iou_hist[0][0]; }
extern "C" int* omni_debug_iou_rounds() { return g_iou_rounds; }
#endif

namespace {

constexpr float IOU_RETRY = -1.0f;   // first-pass marker: "this pair's triangle list outgrew the small LDS lists, recompute it"

// MODE 0: matrix (pair p -> a = p / M, b = p % M); MODE 1: indexed pairs.
// First pass.  A wave takes 64 consecutive pairs: every lane screens one pair (validity mask, bounding spheres) and writes the
// zeros of the rejected ones; the survivors are then worked off G = 64 / SUB at a time, SUB lanes per pair, lists of CAPT
// triangles.  RETRY (CAPT below the full capacity): a pair whose list outgrows CAPT is marked with iou = IOU_RETRY for
// iou_box3d_retry_kernel instead of being counted as an overflow.
template <int MODE, int SUB, int CAPT, bool RETRY>
__global__ void __launch_bounds__(64) OMNI_WAVES_PER_EU(4) iou_box3d_kernel(
    const float* __restrict__ boxes1, const float* __restrict__ boxes2, const int* __restrict__ idx1, const int* __restrict__ idx2,
    const int* __restrict__ valid1, long long npairs, int M, float* __restrict__ vol_out, float* __restrict__ iou_out,
    int* __restrict__ overflow, int chunk) {
    constexpr int G = 64 / SUB;
    __shared__ PairLds<CAPT> Lall[G];
    const int lane = threadIdx.x;
    // `chunk` (16 | 32 | 64) pairs are screened per round by the first `chunk` lanes: smaller chunks = more waves for the same
    // problem (the launcher keeps >= ~4096 of them when the problem allows), the screening itself is cheap
    for (long long c0 = (long long)blockIdx.x * chunk; c0 < npairs; c0 += (long long)gridDim.x * chunk) {
        const long long q = c0 + lane;
        int ia = 0, ib = 0;
        bool live = false;
        if (lane < chunk && q < npairs) {
            if (MODE == 0) { ia = (int)(q / M); ib = (int)(q % M); }
            else { ia = idx1[q]; ib = idx2[q]; }
            live = !(valid1 != nullptr && valid1[ia] == 0) && !spheres_disjoint(boxes1 + (size_t)ia * 24, boxes2 + (size_t)ib * 24);
            if (!live) { if (vol_out) vol_out[q] = 0.f; iou_out[q] = 0.f; }
        }
        iou_pair_survivors<SUB, CAPT>(Lall, __ballot(live), ia, ib, boxes1, boxes2, lane,
                                      [&](int, int, int j, float vol, float iou, bool over) {
            const long long p = c0 + j;
            if (RETRY && over) { vol = 0.f; iou = IOU_RETRY; }
            if (vol_out) vol_out[p] = vol;
            iou_out[p] = iou;
            if (!RETRY && over && overflow) atomicAdd(overflow, 1);
        });
    }
}

// Second pass of a RETRY launch: every wave scans 64 results at a time for the marker and recomputes the marked pairs, one per
// wave, with the full-capacity lists.  With no marked pair (the usual case: a joint list longer than 96 needs near-identical
// boxes) this is one read of the result vector.
template <int MODE>
__global__ void __launch_bounds__(64) iou_box3d_retry_kernel(const float* __restrict__ boxes1, const float* __restrict__ boxes2,
                                                             const int* __restrict__ idx1, const int* __restrict__ idx2, long long npairs,
                                                             int M, float* __restrict__ vol_out, float* __restrict__ iou_out,
                                                             int* __restrict__ overflow) {
    __shared__ PairLds<CAP> L;
    const int lane = threadIdx.x;
    for (long long c0 = (long long)blockIdx.x * 64; c0 < npairs; c0 += (long long)gridDim.x * 64) {
        const long long q = c0 + lane;
        const bool marked = q < npairs && iou_out[q] == IOU_RETRY;
        int ia = 0, ib = 0;
        if (marked) {
            if (MODE == 0) { ia = (int)(q / M); ib = (int)(q % M); }
            else { ia = idx1[q]; ib = idx2[q]; }
        }
        iou_pair_survivors<64, CAP>(&L, __ballot(marked), ia, ib, boxes1, boxes2, lane, [&](int, int, int j, float vol, float iou, bool over) {
            if (vol_out) vol_out[c0 + j] = vol;
            iou_out[c0 + j] = iou;
            if (over && overflow) atomicAdd(overflow, 1);
        });
    }
}

// _check_coplanar & _check_nonzero (omni3d_evaluation.py:65-104): one lane per dt box.
// valid[i] = 1 iff both pass; counts[0] += #non-coplanar, counts[1] += #zero-area.
__global__ void box3d_validity_kernel(const float* __restrict__ boxes, int N, float eps_coplanar, float eps_nonzero,
                                      int* __restrict__ valid, int* __restrict__ counts) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float* B = boxes + (size_t)i * 24;
    const Box3dValidity v = box3d_validity(B, eps_coplanar, eps_nonzero);
    valid[i] = (v.coplanar && v.nonzero) ? 1 : 0;
    if (counts) {
        if (!v.coplanar) atomicAdd(&counts[0], 1);
        if (!v.nonzero) atomicAdd(&counts[1], 1);
    }
}

// production launch: 32 lanes per pair over 96-triangle lists (7.4 KB of LDS per pair: 10 two-pair waves per CU instead of 6
// with the full 160-triangle lists), marked pairs redone at full capacity by the retry pass
constexpr int IOU_VARIANT = 1032;      // (set from tools/bench_iou3d.py: profiles/r03_iou3d_variants*.log)

inline int iou_grid(long long npairs) {
    // 256 CUs x up to 16 single-wave workgroups per CU (LDS-limited); grid-stride beyond that
    const int chunk = iou_chunk(npairs);
    const long long waves = (npairs + chunk - 1) / chunk;
    long long g = waves < 256 * 16 ? waves : 256 * 16;
    return (int)(g < 1 ? 1 : g);
}

// variant = lanes_per_pair (64 | 32 | 16) + 1000 when the first pass uses the small lists + retry pass; 0 = production
template <int MODE>
inline int iou_launch(int variant, const float* boxes1, const float* boxes2, const int* idx1, const int* idx2, const int* valid1,
                      long long np, int M, float* vol, float* iou, int* overflow, void* stream) {
    if (variant == 0) variant = IOU_VARIANT;
    const bool small = variant >= 1000;
    const int cap_code = variant / 1000;                 // 0: full lists | 1: 96 | 2: 64 | 3: 48 triangles in the first pass
    const int sub = variant % 1000;
    hipStream_t st = (hipStream_t)stream;
#define OMNI_IOU(SUB_, CAP_, RETRY_)                                                                                          \
    hipLaunchKernelGGL(HIP_KERNEL_NAME(iou_box3d_kernel<MODE, SUB_, CAP_, RETRY_>), dim3(iou_grid(np)), dim3(64), 0, st,       \
                       boxes1, boxes2, idx1, idx2, valid1, np, M, vol, iou, overflow, iou_chunk(np))
    if (!small) {
        if (sub == 64) OMNI_IOU(64, CAP, false);
        else if (sub == 32) OMNI_IOU(32, CAP, false);
        else if (sub == 16) OMNI_IOU(16, CAP, false);
        else return OMNI_ERR_ARG;
    } else {
        if (cap_code == 1 && sub == 64) OMNI_IOU(64, 96, true);
        else if (cap_code == 1 && sub == 32) OMNI_IOU(32, 96, true);
        else if (cap_code == 1 && sub == 16) OMNI_IOU(16, 96, true);
        else if (cap_code == 2 && sub == 32) OMNI_IOU(32, 64, true);
        else if (cap_code == 2 && sub == 64) OMNI_IOU(64, 64, true);
        else if (cap_code == 3 && sub == 32) OMNI_IOU(32, 48, true);
        else return OMNI_ERR_ARG;
        const long long chunks = (np + 63) / 64;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(iou_box3d_retry_kernel<MODE>), dim3((unsigned)(chunks < 2048 ? chunks : 2048)), dim3(64), 0, st,
                           boxes1, boxes2, idx1, idx2, np, M, vol, iou, overflow);
    }
#undef OMNI_IOU
    return omni_launch_status();
}

}  // namespace

extern "C" {

int omni_iou_box3d(const float* boxes1, int N, const float* boxes2, int M, const int* valid1, float* vol, float* iou,
                   int* overflow, void* stream) {
    if (N < 0 || M < 0) return OMNI_ERR_ARG;
    const long long np = (long long)N * M;
    if (np == 0) return OMNI_OK;
    return iou_launch<0>(0, boxes1, boxes2, nullptr, nullptr, valid1, np, M, vol, iou, overflow, stream);
}

int omni_iou_box3d_pairs(const float* boxes1, const float* boxes2, const int* idx1, const int* idx2, long long npairs,
                         const int* valid1, float* vol, float* iou, int* overflow, void* stream) {
    if (npairs < 0) return OMNI_ERR_ARG;
    if (npairs == 0) return OMNI_OK;
    return iou_launch<1>(0, boxes1, boxes2, idx1, idx2, valid1, npairs, 1, vol, iou, overflow, stream);
}

// lanes_per_pair in {64, 32, 16}: one launch with the full-capacity triangle lists; 1000 / 2000 / 3000 + lanes: first pass over
// 96- / 64- / 48-triangle lists + retry pass (0 = the production choice).  A/B entry point of tools/bench_iou3d.py and of the parity tests, which
// run every variant against the oracle
int omni_iou_box3d_pairs_algo(const float* boxes1, const float* boxes2, const int* idx1, const int* idx2, long long npairs,
                              const int* valid1, float* vol, float* iou, int* overflow, int lanes_per_pair, void* stream) {
    if (npairs < 0) return OMNI_ERR_ARG;
    if (npairs == 0) return OMNI_OK;
    return iou_launch<1>(lanes_per_pair, boxes1, boxes2, idx1, idx2, valid1, npairs, 1, vol, iou, overflow, stream);
}

int omni_box3d_validity(const float* boxes, int N, float eps_coplanar, float eps_nonzero, int* valid, int* counts,
                        void* stream) {
    if (N < 0) return OMNI_ERR_ARG;
    if (N == 0) return OMNI_OK;
    hipLaunchKernelGGL(box3d_validity_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, boxes, N,
                       eps_coplanar, eps_nonzero, valid, counts);
    return omni_launch_status();
}

}  // extern "C"
