// nms3d.hip -- suppression of duplicate cuboids at inference for gfx950 (CDNA4): omni_nms3d decides by the evaluator's pair algorithm
// (box3d_pair.h), omni_nms3d_exact (further down) by the exact IoU3D of cuboid_exact.h; they share the pair numbering, the validity
// ballots and the pick kernel.  omni_fuse3d (last) merges overlapping cuboids instead of dropping them: the exact pair matrix, then
// the pick kernel's ranking and walk followed by a weighted mean per cluster, reduced by ONE THREAD PER CLUSTER that walks its members
// in rank order: the clusters of test-time augmentation are many and small, so a wave per cluster would idle most of its lanes, and a
// fixed walk needs no reduction tree to make two runs give the same bits (the block comment above fuse3d_kernel has the steps).
#include <device_rt.h>
#pragma clang fp contract(off)
#include "box3d_pair.h"

// omni_nms3d -- suppression of duplicate cuboids at inference (the reference has no such step: `fast_rcnn_inference` suppresses per
// class and in 2D only).  Two launches over the fixed (B, S) slots of the inference pass:
//   nms3d_iou_kernel   the block-diagonal self-overlap: for every image the IoU3D of its slot pairs i < j, mirrored into a full
//                      (S, S) matrix.  The pair index is turned into (i, j) by arithmetic; a lane screens its pair out (exact 0) when
//                      j lies behind the image's count, the classes differ (class-specific mode), a box fails the validity test, or
//                      the bounding spheres are disjoint; the survivors go through iou_pair_body, 32 lanes per pair over the
//                      full-capacity lists (one launch, no retry pass).  Two launches leave no place for a device-wide per-box pass,
//                      so every wave takes the validity of its image's boxes ONCE, as ballots into LDS, before its first pair.
//   nms3d_pick_kernel  one 256-thread workgroup per image: bitonic sort of 64-bit keys [~ordered score bits | slot] (the network of
//                      csrc/train_vis.hip), a walk down the ranking in which a live candidate removes the later candidates whose
//                      IoU3D with it is > iou_thr (a candidate whose row holds no such value is passed over without a load or a
//                      barrier), then an ordered compaction of the surviving slots by wave ballots.  No atomics.
// A slot whose box is invalid (or has a non-finite vertex) or whose score is not finite is kept, never suppresses and is never
// suppressed: it sorts behind every ranked slot and the walk ends at the first such key.
namespace {

constexpr int NMS3D_MAXS = 1024;                     // slots per image the LDS arrays of the pick kernel hold
constexpr unsigned NMS3D_UNRANKED = 0xFFFFFFFFu;     // high key word of padding and of the slots that take no part in the suppression

// a slot's box takes part iff it passes the evaluator's validity test and has no non-finite vertex
__device__ __forceinline__ bool nms3d_box_valid(const float* __restrict__ B, float eps_coplanar, float eps_nonzero) {
    bool finite = true;
    for (int k = 0; k < 24; ++k) finite = finite && cx_finite(B[k]);
    const Box3dValidity v = box3d_validity(B, eps_coplanar, eps_nonzero);
    return finite && v.coplanar && v.nonzero;
}

// pair q of the S (S - 1) / 2 pairs i < j of one image, rows of the upper triangle one after another: row i starts at
// i (2S - 1 - i) / 2.  The float root is exact to a unit for S <= 1024 ((2S - 1)^2 and 8q are integers below 2^24); the two loops
// settle the last unit.
__device__ __forceinline__ void nms3d_pair(int q, int S, int& i, int& j) {
    const float t = (float)(2 * S - 1);
    int r = (int)((t - sqrtf(t * t - 8.0f * (float)q)) * 0.5f);
    r = r < 0 ? 0 : (r > S - 2 ? S - 2 : r);
    while (r > 0 && r * (2 * S - 1 - r) / 2 > q) --r;
    while ((r + 1) * (2 * S - 2 - r) / 2 <= q) ++r;
    i = r;
    j = q - r * (2 * S - 1 - r) / 2 + r + 1;
}

// Prologue of a pair-matrix workgroup (one wave) of image b: count_b = count[b] -> the count clamped to [0, S]; s_valid bit s = slot s
// is in use and slot_ok(s) holds (asked of the slots in use only), taken once as ballots before the wave's first pair; the first
// workgroup of the image zeroes the diagonal of its matrix O.
template <class Pred>
__device__ __forceinline__ int nms3d_slots(int count_b, int S, float* __restrict__ O, unsigned long long* s_valid,
                                           Pred slot_ok) {
    const int lane = threadIdx.x;
    int n = count_b;
    n = n < 0 ? 0 : (n > S ? S : n);
    for (int s0 = 0; s0 < S; s0 += 64) {
        const int s = s0 + lane;
        const unsigned long long m = __ballot(s < n && slot_ok(s));
        if (lane == 0) s_valid[s0 >> 6] = m;
    }
    __syncthreads();
    if (blockIdx.x == 0)
        for (int s = lane; s < S; s += 64) O[(size_t)s * S + s] = 0.f;
    return n;
}

// pair ia < ib has an overlap to compute: both slots in use, of one class (class-specific mode) and valid
__device__ __forceinline__ bool nms3d_pair_live(int ia, int ib, int n, int class_agnostic, const int* __restrict__ C,
                                                const unsigned long long* s_valid) {
    return ib < n && (class_agnostic != 0 || C[ia] == C[ib]) && ((s_valid[ia >> 6] >> (ia & 63)) & 1ull) != 0ull &&
           ((s_valid[ib >> 6] >> (ib & 63)) & 1ull) != 0ull;
}

template <int SUB, int CAPT>
__global__ void __launch_bounds__(64) OMNI_WAVES_PER_EU(4) nms3d_iou_kernel(
    const float* __restrict__ verts, const int* __restrict__ cls, const int* __restrict__ count, int S, int class_agnostic,
    float eps_coplanar, float eps_nonzero, float* __restrict__ iou_out, int* __restrict__ overflow, int chunk) {
    constexpr int G = 64 / SUB;
    __shared__ PairLds<CAPT> Lall[G];
    __shared__ unsigned long long s_valid[NMS3D_MAXS / 64];      // bit s: slot s is in use and its box is valid
    const int lane = threadIdx.x;
    const int b = blockIdx.y;
    const float* V = verts + (size_t)b * S * 24;
    const int* C = cls + (size_t)b * S;
    float* O = iou_out + (size_t)b * S * S;
    const int n = nms3d_slots(count[b], S, O, s_valid, [&](int s) { return nms3d_box_valid(V + (size_t)s * 24, eps_coplanar, eps_nonzero); });
    const int P = S * (S - 1) / 2;
    for (int c0 = blockIdx.x * chunk; c0 < P; c0 += gridDim.x * chunk) {
        const int q = c0 + lane;
        int ia = 0, ib = 0;
        bool live = false;
        if (lane < chunk && q < P) {
            nms3d_pair(q, S, ia, ib);
            live = nms3d_pair_live(ia, ib, n, class_agnostic, C, s_valid) && !spheres_disjoint(V + (size_t)ia * 24, V + (size_t)ib * 24);
            if (!live) { O[(size_t)ia * S + ib] = 0.f; O[(size_t)ib * S + ia] = 0.f; }
        }
        iou_pair_survivors<SUB, CAPT>(Lall, __ballot(live), ia, ib, V, V, lane, [&](int pa, int pb, int, float, float iou, bool over) {
            O[(size_t)pa * S + pb] = iou;
            O[(size_t)pb * S + pa] = iou;
            if (over && overflow) atomicAdd(overflow, 1);
        });
    }
}

// ---- the steps the pick kernel and the fusion kernel (fuse3d_kernel, further down) share: 256 threads, one image ----
// High key word of slot j < n: a bit pattern that shrinks as the score grows, NMS3D_UNRANKED for a slot that takes no part (score not
// finite, box invalid, and with FIT also a box that the fit of cuboid_exact.h refuses).
template <bool FIT>
__device__ __forceinline__ unsigned nms3d_rank_hi(const float* __restrict__ box, float sc, float eps_coplanar, float eps_nonzero) {
    sc = sc + 0.0f;                                            // (-0 -> +0)
    bool ok = cx_finite(sc) && nms3d_box_valid(box, eps_coplanar, eps_nonzero);
    if (FIT && ok) {
        CxBox fitted;
        ok = cuboid_fit(box, CX_EPS_DIM, CX_FIT_TOL, fitted);
    }
    if (!ok) return NMS3D_UNRANKED;
    // bit pattern that grows with the value, for either sign; a finite score never maps to 0, so ~u is never UNRANKED
    const unsigned u = __float_as_uint(sc);
    return ~((u & 0x80000000u) ? ~u : (u | 0x80000000u));
}

// rows that can suppress anything at all, one row per wave and round, all loads independent: a step of the walk below costs a
// dependent global load and a barrier (0.7 us measured), and most rows of a real image overlap nothing
__device__ __forceinline__ void nms3d_hot_rows(const float* __restrict__ iou_b, int S, int n, float iou_thr, unsigned char* s_hot) {
    const int t = threadIdx.x;
    for (int r = t >> 6; r < n; r += 4) {
        const float* R = iou_b + (size_t)r * S;
        bool any = false;
        for (int j = t & 63; j < n; j += 64) any = any || R[j] > iou_thr;
        const unsigned long long m = __ballot(any);
        if ((t & 63) == 0) s_hot[r] = m != 0ull ? 1 : 0;
    }
}

// bitonic sort of NP (a power of two) 64-bit keys in LDS, ascending; ends on a barrier
__device__ __forceinline__ void nms3d_sort_keys(unsigned long long* s_key, int NP) {
    const int t = threadIdx.x;
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
}

// the greedy walk down the sorted keys (every thread sees the same `cur` and the same flags, so the barriers are uniform): a live
// candidate marks the later live candidates whose IoU3D with it is > iou_thr dead and reports each as removed(its slot, the head's)
template <class Removed>
__device__ __forceinline__ void nms3d_walk(const unsigned long long* s_key, unsigned char* s_dead, const unsigned char* s_hot,
                                           const float* __restrict__ iou_b, int S, int n, float iou_thr, Removed removed) {
    const int t = threadIdx.x;
    for (int cur = 0; cur < n; ++cur) {
        const unsigned long long key = s_key[cur];
        if ((unsigned)(key >> 32) == NMS3D_UNRANKED) break;          // the unranked slots sort last
        if (s_dead[cur] || !s_hot[(unsigned)key]) continue;          // (both written before the last barrier)
        const float* R = iou_b + (size_t)(unsigned)key * S;
        for (int j = cur + 1 + t; j < n; j += 256) {
            const unsigned long long kj = s_key[j];
            if ((unsigned)(kj >> 32) == NMS3D_UNRANKED) break;
            if (!s_dead[j] && R[(unsigned)kj] > iou_thr) { s_dead[j] = 1; removed((int)(unsigned)kj, (int)(unsigned)key); }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) nms3d_pick_kernel(const float* __restrict__ verts, const float* __restrict__ score,
                                                         const int* __restrict__ count, int S, float iou_thr, float eps_coplanar,
                                                         float eps_nonzero, const float* __restrict__ iou, int* __restrict__ keep,
                                                         int* __restrict__ order, int* __restrict__ new_count) {
    __shared__ unsigned long long s_key[NMS3D_MAXS];      // sorted: [~ordered score bits | slot]
    __shared__ unsigned char s_dead[NMS3D_MAXS];          // by sorted position
    __shared__ unsigned char s_keep[NMS3D_MAXS];          // by slot
    __shared__ unsigned char s_hot[NMS3D_MAXS];           // by slot: some IoU of its row exceeds the threshold
    __shared__ int s_tot[NMS3D_MAXS / 64];                // kept slots per group of 64
    const int t = threadIdx.x, b = blockIdx.x;
    int n = count[b];
    n = n < 0 ? 0 : (n > S ? S : n);
    int NP = 1;
    while (NP < n) NP <<= 1;
    // ---- 1. keys ----
    for (int j = t; j < NP; j += 256) {
        const unsigned hi = j < n ? nms3d_rank_hi<false>(verts + ((size_t)b * S + j) * 24, score[(size_t)b * S + j], eps_coplanar, eps_nonzero)
                                  : NMS3D_UNRANKED;
        s_key[j] = ((unsigned long long)hi << 32) | (unsigned)j;
        s_dead[j] = 0;
    }
    for (int s = t; s < NMS3D_MAXS; s += 256) s_keep[s] = s < n ? 1 : 0;
    nms3d_hot_rows(iou + (size_t)b * S * S, S, n, iou_thr, s_hot);
    __syncthreads();
    // ---- 2. bitonic sort, ascending keys = descending score, ties to the lower slot ----
    nms3d_sort_keys(s_key, NP);
    // ---- 3. the walk ----
    nms3d_walk(s_key, s_dead, s_hot, iou + (size_t)b * S * S, S, n, iou_thr, [&](int slot, int) { s_keep[slot] = 0; });
    // ---- 4. the kept slots in ascending order: ballots per wave, totals per group of 64 slots ----
    unsigned long long mine[NMS3D_MAXS / 256];
#pragma unroll
    for (int r = 0; r < NMS3D_MAXS / 256; ++r) {
        const int s = r * 256 + t;
        mine[r] = __ballot(s_keep[s] != 0);
        if ((t & 63) == 0) s_tot[s >> 6] = __popcll(mine[r]);
    }
    __syncthreads();
    int total = 0;
    for (int k = 0; k < NMS3D_MAXS / 64; ++k) total += s_tot[k];
#pragma unroll
    for (int r = 0; r < NMS3D_MAXS / 256; ++r) {
        const int s = r * 256 + t;
        if (s < S) {
            int pos = 0;
            for (int k = 0; k < (s >> 6); ++k) pos += s_tot[k];
            const int l = t & 63;
            pos += __popcll(mine[r] & (l == 0 ? 0ull : (~0ull >> (64 - l))));
            const bool kept = ((mine[r] >> l) & 1ull) != 0ull;
            keep[(size_t)b * S + s] = kept ? 1 : 0;
            if (kept) order[(size_t)b * S + pos] = s;
            if (s >= total) order[(size_t)b * S + s] = -1;
        }
    }
    if (t == 0) new_count[b] = total;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// omni_nms3d_exact -- omni_nms3d deciding with the exact IoU3D of cuboid_exact.h instead of the evaluator's pair algorithm, which is up
// to 0.3 off on the near-aligned duplicates this step exists for.  Launch 2 is nms3d_pick_kernel as it stands.
//   nms3d_exact_iou_kernel  one THREAD per slot pair i < j of one image, mirrored into the full (S, S) matrix; the diagonal is 0 and
//                           every entry is written.  As in nms3d_iou_kernel every wave takes the validity of its image's slots once, as
//                           ballots into LDS: a slot takes part if it passes the evaluator's test AND the fit of cuboid_exact.h.  A
//                           thread fits the two boxes of its pair itself (a twentieth of the clipping that follows) and keeps its clip
//                           lists in a [slot][thread] LDS slice (the float32 sphere screen of nms3d_iou_kernel in front of the fits was
//                           measured and costs more than it saves: +6 us clustered, +2 us sparse at B = 4, S = 100).  The slots < count whose fit fails are counted into `invalid` by the
//                           first workgroup of the image, one integer atomic each.  No atomics on the pair path, no arrival order.

__global__ void __launch_bounds__(64) nms3d_exact_iou_kernel(const float* __restrict__ verts, const int* __restrict__ cls,
                                                             const int* __restrict__ count, int S, int class_agnostic, float eps_coplanar,
                                                             float eps_nonzero, float* __restrict__ iou_out, int* __restrict__ invalid) {
    __shared__ double s_v[2 * 2 * CX_CAP * 64];                   // two clip lists [vertex][x | y][thread]: 20 KB
    __shared__ unsigned long long s_valid[NMS3D_MAXS / 64];       // bit s: slot s is in use, valid for the evaluator and a cuboid
    const int lane = threadIdx.x;
    const int b = blockIdx.y;
    const float* V = verts + (size_t)b * S * 24;
    const int* C = cls + (size_t)b * S;
    float* O = iou_out + (size_t)b * S * S;
    const int n = nms3d_slots(count[b], S, O, s_valid, [&](int s) {
        CxBox box;
        const bool fit = cuboid_fit(V + (size_t)s * 24, CX_EPS_DIM, CX_FIT_TOL, box);
        if (!fit && blockIdx.x == 0 && invalid) atomicAdd(invalid, 1);
        return fit && nms3d_box_valid(V + (size_t)s * 24, eps_coplanar, eps_nonzero);
    });
    const int P = S * (S - 1) / 2;
    for (int q = blockIdx.x * 64 + lane; q < P; q += gridDim.x * 64) {
        int ia, ib;
        nms3d_pair(q, S, ia, ib);
        float vol = 0.f, iou = 0.f;
        if (nms3d_pair_live(ia, ib, n, class_agnostic, C, s_valid)) {
            CxBox A, Bx;
            cuboid_fit(V + (size_t)ia * 24, CX_EPS_DIM, CX_FIT_TOL, A);
            cuboid_fit(V + (size_t)ib * 24, CX_EPS_DIM, CX_FIT_TOL, Bx);
            cuboid_pair_iou<64>(A, Bx, s_v + lane, s_v + 2 * CX_CAP * 64 + lane, vol, iou);
        }
        O[(size_t)ia * S + ib] = iou;
        O[(size_t)ib * S + ia] = iou;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// omni_fuse3d -- weighted fusion of overlapping cuboids (test-time augmentation: the views' detections share the slots of one image).
// Launch 1 is nms3d_exact_iou_kernel as it stands.  Launch 2, fuse3d_kernel, one 256-thread workgroup per image:
//   1. ranking    the keys, the sort and the walk of nms3d_pick_kernel (the shared functions above); a slot takes part only if the
//                 fit accepts it too.  The walk records, per removed slot, the head that removed it.
//   2. clusters   a head is a ranked position that is not dead, or an unranked slot < count (a cluster of its own).  One thread per
//                 head links its members into a chain s_next[position] in rank order, sums their raw scores in that order and
//                 writes the key [~ordered fused score bits | head slot] of the second sort (a fused score that is not finite sorts
//                 behind the finite ones, by slot; the positions that are no head sort behind everything).
//   3. fusion     ONE THREAD PER CLUSTER walks its chain: members in rank order, every sum in double in that order.  The clusters
//                 of test-time augmentation are many and small (at most one member per view when the views agree), so a thread per
//                 cluster keeps the lanes busy where a wave per cluster would idle 60 of 64, and the order of every sum is fixed
//                 without a reduction tree.  A cluster of one member, or of total weight 0, hands its head through bit for bit.
//   4. aux        one thread per (output row, column), the same chain and the same weights.
// LDS: two key arrays (16 KB), flags (2 KB), head / position / next as 16-bit (6 KB): 24 KB at S = 1024.  No atomics; nothing
// depends on the order in which threads arrive.

constexpr unsigned long long FUSE3D_PAD = ~0ull;      // key of a sorted position that heads no cluster

// member `m` re-expressed in the axis naming of head `h`: the first permutation p of (0,1,2) in lexicographic order that maximises
// sum_k |h.x[k] . m.x[p(k)]|, the signs that make every such product >= 0 -> ax[k] = s_k m.x[p(k)], dd[k] = m.d[p(k)]
__device__ __forceinline__ void fuse3d_align(const CxBox& h, const CxBox& m, double ax[3][3], double dd[3]) {
    double dot[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j) dot[k][j] = h.x[k][0] * m.x[j][0] + h.x[k][1] * m.x[j][1] + h.x[k][2] * m.x[j][2];
    constexpr int P[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    double best = -1.0;
    int pick = 0;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const double v = (fabs(dot[0][P[q][0]]) + fabs(dot[1][P[q][1]])) + fabs(dot[2][P[q][2]]);
        if (v > best) { best = v; pick = q; }
    }
#pragma unroll
    for (int q = 0; q < 6; ++q)                        // constant indices only: nothing here is indexed at run time
        if (q == pick) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double sg = dot[k][P[q][k]] >= 0.0 ? 1.0 : -1.0;
                dd[k] = m.d[P[q][k]];
#pragma unroll
                for (int a = 0; a < 3; ++a) ax[k][a] = sg * m.x[P[q][k]][a];
            }
        }
}

// the orthogonal polar factor of X (close to orthogonal): Newton's X <- (X + X^-T) / 2, whose error squares with every step; a
// matrix that has no inverse to speak of is left as it is (the caller falls back to the head's axes)
__device__ __forceinline__ bool fuse3d_polar(double X[3][3]) {
    for (int it = 0; it < 8; ++it) {
        double C[3][3];                                // cofactors: X^-T = C / det
        C[0][0] = X[1][1] * X[2][2] - X[1][2] * X[2][1]; C[0][1] = X[1][2] * X[2][0] - X[1][0] * X[2][2]; C[0][2] = X[1][0] * X[2][1] - X[1][1] * X[2][0];
        C[1][0] = X[2][1] * X[0][2] - X[2][2] * X[0][1]; C[1][1] = X[2][2] * X[0][0] - X[2][0] * X[0][2]; C[1][2] = X[2][0] * X[0][1] - X[2][1] * X[0][0];
        C[2][0] = X[0][1] * X[1][2] - X[0][2] * X[1][1]; C[2][1] = X[0][2] * X[1][0] - X[0][0] * X[1][2]; C[2][2] = X[0][0] * X[1][1] - X[0][1] * X[1][0];
        const double det = (X[0][0] * C[0][0] + X[0][1] * C[0][1]) + X[0][2] * C[0][2];
        if (!(fabs(det) > 1e-6)) return false;
        const double inv = 1.0 / det;
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int a = 0; a < 3; ++a) X[k][a] = 0.5 * (X[k][a] + C[k][a] * inv);
    }
    return true;
}

__global__ void __launch_bounds__(256) fuse3d_kernel(
    const float* __restrict__ verts, const float* __restrict__ score, const int* __restrict__ cls, const int* __restrict__ count,
    const float* __restrict__ aux, int S, int A, int views, float iou_thr, float eps_coplanar, float eps_nonzero,
    const float* __restrict__ iou, int* __restrict__ cluster, float* __restrict__ out_verts, float* __restrict__ out_centre,
    float* __restrict__ out_axes, float* __restrict__ out_dims, float* __restrict__ out_score, int* __restrict__ out_cls,
    float* __restrict__ out_aux, int* __restrict__ out_size, int* __restrict__ out_head, int* __restrict__ out_count) {
    __shared__ unsigned long long s_key[NMS3D_MAXS];      // sorted: [~ordered score bits | slot]
    __shared__ unsigned long long s_okey[NMS3D_MAXS];     // sorted: [~ordered fused score bits | head slot], then FUSE3D_PAD
    __shared__ unsigned char s_dead[NMS3D_MAXS];          // by sorted position
    __shared__ unsigned char s_hot[NMS3D_MAXS];           // by slot: some IoU of its row exceeds the threshold
    __shared__ short s_head[NMS3D_MAXS];                  // by slot: the head of its cluster
    __shared__ short s_pos[NMS3D_MAXS];                   // by slot: its sorted position
    __shared__ short s_next[NMS3D_MAXS];                  // by sorted position: the next member of its cluster, -1 at the end
    const int t = threadIdx.x, b = blockIdx.x;
    int n = count[b];
    n = n < 0 ? 0 : (n > S ? S : n);
    int NP = 1;
    while (NP < n) NP <<= 1;
    const float* V = verts + (size_t)b * S * 24;
    const float* SC = score + (size_t)b * S;
    const float* IOU = iou + (size_t)b * S * S;
    // ---- 1. ranking ----
    for (int j = t; j < NP; j += 256) {
        const unsigned hi = j < n ? nms3d_rank_hi<true>(V + (size_t)j * 24, SC[j], eps_coplanar, eps_nonzero) : NMS3D_UNRANKED;
        s_key[j] = ((unsigned long long)hi << 32) | (unsigned)j;
        s_dead[j] = 0;
        s_head[j] = (short)j;
    }
    nms3d_hot_rows(IOU, S, n, iou_thr, s_hot);
    __syncthreads();
    nms3d_sort_keys(s_key, NP);
    nms3d_walk(s_key, s_dead, s_hot, IOU, S, n, iou_thr, [&](int slot, int head) { s_head[slot] = (short)head; });
    __syncthreads();
    // ---- 2. clusters: chains, fused scores, keys of the output order ----
    for (int p = t; p < NP; p += 256) {
        unsigned long long okey = FUSE3D_PAD;
        if (p < n) {
            const unsigned long long key = s_key[p];
            const int slot = (int)(unsigned)key;
            const bool ranked = (unsigned)(key >> 32) != NMS3D_UNRANKED;
            s_pos[slot] = (short)p;
            if (!ranked || !s_dead[p]) {
                double ssum = (double)SC[slot];
                int members = 1, prev = p;
                if (ranked && s_hot[slot])
                    for (int q = p + 1; q < n; ++q) {
                        const unsigned long long kq = s_key[q];
                        if ((unsigned)(kq >> 32) == NMS3D_UNRANKED) break;
                        if (s_dead[q] && s_head[(unsigned)kq] == slot) {
                            s_next[prev] = (short)q;
                            prev = q;
                            ++members;
                            ssum += (double)SC[(unsigned)kq];
                        }
                    }
                s_next[prev] = -1;
                const float fs = (float)(ssum / (double)(members > views ? members : views)) + 0.0f;
                const unsigned u = __float_as_uint(fs);
                const unsigned hi = cx_finite(fs) ? ~((u & 0x80000000u) ? ~u : (u | 0x80000000u)) : NMS3D_UNRANKED;
                okey = ((unsigned long long)hi << 32) | (unsigned)slot;
            }
        }
        s_okey[p] = okey;
    }
    __syncthreads();
    nms3d_sort_keys(s_okey, NP);
    int ncl = 0;                                          // the clusters sort in front of the padding
    for (int step = NP; step > 0; step >>= 1)
        if (ncl + step <= NP && s_okey[ncl + step - 1] != FUSE3D_PAD) ncl += step;
    // ---- 3. fusion: a thread per output row ----
    for (int r = t; r < S; r += 256) {
        const size_t g = (size_t)b * S + r;
        if (r >= ncl) {
            for (int k = 0; k < 24; ++k) out_verts[g * 24 + k] = 0.f;
            for (int k = 0; k < 9; ++k) out_axes[g * 9 + k] = 0.f;
            for (int k = 0; k < 3; ++k) { out_centre[g * 3 + k] = 0.f; out_dims[g * 3 + k] = 0.f; }
            out_score[g] = 0.f; out_cls[g] = 0; out_size[g] = 0; out_head[g] = -1;
            continue;
        }
        const int slot = (int)(unsigned)s_okey[r];
        const int p = s_pos[slot];
        CxBox H;
        cuboid_fit(V + (size_t)slot * 24, CX_EPS_DIM, CX_FIT_TOL, H);          // zeros for a box that is none
        const double wh = fmax((double)SC[slot], 0.0);
        double sw = wh, ssum = (double)SC[slot], sc[3], sd[3], M[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            sc[k] = wh * H.c[k];
            sd[k] = wh * H.d[k];
#pragma unroll
            for (int a = 0; a < 3; ++a) M[k][a] = wh * H.x[k][a];
        }
        int members = 1;
        for (int q = s_next[p]; q >= 0; q = s_next[q]) {
            const int js = (int)(unsigned)s_key[q];
            CxBox Mb;
            cuboid_fit(V + (size_t)js * 24, CX_EPS_DIM, CX_FIT_TOL, Mb);
            double ax[3][3], dd[3];
            fuse3d_align(H, Mb, ax, dd);
            const double w = fmax((double)SC[js], 0.0);
            sw += w;
            ssum += (double)SC[js];
            ++members;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                sc[k] += w * Mb.c[k];
                sd[k] += w * dd[k];
#pragma unroll
                for (int a = 0; a < 3; ++a) M[k][a] += w * ax[k][a];
            }
        }
        bool fused = members > 1 && sw > 0.0;
        if (fused) {
            const double inv = 1.0 / sw;
            double X[3][3];
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int a = 0; a < 3; ++a) X[k][a] = M[k][a] * inv;
            if (fuse3d_polar(X)) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    H.c[k] = sc[k] * inv;
                    H.d[k] = sd[k] * inv;
#pragma unroll
                    for (int a = 0; a < 3; ++a) H.x[k][a] = X[k][a];
                }
            } else {
                fused = false;
            }
        }
        if (fused) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {                  // the corner order of boxgen.UNIT, as in cuboid_fit
                const double s0 = (k == 1 || k == 2 || k == 5 || k == 6) ? 0.5 : -0.5;
                const double s1 = (k == 2 || k == 3 || k == 6 || k == 7) ? 0.5 : -0.5;
                const double s2 = k >= 4 ? 0.5 : -0.5;
#pragma unroll
                for (int a = 0; a < 3; ++a)
                    out_verts[g * 24 + 3 * k + a] = (float)(H.c[a] + ((s0 * H.d[0]) * H.x[0][a] + (s1 * H.d[1]) * H.x[1][a] + (s2 * H.d[2]) * H.x[2][a]));
            }
        } else {
            for (int k = 0; k < 24; ++k) out_verts[g * 24 + k] = V[(size_t)slot * 24 + k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            out_centre[g * 3 + k] = (float)H.c[k];
            out_dims[g * 3 + k] = (float)H.d[k];
#pragma unroll
            for (int a = 0; a < 3; ++a) out_axes[g * 9 + 3 * k + a] = (float)H.x[k][a];
        }
        out_score[g] = (float)(ssum / (double)(members > views ? members : views));
        out_cls[g] = cls[(size_t)b * S + slot];
        out_size[g] = members;
        out_head[g] = slot;
    }
    // ---- 4. aux columns: a thread per (row, column) ----
    const long long cells = (long long)S * A;
    for (long long e = t; e < cells; e += 256) {
        const int r = (int)(e / A), col = (int)(e % A);
        float v = 0.f;
        if (r < ncl) {
            const int slot = (int)(unsigned)s_okey[r];
            const float* AX = aux + (size_t)b * S * A;
            const double wh = fmax((double)SC[slot], 0.0);
            double sw = wh, sa = wh * (double)AX[(size_t)slot * A + col];
            int members = 1;
            for (int q = s_next[s_pos[slot]]; q >= 0; q = s_next[q]) {
                const int js = (int)(unsigned)s_key[q];
                const double w = fmax((double)SC[js], 0.0);
                sw += w;
                sa += w * (double)AX[(size_t)js * A + col];
                ++members;
            }
            v = members > 1 && sw > 0.0 ? (float)(sa / sw) : AX[(size_t)slot * A + col];
        }
        out_aux[((size_t)b * S + r) * A + col] = v;
    }
    for (int s = t; s < S; s += 256) cluster[(size_t)b * S + s] = s < n ? (int)s_head[s] : -1;
    if (t == 0) out_count[b] = ncl;
}

// the pair-matrix launch (launch_pairs(grid, stream): S (S - 1) / 2 pairs per image, `per_wave` of them per wave and round, at most
// ~max_waves workgroups over the B images), then the pick launch
static dim3 nms3d_pair_grid(int per_wave, int max_waves, int B, int S) {
    const long long P = (long long)S * (S - 1) / 2;
    long long gx = (P + per_wave - 1) / per_wave, cap = (max_waves + B - 1) / B;
    gx = gx > cap ? cap : gx;
    gx = gx < 1 ? 1 : gx;
    return dim3((unsigned)gx, (unsigned)B);
}

template <class LaunchPairs>
static int nms3d_launch(int per_wave, int max_waves, const float* verts, const float* score, const int* count, int B, int S, float iou_thr,
                        float eps_coplanar, float eps_nonzero, float* iou, int* keep, int* order, int* new_count, void* stream,
                        LaunchPairs launch_pairs) {
    hipStream_t st = (hipStream_t)stream;
    launch_pairs(nms3d_pair_grid(per_wave, max_waves, B, S), st);
    hipLaunchKernelGGL(nms3d_pick_kernel, dim3((unsigned)B), dim3(256), 0, st, verts, score, count, S, iou_thr, eps_coplanar,
                       eps_nonzero, iou, keep, order, new_count);
    return omni_launch_status();
}

}  // namespace

extern "C" {

// verts (B*S, 8, 3), score (B*S), cls (B*S), count (B) -> iou (B, S, S) (every entry written), keep (B, S), order (B, S), new_count (B);
// overflow (1) is incremented like that of omni_iou_box3d
int omni_nms3d(const float* verts, const float* score, const int* cls, const int* count, int B, int S, float iou_thr,
               int class_agnostic, float eps_coplanar, float eps_nonzero, float* iou, int* keep, int* order, int* new_count,
               int* overflow, void* stream) {
    if (B < 0 || S < 0 || S > NMS3D_MAXS || B > 65535) return OMNI_ERR_ARG;
    if (B == 0 || S == 0) return OMNI_OK;
    const int chunk = iou_chunk((long long)S * (S - 1) / 2 * B);
    return nms3d_launch(chunk, 256 * 16, verts, score, count, B, S, iou_thr, eps_coplanar, eps_nonzero, iou, keep, order, new_count, stream,
                        [&](dim3 grid, hipStream_t st) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(nms3d_iou_kernel<32, CAP>), grid, dim3(64), 0, st, verts, cls, count, S, class_agnostic,
                           eps_coplanar, eps_nonzero, iou, overflow, chunk);
    });
}

// the arguments of omni_nms3d; `invalid` (1) is incremented once per slot < count whose corners are no cuboid (the caller zeroes it)
int omni_nms3d_exact(const float* verts, const float* score, const int* cls, const int* count, int B, int S, float iou_thr,
                     int class_agnostic, float eps_coplanar, float eps_nonzero, float* iou, int* keep, int* order, int* new_count,
                     int* invalid, void* stream) {
    if (B < 0 || S < 0 || S > NMS3D_MAXS || B > 65535) return OMNI_ERR_ARG;
    if (B == 0 || S == 0) return OMNI_OK;
    if (!verts || !score || !cls || !count || !iou || !keep || !order || !new_count) return OMNI_ERR_ARG;
    return nms3d_launch(64, 256 * 8, verts, score, count, B, S, iou_thr, eps_coplanar, eps_nonzero, iou, keep, order, new_count, stream,
                        [&](dim3 grid, hipStream_t st) {
        hipLaunchKernelGGL(nms3d_exact_iou_kernel, grid, dim3(64), 0, st, verts, cls, count, S, class_agnostic, eps_coplanar, eps_nonzero,
                           iou, invalid);
    });
}

// the inputs of omni_nms3d_exact + aux (B*S, A) [null when A == 0] and the number of views -> iou (B, S, S), cluster (B, S) and the
// fused rows in descending fused score (include/omni3d_hip.h)
int omni_fuse3d(const float* verts, const float* score, const int* cls, const int* count, const float* aux, int B, int S, int A, int views,
                float iou_thr, int class_agnostic, float eps_coplanar, float eps_nonzero, float* iou, int* cluster, float* out_verts,
                float* out_centre, float* out_axes, float* out_dims, float* out_score, int* out_cls, float* out_aux, int* out_size,
                int* out_head, int* out_count, int* invalid, void* stream) {
    if (B < 0 || S < 0 || S > NMS3D_MAXS || B > 65535 || A < 0 || views < 1) return OMNI_ERR_ARG;
    if (B == 0 || S == 0) return OMNI_OK;
    if (!verts || !score || !cls || !count || !iou || !cluster || !out_verts || !out_centre || !out_axes || !out_dims || !out_score ||
        !out_cls || !out_size || !out_head || !out_count || (A > 0 && (!aux || !out_aux)))
        return OMNI_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(nms3d_exact_iou_kernel, nms3d_pair_grid(64, 256 * 8, B, S), dim3(64), 0, st, verts, cls, count, S, class_agnostic,
                       eps_coplanar, eps_nonzero, iou, invalid);
    hipLaunchKernelGGL(fuse3d_kernel, dim3((unsigned)B), dim3(256), 0, st, verts, score, cls, count, aux, S, A, views, iou_thr, eps_coplanar,
                       eps_nonzero, (const float*)iou, cluster, out_verts, out_centre, out_axes, out_dims, out_score, out_cls, out_aux, out_size,
                       out_head, out_count);
    return omni_launch_status();
}

}  // extern "C"
