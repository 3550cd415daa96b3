// tp_errors.hip -- the true-positive errors of the centre-distance protocol (nuScenes): how far, how much too large and how much turned
// a matched cuboid is, and their averages along the recall curve (ATE / ASE / AOE).  The reference has no counterpart: its evaluator
// reports AP by 2D IoU or IoU3D only; `Omni3Deval(mode="DIST")` (cubercnn/evaluation/omni3d_evaluation.py) is built on these two.
//
//   pair_errors_kernel     one thread per pair of fitted cuboids (omni_cuboid_fit: centre, unit axes, dimensions, all double):
//                            trans   |d|, d = centre1 - centre2; with an up vector u the distance in the ground plane orthogonal to it,
//                                    sqrt(max(0, |d|^2 - (d.u)^2))
//                            scale   1 - inter / (V1 + V2 - inter), inter = prod_k min(dims1[k], dims2[k]): one minus the IoU of the two
//                                    boxes after aligning centre and orientation, axis k paired with axis k
//                            orient  the geodesic angle of R = R1 R2^T (R = the matrix whose columns are the unit axes),
//                                    atan2(0.5 |(R32 - R23, R13 - R31, R21 - R12)|, 0.5 (trace R - 1)): in [0, pi], well conditioned at
//                                    both ends (acos of the trace alone loses half the digits there)
//                          (+inf, NaN, NaN) for a pair with an invalid box or an index outside its set.  No atomics, no barrier.
//   tp_errors_kernel       one 64-lane wave per (category k, depth range a), laid out like eval_accumulate_kernel (csrc/eval_match.hip).
//                          The category's detections are walked in the merge order of accumulate() in chunks of 64; a detection that
//                          is matched and not ignored is a true positive, its error row is pair_row[d] + dt_match[d].  The running
//                          number of true positives is a ballot prefix, the three running sums an inclusive Hillis-Steele scan over
//                          the lanes plus the carry of the chunks before; at the c-th true positive m_c = sums / c, and it is taken
//                          by every recall threshold r_j >= min_recall with (c-1)/npig < r_j <= c/npig -- the doubles, expressions and
//                          binary searches of eval_accumulate_kernel.  Each lane keeps what its own true positives were taken for,
//                          a butterfly adds the lanes at the end: the order of every addition depends on lane numbers only, so two
//                          launches give the same bits.  No floating-point atomics.
//
// No fused multiply-add in this file: the host emulator and the device then do the same arithmetic.
#include <device_rt.h>

#pragma clang fp contract(off)

namespace {

constexpr int TPE_T = 64;          // threads per workgroup: one wave

struct TpeBox {
    double c[3], x[3][3], d[3];
};

__device__ __forceinline__ void tpe_load(TpeBox& b, const double* __restrict__ centre, const double* __restrict__ axes,
                                         const double* __restrict__ dims, long i) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        b.c[a] = centre[3 * i + a];
        b.d[a] = dims[3 * i + a];
#pragma unroll
        for (int k = 0; k < 3; ++k) b.x[k][a] = axes[9 * i + 3 * k + a];
    }
}

__global__ void __launch_bounds__(TPE_T) pair_errors_kernel(const double* __restrict__ centre1, const double* __restrict__ axes1,
                                                            const double* __restrict__ dims1, const int* __restrict__ valid1, int n1,
                                                            const double* __restrict__ centre2, const double* __restrict__ axes2,
                                                            const double* __restrict__ dims2, const int* __restrict__ valid2, int n2,
                                                            const int* __restrict__ idx1, const int* __restrict__ idx2, long P, double ux,
                                                            double uy, double uz, double* __restrict__ err) {
    const long p = (long)blockIdx.x * TPE_T + threadIdx.x;
    if (p >= P) return;
    const int i1 = idx1[p], i2 = idx2[p];
    const double nan = __builtin_nan(""), inf = __builtin_huge_val();
    double trans = inf, scale = nan, orient = nan;
    if ((unsigned)i1 < (unsigned)n1 && (unsigned)i2 < (unsigned)n2 && valid1[i1] != 0 && valid2[i2] != 0) {
        TpeBox A, B;
        tpe_load(A, centre1, axes1, dims1, i1);
        tpe_load(B, centre2, axes2, dims2, i2);
        // a set that did not come from omni_cuboid_fit: a box without a volume is an invalid one
        if (A.d[0] > 0.0 && A.d[1] > 0.0 && A.d[2] > 0.0 && B.d[0] > 0.0 && B.d[1] > 0.0 && B.d[2] > 0.0) {
            const double d0 = A.c[0] - B.c[0], d1 = A.c[1] - B.c[1], d2 = A.c[2] - B.c[2];
            const double along = (d0 * ux + d1 * uy) + d2 * uz;            // 0 without an up vector
            trans = sqrt(fmax(((d0 * d0 + d1 * d1) + d2 * d2) - along * along, 0.0));
            const double inter = (fmin(A.d[0], B.d[0]) * fmin(A.d[1], B.d[1])) * fmin(A.d[2], B.d[2]);
            const double va = (A.d[0] * A.d[1]) * A.d[2], vb = (B.d[0] * B.d[1]) * B.d[2];
            scale = 1.0 - inter / ((va + vb) - inter);
            double R[3][3];                                                 // R[i][j] = sum_k A.x[k][i] B.x[k][j]
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) R[i][j] = (A.x[0][i] * B.x[0][j] + A.x[1][i] * B.x[1][j]) + A.x[2][i] * B.x[2][j];
            const double v0 = R[2][1] - R[1][2], v1 = R[0][2] - R[2][0], v2 = R[1][0] - R[0][1];
            const double s = 0.5 * sqrt((v0 * v0 + v1 * v1) + v2 * v2);
            const double c = 0.5 * (((R[0][0] + R[1][1]) + R[2][2]) - 1.0);
            orient = atan2(s, c);
        }
    }
    err[3 * p] = trans;
    err[3 * p + 1] = scale;
    err[3 * p + 2] = orient;
}

struct TpeP {
    const int* order;            // (N) detection index by sorted position (the merge order of accumulate())
    const int* cat_off;          // (K + 1) ranges of `order` per category
    const int* dt_match;         // (A, sumD) at the tpDist threshold: >= 0 matched (index of the gt inside its group)
    const unsigned char* dt_ig;  // (A, sumD)
    const long long* pair_row;   // (sumD) row of the pair (d, gt 0) in err
    const double* err;           // (P, 3)
    const int* npig;             // (K, A)
    const int* has_e;            // (K)
    const double* rec_thrs;      // (R) ascending
    double min_recall;
    int K, A, R, sumD;
    long long P;
    double* tp_err;              // (K, A, 3)
    int* tp_count;               // (K, A)
};

__device__ __forceinline__ double tpe_scan(double v, int lane) {      // inclusive prefix sum over the lanes, lane order fixed
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_up(v, (unsigned)d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

__device__ __forceinline__ double tpe_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__device__ __forceinline__ int tpe_upper(const double* __restrict__ thr, int R, double x) {       // #thr <= x
    int lo = 0, hi = R;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (thr[mid] <= x) lo = mid + 1; else hi = mid; }
    return lo;
}

__global__ void __launch_bounds__(TPE_T) tp_errors_kernel(TpeP p) {
    const int a = blockIdx.x % p.A, k = blockIdx.x / p.A;
    const int lane = threadIdx.x;
    if (!p.has_e[k]) return;                                      // no evaluated image: the -1 of the caller stays
    const int npig = p.npig[k * p.A + a];
    if (npig == 0) return;
    const int s0 = p.cat_off[k], s1 = p.cat_off[k + 1];
    const int* dtm = p.dt_match + (long)a * p.sumD;
    const unsigned char* dtg = p.dt_ig + (long)a * p.sumD;
    int jmin = 0, hi = p.R;                                       // #thr < min_recall
    while (jmin < hi) { const int mid = (jmin + hi) >> 1; if (p.rec_thrs[mid] < p.min_recall) jmin = mid + 1; else hi = mid; }
    const double nan = __builtin_nan("");
    int tp_before = 0, taken = 0;
    double carry0 = 0.0, carry1 = 0.0, carry2 = 0.0, acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
    const int nchunk = (s1 - s0 + 63) / 64;
    for (int c = 0; c < nchunk; ++c) {
        const int s = s0 + c * 64 + lane;
        bool is_tp = false;
        double e0 = 0.0, e1 = 0.0, e2 = 0.0;
        if (s < s1) {
            const int d = p.order[s];
            if ((unsigned)d < (unsigned)p.sumD && dtm[d] >= 0 && dtg[d] == 0) {
                is_tp = true;
                const long long row = p.pair_row[d] + dtm[d];
                const bool in = row >= 0 && row < p.P;              // a row outside the table: NaN, nothing is read
                e0 = in ? p.err[3 * row] : nan;
                e1 = in ? p.err[3 * row + 1] : nan;
                e2 = in ? p.err[3 * row + 2] : nan;
            }
        }
        const unsigned long long tpm = __ballot(is_tp);
        const unsigned long long upto = lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1ull);
        const int cnt = tp_before + __popcll(tpm & upto);         // true positives up to and including this element
        const double c0 = tpe_scan(e0, lane), c1 = tpe_scan(e1, lane), c2 = tpe_scan(e2, lane);
        if (is_tp) {
            const double rc = (double)cnt / npig, rc_prev = (double)(cnt - 1) / npig;
            const int jlo = max(tpe_upper(p.rec_thrs, p.R, rc_prev), jmin), jhi = tpe_upper(p.rec_thrs, p.R, rc);
            if (jhi > jlo) {
                const double w = (double)(jhi - jlo), n = (double)cnt;
                acc0 += w * ((carry0 + c0) / n);
                acc1 += w * ((carry1 + c1) / n);
                acc2 += w * ((carry2 + c2) / n);
                taken += jhi - jlo;
            }
        }
        tp_before += __popcll(tpm);
        carry0 += __shfl(c0, 63, 64);
        carry1 += __shfl(c1, 63, 64);
        carry2 += __shfl(c2, 63, 64);
    }
    taken = wave_sum_i(taken);
    acc0 = tpe_sum(acc0);
    acc1 = tpe_sum(acc1);
    acc2 = tpe_sum(acc2);
    if (lane == 0) {
        double* o = p.tp_err + 3L * (k * p.A + a);
        o[0] = taken ? acc0 / taken : 1.0;                        // ground truth but no recall threshold reached: 1
        o[1] = taken ? acc1 / taken : 1.0;
        o[2] = taken ? acc2 / taken : 1.0;
        p.tp_count[k * p.A + a] = tp_before;
    }
}

}  // namespace

extern "C" {

int omni_pair_errors(const double* centre1, const double* axes1, const double* dims1, const int* valid1, int n1, const double* centre2,
                     const double* axes2, const double* dims2, const int* valid2, int n2, const int* idx1, const int* idx2,
                     long long npairs, double upx, double upy, double upz, double* err, void* stream) {
    if (n1 < 0 || n2 < 0 || npairs < 0 || npairs > (long long)TPE_T * 0x7fffffffLL) return OMNI_ERR_ARG;
    const double u2 = (upx * upx + upy * upy) + upz * upz;        // all zeros, or a unit vector (also refuses a NaN)
    if (!(u2 == 0.0 || fabs(u2 - 1.0) <= 1e-9)) return OMNI_ERR_ARG;
    if (npairs == 0) return OMNI_OK;
    if (!idx1 || !idx2 || !err) return OMNI_ERR_ARG;
    if ((n1 > 0 && (!centre1 || !axes1 || !dims1 || !valid1)) || (n2 > 0 && (!centre2 || !axes2 || !dims2 || !valid2))) return OMNI_ERR_ARG;
    hipLaunchKernelGGL(pair_errors_kernel, dim3((unsigned)((npairs + TPE_T - 1) / TPE_T)), dim3(TPE_T), 0, (hipStream_t)stream, centre1,
                       axes1, dims1, valid1, n1, centre2, axes2, dims2, valid2, n2, idx1, idx2, (long)npairs, upx, upy, upz, err);
    return omni_launch_status();
}

int omni_eval_tp_errors(const int* order, const int* cat_off, const int* dt_match, const unsigned char* dt_ignore,
                        const long long* pair_row, const double* err, long long npairs, const int* npig, const int* has_e,
                        const double* rec_thrs, double min_recall, int K, int A, int R, int sumD, double* tp_err, int* tp_count,
                        void* stream) {
    if (K < 0 || A <= 0 || R <= 0 || sumD < 0 || npairs < 0 || !(min_recall >= 0.0 && min_recall <= 1.0)) return OMNI_ERR_ARG;
    if ((long long)K * A > 0x7fffffffLL) return OMNI_ERR_ARG;
    if (K == 0) return OMNI_OK;
    if (!cat_off || !npig || !has_e || !rec_thrs || !tp_err || !tp_count) return OMNI_ERR_ARG;
    if (sumD > 0 && (!order || !dt_match || !dt_ignore || !pair_row)) return OMNI_ERR_ARG;
    if (npairs > 0 && !err) return OMNI_ERR_ARG;
    TpeP p{order, cat_off, dt_match, dt_ignore, pair_row, err, npig, has_e, rec_thrs, min_recall, K, A, R, sumD, npairs, tp_err, tp_count};
    hipLaunchKernelGGL(tp_errors_kernel, dim3((unsigned)((long)K * A)), dim3(TPE_T), 0, (hipStream_t)stream, p);
    return omni_launch_status();
}

}  // extern "C"
