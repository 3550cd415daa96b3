// let_iou.hip -- the longitudinal-error-tolerant 3D metrics (LET-3D-AP / LET-3D-APL, Hung et al. 2022, the camera-only metric of the
// Waymo Open Dataset): a monocular detection may slide along its own line of sight onto the ground truth before the IoU3D is taken,
// and the precision is scaled by how little sliding that needed.  The reference has no counterpart; `Omni3Deval(mode="LET")`
// (cubercnn/evaluation/omni3d_evaluation.py) is built on these two.
//
//   let_pairs_kernel       one thread per pair of fitted cuboids (omni_cuboid_fit), detection P and ground truth G, the sensor at the
//                          origin, all in double:
//                            u    = P / |P|                          the detection's line of sight
//                            lon  = (G - P) . u                      signed longitudinal error, > 0: predicted too near
//                            T    = max(tol_frac |G|, tol_min)
//                            aff  = 1 - min(|lon| / T, 1)            longitudinal affinity in [0, 1]
//                            iou  = the exact IoU3D (cuboid_pair_iou of cuboid_exact.h) of the ground truth and the detection with its
//                                   centre moved to P + lon u, the point of its ray closest to G, when aff > 0; exactly 0 otherwise
//                          (0, 0, NaN) for a gated pair: an invalid box, an index outside its set, or |P| <= CX_EPS_DIM.  The clip
//                          lists are the per-thread LDS slices of iou3d_exact_pairs_kernel (csrc/iou3d_exact.hip): one wave per
//                          workgroup, 20 KB.  No atomics, no barrier.
//   let_accumulate_kernel  one 64-lane wave per (category k, depth range a, maxDets m, threshold t), laid out like
//                          eval_accumulate_kernel (csrc/eval_match.hip), on the same merge order and match tables.  At list position s
//                          the longitudinal precision is prec_L(s) = (sum of aff over the true positives up to s) / (tp + fp + eps);
//                          precision_l[j] = max of prec_L over the positions from the one that first reaches recall threshold r_j on
//                          (the monotone envelope sampled by searchsorted(side='left'), as `precision` is).  The list is walked FORWARD
//                          in chunks of 64: tp / fp are ballot prefixes, the sums of aff and lon an inclusive Hillis-Steele scan over
//                          the lanes plus the carry of the chunks before (tp_errors_kernel's), the envelope inside a chunk a suffix
//                          maximum over the lanes.  Lane l owns the thresholds l, l + 64, ... : the list is walked once per batch of
//                          64 thresholds, and an owner reads the chunk's suffix maximum at the lane of the true positive that reaches
//                          its threshold (lane 0 once reached).  The order of every addition depends on lane numbers only: two
//                          launches give the same bits.  No floating-point atomics.
//
// No fused multiply-add in this file: the host emulator and the device then take the same decisions on the same bits.
#include <device_rt.h>

#pragma clang fp contract(off)

#include "cuboid_exact.h"

namespace {

constexpr int LET_T = 64;          // threads per workgroup: one wave

__device__ __forceinline__ void let_load(CxBox& b, const double* __restrict__ centre, const double* __restrict__ axes,
                                         const double* __restrict__ dims, long i) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        b.c[a] = centre[3 * i + a];
        b.d[a] = dims[3 * i + a];
#pragma unroll
        for (int k = 0; k < 3; ++k) b.x[k][a] = axes[9 * i + 3 * k + a];
    }
}

__global__ void __launch_bounds__(LET_T) let_pairs_kernel(const double* __restrict__ centre1, const double* __restrict__ axes1,
                                                          const double* __restrict__ dims1, const int* __restrict__ valid1, int n1,
                                                          const double* __restrict__ centre2, const double* __restrict__ axes2,
                                                          const double* __restrict__ dims2, const int* __restrict__ valid2, int n2,
                                                          const int* __restrict__ idx1, const int* __restrict__ idx2, long P,
                                                          double tol_frac, double tol_min, float* __restrict__ iou,
                                                          double* __restrict__ aff, double* __restrict__ lon) {
    __shared__ double s_v[2 * 2 * CX_CAP * LET_T];                 // two lists [vertex][x | y][thread]: 20 KB
    const int t = threadIdx.x;
    const long p = (long)blockIdx.x * LET_T + t;
    if (p >= P) return;
    const int i1 = idx1[p], i2 = idx2[p];
    float r = 0.0f;
    double af = 0.0, lo = __builtin_nan("");
    if ((unsigned)i1 < (unsigned)n1 && (unsigned)i2 < (unsigned)n2 && valid1[i1] != 0 && valid2[i2] != 0) {
        CxBox A, B;
        let_load(A, centre1, axes1, dims1, i1);
        let_load(B, centre2, axes2, dims2, i2);
        const double range = sqrt((A.c[0] * A.c[0] + A.c[1] * A.c[1]) + A.c[2] * A.c[2]);
        // a set that did not come from omni_cuboid_fit: a box without a volume is an invalid one; a detection on the sensor has no ray
        if (A.d[0] > 0.0 && A.d[1] > 0.0 && A.d[2] > 0.0 && B.d[0] > 0.0 && B.d[1] > 0.0 && B.d[2] > 0.0 && range > CX_EPS_DIM) {
            const double u0 = A.c[0] / range, u1 = A.c[1] / range, u2 = A.c[2] / range;
            const double l = ((B.c[0] - A.c[0]) * u0 + (B.c[1] - A.c[1]) * u1) + (B.c[2] - A.c[2]) * u2;
            const double tol = fmax(tol_frac * sqrt((B.c[0] * B.c[0] + B.c[1] * B.c[1]) + B.c[2] * B.c[2]), tol_min);
            const double a = 1.0 - fmin(fabs(l) / tol, 1.0);
            if (l == l && a == a) {                                // non-finite centres in a hand-made set: the pair stays gated
                lo = l;
                af = a;
                if (a > 0.0) {
                    A.c[0] += l * u0;
                    A.c[1] += l * u1;
                    A.c[2] += l * u2;
                    float v;
                    cuboid_pair_iou<LET_T>(A, B, s_v + t, s_v + 2 * CX_CAP * LET_T + t, v, r);
                }
            }
        }
    }
    iou[p] = r == r ? r : 0.0f;
    aff[p] = af;
    lon[p] = lo;
}

struct LetP {
    const int* order;            // (N) detection index by sorted position (the merge order of accumulate())
    const int* cat_off;          // (K + 1) ranges of `order` per category
    const int* rank;             // (sumD) rank of a detection inside its (image, category) list
    const int* dt_match;         // (A, T, sumD) >= 0 matched (index of the gt inside its group)
    const unsigned char* dt_ig;  // (A, T, sumD)
    const long long* pair_row;   // (sumD) row of the pair (d, gt 0) in aff / lon
    const double* aff;           // (P)
    const double* lon;           // (P)
    const int* npig;             // (K, A)
    const int* has_e;            // (K)
    const double* rec_thrs;      // (R) ascending
    const int* max_dets;         // (M)
    int K, A, M, T, R, sumD;
    long long P;
    double* precision_l;         // (T, R, K, A, M)
    double* tp_aff;              // (T, K, A, M)
    double* tp_lon;              // (T, K, A, M)
};

__device__ __forceinline__ double let_scan(double v, int lane) {      // inclusive prefix sum over the lanes, lane order fixed
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_up(v, (unsigned)d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

__device__ __forceinline__ double let_max(double a, double b) { return (b > a || b != b) ? b : a; }      // a NaN stays

__global__ void __launch_bounds__(LET_T) let_accumulate_kernel(LetP p) {
    int id = blockIdx.x;
    const int t = id % p.T; id /= p.T;
    const int m = id % p.M; id /= p.M;
    const int a = id % p.A;
    const int k = id / p.A;
    const int lane = threadIdx.x;
    if (!p.has_e[k]) return;                                      // no evaluated image: the -1 of the caller stays
    const int npig = p.npig[k * p.A + a];
    if (npig == 0) return;
    const int s0 = p.cat_off[k], s1 = p.cat_off[k + 1], maxdet = p.max_dets[m];
    const int* dtm = p.dt_match + ((long)a * p.T + t) * p.sumD;
    const unsigned char* dtg = p.dt_ig + ((long)a * p.T + t) * p.sumD;
    const double eps = 2.220446049250313e-16;                     // np.spacing(1)
    const double nan = __builtin_nan("");
    const int nchunk = (s1 - s0 + 63) / 64;
    for (int jb = 0; jb < p.R; jb += 64) {                        // one walk of the list per batch of 64 recall thresholds
        const int j = jb + lane;
        // the number of true positives that reaches threshold j: 0 for r_j <= 0 (the first element of the list), the smallest c with
        // r_j <= c / npig otherwise (the expression of eval_accumulate_kernel), npig + 1 when no c does
        int need = 0x7fffffff;
        if (j < p.R) {
            const double thr = p.rec_thrs[j];
            if (thr <= 0.0) {
                need = 0;
            } else {
                int lo = 1, hi = npig + 1;
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (thr <= (double)mid / npig) hi = mid; else lo = mid + 1; }
                need = lo;
            }
        }
        double best = 0.0;                                        // as `precision`: 0 where the threshold is not reached
        int tp_before = 0, fp_before = 0;
        double carry_a = 0.0, carry_l = 0.0;
        for (int c = 0; c < nchunk; ++c) {
            const int s = s0 + c * 64 + lane;
            bool incl = false, is_tp = false, is_fp = false;
            double af = 0.0, lo = 0.0;
            if (s < s1) {
                const int d = p.order[s];
                if ((unsigned)d < (unsigned)p.sumD && p.rank[d] < maxdet) {
                    incl = true;
                    const bool ig = dtg[d] != 0, mt = dtm[d] >= 0;
                    is_tp = mt && !ig;
                    is_fp = !mt && !ig;
                    if (is_tp) {
                        const long long row = p.pair_row[d] + dtm[d];
                        const bool in = row >= 0 && row < p.P;      // a row outside the table: NaN, nothing is read
                        af = in ? p.aff[row] : nan;
                        lo = in ? p.lon[row] : nan;
                    }
                }
            }
            const unsigned long long tpm = __ballot(is_tp), fpm = __ballot(is_fp);
            const unsigned long long upto = lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1ull);
            const int tp_i = tp_before + __popcll(tpm & upto);    // cumulative counts up to and including this element
            const int fp_i = fp_before + __popcll(fpm & upto);
            const double ca = let_scan(af, lane), cl = let_scan(lo, lane);
            double env = incl ? (carry_a + ca) / ((double)fp_i + (double)tp_i + eps) : -1.0;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {                    // inclusive suffix maximum over the lanes >= this one
                const double o = __shfl_down(env, (unsigned)d, 64);
                if (lane + d < 64) env = let_max(env, o);
            }
            // the lane from which this chunk counts for the owned threshold: 0 once reached, the lane of the true positive that
            // reaches it, none before
            const int ntp = __popcll(tpm);
            int q = -1;
            if (need <= tp_before) {
                q = 0;
            } else if (need <= tp_before + ntp) {
                const int n = need - tp_before;                   // the n-th true positive of this chunk, 1 <= n <= ntp
                q = 0;
#pragma unroll
                for (int step = 32; step >= 1; step >>= 1)
                    if (q + step <= 63 && __popcll(tpm & ((1ull << (q + step)) - 1ull)) < n) q += step;
            }
            const double got = __shfl(env, q < 0 ? 0 : q, 64);
            if (q >= 0) best = let_max(best, got);
            tp_before += ntp;
            fp_before += __popcll(fpm);
            carry_a += __shfl(ca, 63, 64);
            carry_l += __shfl(cl, 63, 64);
        }
        if (j < p.R) p.precision_l[((((long)t * p.R + j) * p.K + k) * p.A + a) * p.M + m] = best;
        if (jb == 0 && lane == 0 && tp_before > 0) {
            const long o = (((long)t * p.K + k) * p.A + a) * p.M + m;
            p.tp_aff[o] = carry_a / tp_before;
            p.tp_lon[o] = carry_l / tp_before;
        }
    }
}

}  // namespace

extern "C" {

int omni_let_pairs(const double* centre1, const double* axes1, const double* dims1, const int* valid1, int n1, const double* centre2,
                   const double* axes2, const double* dims2, const int* valid2, int n2, const int* idx1, const int* idx2,
                   long long npairs, double tol_frac, double tol_min, float* iou, double* aff, double* lon, void* stream) {
    if (n1 < 0 || n2 < 0 || npairs < 0 || npairs > (long long)LET_T * 0x7fffffffLL) return OMNI_ERR_ARG;
    if (!(tol_frac >= 0.0 && tol_frac < 1e300) || !(tol_min > 0.0 && tol_min < 1e300)) return OMNI_ERR_ARG;      // also refuses a NaN
    if (npairs == 0) return OMNI_OK;
    if (!idx1 || !idx2 || !iou || !aff || !lon) return OMNI_ERR_ARG;
    if ((n1 > 0 && (!centre1 || !axes1 || !dims1 || !valid1)) || (n2 > 0 && (!centre2 || !axes2 || !dims2 || !valid2))) return OMNI_ERR_ARG;
    hipLaunchKernelGGL(let_pairs_kernel, dim3((unsigned)((npairs + LET_T - 1) / LET_T)), dim3(LET_T), 0, (hipStream_t)stream, centre1, axes1,
                       dims1, valid1, n1, centre2, axes2, dims2, valid2, n2, idx1, idx2, (long)npairs, tol_frac, tol_min, iou, aff, lon);
    return omni_launch_status();
}

int omni_eval_accumulate_let(const int* order, const int* cat_off, const int* rank, const int* dt_match, const unsigned char* dt_ignore,
                             const long long* pair_row, const double* aff, const double* lon, long long npairs, const int* npig,
                             const int* has_e, const double* rec_thrs, const int* max_dets, int K, int A, int M, int T, int R, int sumD,
                             double* precision_l, double* tp_affinity, double* tp_lon, void* stream) {
    if (K < 0 || A <= 0 || M <= 0 || T <= 0 || R <= 0 || sumD < 0 || npairs < 0) return OMNI_ERR_ARG;
    if ((long long)K * A * M * T > 0x7fffffffLL) return OMNI_ERR_ARG;
    if (K == 0) return OMNI_OK;
    if (!cat_off || !npig || !has_e || !rec_thrs || !max_dets || !precision_l || !tp_affinity || !tp_lon) return OMNI_ERR_ARG;
    if (sumD > 0 && (!order || !rank || !dt_match || !dt_ignore || !pair_row)) return OMNI_ERR_ARG;
    if (npairs > 0 && (!aff || !lon)) return OMNI_ERR_ARG;
    LetP p{order, cat_off, rank, dt_match, dt_ignore, pair_row, aff, lon, npig, has_e, rec_thrs, max_dets, K, A, M, T, R, sumD, npairs,
           precision_l, tp_affinity, tp_lon};
    hipLaunchKernelGGL(let_accumulate_kernel, dim3((unsigned)((long)K * A * M * T)), dim3(LET_T), 0, (hipStream_t)stream, p);
    return omni_launch_status();
}

}  // extern "C"
