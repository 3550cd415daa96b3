// eval_kitti.hip -- the KITTI object benchmark's protocol (AP|R40 / AP|R11 at Easy / Moderate / Hard) on the device.
//
// The protocol is the project's reading of the devkit's evaluate_object ("KITTI-protocol evaluation"; the float64
// statement of it is tests/exact_kitti.py).  It is not a variation of eval_match.hip: it walks GROUND TRUTHS, runs one greedy
// pass to harvest the scores of the true positives, derives up to 41 score thresholds from them and runs another greedy pass
// per threshold.  A "slot" is one (class c, difficulty d, metric m, overlap set o), s = ((c * Dn + d) * M + m) * O + o.
//   omni_kitti_match_tp      one 64-lane wave per (image, slot): pass 1
//   omni_kitti_thresholds    one workgroup per slot: the scores at the ranks the recall sampling emits (radix selection)
//   omni_kitti_match_counts  one 64-lane wave per (image, slot, threshold k < K[slot]): pass 2 with the DontCare step
//   omni_kitti_finalize      precision / recall / AP per slot
// AOS (average orientation similarity, the devkit's compute_aos path as this project reads it, written from memory like the rest;
// float64 statement: tests/exact_kitti_aos.py) is one more template parameter on pass 2 and on the finalize:
//   omni_kitti_match_counts_aos  pass 2, and per true positive q = (1 + cos(gt_alpha - dt_alpha)) / 2 summed in fixed point
//   omni_kitti_finalize_aos      aos = sim_sum 2^-40 / (tp + fp), made monotone and averaged like precision
// The <false> instantiations are the kernels behind the plain entry points, unchanged.
// As in eval_match.hip the sequential side (here the ground truths) is walked by the wave, the parallel side (the detections,
// at most 1024 = 16 per lane) is spread over the lanes and reduced with shuffles; the overlaps are compared with the
// min-overlap as doubles.  "Assigned" is one bit per detection in a register of the lane that owns it: no LDS in the matching.
// Sums are integer atomics: two runs give the same bits.
#include <device_rt.h>

namespace {

constexpr int KITTI_MAXN = 1024;          // detections / ground-truth rows of one image
constexpr int KITTI_NPTS_MAX = 64;        // recall sample points (the benchmark: 41)
constexpr int KITTI_NONE = 0x7fffffff;

struct KittiP {
    const float* sim;          // (M, P): metric m's ragged matrices; image i holds (G_i, D_i) row-major (detections fastest) at sim_off[i]
    long long P;
    const long long* sim_off;  // (I)
    const int* dt_off;         // (I + 1)
    const int* gt_off;         // (I + 1)
    const int* dt_code;        // (sumD) class code
    const double* dt_height;   // (sumD)
    const double* dt_score;    // (sumD)
    const int* gt_code;        // (sumG)
    const double* gt_height;   // (sumG)
    const int* gt_occ;         // (sumG)
    const double* gt_trunc;    // (sumG)
    const int* cls_tab;        // (C, ncodes): 0 the class itself, 1 a neighbour class, 2 the class but set aside, anything else: other
    const double* diffs;       // (Dn, 3): min height, max occlusion, max truncation
    const double* min_ov;      // (O, C)
    int I, C, Dn, M, O, ncodes, sumD, sumG, npts;
    // pass 1
    double* tp_score;          // (S, sumG): the score of the true positive found for the row, -inf otherwise
    int* n_gt;                 // (S)
    // pass 2
    const float* dc_ov;        // ragged: image i holds (R_i, D_i) row-major at dc_pair_off[i]
    const long long* dc_pair_off;   // (I)
    const int* dc_off;         // (I + 1)
    const int* dc_metric;      // (M)
    const double* thresholds;  // (S, npts)
    const int* K;              // (S)
    int* counts;               // (S, npts, 3) tp, fp, fn
};

// pass 2 with AOS: the headings (NaN: none) and the table of fixed-point sums
struct KittiAosP : KittiP {
    const double* dt_alpha;    // (sumD) observation angle, NaN: no heading
    const double* gt_alpha;    // (sumG)
    const int* aos_metric;     // (M): the metrics whose slots accumulate
    unsigned long long* sim_sum;   // (S, npts): sum of llrint(q 2^40) over the true positives
};
template <bool AOS> struct KittiArg { typedef KittiP type; };
template <> struct KittiArg<true> { typedef KittiAosP type; };
constexpr double KITTI_AOS_ONE = 1099511627776.0;      // 2^40

struct Slot { int c, d, m, o; double mo, hmin, omax, tmax; };

__device__ __forceinline__ Slot kitti_slot(const KittiP& p, int s) {
    Slot q;
    q.o = s % p.O; s /= p.O;
    q.m = s % p.M; s /= p.M;
    q.d = s % p.Dn;
    q.c = s / p.Dn;
    q.mo = p.min_ov[q.o * p.C + q.c];
    q.hmin = p.diffs[3 * q.d]; q.omax = p.diffs[3 * q.d + 1]; q.tmax = p.diffs[3 * q.d + 2];
    return q;
}

__device__ __forceinline__ int kitti_rel(const KittiP& p, int c, int code) {
    return (code >= 0 && code < p.ncodes) ? p.cls_tab[c * p.ncodes + code] : -1;
}

// 0 counted, 1 neutral (a neighbour class, or the class itself outside the difficulty), -1 not a candidate (another class, or a row
// of the class that is set aside -- rel 2 -- although the difficulty would count it)
__device__ __forceinline__ int kitti_gt_flag(const KittiP& p, const Slot& q, int row) {
    const int rel = kitti_rel(p, q.c, p.gt_code[row]);
    if (rel == 1) return 1;
    if (rel != 0 && rel != 2) return -1;
    const bool hard = (double)p.gt_occ[row] > q.omax || p.gt_trunc[row] > q.tmax || p.gt_height[row] < q.hmin;
    return hard ? 1 : (rel == 0 ? 0 : -1);
}

// the masks of this lane's detections d = lane + 64 j: `cls` of the slot's class (with score >= thr), `small` below the height
__device__ __forceinline__ void kitti_dt_masks(const KittiP& p, const Slot& q, int d0, int D, int lane, double thr, unsigned& cls, unsigned& small) {
    cls = 0u; small = 0u;
#pragma unroll 1
    for (int j = 0, d = lane; d < D; ++j, d += 64) {
        if (kitti_rel(p, q.c, p.dt_code[d0 + d]) == 0 && p.dt_score[d0 + d] >= thr) {
            cls |= 1u << j;
            if (p.dt_height[d0 + d] < q.hmin) small |= 1u << j;
        }
    }
}

__global__ void __launch_bounds__(64) kitti_match_tp_kernel(KittiP p) {
    const int lane = threadIdx.x;
    const int S = p.C * p.Dn * p.M * p.O;
    const int s = blockIdx.x % S, img = blockIdx.x / S;
    const Slot q = kitti_slot(p, s);
    const int d0 = p.dt_off[img], D = p.dt_off[img + 1] - d0;
    const int g0 = p.gt_off[img], G = p.gt_off[img + 1] - g0;
    const float* sim = p.sim + (long long)q.m * p.P + p.sim_off[img];
    double* out = p.tp_score + (long long)s * p.sumG + g0;
    unsigned cls, small, assigned = 0u;
    kitti_dt_masks(p, q, d0, D, lane, -INFINITY, cls, small);
    int ngt = 0;
    for (int g = 0; g < G; ++g) {
        const int gf = kitti_gt_flag(p, q, g0 + g);
        if (gf < 0) {
            if (lane == 0) out[g] = -INFINITY;
            continue;
        }
        ngt += gf == 0;
        // the usable detection above the overlap with the largest score, the earliest among equal scores
        double bs = 0.0;
        int bi = KITTI_NONE;
        const unsigned live = cls & ~assigned;
#pragma unroll 1
        for (int j = 0, d = lane; d < D; ++j, d += 64) {
            if (!((live >> j) & 1u)) continue;
            if (!((double)sim[(long long)g * D + d] > q.mo)) continue;
            const double sc = p.dt_score[d0 + d];
            if (bi == KITTI_NONE || sc > bs) { bs = sc; bi = d; }
        }
        if (!__any(bi != KITTI_NONE)) {
            if (lane == 0) out[g] = -INFINITY;
            continue;
        }
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1) {
            const double os = __shfl_xor(bs, sh, 64);
            const int oi = __shfl_xor(bi, sh, 64);
            if (oi != KITTI_NONE && (bi == KITTI_NONE || os > bs || (os == bs && oi < bi))) { bs = os; bi = oi; }
        }
        double rec = -INFINITY;
        if (bi != KITTI_NONE) {
            const int owner = bi & 63, j = bi >> 6;
            const int is_small = (__shfl(small, owner, 64) >> j) & 1u;
            if (lane == owner) assigned |= 1u << j;
            if (gf == 0 && !is_small) rec = bs;
        }
        if (lane == 0) out[g] = rec;
    }
    if (lane == 0 && ngt > 0) atomicAdd(p.n_gt + s, ngt);
}

template <bool AOS>
__global__ void __launch_bounds__(64) kitti_match_counts_kernel(typename KittiArg<AOS>::type p) {
    const int lane = threadIdx.x;
    const int S = p.C * p.Dn * p.M * p.O;
    int b = blockIdx.x;
    const int k = b % p.npts; b /= p.npts;
    const int s = b % S, img = b / S;
    if (k >= p.K[s]) return;
    const Slot q = kitti_slot(p, s);
    const double thr = p.thresholds[s * p.npts + k];
    const int d0 = p.dt_off[img], D = p.dt_off[img + 1] - d0;
    const int g0 = p.gt_off[img], G = p.gt_off[img + 1] - g0;
    const float* sim = p.sim + (long long)q.m * p.P + p.sim_off[img];
    unsigned cls, small, assigned = 0u;
    kitti_dt_masks(p, q, d0, D, lane, thr, cls, small);
    int tp = 0, fn = 0;
    unsigned long long sim_q = 0ull;                    // AOS: lane 0's fixed-point sum of q over this wave's true positives
    bool aos_on = false;
    if constexpr (AOS) aos_on = p.aos_metric[q.m] != 0;
    for (int g = 0; g < G; ++g) {
        const int gf = kitti_gt_flag(p, q, g0 + g);
        if (gf < 0) continue;
        // One key per lane, reduced by its maximum: a detection of full height carries the bits of its overlap (positive floats order
        // like their bits) above the inverted index, so the largest overlap and among equals the earliest wins; a detection below the
        // height carries the inverted index alone, so it loses to every one of full height and the earliest of its kind wins.
        unsigned long long key = 0ull;
        const unsigned live = cls & ~assigned;
#pragma unroll 1
        for (int j = 0, d = lane; d < D; ++j, d += 64) {
            if (!((live >> j) & 1u)) continue;
            const float v = sim[(long long)g * D + d];
            if (!((double)v > q.mo)) continue;
            const unsigned long long hi = ((small >> j) & 1u) ? 0ull : (unsigned long long)__float_as_uint(v);
            const unsigned long long kk = (hi << 32) | (unsigned long long)(0xffffffffu - (unsigned)d);
            if (kk > key) key = kk;
        }
        if (!__any(key != 0ull)) {
            fn += gf == 0;
            continue;
        }
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1) {
            const unsigned long long ok = __shfl_xor(key, sh, 64);
            if (ok > key) key = ok;
        }
        const int bi = (int)(0xffffffffu - (unsigned)(key & 0xffffffffull));
        if (lane == (bi & 63)) assigned |= 1u << (bi >> 6);
        tp += (gf == 0 && (key >> 32) != 0ull);
        if constexpr (AOS) {
            if (aos_on && lane == 0 && gf == 0 && (key >> 32) != 0ull) {
                const double ga = p.gt_alpha[g0 + g], da = p.dt_alpha[d0 + bi];
                // no heading on either side contributes 0
                const double qq = (isfinite(ga) && isfinite(da)) ? 0.5 * (1.0 + cos(ga - da)) : 0.0;
                sim_q += (unsigned long long)llrint(qq * KITTI_AOS_ONE);
            }
        }
    }
    // false positives: the usable detections of full height nobody took, less those a DontCare region covers
    unsigned open = cls & ~small & ~assigned;
    int fp = __popc(open);
    if (p.dc_metric[q.m]) {
        const int r0 = p.dc_off[img], R = p.dc_off[img + 1] - r0;
        const float* ov = p.dc_ov + p.dc_pair_off[img];
#pragma unroll 1
        for (int j = 0, d = lane; d < D; ++j, d += 64) {
            if (!((open >> j) & 1u)) continue;
            for (int r = 0; r < R; ++r)
                if ((double)ov[(long long)r * D + d] > q.mo) { --fp; break; }
        }
    }
    fp = __any(fp != 0) ? wave_sum_i(fp) : 0;
    if (lane == 0) {
        int* c = p.counts + ((long long)s * p.npts + k) * 3;
        if (tp) atomicAdd(c, tp);
        if (fp) atomicAdd(c + 1, fp);
        if (fn) atomicAdd(c + 2, fn);
        if constexpr (AOS) {
            if (sim_q) atomicAdd(p.sim_sum + ((long long)s * p.npts + k), sim_q);
        }
    }
}

// ---- thresholds ---------------------------------------------------------------------------------------------------------------
// an order-preserving map of the doubles to unsigned integers (-inf, the "no true positive" mark, is the smallest of all)
__device__ __forceinline__ unsigned long long kitti_key(double v) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

constexpr int KITTI_THR_BLOCK = 256;

__global__ void __launch_bounds__(KITTI_THR_BLOCK) kitti_thresholds_kernel(const double* __restrict__ tp_score, const int* __restrict__ n_gt, int sumG,
                                                                           int npts, double* __restrict__ thresholds, int* __restrict__ K) {
    __shared__ int s_hist[256];
    __shared__ int s_rank[KITTI_NPTS_MAX];
    __shared__ int s_n, s_K, s_rem;
    __shared__ unsigned long long s_prefix;
    const int t = threadIdx.x, s = blockIdx.x;
    const double* v = tp_score + (long long)s * sumG;
    if (t == 0) s_n = 0;
    __syncthreads();
    int mine = 0;
    for (int i = t; i < sumG; i += KITTI_THR_BLOCK) mine += v[i] > -INFINITY;
    if (mine) atomicAdd(&s_n, mine);
    __syncthreads();
    if (t == 0) {
        // the ranks (descending score order) the recall sampling keeps: they depend on the two counts only
        const int n = s_n;
        const double ngt = (double)n_gt[s], step = 1.0 / (double)(npts - 1);
        double cur = 0.0;
        int k = 0;
        for (int i = 0; i < n && k < npts; ++i) {
            const double l = (double)(i + 1) / ngt;
            const double r = i < n - 1 ? (double)(i + 2) / ngt : l;
            if (i < n - 1 && (r - cur) < (cur - l)) continue;
            s_rank[k++] = i;
            cur += step;
        }
        s_K = k;
        K[s] = k;
    }
    __syncthreads();
    const int nk = s_K;
    for (int k = nk + t; k < npts; k += KITTI_THR_BLOCK) thresholds[s * npts + k] = 0.0;
    for (int k = 0; k < nk; ++k) {
        // radix selection of the element of descending rank s_rank[k], one byte per pass from the top
        if (t == 0) { s_rem = s_rank[k]; s_prefix = 0ull; }
        for (int byte = 7; byte >= 0; --byte) {
            s_hist[t] = 0;
            __syncthreads();
            const unsigned long long prefix = s_prefix;
            const int shift = 8 * byte;
            for (int i = t; i < sumG; i += KITTI_THR_BLOCK) {
                const unsigned long long u = kitti_key(v[i]);
                if (byte == 7 || (u >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&s_hist[(int)((u >> shift) & 0xffull)], 1);
            }
            __syncthreads();
            if (t == 0) {
                int rem = s_rem, dg = 255;
                while (dg > 0 && rem >= s_hist[dg]) { rem -= s_hist[dg]; --dg; }
                s_rem = rem;
                s_prefix = prefix | ((unsigned long long)dg << shift);
            }
            __syncthreads();
        }
        if (t == 0) {
            const unsigned long long u = s_prefix;
            const unsigned long long bits = (u >> 63) ? (u & 0x7fffffffffffffffull) : ~u;
            thresholds[s * npts + k] = __builtin_bit_cast(double, bits);
        }
        __syncthreads();
    }
}

// AOS: `precision` is the table of orientation similarities, `recall` is not written, and the last four arguments are in use
template <bool AOS>
__global__ void __launch_bounds__(64) kitti_finalize_kernel(const int* __restrict__ counts, const int* __restrict__ K, int S, int npts,
                                                            double* __restrict__ precision, double* __restrict__ recall, double* __restrict__ ap,
                                                            const unsigned long long* __restrict__ sim_sum, const int* __restrict__ aos_metric,
                                                            int M, int O) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= S) return;
    const int nk = K[s];
    double* pr = precision + (long long)s * npts;
    double* rc = recall + (long long)s * npts;
    if constexpr (AOS) {
        if (!aos_metric[(s / O) % M]) {                 // a slot of a metric without AOS
            const double nan = __builtin_nan("");
            for (int k = 0; k < npts; ++k) pr[k] = nan;
            ap[2 * s] = ap[2 * s + 1] = nan;
            return;
        }
    }
    for (int k = 0; k < npts; ++k) {
        double a = 0.0, b = 0.0;
        if (k < nk) {
            const int* c = counts + ((long long)s * npts + k) * 3;
            const double tp = (double)c[0], fp = (double)c[1], fn = (double)c[2];
            if constexpr (AOS) a = tp + fp > 0.0 ? (double)sim_sum[(long long)s * npts + k] * (1.0 / KITTI_AOS_ONE) / (tp + fp) : 0.0;
            else a = tp + fp > 0.0 ? tp / (tp + fp) : 0.0;
            b = tp + fn > 0.0 ? tp / (tp + fn) : 0.0;
        }
        pr[k] = a;
        if constexpr (!AOS) rc[k] = b;
    }
    double run = 0.0;
    for (int k = nk - 1; k >= 0; --k) {             // right-to-left running maximum over the thresholds in use
        run = pr[k] > run ? pr[k] : run;
        pr[k] = run;
    }
    double s40 = 0.0, s11 = 0.0;
    for (int k = 1; k < npts; ++k) s40 += pr[k];
    for (int k = 0; k < npts; k += 4) s11 += pr[k];
    ap[2 * s] = 100.0 * (s40 / (double)(npts - 1));
    ap[2 * s + 1] = 100.0 * (s11 / (double)((npts + 3) / 4));
}

int kitti_check(int I, int C, int Dn, int M, int O, int ncodes, int sumD, int sumG, int max_dt, int max_gt, int npts, long long per_image) {
    if (I < 0 || C < 0 || Dn < 0 || M < 0 || O < 0 || ncodes < 0 || sumD < 0 || sumG < 0 || max_dt < 0 || max_gt < 0) return OMNI_ERR_ARG;
    if (max_dt > KITTI_MAXN || max_gt > KITTI_MAXN) return OMNI_ERR_ARG;
    if (npts < 2 || npts > KITTI_NPTS_MAX) return OMNI_ERR_ARG;
    const long long S = (long long)C * Dn * M * O;
    // one 64-lane workgroup per problem: the grid may hold fewer than 2^32 threads
    if (S >= (1ll << 26) / npts || (long long)I * S * per_image >= (1ll << 26)) return OMNI_ERR_ARG;
    return OMNI_OK;
}

}  // namespace

extern "C" {

int omni_kitti_match_tp(const float* sim, long long P, const long long* sim_off, const int* dt_off, const int* gt_off, const int* dt_code,
                        const double* dt_height, const double* dt_score, const int* gt_code, const double* gt_height, const int* gt_occ,
                        const double* gt_trunc, const int* cls_tab, int ncodes, const double* diffs, const double* min_ov, int I, int C,
                        int Dn, int M, int O, int sumD, int sumG, int max_dt, int max_gt, double* tp_score, int* n_gt, void* stream) {
    const int rc = kitti_check(I, C, Dn, M, O, ncodes, sumD, sumG, max_dt, max_gt, 41, 1);
    if (rc != OMNI_OK || P < 0) return OMNI_ERR_ARG;
    const int S = C * Dn * M * O;
    if (I == 0 || S == 0) return OMNI_OK;
    KittiP p{};
    p.sim = sim; p.P = P; p.sim_off = sim_off; p.dt_off = dt_off; p.gt_off = gt_off; p.dt_code = dt_code; p.dt_height = dt_height;
    p.dt_score = dt_score; p.gt_code = gt_code; p.gt_height = gt_height; p.gt_occ = gt_occ; p.gt_trunc = gt_trunc; p.cls_tab = cls_tab;
    p.diffs = diffs; p.min_ov = min_ov; p.I = I; p.C = C; p.Dn = Dn; p.M = M; p.O = O; p.ncodes = ncodes; p.sumD = sumD; p.sumG = sumG;
    p.npts = 41; p.tp_score = tp_score; p.n_gt = n_gt;
    hipLaunchKernelGGL(kitti_match_tp_kernel, dim3((unsigned)((long long)I * S)), dim3(64), 0, (hipStream_t)stream, p);
    return omni_launch_status();
}

int omni_kitti_thresholds(const double* tp_score, const int* n_gt, int S, int sumG, int npts, double* thresholds, int* K, void* stream) {
    if (S < 0 || sumG < 0 || npts < 2 || npts > KITTI_NPTS_MAX) return OMNI_ERR_ARG;
    if (S == 0) return OMNI_OK;
    hipLaunchKernelGGL(kitti_thresholds_kernel, dim3((unsigned)S), dim3(KITTI_THR_BLOCK), 0, (hipStream_t)stream, tp_score, n_gt, sumG, npts,
                       thresholds, K);
    return omni_launch_status();
}

int omni_kitti_match_counts(const float* sim, long long P, const long long* sim_off, const int* dt_off, const int* gt_off, const int* dt_code,
                            const double* dt_height, const double* dt_score, const int* gt_code, const double* gt_height, const int* gt_occ,
                            const double* gt_trunc, const int* cls_tab, int ncodes, const double* diffs, const double* min_ov,
                            const float* dc_ov, const long long* dc_pair_off, const int* dc_off, const int* dc_metric,
                            const double* thresholds, const int* K, int npts, int I, int C, int Dn, int M, int O, int sumD, int sumG,
                            int max_dt, int max_gt, int* counts, void* stream) {
    const int rc = kitti_check(I, C, Dn, M, O, ncodes, sumD, sumG, max_dt, max_gt, npts, npts);
    if (rc != OMNI_OK || P < 0) return OMNI_ERR_ARG;
    const int S = C * Dn * M * O;
    if (I == 0 || S == 0) return OMNI_OK;
    KittiP p{};
    p.sim = sim; p.P = P; p.sim_off = sim_off; p.dt_off = dt_off; p.gt_off = gt_off; p.dt_code = dt_code; p.dt_height = dt_height;
    p.dt_score = dt_score; p.gt_code = gt_code; p.gt_height = gt_height; p.gt_occ = gt_occ; p.gt_trunc = gt_trunc; p.cls_tab = cls_tab;
    p.diffs = diffs; p.min_ov = min_ov; p.I = I; p.C = C; p.Dn = Dn; p.M = M; p.O = O; p.ncodes = ncodes; p.sumD = sumD; p.sumG = sumG;
    p.npts = npts; p.dc_ov = dc_ov; p.dc_pair_off = dc_pair_off; p.dc_off = dc_off; p.dc_metric = dc_metric; p.thresholds = thresholds;
    p.K = K; p.counts = counts;
    hipLaunchKernelGGL(kitti_match_counts_kernel<false>, dim3((unsigned)((long long)I * S * npts)), dim3(64), 0, (hipStream_t)stream, p);
    return omni_launch_status();
}

int omni_kitti_match_counts_aos(const float* sim, long long P, const long long* sim_off, const int* dt_off, const int* gt_off, const int* dt_code,
                                const double* dt_height, const double* dt_score, const int* gt_code, const double* gt_height, const int* gt_occ,
                                const double* gt_trunc, const int* cls_tab, int ncodes, const double* diffs, const double* min_ov,
                                const float* dc_ov, const long long* dc_pair_off, const int* dc_off, const int* dc_metric,
                                const double* thresholds, const int* K, int npts, int I, int C, int Dn, int M, int O, int sumD, int sumG,
                                int max_dt, int max_gt, const double* dt_alpha, const double* gt_alpha, const int* aos_metric, int* counts,
                                long long* sim_sum, void* stream) {
    const int rc = kitti_check(I, C, Dn, M, O, ncodes, sumD, sumG, max_dt, max_gt, npts, npts);
    // sumG < 2^23 true positives of at most 2^40 each: the 64-bit sum cannot overflow
    if (rc != OMNI_OK || P < 0 || sumG >= (1 << 23)) return OMNI_ERR_ARG;
    const int S = C * Dn * M * O;
    if (I == 0 || S == 0) return OMNI_OK;
    KittiAosP p{};
    p.sim = sim; p.P = P; p.sim_off = sim_off; p.dt_off = dt_off; p.gt_off = gt_off; p.dt_code = dt_code; p.dt_height = dt_height;
    p.dt_score = dt_score; p.gt_code = gt_code; p.gt_height = gt_height; p.gt_occ = gt_occ; p.gt_trunc = gt_trunc; p.cls_tab = cls_tab;
    p.diffs = diffs; p.min_ov = min_ov; p.I = I; p.C = C; p.Dn = Dn; p.M = M; p.O = O; p.ncodes = ncodes; p.sumD = sumD; p.sumG = sumG;
    p.npts = npts; p.dc_ov = dc_ov; p.dc_pair_off = dc_pair_off; p.dc_off = dc_off; p.dc_metric = dc_metric; p.thresholds = thresholds;
    p.K = K; p.counts = counts;
    p.dt_alpha = dt_alpha; p.gt_alpha = gt_alpha; p.aos_metric = aos_metric; p.sim_sum = (unsigned long long*)sim_sum;
    hipLaunchKernelGGL(kitti_match_counts_kernel<true>, dim3((unsigned)((long long)I * S * npts)), dim3(64), 0, (hipStream_t)stream, p);
    return omni_launch_status();
}

int omni_kitti_finalize(const int* counts, const int* K, int S, int npts, double* precision, double* recall, double* ap, void* stream) {
    if (S < 0 || npts < 2 || npts > KITTI_NPTS_MAX) return OMNI_ERR_ARG;
    if (S == 0) return OMNI_OK;
    hipLaunchKernelGGL(kitti_finalize_kernel<false>, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, (hipStream_t)stream, counts, K, S, npts, precision,
                       recall, ap, (const unsigned long long*)nullptr, (const int*)nullptr, 1, 1);
    return omni_launch_status();
}

int omni_kitti_finalize_aos(const int* counts, const long long* sim_sum, const int* K, const int* aos_metric, int S, int M, int O, int npts,
                            double* aos, double* aos_ap, void* stream) {
    if (S < 0 || M < 0 || O < 0 || npts < 2 || npts > KITTI_NPTS_MAX) return OMNI_ERR_ARG;
    if (S == 0) return OMNI_OK;
    if (M < 1 || O < 1) return OMNI_ERR_ARG;
    hipLaunchKernelGGL(kitti_finalize_kernel<true>, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, (hipStream_t)stream, counts, K, S, npts, aos,
                       (double*)nullptr, aos_ap, (const unsigned long long*)sim_sum, aos_metric, M, O);
    return omni_launch_status();
}

}  // extern "C"
