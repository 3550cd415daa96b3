// eval_bootstrap.hip -- the image-level bootstrap of Omni3Deval.accumulate: AP and recall of B resampled data sets from the ONE set of
// match tables `omni_eval_match` made, in one launch.  The reference has no counterpart; `Omni3Deval.bootstrap`
// (cubercnn/evaluation/omni3d_evaluation.py) is built on these two.
//
// A replicate b is a vector of I non-negative image multiplicities weights[b][.]; its result is by definition what
// eval_accumulate_kernel (csrc/eval_match.hip) gives on the data set that holds image i weights[b][i] times: in the merge order of
// accumulate() a detection d counts as weights[b][det_img[d]] consecutive identical entries (none when that is 0).  Precision only rises
// along the copies of a true positive and only falls along the copies of a false positive, so the right-to-left envelope is attained at
// the LAST copy of a true positive and weighted inclusive prefix sums are all it takes: at list position s with TP = sum of the weights of
// the true positives up to and including s, FP likewise, prec = TP / (FP + TP + eps) (the expression and eps of eval_accumulate_kernel); a
// true positive of weight w serves the recall thresholds in ((TP - w) / npig_b, TP / npig_b], found by the same `<=` searches, and the
// thresholds <= 0 take the envelope of the whole list.
//
//   bootstrap_counts_kernel  one 64-lane wave per (replicate b, category k): npig_b[b][k][a] = sum over the (image, category) groups of k
//                            of weights[b][image] x the group's non-ignored ground truths in range a, has_e_b[b][k] = some group of k
//                            has a positive weight.  Integer sums: exact.
//   eval_bootstrap_kernel    one workgroup of four waves per (k, a, m, t) x slab of BS_NB replicates.  The (k, a, m, t) list is the same for
//                            every replicate, so the workgroup stages it ONCE per slab in LDS, BS_CHUNK elements at a time: one int per
//                            element = (det_img << 2) | class, class 0 true positive, 1 false positive, 2 ignored; -1 for a detection
//                            past maxDets (rank >= max_dets[m]).  Each wave then walks the staged elements for one replicate after
//                            another, gathering weights[b][det_img]: pass 1 forward for the totals, pass 2 BACKWARD like
//                            eval_accumulate_kernel, 64 elements at a time: TP and FP travel as the two halves of one 64-bit inclusive
//                            scan over the lanes (the entry refuses counts that would not fit 31 bits), the envelope is a suffix
//                            maximum over the lanes plus the carry of what lies behind.  The state a replicate carries from one
//                            staged chunk to the next (totals, counts behind, envelope, sum, thresholds already served) is six words
//                            in LDS.  The number of thresholds <= x is a ballot over the lanes' own thresholds; the per-lane searches run
//                            only in the at most R steps in which some threshold is served.
//                            ap = (the sum of the R precisions, in double, in the fixed order of the backward walk) / R: it is NOT the
//                            sum in ascending r, from which it differs by rounding only (< R x 2^-53).  Every order depends on list
//                            positions and lane numbers alone: two launches, and a replicate in slabs of any size, give the same bits.
//                            No atomics.
#include <device_rt.h>

#pragma clang fp contract(off)

namespace {

constexpr int BS_WAVES = 4;                 // waves per workgroup
constexpr int BS_T = 64 * BS_WAVES;
constexpr int BS_CHUNK = 4096;              // staged elements: 16 KB of LDS
constexpr int BS_NB = 64;                   // replicates per workgroup
constexpr int BS_MAX_I = 1 << 29;           // det_img shares an int with the class

struct BootP {
    const int* order;            // (N) detection index by sorted position (the merge order of accumulate())
    const int* cat_off;          // (K + 1) ranges of `order` per category
    const int* rank;             // (sumD) rank of a detection inside its (image, category) list
    const int* dt_match;         // (A, T, sumD) >= 0 matched
    const unsigned char* dt_ig;  // (A, T, sumD)
    const int* det_img;          // (sumD) index of the detection's image in [0, I)
    const int* weights;          // (B, I) image multiplicities in [0, max_weight]
    const int* npig_b;           // (B, K, A)
    const int* has_e_b;          // (B, K)
    const double* rec_thrs;      // (R) ascending
    const int* max_dets;         // (M)
    int K, A, M, T, R, sumD, B, I, max_weight;
    double* ap;                  // (B, T, K, A, M)
    double* ar;                  // (B, T, K, A, M)
};

typedef unsigned long long u64;

__device__ __forceinline__ u64 boot_sum(u64 v) {                  // the same total in every lane
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// the number of thresholds <= x: th0 / th1 are the lane's own thresholds `lane` and `lane + 64` (+inf past R), the rest is read
__device__ __forceinline__ int boot_count_le(double x, double th0, double th1, const double* thr, int R, int lane) {
    int n = __popcll(__ballot(th0 <= x)) + __popcll(__ballot(th1 <= x));
    for (int jb = 128; jb < R; jb += 64) n += __popcll(__ballot(jb + lane < R && thr[jb + lane] <= x));
    return n;
}

__global__ void __launch_bounds__(BS_T) eval_bootstrap_kernel(BootP p) {
    __shared__ int s_code[BS_CHUNK];
    __shared__ u64 s_tot[BS_NB];               // (TP << 32) | FP over the whole list
    __shared__ u64 s_after[BS_NB];             // the same over what the backward walk has passed
    __shared__ double s_max[BS_NB], s_sum[BS_NB];
    __shared__ int s_npig[BS_NB], s_nd[BS_NB], s_jend[BS_NB];
    int id = blockIdx.x;
    const int t = id % p.T; id /= p.T;
    const int m = id % p.M; id /= p.M;
    const int a = id % p.A;
    const int k = id / p.A;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = (int)blockIdx.y * BS_NB, nb = min(BS_NB, p.B - b0);
    const int s0 = p.cat_off[k], s1 = p.cat_off[k + 1], maxdet = p.max_dets[m];
    const int* dtm = p.dt_match + ((long)a * p.T + t) * p.sumD;
    const unsigned char* dtg = p.dt_ig + ((long)a * p.T + t) * p.sumD;
    const int nchunk = (s1 - s0 + BS_CHUNK - 1) / BS_CHUNK;
    const double eps = 2.220446049250313e-16;                     // np.spacing(1)
    const double inf = __builtin_inf();
    const double th0 = lane < p.R ? p.rec_thrs[lane] : inf, th1 = lane + 64 < p.R ? p.rec_thrs[lane + 64] : inf;
    auto out = [&](int r) { return (((((long)(b0 + r)) * p.T + t) * p.K + k) * p.A + a) * p.M + m; };
    // no evaluated image or no ground truth in this replicate: npig 0, the -1 of the caller stays
    if (tid < nb) {
        const long bk = (long)(b0 + tid) * p.K + k;
        s_npig[tid] = p.has_e_b[bk] ? max(p.npig_b[bk * p.A + a], 0) : 0;
        s_tot[tid] = 0ull;
        s_nd[tid] = 0;
    }
    auto stage = [&](int c) -> int {                               // -> the number of elements staged
        const int base = s0 + c * BS_CHUNK, n = min(BS_CHUNK, s1 - base);
        for (int e = tid; e < n; e += BS_T) {
            const int d = p.order[base + e];
            int code = -1;
            if ((unsigned)d < (unsigned)p.sumD && p.rank[d] < maxdet) {
                const int img = p.det_img[d];
                if ((unsigned)img < (unsigned)p.I) code = (img << 2) | (dtg[d] != 0 ? 2 : dtm[d] >= 0 ? 0 : 1);
            }
            s_code[e] = code;
        }
        return n;
    };
    auto weight = [&](const int* wrow, int code) -> int {          // a weight outside [0, max_weight] counts as 0
        if (code < 0) return 0;
        const int w = wrow[code >> 2];
        return (unsigned)w <= (unsigned)p.max_weight ? w : 0;
    };
    __syncthreads();
    // ---- pass 1: the totals over the included detections
    int n = 0;
    for (int c = 0; c < nchunk; ++c) {
        if (c > 0) __syncthreads();
        n = stage(c);
        __syncthreads();
        for (int r = wave; r < nb; r += BS_WAVES) {
            if (s_npig[r] == 0) continue;
            const int* wrow = p.weights + (long)(b0 + r) * p.I;
            u64 acc = 0ull;
            int any = 0;
            for (int e = lane; e < n; e += 64) {
                const int code = s_code[e], w = weight(wrow, code), cls = code & 3;
                acc += cls == 0 ? ((u64)(unsigned)w << 32) : cls == 1 ? (u64)(unsigned)w : 0ull;
                any |= w > 0;
            }
            acc = boot_sum(acc);
            any = __ballot(any) != 0ull;
            if (lane == 0) { s_tot[r] += acc; s_nd[r] |= any; }
        }
    }
    __syncthreads();
    for (int r = wave; r < nb; r += BS_WAVES) {                    // a replicate stays with its wave from here to the end
        const int npig = s_npig[r];
        if (npig == 0) continue;
        const int tp_tot = (int)(s_tot[r] >> 32);
        const int jend = boot_count_le((double)tp_tot / npig, th0, th1, p.rec_thrs, p.R, lane);
        if (lane == 0) {
            p.ar[out(r)] = s_nd[r] ? (double)tp_tot / npig : 0.0;
            s_after[r] = 0ull;
            s_max[r] = -1.0;
            s_sum[r] = 0.0;
            s_jend[r] = jend;
        }
    }
    __syncthreads();
    // ---- pass 2: backward sweep; the last chunk is still staged
    for (int c = nchunk - 1; c >= 0; --c) {
        if (c != nchunk - 1) {
            __syncthreads();
            n = stage(c);
            __syncthreads();
        }
        const int nsub = (n + 63) / 64;
        for (int r = wave; r < nb; r += BS_WAVES) {
            const int npig = s_npig[r];
            if (npig == 0 || !s_nd[r]) continue;
            const int* wrow = p.weights + (long)(b0 + r) * p.I;
            const u64 tot = s_tot[r];
            u64 after = s_after[r];
            double carry_max = s_max[r], sum = s_sum[r];
            int jend = s_jend[r];
            int e = (nsub - 1) * 64 + lane;
            int code = e < n ? s_code[e] : -1, w = weight(wrow, code);
            for (int q = nsub - 1; q >= 0; --q) {
                const int code_c = code, w_c = w;
                if (q > 0) {                                      // the gather of the next step travels while this one is scanned
                    e -= 64;
                    code = s_code[e];
                    w = weight(wrow, code);
                }
                const int cls = code_c & 3;
                const bool is_tp = w_c > 0 && cls == 0;
                u64 pre = cls == 0 ? ((u64)(unsigned)w_c << 32) : cls == 1 ? (u64)(unsigned)w_c : 0ull;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {                // inclusive prefix sum over the lanes, both halves at once
                    const u64 o = __shfl_up(pre, (unsigned)d, 64);
                    if (lane >= d) pre += o;
                }
                const u64 here = __shfl(pre, 63, 64);
                const u64 before = tot - after - here;             // what precedes these 64 elements
                const u64 cum = before + pre;                      // up to and including this element
                const int tp_i = (int)(cum >> 32), fp_i = (int)(cum & 0xffffffffull);
                double env = w_c > 0 ? (double)tp_i / ((double)fp_i + (double)tp_i + eps) : -1.0;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {                // inclusive suffix maximum over the lanes >= this one
                    const double o = __shfl_down(env, (unsigned)d, 64);
                    if (lane + d < 64) env = fmax(env, o);
                }
                env = fmax(env, carry_max);
                const int jbeg = boot_count_le((double)(int)(before >> 32) / npig, th0, th1, p.rec_thrs, p.R, lane);
                if (jbeg != jend) {                                // some threshold is served by a true positive among these 64
                    double part = 0.0;
                    if (is_tp) {
                        const double rc = (double)tp_i / npig, rc_prev = (double)(tp_i - w_c) / npig;
                        int lo = 0, hi = p.R;                       // jlo = #thr <= rc_prev
                        while (lo < hi) { const int mid = (lo + hi) >> 1; if (p.rec_thrs[mid] <= rc_prev) lo = mid + 1; else hi = mid; }
                        const int jlo = lo;
                        lo = 0; hi = p.R;                           // jhi = #thr <= rc
                        while (lo < hi) { const int mid = (lo + hi) >> 1; if (p.rec_thrs[mid] <= rc) lo = mid + 1; else hi = mid; }
                        for (int j = jlo; j < lo; ++j) part += env;
                    }
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d, 64);
                    sum += part;
                    jend = jbeg;
                }
                after += here;
                carry_max = __shfl(env, 0, 64);                    // lane 0 holds the maximum over these 64 and everything after
            }
            if (lane == 0) { s_after[r] = after; s_max[r] = carry_max; s_sum[r] = sum; s_jend[r] = jend; }
        }
    }
    __syncthreads();
    // thresholds <= 0 take the envelope of the whole list; without an included detection precision is 0 everywhere
    for (int r = wave; r < nb; r += BS_WAVES) {
        if (s_npig[r] == 0) continue;
        const int nle0 = boot_count_le(0.0, th0, th1, p.rec_thrs, p.R, lane);
        if (lane == 0) {
            double sum = 0.0;
            if (s_nd[r]) {
                sum = s_sum[r];
                for (int j = 0; j < nle0; ++j) sum += s_max[r];
            }
            p.ap[out(r)] = sum / p.R;
        }
    }
}

struct CountP {
    const int* grp_off;          // (K + 1) ranges of the groups per category
    const int* grp_img;          // (G) index of the group's image in [0, I)
    const int* grp_npig;         // (G, A) non-ignored ground truths of the group per range
    const int* weights;          // (B, I)
    int K, A, G, B, I, max_weight;
    int* npig_b;                 // (B, K, A)
    int* has_e_b;                // (B, K)
};

__global__ void __launch_bounds__(64) bootstrap_counts_kernel(CountP p) {
    const int k = blockIdx.x % p.K, b = blockIdx.x / p.K, lane = threadIdx.x;
    const int g0 = max(p.grp_off[k], 0), g1 = min(p.grp_off[k + 1], p.G);
    const int* wrow = p.weights + (long)b * p.I;
    int any = 0;
    for (int g = g0 + lane; g < g1; g += 64) {
        const int img = p.grp_img[g];
        if ((unsigned)img < (unsigned)p.I) any |= (unsigned)(wrow[img] - 1) < (unsigned)p.max_weight;      // 1 <= w <= max_weight
    }
    any = __ballot(any) != 0ull;
    if (lane == 0) p.has_e_b[(long)b * p.K + k] = any;
    for (int a = 0; a < p.A; ++a) {
        int acc = 0;
        for (int g = g0 + lane; g < g1; g += 64) {
            const int img = p.grp_img[g];
            if ((unsigned)img >= (unsigned)p.I) continue;
            const int w = wrow[img];
            if ((unsigned)w <= (unsigned)p.max_weight) acc += w * p.grp_npig[(long)g * p.A + a];
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
        if (lane == 0) p.npig_b[((long)b * p.K + k) * p.A + a] = acc;
    }
}

}  // namespace

extern "C" {

int omni_eval_bootstrap_counts(const int* grp_off, const int* grp_img, const int* grp_npig, const int* weights, int max_weight, int K,
                               int A, int G, int sumG, int B, int I, int* npig_b, int* has_e_b, void* stream) {
    if (K < 0 || A <= 0 || G < 0 || sumG < 0 || B <= 0 || I < 0 || max_weight < 0) return OMNI_ERR_ARG;
    if ((long long)sumG * max_weight >= 0x80000000LL || (long long)B * K > 0x7fffffffLL) return OMNI_ERR_ARG;
    if (K == 0) return OMNI_OK;
    if (!grp_off || !npig_b || !has_e_b || (G > 0 && (!grp_img || !grp_npig || !weights))) return OMNI_ERR_ARG;
    CountP p{grp_off, grp_img, grp_npig, weights, K, A, G, B, I, max_weight, npig_b, has_e_b};
    hipLaunchKernelGGL(bootstrap_counts_kernel, dim3((unsigned)((long)B * K)), dim3(64), 0, (hipStream_t)stream, p);
    return omni_launch_status();
}

int omni_eval_bootstrap(const int* order, const int* cat_off, const int* rank, const int* dt_match, const unsigned char* dt_ignore,
                        const int* det_img, const int* weights, int max_weight, const int* npig_b, const int* has_e_b,
                        const double* rec_thrs, const int* max_dets, int K, int A, int M, int T, int R, int sumD, int B, int I,
                        double* ap, double* ar, void* stream) {
    if (K < 0 || A <= 0 || M <= 0 || T <= 0 || R <= 0 || sumD < 0 || B <= 0 || I < 0 || max_weight < 0) return OMNI_ERR_ARG;
    if (I >= BS_MAX_I || (long long)sumD * max_weight >= 0x80000000LL) return OMNI_ERR_ARG;          // the counts stay below 2^31
    if ((long long)K * A * M * T > 0x7fffffffLL || (B + BS_NB - 1) / BS_NB > 65535) return OMNI_ERR_ARG;
    if (K == 0) return OMNI_OK;
    if (!cat_off || !npig_b || !has_e_b || !rec_thrs || !max_dets || !ap || !ar) return OMNI_ERR_ARG;
    if (sumD > 0 && (!order || !rank || !dt_match || !dt_ignore || !det_img || !weights)) return OMNI_ERR_ARG;
    BootP p{order, cat_off, rank, dt_match, dt_ignore, det_img, weights, npig_b, has_e_b, rec_thrs, max_dets,
            K, A, M, T, R, sumD, B, I, max_weight, ap, ar};
    hipLaunchKernelGGL(eval_bootstrap_kernel, dim3((unsigned)((long)K * A * M * T), (unsigned)((B + BS_NB - 1) / BS_NB)), dim3(BS_T), 0,
                       (hipStream_t)stream, p);
    return omni_launch_status();
}

}  // extern "C"
