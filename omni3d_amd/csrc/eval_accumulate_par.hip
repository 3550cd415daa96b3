// eval_accumulate_par.hip -- Omni3Deval.accumulate over MANY workgroups per list: the tables of eval_accumulate_kernel
// (csrc/eval_match.hip), bit for bit, when a (category, range, maxDets, threshold) list is too long for one wave.  With useCats = 0 there
// is ONE list of all detections of the data set and only A x M x T waves; here every list is cut into blocks of `block` elements of
// `order` and every block is one 64-lane wave.
//
// Every quantity of the accumulation is an integer count, a maximum of doubles, or a quotient of counts, so the split changes no bit:
//   acc_par_count_kernel  per block: the number of included elements (rank < maxDets), its true and false positives, the position of the
//                         first included element.  Block 0 of a list also zero-fills the list's precision / scores cells, as
//                         eval_accumulate_kernel does before its walk.
//   acc_par_prec_kernel   each block sums the totals of the blocks before it (integers: any order gives the same sum), keeps that prefix
//                         for the last launch, forms tp_i / (fp_i + tp_i + eps) for its included elements with the expression and eps
//                         of eval_accumulate_kernel, and writes the maximum over the block (-1 without an included element).
//   acc_par_sweep_kernel  each block takes the maximum over the LATER blocks as its carry (a maximum of doubles without NaN: any order
//                         gives the same value), sweeps its own elements backwards exactly like eval_accumulate_kernel and writes the
//                         thresholds its true positives serve: a threshold in ((c-1)/npig, c/npig] belongs to the c-th true positive
//                         alone, so no two blocks write the same cell.  Block 0 writes `recall` and the thresholds <= 0.
// The dependency between the phases is the launch boundary: plain launches on one stream, no grid-wide barrier, no flag another workgroup
// waits for, no atomics.  The workspace belongs to the caller: one AccBlk per (list, block slot).
#include <device_rt.h>

#pragma clang fp contract(off)

namespace {

struct AccBlk {                  // one per (list, block): 32 bytes
    int nd, tp, fp, first;       // launch 1: totals over the block, first included position (0x7fffffff without one)
    int tp_pre, fp_pre;          // launch 2: totals over the blocks before it
    double bmax;                 // launch 2: the largest precision of the block, -1 without an included element
};

struct AccParP {
    const int* order;            // (N) detection index (into the group-concatenated arrays) by sorted position
    const int* cat_off;          // (K + 1) ranges of `order` per category
    const int* rank;             // (sumD) rank of a detection inside its image's list (descending score)
    const double* score;         // (sumD)
    const int* dt_match;         // (A, T, sumD) >= 0 matched
    const unsigned char* dt_ig;  // (A, T, sumD)
    const int* npig;             // (K, A) number of non-ignored ground truths
    const int* has_e;            // (K)
    const double* rec_thrs;      // (R) ascending
    const int* max_dets;         // (M)
    int K, A, M, T, R, sumD;
    int block, nb;               // elements per block (a multiple of 64), block slots per list
    AccBlk* ws;                  // (K * A * M * T, nb)
    double* precision;           // (T, R, K, A, M)
    double* recall;              // (T, K, A, M)
    double* scores;              // (T, R, K, A, M)
};

// what every phase needs of its (list, block): false when the workgroup has nothing to do
struct AccCtx {
    int k, a, m, t, b, lane;
    int npig, maxdet, nblk;      // nblk: the blocks of this list that hold elements
    int e0, e1;                  // this block's range of `order`
    const int* dtm;
    const unsigned char* dtg;
    AccBlk* slots;               // the list's nb slots
};

__device__ __forceinline__ bool acc_ctx(const AccParP& p, AccCtx& c) {
    long long id = blockIdx.x;
    c.b = (int)(id % p.nb); id /= p.nb;
    c.t = (int)(id % p.T); id /= p.T;
    c.m = (int)(id % p.M); id /= p.M;
    c.a = (int)(id % p.A);
    c.k = (int)(id / p.A);
    c.lane = threadIdx.x;
    if (!p.has_e[c.k]) return false;                           // E empty: the -1 of the caller stays
    c.npig = p.npig[c.k * p.A + c.a];
    if (c.npig == 0) return false;
    const int s0 = p.cat_off[c.k], s1 = p.cat_off[c.k + 1];
    c.nblk = (int)(((long long)(s1 - s0) + p.block - 1) / p.block);
    if (c.nblk > p.nb) c.nblk = p.nb;                          // a list longer than the entry was told of: never past the workspace
    if (c.b >= c.nblk && c.b != 0) return false;               // block 0 runs for an empty list too: it owns recall and the zero fill
    const long long e0 = (long long)s0 + (long long)c.b * p.block;
    c.e0 = (int)(e0 < s1 ? e0 : s1);
    c.e1 = (int)(e0 + p.block < s1 ? e0 + p.block : s1);
    c.maxdet = p.max_dets[c.m];
    const long long slice = ((long long)c.a * p.T + c.t) * p.sumD;
    c.dtm = p.dt_match + slice;
    c.dtg = p.dt_ig + slice;
    c.slots = p.ws + ((((long long)c.k * p.A + c.a) * p.M + c.m) * p.T + c.t) * p.nb;
    return true;
}

__device__ __forceinline__ long long acc_pidx(const AccParP& p, const AccCtx& c, int r) {
    return ((((long long)c.t * p.R + r) * p.K + c.k) * p.A + c.a) * p.M + c.m;
}

__device__ __forceinline__ double acc_shfl_down_d(double v, int d) { return __shfl_down(v, (unsigned)d, 64); }

// ---- launch 1 ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) acc_par_count_kernel(AccParP p) {
    AccCtx c;
    if (!acc_ctx(p, c)) return;
    if (c.b == 0)
        for (int r = c.lane; r < p.R; r += 64) { p.precision[acc_pidx(p, c, r)] = 0.0; p.scores[acc_pidx(p, c, r)] = 0.0; }
    int tp = 0, fp = 0, nd = 0, first = 0x7fffffff;
    for (int s = c.e0 + c.lane; s < c.e1; s += 64) {
        const int d = p.order[s];
        if (p.rank[d] < c.maxdet) {
            ++nd;
            first = min(first, s);
            const bool ig = c.dtg[d] != 0, mt = c.dtm[d] >= 0;
            tp += (mt && !ig);
            fp += (!mt && !ig);
        }
    }
    tp = wave_sum_i(tp);
    fp = wave_sum_i(fp);
    nd = wave_sum_i(nd);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) first = min(first, __shfl_xor(first, d, 64));
    if (c.lane == 0) {
        AccBlk* w = c.slots + c.b;
        w->nd = nd; w->tp = tp; w->fp = fp; w->first = first;
        w->tp_pre = 0; w->fp_pre = 0; w->bmax = -1.0;
    }
}

// ---- launch 2 ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) acc_par_prec_kernel(AccParP p) {
    AccCtx c;
    if (!acc_ctx(p, c)) return;
    if (c.b >= c.nblk) return;                                 // block 0 of an empty list
    int tp_pre = 0, fp_pre = 0;
    for (int q = c.lane; q < c.b; q += 64) { tp_pre += c.slots[q].tp; fp_pre += c.slots[q].fp; }
    tp_pre = wave_sum_i(tp_pre);
    fp_pre = wave_sum_i(fp_pre);
    const double eps = 2.220446049250313e-16;                 // np.spacing(1)
    int tp_run = tp_pre, fp_run = fp_pre;
    double best = -1.0;
    for (int s0 = c.e0; s0 < c.e1; s0 += 64) {
        const int s = s0 + c.lane;
        bool incl = false, is_tp = false, is_fp = false;
        if (s < c.e1) {
            const int d = p.order[s];
            if (p.rank[d] < c.maxdet) {
                incl = true;
                const bool ig = c.dtg[d] != 0, mt = c.dtm[d] >= 0;
                is_tp = mt && !ig;
                is_fp = !mt && !ig;
            }
        }
        const unsigned long long tpm = __ballot(is_tp), fpm = __ballot(is_fp);
        const unsigned long long upto = c.lane == 63 ? ~0ull : ((1ull << (c.lane + 1)) - 1ull);
        const int tp_i = tp_run + __popcll(tpm & upto);        // cumulative counts up to and including this element
        const int fp_i = fp_run + __popcll(fpm & upto);
        if (incl) best = fmax(best, (double)tp_i / ((double)fp_i + (double)tp_i + eps));
        tp_run += __popcll(tpm);
        fp_run += __popcll(fpm);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) best = fmax(best, __shfl_xor(best, d, 64));
    if (c.lane == 0) {
        AccBlk* w = c.slots + c.b;
        w->tp_pre = tp_pre; w->fp_pre = fp_pre; w->bmax = best;
    }
}

// ---- launch 3 ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) acc_par_sweep_kernel(AccParP p) {
    AccCtx c;
    if (!acc_ctx(p, c)) return;
    const int lane = c.lane, npig = c.npig;
    // the maximum over everything behind this block
    double carry_max = -1.0;
    for (int q = c.b + 1 + lane; q < c.nblk; q += 64) carry_max = fmax(carry_max, c.slots[q].bmax);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) carry_max = fmax(carry_max, __shfl_xor(carry_max, d, 64));
    int nd_all = 0, tp_all = 0, first = 0x7fffffff;
    if (c.b == 0) {                                            // totals of the list: recall (:1278-1282)
        for (int q = lane; q < c.nblk; q += 64) { nd_all += c.slots[q].nd; tp_all += c.slots[q].tp; first = min(first, c.slots[q].first); }
        nd_all = wave_sum_i(nd_all);
        tp_all = wave_sum_i(tp_all);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) first = min(first, __shfl_xor(first, d, 64));
        if (lane == 0) p.recall[(((long long)c.t * p.K + c.k) * p.A + c.a) * p.M + c.m] = nd_all ? (double)tp_all / npig : 0.0;
        if (nd_all == 0) return;
    }
    if (c.b < c.nblk && c.slots[c.b].nd > 0) {
        const AccBlk w = c.slots[c.b];
        const double eps = 2.220446049250313e-16;             // np.spacing(1)
        const int tp_end = w.tp_pre + w.tp, fp_end = w.fp_pre + w.fp;      // cumulative counts at the end of this block
        int tp_after = 0, fp_after = 0;
        const int nchunk = (c.e1 - c.e0 + 63) / 64;
        for (int ch = nchunk - 1; ch >= 0; --ch) {
            const int s = c.e0 + ch * 64 + lane;
            bool incl = false, is_tp = false, is_fp = false;
            double sc = 0.0;
            if (s < c.e1) {
                const int d = p.order[s];
                if (p.rank[d] < c.maxdet) {
                    incl = true;
                    const bool ig = c.dtg[d] != 0, mt = c.dtm[d] >= 0;
                    is_tp = mt && !ig;
                    is_fp = !mt && !ig;
                    sc = p.score[d];
                }
            }
            const unsigned long long tpm = __ballot(is_tp), fpm = __ballot(is_fp);
            const unsigned long long higher = lane == 63 ? 0ull : (~0ull << (lane + 1));
            const int tp_i = tp_end - tp_after - __popcll(tpm & higher);
            const int fp_i = fp_end - fp_after - __popcll(fpm & higher);
            double env = incl ? (double)tp_i / ((double)fp_i + (double)tp_i + eps) : -1.0;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {                // inclusive suffix maximum over the lanes >= this one
                const double o = acc_shfl_down_d(env, d);
                if (lane + d < 64) env = fmax(env, o);
            }
            env = fmax(env, carry_max);
            if (is_tp) {
                const double rc = (double)tp_i / npig, rc_prev = (double)(tp_i - 1) / npig;
                int lo = 0, hi = p.R;                           // jlo = #thr <= rc_prev
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (p.rec_thrs[mid] <= rc_prev) lo = mid + 1; else hi = mid; }
                const int jlo = lo;
                lo = 0; hi = p.R;                               // jhi = #thr <= rc
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (p.rec_thrs[mid] <= rc) lo = mid + 1; else hi = mid; }
                for (int j = jlo; j < lo; ++j) { p.precision[acc_pidx(p, c, j)] = env; p.scores[acc_pidx(p, c, j)] = sc; }
            }
            tp_after += __popcll(tpm);
            fp_after += __popcll(fpm);
            carry_max = __shfl(env, 0, 64);                    // lane 0: the maximum over this chunk and everything after it
        }
    }
    // thresholds <= 0 (recThrs[0] = 0): searchsorted gives index 0 = the first included element of the list
    if (c.b == 0 && lane == 0) {
        const double sc0 = p.score[p.order[first]];
        for (int j = 0; j < p.R && p.rec_thrs[j] <= 0.0; ++j) { p.precision[acc_pidx(p, c, j)] = carry_max; p.scores[acc_pidx(p, c, j)] = sc0; }
    }
}

// block slots per list: a list is at most sumD long
inline long long acc_par_slots(int sumD, int block) { return sumD > 0 ? ((long long)sumD + block - 1) / block : 1; }

}  // namespace

extern "C" {

int omni_eval_accumulate_par_workspace(int K, int A, int M, int T, int sumD, int block, long long* bytes) {
    if (K < 0 || A <= 0 || M <= 0 || T <= 0 || sumD < 0 || block < 64 || block % 64 != 0 || !bytes) return OMNI_ERR_ARG;
    *bytes = (long long)K * A * M * T * acc_par_slots(sumD, block) * (long long)sizeof(AccBlk);
    return OMNI_OK;
}

int omni_eval_accumulate_par(const int* order, const int* cat_off, const int* rank, const double* score, const int* dt_match,
                             const unsigned char* dt_ignore, const int* npig, const int* has_e, const double* rec_thrs,
                             const int* max_dets, int K, int A, int M, int T, int R, int sumD, int block, void* workspace,
                             long long workspace_bytes, double* precision, double* recall, double* scores, void* stream) {
    if (K < 0 || A <= 0 || M <= 0 || T <= 0 || R <= 0 || sumD < 0 || block < 64 || block % 64 != 0) return OMNI_ERR_ARG;
    if (K == 0) return OMNI_OK;
    const long long nb = acc_par_slots(sumD, block), grid = (long long)K * A * M * T * nb;
    if (grid >= (1ll << 31)) return OMNI_ERR_ARG;
    if (!workspace || ((unsigned long long)workspace & 7ull) || workspace_bytes < grid * (long long)sizeof(AccBlk)) return OMNI_ERR_ARG;
    AccParP p{order, cat_off, rank, score, dt_match, dt_ignore, npig, has_e, rec_thrs, max_dets, K, A, M, T, R, sumD,
              block, (int)nb, (AccBlk*)workspace, precision, recall, scores};
    hipLaunchKernelGGL(acc_par_count_kernel, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, p);
    hipLaunchKernelGGL(acc_par_prec_kernel, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, p);
    hipLaunchKernelGGL(acc_par_sweep_kernel, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, p);
    return omni_launch_status();
}

}  // extern "C"
