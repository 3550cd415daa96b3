// eval_errors.hip -- the error decomposition of the Omni3D evaluator (`Omni3Deval.errors`): every detection of a data set gets one of
// seven codes (true positive, ignored, or one of the five false-positive types of TIDE: Bolya et al., "TIDE: A General Toolbox for
// Identifying Object Detection Errors", ECCV 2020), the ground truth it is attributed to, and whether it wins the contest for that
// ground truth under the Loc / Cls oracles; every ground truth gets its Miss flag.  One launch for the whole data set.  The reference
// has no counterpart and no call site: the definitions are this project's and stand in the docstring of `Omni3Deval.errors`.
//
// Input is the IMAGE-level similarity (all detections of an image against all its ground truths, over all categories) and, per row, the
// outcome of the greedy matching at one (range, threshold): matched / ignored.  A ground truth that is `_ignore` is no candidate.  For
// a false positive of category c:
//   s_free  = max similarity to an unmatched candidate of category c,   s_used = the same over the matched candidates of category c,
//   s_other = the same over the candidates of every other category;     -inf for an empty set, the LATER row among equal values
//   (eval_match's rule).  In this order: Loc if s_free >= t_bg, Cls if s_other >= t_fg, Dupe if s_used >= t_fg, Bkg if all three
//   < t_bg, Both otherwise.  Attributed: the arg-max of the deciding set for Loc / Cls / Dupe, -1 otherwise.
// The similarities are float32; they are compared with the double thresholds as doubles (eval_match_kernel's rule), `>=` / `<` as written.
// Contest: among the Loc (Cls) detections attributed to one ground truth the highest score wins, the lower row among equal scores;
// `win_cls` is set only when that ground truth is unmatched (a matched one takes no second true positive).  Miss: an unmatched candidate
// that no Loc or Cls detection is attributed to.
//
//   error_types_kernel   one 256-thread workgroup per image, ONE DETECTION PER THREAD (detections are independent here, unlike in the
//                        greedy matching, and an image has several times more detections than ground truths: lanes spread over the
//                        ground truths would idle and pay three shuffle arg-max reductions per detection).  The ground truths'
//                        category and flags are staged through LDS in chunks of 64; a thread walks its own row of the matrix with
//                        three running maxima in registers.  The contests are two integer LDS atomics per claimed ground truth:
//                        atomicMax on the order-preserving integer image of the score, then atomicMin on the row among the holders of
//                        that maximum.  Integer max / min do not depend on arrival order and there is no floating-point atomic: the
//                        result is a function of (score bits, row) alone and two runs give the same bits.
// Capacity: the contest tables hold ERR_MAXG = 1024 ground truths per image; more is refused before the launch, nothing is truncated.
#include <device_rt.h>

namespace {

constexpr int ERR_MAXG = 1024;   // ground truths per image (contest tables in LDS)
constexpr int CHUNK = 64;        // ground-truth metadata staged in LDS at a time
constexpr int NT = 256;

enum { TY_TP = 0, TY_IGN = 1, TY_CLS = 2, TY_LOC = 3, TY_BOTH = 4, TY_DUPE = 5, TY_BKG = 6 };

struct ErrP {
    const float* sim;                 // ragged: image i holds a (D_i, G_i) row-major matrix at sim_off[i]
    const long long* sim_off;         // (I + 1)
    const int* dt_off;                // (I + 1)
    const int* gt_off;                // (I + 1)
    const int* dt_cat;                // (sumD)
    const unsigned char* dt_matched;  // (sumD) dt_match >= 0
    const unsigned char* dt_ignore;   // (sumD)
    const double* dt_score;           // (sumD)
    const int* gt_cat;                // (sumG)
    const unsigned char* gt_matched;  // (sumG)
    const unsigned char* gt_ignore;   // (sumG) `_ignore` at the chosen range
    double t_fg, t_bg;
    signed char* type;                // (sumD)
    int* attr;                        // (sumD) global ground-truth row or -1
    float* smax;                      // (sumD, 3) s_free, s_used, s_other
    unsigned char* win_loc;           // (sumD)
    unsigned char* win_cls;           // (sumD)
    unsigned char* gt_missed;         // (sumG)
};

// an unsigned integer that orders like the double (negative values below positive ones); 0 is kept for "nobody"
__device__ __forceinline__ unsigned long long score_key(double s) {
    unsigned long long u;
    __builtin_memcpy(&u, &s, 8);
    u = (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    return u ? u : 1ull;
}

__global__ void __launch_bounds__(NT) error_types_kernel(ErrP p) {
    __shared__ unsigned long long s_key_loc[ERR_MAXG];
    __shared__ unsigned long long s_key_cls[ERR_MAXG];
    __shared__ int s_row_loc[ERR_MAXG];
    __shared__ int s_row_cls[ERR_MAXG];
    __shared__ int s_cat[CHUNK];
    __shared__ unsigned char s_flag[CHUNK];       // bit 0 matched, bit 1 ignored
    const int t = threadIdx.x, img = blockIdx.x;
    const int d0 = p.dt_off[img], d1 = p.dt_off[img + 1], g0 = p.gt_off[img], G = p.gt_off[img + 1] - g0;
    const float* S = p.sim + p.sim_off[img];
    const float ninf = -__builtin_huge_valf();
    for (int g = t; g < G; g += NT) { s_key_loc[g] = 0ull; s_key_cls[g] = 0ull; s_row_loc[g] = 0x7fffffff; s_row_cls[g] = 0x7fffffff; }
    __syncthreads();
    // ---- pass 1: the three maxima, the code, the attributed ground truth, the claims ----
    for (int base = d0; base < d1; base += NT) {           // the same trip count in every thread: the barriers below are uniform
        const int d = base + t;
        const bool active = d < d1;
        const int cat = active ? p.dt_cat[d] : -1;
        const float* row = S + (long)(d - d0) * G;
        float vf = ninf, vu = ninf, vo = ninf;
        int af = -1, au = -1, ao = -1;
        for (int c0 = 0; c0 < G; c0 += CHUNK) {
            const int n = min(CHUNK, G - c0);
            __syncthreads();                               // the previous chunk has been read by everyone
            if (t < n) {
                s_cat[t] = p.gt_cat[g0 + c0 + t];
                s_flag[t] = (unsigned char)((p.gt_matched[g0 + c0 + t] ? 1 : 0) | (p.gt_ignore[g0 + c0 + t] ? 2 : 0));
            }
            __syncthreads();
            if (active) {
                for (int j = 0; j < n; ++j) {
                    const int f = s_flag[j];
                    if (f & 2) continue;                   // no candidate
                    const float v = row[c0 + j];           // float >= float is the comparison of the two as doubles; NaN never wins
                    if (s_cat[j] != cat) { if (v >= vo) { vo = v; ao = c0 + j; } }          // ascending rows: the later row wins a tie
                    else if (f & 1) { if (v >= vu) { vu = v; au = c0 + j; } }
                    else { if (v >= vf) { vf = v; af = c0 + j; } }
                }
            }
        }
        if (!active) continue;
        int ty, at = -1;
        if (p.dt_ignore[d]) ty = TY_IGN;
        else if (p.dt_matched[d]) ty = TY_TP;
        else {
            const double f = (double)vf, u = (double)vu, o = (double)vo;
            if (f >= p.t_bg) { ty = TY_LOC; at = af; }
            else if (o >= p.t_fg) { ty = TY_CLS; at = ao; }
            else if (u >= p.t_fg) { ty = TY_DUPE; at = au; }
            else if (fmax(f, fmax(u, o)) < p.t_bg) ty = TY_BKG;
            else ty = TY_BOTH;
        }
        p.type[d] = (signed char)ty;
        p.attr[d] = at >= 0 ? g0 + at : -1;
        p.smax[3L * d] = vf; p.smax[3L * d + 1] = vu; p.smax[3L * d + 2] = vo;
        if (ty == TY_LOC) atomicMax(&s_key_loc[at], score_key(p.dt_score[d]));
        else if (ty == TY_CLS) atomicMax(&s_key_cls[at], score_key(p.dt_score[d]));
    }
    __syncthreads();
    // ---- pass 2: among the holders of the best score of a ground truth, the lowest row ----
    for (int base = d0; base < d1; base += NT) {
        const int d = base + t;
        if (d >= d1) continue;
        const int ty = p.type[d];                          // this thread's own stores
        if (ty != TY_LOC && ty != TY_CLS) continue;
        const int at = p.attr[d] - g0;
        const unsigned long long key = score_key(p.dt_score[d]);
        if (ty == TY_LOC) { if (key == s_key_loc[at]) atomicMin(&s_row_loc[at], d - d0); }
        else if (key == s_key_cls[at]) atomicMin(&s_row_cls[at], d - d0);
    }
    __syncthreads();
    // ---- pass 3: the winners and the missed ground truths ----
    for (int base = d0; base < d1; base += NT) {
        const int d = base + t;
        if (d >= d1) continue;
        const int ty = p.type[d];
        const int at = p.attr[d] - g0;
        p.win_loc[d] = (ty == TY_LOC && s_row_loc[at] == d - d0) ? 1 : 0;
        p.win_cls[d] = (ty == TY_CLS && s_row_cls[at] == d - d0 && !p.gt_matched[g0 + at]) ? 1 : 0;
    }
    for (int g = t; g < G; g += NT)
        p.gt_missed[g0 + g] = (!p.gt_ignore[g0 + g] && !p.gt_matched[g0 + g] && s_key_loc[g] == 0ull && s_key_cls[g] == 0ull) ? 1 : 0;
}

}  // namespace

extern "C" {

int omni_eval_error_types(const float* sim, const long long* sim_off, const int* dt_off, const int* gt_off, const int* dt_cat,
                          const unsigned char* dt_matched, const unsigned char* dt_ignore, const double* dt_score, const int* gt_cat,
                          const unsigned char* gt_matched, const unsigned char* gt_ignore, double t_fg, double t_bg, int I, int sumD,
                          int sumG, int max_gt, signed char* type, int* attr, float* smax, unsigned char* win_loc,
                          unsigned char* win_cls, unsigned char* gt_missed, void* stream) {
    if (I < 0 || sumD < 0 || sumG < 0 || max_gt < 0 || max_gt > ERR_MAXG || (I == 0 && (sumD > 0 || sumG > 0))) return OMNI_ERR_ARG;
    if (!(t_bg > 0.0 && t_bg < t_fg)) return OMNI_ERR_ARG;                       // NaN included
    if (I == 0) return OMNI_OK;
    if (!sim_off || !dt_off || !gt_off) return OMNI_ERR_ARG;
    if (sumD > 0 && (!dt_cat || !dt_matched || !dt_ignore || !dt_score || !type || !attr || !smax || !win_loc || !win_cls)) return OMNI_ERR_ARG;
    if (sumG > 0 && (!gt_cat || !gt_matched || !gt_ignore || !gt_missed)) return OMNI_ERR_ARG;
    ErrP p{sim, sim_off, dt_off, gt_off, dt_cat, dt_matched, dt_ignore, dt_score, gt_cat, gt_matched, gt_ignore, t_fg, t_bg,
           type, attr, smax, win_loc, win_cls, gt_missed};
    hipLaunchKernelGGL(error_types_kernel, dim3((unsigned)I), dim3(NT), 0, (hipStream_t)stream, p);
    return omni_launch_status();
}

}  // extern "C"
