// select_nms.hip -- index-exact selection kernels: row-wise sorted top-k and greedy NMS.
//
// Replaces (bit-exact on the selected indices):
//   logits.sort(descending)[:k] per level            detectron2 find_top_rpn_proposals (RPN of
//                                                     /root/reference/configs/Base.yaml:49-54)
//   torch.multinomial(w, k) == topk(w / Exp(1), k)   /root/reference/cubercnn/modeling/proposal_generator/rpn.py:318,322
//   torchvision.ops.nms via detectron2 batched_nms   rpn [upstream]; cubercnn/modeling/roi_heads/fast_rcnn.py:105
//
// Top-k: one 1024-thread workgroup per row.  Keys become order-preserving 64-bit integers
// (float bits, then ~index so that equal scores resolve to the LOWER index = a stable descending
// sort); an 8-pass MSB-first radix select finds the k-th largest key exactly, survivors are
// compacted into LDS and bitonic-sorted.  k <= 8192.  Rows of up to 65536 elements (every row of the training step:
// 49152 anchors of the finest level, 65472 sampling keys per image) are read from memory ONCE: each thread keeps the score bits
// of its <= 64 elements in registers and the radix passes and the compaction run on those.
// Up to 2048 keys are sorted two per thread in registers: strides below 128 are shuffles inside a wave, only the 10 passes of a
// 2048-key sort whose partner sits in another wave go through LDS and a barrier (all 66 did before).
// What bounds it (MI355X, the step's 4 x [49152 .. 192] -> 2000 launch, 60.8 us in the kernel trace, 66.8 before): about 23 us are
// there for a 3072-element row with k = 64 (the two radix selections: up to 8 passes of 4 barriers each), about 10 us more for
// k = 2000 (compaction, sort, output), and about 28 us more for the 49152-element row (load, the per-thread top 4 over 48
// elements, the compaction loop); the launch lasts as long as that one row.  Splitting the long row over workgroups does not
// pay while the fixed part is this large: by the timings per row length a 16384-element slice still costs ~45 us and a
// finishing selection over 3 x 2000 candidates ~35 us more.
// The compactions need no hand-written wave aggregation: the compiler already turns the per-lane LDS atomicAdd(.., 1) into one
// add of the active-lane count per wave (v_mbcnt + s_bcnt1 in the ISA).
//
// NMS: boxes arrive sorted by descending score.  nms_mask_kernel writes a 64x64-bit suppression tile per wave (strict
// IoU > thr, areas (x2-x1)*(y2-y1), no +1; the quotient is only evaluated in a band of 2^-20 around the threshold), then
// nms_scan_kernel, one workgroup per problem, walks the rows in 64-box chunks: the chunk is resolved from its diagonal words by a
// fixed-point iteration of ballots, then the kept rows OR their mask rows into the running `removed` words (one 64-bit word
// per lane), with the rows of two chunks in flight.  Measured for the step's 20 x 2000 problems at 0.7: mask 70.6 -> 56.1 us
// (instruction issue: ~23 vector instructions per column and row block, 37 before), scan 115.4 -> 37.0 us (it was a chain of
// exposed load latencies and 64 cross-lane steps per chunk); with the per-problem counts the proposal path now passes, the
// padding of the two coarse levels is not visited and both together take 70 us (187 before).  profiles/r07_select_breakdown.log.
#include <device_rt.h>

namespace {

constexpr int TOPK_THREADS = 1024;
constexpr int TOPK_MAXK = 8192;      // 64 KB of LDS keys; the batched-inference candidate sort uses the full size

__device__ __forceinline__ unsigned score_bits(float f) {
    unsigned u = __float_as_uint(f);
    if (f != f) u = 0u;  // NaN sorts last
    else if (f == 0.f) u = 0x80000000u;  // -0.0 and +0.0 compare equal (torch.sort): one key, the index decides
    else u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return u;
}
__device__ __forceinline__ unsigned long long key_of_bits(unsigned u, int idx) {
    return ((unsigned long long)u << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)idx);
}
__device__ __forceinline__ unsigned long long make_key(float f, int idx) { return key_of_bits(score_bits(f), idx); }
// key_of_bits(u, idx) >= thr, on the two 32-bit halves (cached rows keep ONE register per element: a 64-bit key per element that
// lives across the passes doubles them)
// sel[slot] = key_of_bits(u, idx) as two 32-bit stores: a 64-bit store makes the register allocator keep every cached score word
// in the odd half of an aligned pair
__device__ __forceinline__ void store_key(unsigned long long* sel, int slot, unsigned u, int idx) {
    unsigned* w = reinterpret_cast<unsigned*>(sel + slot);
    w[0] = 0xFFFFFFFFu - (unsigned)idx;
    w[1] = u;
}
__device__ __forceinline__ bool key_ge(unsigned u, int idx, unsigned thi, unsigned tlo) {
    return u > thi || (u == thi && (0xFFFFFFFFu - (unsigned)idx) >= tlo);
}
__device__ __forceinline__ float key_value(unsigned long long k) {
    unsigned u = (unsigned)(k >> 32);
    u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
    return __uint_as_float(u);
}
__device__ __forceinline__ int key_index(unsigned long long k) { return (int)(0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull)); }

// Column segments of a row: segment s covers elements [off[s], off[s] + n[s]); one workgroup per (row, segment).
constexpr int TOPK_MAXSEG = 8;
struct SegP {
    int S;
    int off[TOPK_MAXSEG], n[TOPK_MAXSEG];
};

// ---- radix selection machinery (one 1024-thread workgroup) ----------------------------------------------------------------
// Scores cluster (the sign/exponent byte of RPN logits takes 2-3 values), so plain LDS atomics would serialise tens of thousands
// of adds on one bin: each wave first folds its lanes that share the leader's digit into ONE add (4 rounds), the rest fall back
// to per-lane atomics.  Must be called by whole waves (ballots / shuffles).
__device__ __forceinline__ void count_digit(unsigned* hist, bool todo, unsigned digit) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int round = 0; round < 4; ++round) {
        const unsigned long long pending = __ballot(todo);
        if (pending == 0ull) break;
        const int leader = __ffsll((long long)pending) - 1;
        const unsigned d = (unsigned)__shfl((int)digit, leader, 64);
        const unsigned long long same = __ballot(todo && digit == d);
        if (lane == leader) atomicAdd(&hist[d], (unsigned)__popcll(same));
        if (todo && digit == d) todo = false;
    }
    if (todo) atomicAdd(&hist[digit], 1u);
}

struct RadixShared {
    unsigned hist[256];
    unsigned wsum[4];
    unsigned long long prefix;
    int need, done;
};

// After a pass's histogram is complete (and a barrier): the bin that holds the `need`-th largest candidate, found by a suffix scan
// of the 256 bins over 256 threads (round 3: thread 0 used to walk the bins one dependent LDS read at a time, ~3 us per pass).
// Extends the prefix by that digit, lowers `need` by the candidates in the higher bins, sets `done` when every remaining candidate
// is needed.  Contains one barrier; the caller adds one after it.
__device__ __forceinline__ void radix_pick_bin(RadixShared& R, int shift) {
    const int t = threadIdx.x;
    const int need = R.need;                       // (read by everyone before the barrier below, written after it)
    const unsigned long long prefix = R.prefix;
    unsigned v = 0u, incl = 0u;
    if (t < 256) {
        v = R.hist[255 - t];                        // thread t looks at digit 255 - t: inclusive scan = candidates with digit >= d
        incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned u = __shfl_up(incl, o, 64);
            if ((t & 63) >= o) incl += u;
        }
        if ((t & 63) == 63) R.wsum[t >> 6] = incl;
    }
    __syncthreads();
    if (t < 256) {
        for (int w = 0; w < (t >> 6); ++w) incl += R.wsum[w];
        const unsigned above = incl - v;            // candidates in the bins above this one
        // the first bin (from the top) whose cumulative count reaches `need`; digit 0 takes whatever is left
        if (((int)incl >= need || t == 255) && (int)above < need) {
            R.need = need - (int)above;
            R.prefix = prefix | ((unsigned long long)(255 - t) << shift);
            // all remaining candidates share the prefix and every one of them is needed: the lower bytes cannot separate
            // anything any more (distinct scores settle after the 4 score bytes; the index bytes only matter when equal scores
            // straddle the k-th place)
            R.done = ((int)v == need - (int)above) ? 1 : 0;
        }
    }
}

// k-th largest (kth >= 1, at most the number of valid entries) of the 64-bit keys (eu[c] << 32 | el[c]) spread over the threads'
// register lists; -> threshold: exactly kth keys are >= it (keys are unique).  Whole workgroup; barriers inside.
template <int CNT>
__device__ __forceinline__ unsigned long long radix_kth(RadixShared& R, const unsigned (&eu)[CNT], const unsigned (&el)[CNT],
                                                        const bool (&ev)[CNT], int kth) {
    const int t = threadIdx.x;
    if (t == 0) { R.prefix = 0ull; R.need = kth; }
    __syncthreads();
    for (int pass = 7; pass >= 0; --pass) {
        if (t < 256) R.hist[t] = 0u;
        __syncthreads();
        const unsigned long long prefix = R.prefix;
        const unsigned phi = (unsigned)(prefix >> 32), plo = (unsigned)prefix;
        const bool hi = pass >= 4;
        const int sh = hi ? pass * 8 - 32 : pass * 8;
#pragma unroll
        for (int c = 0; c < CNT; ++c) {
            const unsigned w = hi ? eu[c] : el[c], pw = hi ? phi : plo;
            bool todo = ev[c] && (hi || eu[c] == phi);
            if (sh < 24) todo = todo && ((w >> (sh + 8)) == (pw >> (sh + 8)));
            count_digit(R.hist, todo, (w >> sh) & 255u);
        }
        __syncthreads();
        radix_pick_bin(R, pass * 8);
        __syncthreads();
        if (R.done) break;
    }
    const unsigned long long thr = R.prefix;
    __syncthreads();                                 // (the next selection resets the shared state)
    return thr;
}

// keys: (rows, n) with row pitch `pitch` and element stride `estride` (floats).
// NPT > 0: every segment has at most NPT * 1024 elements and a thread caches its NPT score words in registers; 0: streamed.
//
// Cached rows with k <= TOPK_PREFILTER_K take a two-level selection (round 3): every thread picks its own 4 largest elements in
// registers; the k-th largest of those 4096 keys (a radix selection over 4 register entries per thread) is a LOWER bound of the
// row's k-th largest key, and because the per-thread maxima are nearly the row's top 4096, only a few more than k elements pass
// it (measured on RPN logits: ~2300 for k = 2000 of 49152).  Those are compacted into LDS and the exact k-th largest is selected
// among them, again 4 entries per thread.  The radix passes therefore touch 4 entries per thread instead of 48-64, and the
// selection is the same set -- the keys are unique 64-bit (score, index) words throughout.
constexpr int TOPK_NPT = 64;
constexpr int TOPK_PREFILTER_K = 3072, TOPK_PREFILTER_CAND = 4096;
// PREF (needs NPT > 0): the two-level selection; a segment it does not settle (k >= n, or more than TOPK_PREFILTER_CAND
// survivors of the bound: adversarial ties) takes the streamed full selection, so that the cached words are dead after level 2
// (both full selections compiled into one kernel keep them live everywhere and spill).
template <int NPT, bool PREF>
__global__ void __launch_bounds__(TOPK_THREADS) topk_rows_kernel(const float* __restrict__ keys, SegP seg, long pitch,
                                                                 int estride, int k, float* __restrict__ out_val,
                                                                 int* __restrict__ out_idx) {
    __shared__ RadixShared R;
    __shared__ unsigned long long sel[TOPK_MAXK];
    __shared__ int s_count;
    const int t = threadIdx.x;
    const int rowid = (int)blockIdx.x / seg.S, sid = (int)blockIdx.x - rowid * seg.S;
    const int n = seg.n[sid];
    const float* row = keys + (long)rowid * pitch + (long)seg.off[sid] * estride;
    const int kk = k < n ? k : n;
    int kpad = 1;
    while (kpad < kk) kpad <<= 1;
    if (kpad < 2) kpad = 2;

    // element j of this thread is i = j * 1024 + t (the loops below have the same, workgroup-uniform, trip count for every thread:
    // the wave-level aggregation uses ballots / shuffles)
    unsigned ku[NPT > 0 ? NPT : 1];
    if (NPT > 0) {
        // all loads issued back to back through a buffer resource sized to the row (elements past n come back as zeros and are
        // never looked at); a guarded global load is a branch + a full wait per element, 64 serial round trips
        const omni_rsrc_t rr = omni_make_rsrc(row, n > 0 ? (unsigned)(((long)(n - 1) * estride + 1) * 4) : 0u);
        int tt = t;
        OMNI_OPAQUE_V(tt);                     // (a private copy of t per loop: see the note in the pass loop)
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
            const int i = j * TOPK_THREADS + tt;
            ku[j] = score_bits(__uint_as_float(omni_bufld1(rr, i < n ? i * estride * 4 : OMNI_OOB)));
        }
    }

    bool selected = false;                      // sel[0 .. kk) already holds the answer set (unsorted), sel[kk .. kpad) zeros
    if (PREF && kk < n && kk <= TOPK_PREFILTER_K) {
        // ---- level 1: per-thread top 4 (ties: the earlier element = lower index = larger key stays ahead) ----
        unsigned bu[4] = {0u, 0u, 0u, 0u};
        int bj[4] = {-1, -1, -1, -1};
        {
            int tt = t, nn = n;
            OMNI_OPAQUE_V(tt);
            OMNI_OPAQUE_S(nn);
#pragma unroll
            for (int j = 0; j < NPT; ++j) {
                if (j * TOPK_THREADS >= nn) break;
                if (j * TOPK_THREADS + tt < nn) {
                    unsigned cu = ku[j];
                    OMNI_OPAQUE_V(cu);          // a copy: otherwise (ku[j], j) become an aligned 64-bit pair for the swaps below
                    int cj = j;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (cj >= 0 && (bj[q] < 0 || cu > bu[q])) {
                            const unsigned su = bu[q]; const int sj = bj[q];
                            bu[q] = cu; bj[q] = cj; cu = su; cj = sj;
                        }
                    }
                }
            }
        }
        unsigned el[4];
        bool ev[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { ev[q] = bj[q] >= 0; el[q] = 0xFFFFFFFFu - (unsigned)(bj[q] * TOPK_THREADS + t); }
        const unsigned long long bound = radix_kth<4>(R, bu, el, ev, kk);      // at least kk elements of the row are >= bound
        // ---- level 2: compact everything >= bound, select among the survivors ----
        if (t == 0) s_count = 0;
        __syncthreads();
        {
            int tt = t, nn = n;
            OMNI_OPAQUE_V(tt);
            OMNI_OPAQUE_S(nn);
            const unsigned bhi = (unsigned)(bound >> 32), blo = (unsigned)bound;
#pragma unroll
            for (int j = 0; j < NPT; ++j) {
                if (j * TOPK_THREADS >= nn) break;
                const int i = j * TOPK_THREADS + tt;
                if (i < nn && key_ge(ku[j], i, bhi, blo)) {
                    const int slot = atomicAdd(&s_count, 1);
                    if (slot < TOPK_PREFILTER_CAND) store_key(sel, slot, ku[j], i);
                }
            }
        }
        __syncthreads();
        const int ncand = s_count;
        if (ncand <= TOPK_PREFILTER_CAND) {              // (otherwise: the full selection below)
            unsigned cu[4], cl[4];
            bool cv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int idx = q * TOPK_THREADS + t;
                cv[q] = idx < ncand;
                const unsigned long long key = cv[q] ? sel[idx] : 0ull;
                cu[q] = (unsigned)(key >> 32);
                cl[q] = (unsigned)key;
            }
            __syncthreads();                             // every candidate is in registers: sel can be rewritten
            if (ncand > kk) {
                const unsigned long long thr = radix_kth<4>(R, cu, cl, cv, kk);
                if (t == 0) s_count = 0;
                __syncthreads();
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const unsigned long long key = ((unsigned long long)cu[q] << 32) | cl[q];
                    if (cv[q] && key >= thr) sel[atomicAdd(&s_count, 1)] = key;
                }
            }
            for (int i = kk + t; i < kpad; i += TOPK_THREADS) sel[i] = 0ull;
            selected = true;
        }
    }

    if (!selected) {
        unsigned long long thr = 0ull;  // keys >= thr are selected
        if (kk < n) {
            if (t == 0) { R.prefix = 0ull; R.need = kk; }
            __syncthreads();
            for (int pass = 7; pass >= 0; --pass) {
                if (t < 256) R.hist[t] = 0u;
                __syncthreads();
                const unsigned long long prefix = R.prefix;
                const int shift = pass * 8;
                if (NPT > 0 && !PREF) {
                    // 32-bit arithmetic on the cached score word / the index word (a 64-bit key per element would double the
                    // registers), and the element index and the trip count are re-derived from opaque copies in every pass:
                    // otherwise the 64 index words, range predicates and loop-exit conditions are hoisted out of the pass loop
                    // as loop invariants and spill.
                    int tt = t, nn = n;
                    OMNI_OPAQUE_V(tt);
                    OMNI_OPAQUE_S(nn);
                    const unsigned phi = (unsigned)(prefix >> 32), plo = (unsigned)prefix;
                    const bool hi = pass >= 4;
                    const int sh = hi ? shift - 32 : shift;                    // shift inside the word this pass looks at
#pragma unroll
                    for (int j = 0; j < NPT; ++j) {
                        if (j * TOPK_THREADS >= nn) break;
                        const int i = j * TOPK_THREADS + tt;
                        const unsigned w = hi ? ku[j] : (0xFFFFFFFFu - (unsigned)i), pw = hi ? phi : plo;
                        // candidates: all bytes above this pass's byte equal the prefix
                        bool todo = i < nn && (hi || ku[j] == phi);
                        if (sh < 24) todo = todo && ((w >> (sh + 8)) == (pw >> (sh + 8)));
                        count_digit(R.hist, todo, (w >> sh) & 255u);
                    }
                } else {
                    // uniform trip count: the wave-level aggregation uses ballots / shuffles
                    for (int base = 0; base < n; base += TOPK_THREADS) {
                        const int i = base + t;
                        bool todo = false;
                        unsigned digit = 0u;
                        if (i < n) {
                            const unsigned long long key = make_key(row[(long)i * estride], i);
                            todo = (pass == 7) || ((key >> (shift + 8)) == (prefix >> (shift + 8)));
                            digit = (unsigned)(key >> shift) & 255u;
                        }
                        count_digit(R.hist, todo, digit);
                    }
                }
                __syncthreads();
                radix_pick_bin(R, shift);
                __syncthreads();
                if (R.done) break;
            }
            thr = R.prefix;  // keys are unique, so exactly kk keys are >= thr
        }
        if (t == 0) s_count = 0;
        for (int i = t; i < kpad; i += TOPK_THREADS) sel[i] = 0ull;
        __syncthreads();
        if (NPT > 0 && !PREF) {
            int tt = t;
            OMNI_OPAQUE_V(tt);
            const unsigned thi = (unsigned)(thr >> 32), tlo = (unsigned)thr;
#pragma unroll
            for (int j = 0; j < NPT; ++j) {
                if (j * TOPK_THREADS >= n) break;
                const int i = j * TOPK_THREADS + tt;
                if (i < n && key_ge(ku[j], i, thi, tlo)) {
                    const int slot = atomicAdd(&s_count, 1);
                    if (slot < TOPK_MAXK) store_key(sel, slot, ku[j], i);
                }
            }
        } else {
            for (int i = t; i < n; i += TOPK_THREADS) {
                const unsigned long long key = make_key(row[(long)i * estride], i);
                if (key >= thr) {
                    const int slot = atomicAdd(&s_count, 1);
                    if (slot < TOPK_MAXK) sel[slot] = key;
                }
            }
        }
    }
    __syncthreads();
    // bitonic sort, descending, kpad a power of two.  The keys are unique, so the order (ties -> lower index) is fixed by them.
    auto lds_pass = [&](int size, int stride) {      // one compare-exchange pass through LDS, ends with a barrier
        for (int i = t; i < (kpad >> 1); i += TOPK_THREADS) {
            const int lo = 2 * i - (i & (stride - 1));
            const int hi = lo + stride;
            const bool desc = ((lo & size) == 0);
            const unsigned long long a = sel[lo], b = sel[hi];
            if ((a < b) == desc) { sel[lo] = b; sel[hi] = a; }
        }
        __syncthreads();
    };
    if (kpad <= 2 * TOPK_THREADS) {
        // up to 2048 keys: thread t keeps elements 2t and 2t + 1 in registers.  Stride 1 is inside the thread, strides 2 .. 64 have
        // the partner in lane ^ (stride / 2) of the same wave (shuffles, no barrier); only strides >= 128 cross waves and go
        // through LDS: 10 of the 66 passes of a 2048-key sort.  Slots at and beyond kpad hold zeros and sort among themselves.
        const int e0 = 2 * t;
        unsigned long long a0 = e0 < kpad ? sel[e0] : 0ull, a1 = e0 + 1 < kpad ? sel[e0 + 1] : 0ull;
        for (int size = 2; size <= kpad; size <<= 1) {
            const bool desc = ((e0 & size) == 0);
            if (size >= 256) {
                if (e0 < kpad) { sel[e0] = a0; sel[e0 + 1] = a1; }
                __syncthreads();
                for (int stride = size >> 1; stride >= 128; stride >>= 1) lds_pass(size, stride);
                if (e0 < kpad) { a0 = sel[e0]; a1 = sel[e0 + 1]; }
            }
            for (int stride = (size >> 1) < 64 ? (size >> 1) : 64; stride >= 2; stride >>= 1) {
                const int lm = stride >> 1;                                  // partner lane = lane ^ lm
                const unsigned long long b0 = __shfl_xor(a0, lm, 64), b1 = __shfl_xor(a1, lm, 64);
                const bool want_max = ((t & lm) == 0) == desc;               // the lower element of a descending pair keeps the larger key
                a0 = ((a0 < b0) == want_max) ? b0 : a0;
                a1 = ((a1 < b1) == want_max) ? b1 : a1;
            }
            if ((a0 < a1) == desc) { const unsigned long long s = a0; a0 = a1; a1 = s; }
        }
        if (e0 < kpad) { sel[e0] = a0; sel[e0 + 1] = a1; }                  // (own slots: nobody else reads them before the barrier)
        __syncthreads();
    } else {
        for (int size = 2; size <= kpad; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) lds_pass(size, stride);
    }
    for (int i = t; i < k; i += TOPK_THREADS) {
        const long o = (long)blockIdx.x * k + i;
        if (i < kk) { out_val[o] = key_value(sel[i]); out_idx[o] = key_index(sel[i]); }
        else { out_val[o] = -INFINITY; out_idx[o] = -1; }
    }
}

// ---- NMS ---------------------------------------------------------------------------------------
// problem q: boxes[q*nmax .. q*nmax + count[q]) sorted by descending score; valid[] == 0 marks boxes
// that take no part (empty / non-finite).  mask: (Q, nmax, words) 64-bit, words = ceil(nmax/64).
// One 4-wave workgroup = 4 row blocks x one column block: the 64 column boxes AND their areas are staged in LDS once for the four.
// The loop over the column boxes is wave-uniform, so the column box is one broadcast 16-byte LDS read and the bit to set is a
// scalar.  The diagonal tile computes all 64 columns too and clears only a row's own bit: the bits below a row's own lane say
// which boxes AHEAD of it overlap it (the expression is symmetric in the two boxes, bit for bit: min / max, the product, the
// commutative sum ai + aj), which is what the scan's chunk resolution reads.
//
// The decision is iou = inter / (ai + aj - inter) > thr.  The division (scale, reciprocal, refinement, fix-up: 11 of the 37
// instructions of the old loop body) is only evaluated where it can matter: with u = ai + aj - inter and t = fl(thr * u) in
// [2^-100, 2^100] and thr > 0 (so u > 0, and t carries a relative error of at most 2^-24),
//     inter > fl(t * (1 + 2^-20))  =>  inter / u > thr * (1 + 2^-20)(1 - 2^-24)^2 > thr * (1 + 2^-21)  =>  fl(inter / u) > thr
//     inter < fl(t * (1 - 2^-20))  =>  inter / u < thr * (1 - 2^-20)(1 + 2^-24)^2 < thr * (1 - 2^-21)  =>  fl(inter / u) <= thr
// (thr * (1 +- 2^-21) lies more than one ulp from thr, and rounding is monotonic).  Every other pair -- the band around the threshold, u <= 0, a non-finite or NaN operand (all
// comparisons false), a non-positive thr -- evaluates the original expression, so the bits equal the plain quotient's everywhere.
constexpr float NMS_MARGIN = 9.5367431640625e-07f;          // 2^-20
constexpr unsigned NMS_T_LO = 0x0D800000u, NMS_T_HI = 0x71800000u;      // float bits of 2^-100 and 2^100
__global__ void __launch_bounds__(256) nms_mask_kernel(const float* __restrict__ boxes, const int* __restrict__ counts,
                                                       int nmax, int words, float thr,
                                                       unsigned long long* __restrict__ mask) {
    // every product and sum below rounds on its own, like the reference's: no fused multiply-add may form (ai + aj - w * h)
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.z, rb = blockIdx.y * 4 + wave, cb = blockIdx.x;
    const int n = counts ? min(max(counts[q], 0), nmax) : nmax;      // (never past the problem's slots, whatever the caller passes)
    if ((int)blockIdx.y * 4 > cb || cb * 64 >= n) return;            // (uniform) nothing above the diagonal / past the count here
    __shared__ float4 cbx[64];
    __shared__ float car[64];
    const float* B = boxes + (long)q * nmax * 4;
    if (wave == 0) {
        const int j = cb * 64 + lane;
        if (j < n) {
            const float u1 = B[j * 4 + 0], v1 = B[j * 4 + 1], u2 = B[j * 4 + 2], v2 = B[j * 4 + 3];
            cbx[lane] = make_float4(u1, v1, u2, v2);
            car[lane] = (u2 - u1) * (v2 - v1);
        }
    }
    __syncthreads();
    if (cb < rb || rb * 64 >= n) return;
    const int i = rb * 64 + lane;
    if (i >= n) return;
    const float x1 = B[i * 4 + 0], y1 = B[i * 4 + 1], x2 = B[i * 4 + 2], y2 = B[i * 4 + 3];
    const float ai = (x2 - x1) * (y2 - y1);
    const bool shortcut = thr > 0.f;                                  // (uniform)
    const float khi = 1.f + NMS_MARGIN, klo = 1.f - NMS_MARGIN;
    const int jmax = (n - cb * 64) < 64 ? (n - cb * 64) : 64;
    unsigned long long bits = 0ull;
#pragma unroll 4
    for (int jj = 0; jj < jmax; ++jj) {
        const float4 c = cbx[jj];
        const float aj = car[jj];
        const float w = fmaxf(fminf(x2, c.z) - fmaxf(x1, c.x), 0.f);
        const float h = fmaxf(fminf(y2, c.w) - fmaxf(y1, c.y), 0.f);
        const float inter = w * h;
        const float u = ai + aj - inter;
        const float t = thr * u;
        const bool ranged = shortcut & ((__float_as_uint(t) - NMS_T_LO) <= (NMS_T_HI - NMS_T_LO));
        bool over = inter > t * khi;
        const bool under = inter < t * klo;
        if (!(ranged & (over | under))) over = inter / u > thr;     // (a branch: a wave skips the division unless a lane needs it)
        if (over) bits |= (1ull << jj);
    }
    if (rb == cb) bits &= ~(1ull << lane);                            // a box does not suppress itself
    mask[((long)q * nmax + i) * words + cb] = bits;
}

// One workgroup of NMS_SCAN_WAVES waves per problem walks the rows in 64-box chunks.  Per chunk: wave 0 resolves the chunk greedily
// from the diagonal words, then every wave ORs the mask rows of the kept boxes among ITS 64 / NMS_SCAN_WAVES rows of the chunk into a
// running per-wave `removed` set that lives in registers (lane l holds words l and 64 + l: <= 128 words = 8192 boxes).  The only
// word anybody needs next is word c + 1, so each wave publishes that one word and wave 0 ORs them -- two barriers per chunk.
//  * Resolution.  Lane j knows `below` = the boxes ahead of it in the chunk that overlap it (the low bits of its own diagonal
//    word: the relation is symmetric).  The greedy keep set K is the only set with  j in K  <=>  j starts alive and no box of
//    `below` is in K  (induction over j), and iterating K <- ballot(alive_j && !(below_j & K)) from K = alive fixes one more lane
//    per round at the least, so it is reached after at most 64 rounds -- in practice after as many rounds as the longest
//    chain "a suppresses b, which would have suppressed c" is long.  A round is a ballot and a handful of scalar instructions;
//    the 64-step walk over the lanes cost two cross-lane reads per lane, whatever the boxes.
//  * Prefetch.  The mask rows, diagonal words included, of TWO chunks are in flight (register sets A and B, the chunk loop is
//    unrolled by two): the rows of chunk c + 2 are requested after the OR of chunk c and consumed two resolutions later.  They are
//    buffer loads whose offset is out of range where a guard fails, not branches around loads: every wave issues the same
//    number of loads per chunk, so the compiler can wait for "all but the youngest set" (a load in a branch forces a wait for
//    everything outstanding, which is what the single-set version did at every resolution).  All 64 rows of a chunk are fetched
//    before its resolution decides which are needed, and selected by the `alive` bits afterwards.
//  * The valid flags become one bit mask in LDS before the first chunk, and the kept bits collect in LDS and are written as keep
//    (and, for the proposal path, masked = keep ? score : -inf) after the last one: the chunk loop has no load that is consumed
//    where it is issued and no store.
// Only entries the mask kernel wrote are ever selected (row < n, word > chunk, word * 64 < n), and nothing outside the problem's
// scratch is loaded (the buffer resource ends with it; word < words, chunk < nchunks), so the scratch needs no zeroing.
constexpr int SCAN_WAVES = 16;      // waves per problem of the scan
// WIDE: more than 64 words per row (nmax > 4096), the second register word of the removed set is in use
template <int NMS_SCAN_WAVES, bool WIDE>
__global__ void __launch_bounds__(64 * NMS_SCAN_WAVES) nms_scan_kernel(const unsigned long long* __restrict__ mask,
                                                                       const int* __restrict__ counts, const int* __restrict__ valid,
                                                                       int nmax, int words, int* __restrict__ keep,
                                                                       const float* __restrict__ scores, float* __restrict__ masked) {
    constexpr int RPW = 64 / NMS_SCAN_WAVES;            // rows of a chunk per wave
    constexpr int NT = 64 * NMS_SCAN_WAVES;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = counts ? min(max(counts[q], 0), nmax) : nmax;      // (never past the problem's slots, whatever the caller passes)
    __shared__ unsigned long long s_alive;
    __shared__ unsigned long long s_next[NMS_SCAN_WAVES];
    __shared__ unsigned long long s_valid[128], s_keep[128];
    const int nchunks = (n + 63) / 64;
    const omni_rsrc_t mr = omni_make_rsrc(mask + (long)q * nmax * words, (unsigned)nmax * (unsigned)words * 8u);
    auto load64 = [&](bool ok, int word_index) -> unsigned long long {
        const int off = ok ? word_index * 8 : OMNI_OOB;                 // (word_index < nmax * words <= 2^20)
        const unsigned lo = omni_bufld1(mr, off), hi = omni_bufld1(mr, ok ? off + 4 : OMNI_OOB);
        return ((unsigned long long)hi << 32) | lo;
    };
    struct Rows { unsigned long long w0[RPW], w1[RPW], diag; };
    Rows A, B;
    auto fetch = [&](int c, Rows& R) {
        const bool live = c < nchunks;
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr) {
            const int row = c * 64 + wave * RPW + rr;
            const int w0 = lane, w1 = 64 + lane;
            R.w0[rr] = load64(live && row < n && w0 > c && w0 < words && w0 * 64 < n, row * words + w0);
            R.w1[rr] = WIDE ? load64(live && row < n && w1 > c && w1 < words && w1 * 64 < n, row * words + w1) : 0ull;
        }
        const int i = c * 64 + lane;
        R.diag = load64(wave == 0 && live && i < n, i * words + c);
    };
    fetch(0, A);
    fetch(1, B);
    {
        // valid flags -> one bit per box.  Buffer loads again, and a fixed trip count (128 chunks at the most): a load under a
        // branch here would be younger than the two fetches above and make the first resolution wait for all three.
        const omni_rsrc_t vr = omni_make_rsrc(valid ? valid + (long)q * nmax : nullptr, valid ? (unsigned)nmax * 4u : 0u);
        unsigned flag[128 / NMS_SCAN_WAVES];
#pragma unroll
        for (int j = 0; j < 128 / NMS_SCAN_WAVES; ++j) {
            const int i = (j * NMS_SCAN_WAVES + wave) * 64 + lane;
            flag[j] = omni_bufld1(vr, i < n ? i * 4 : OMNI_OOB);
        }
#pragma unroll
        for (int j = 0; j < 128 / NMS_SCAN_WAVES; ++j) {             // (whole waves: the ballot)
            const int c = j * NMS_SCAN_WAVES + wave, i = c * 64 + lane;
            const unsigned long long ok = __ballot(i < n && (valid == nullptr || flag[j] != 0u));
            if (lane == 0 && c < nchunks) s_valid[c] = ok;
        }
    }
    __syncthreads();
    unsigned long long acc0 = 0ull, acc1 = 0ull, removed_c = 0ull;
    auto step = [&](int c, Rows& R) {
        if (wave == 0) {
            // start state of this chunk: a valid box that no earlier keep removed
            const bool ok = (((s_valid[c] & ~removed_c) >> lane) & 1ull) != 0ull;
            const unsigned long long below = R.diag & ((1ull << lane) - 1ull);
            unsigned long long alive = __ballot(ok), prev;
            do {
                prev = alive;
                alive = __ballot(ok && (below & prev) == 0ull);
            } while (alive != prev);
            if (lane == 0) { s_alive = alive; s_keep[c] = alive; }
        }
        __syncthreads();
        const unsigned long long alive = s_alive;
#pragma unroll
        for (int rr = 0; rr < RPW; ++rr) {
            if ((alive >> (wave * RPW + rr)) & 1ull) { acc0 |= R.w0[rr]; acc1 |= R.w1[rr]; }
        }
        // word c + 1 of this wave's removed set sits in lane (c + 1) % 64 of acc0 (c + 1 < 64) or acc1
        const int nw = c + 1;
        const unsigned long long mine = __shfl(nw < 64 ? acc0 : acc1, nw & 63, 64);
        if (lane == 0) s_next[wave] = mine;
        fetch(c + 2, R);
        __syncthreads();
        if (wave == 0) {
            removed_c = 0ull;
#pragma unroll
            for (int k = 0; k < NMS_SCAN_WAVES; ++k) removed_c |= s_next[k];
        }
    };
    // (no branch inside the loop body: on a path around step B the loads of set A would be the youngest at the next resolution,
    // and the compiler would have to wait for everything there)
    for (int c = 0; c + 1 < nchunks; c += 2) {
        step(c, A);
        step(c + 1, B);
    }
    if (nchunks & 1) step(nchunks - 1, A);
    // every element of keep (and masked) is written; boxes beyond the count are never kept
    for (int i = tid; i < nmax; i += NT) {
        const bool kept = i < n && ((s_keep[i >> 6] >> (i & 63)) & 1ull) != 0ull;
        keep[(long)q * nmax + i] = kept ? 1 : 0;
        if (masked != nullptr) masked[(long)q * nmax + i] = kept ? scores[(long)q * nmax + i] : -INFINITY;
    }
}

inline void launch_topk(int blocks, int nmax, const float* keys, const SegP& seg, long pitch, int estride, int k, float* out_val,
                        int* out_idx, hipStream_t st) {
    if (nmax <= TOPK_NPT * TOPK_THREADS && k <= TOPK_PREFILTER_K)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(topk_rows_kernel<TOPK_NPT, true>), dim3(blocks), dim3(TOPK_THREADS), 0, st, keys, seg, pitch, estride,
                           k, out_val, out_idx);
    else if (nmax <= TOPK_NPT * TOPK_THREADS)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(topk_rows_kernel<TOPK_NPT, false>), dim3(blocks), dim3(TOPK_THREADS), 0, st, keys, seg, pitch, estride,
                           k, out_val, out_idx);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(topk_rows_kernel<0, false>), dim3(blocks), dim3(TOPK_THREADS), 0, st, keys, seg, pitch, estride, k,
                           out_val, out_idx);
}

}  // namespace

extern "C" {

// Sorted (descending, ties -> lower index) top-k of each row.  keys element (r, i) lives at
// keys[r*pitch + i*estride].  out_val/out_idx are (rows, k); slots beyond min(k, n) hold -inf / -1.
int omni_topk_rows(const float* keys, int rows, int n, long long pitch, int estride, int k, float* out_val, int* out_idx,
                   void* stream) {
    if (rows < 0 || n < 0 || k <= 0 || k > TOPK_MAXK || estride <= 0) return OMNI_ERR_ARG;
    if (rows == 0) return OMNI_OK;
    SegP seg;
    seg.S = 1;
    for (int i = 0; i < TOPK_MAXSEG; ++i) { seg.off[i] = 0; seg.n[i] = n; }
    launch_topk(rows, n, keys, seg, (long)pitch, estride, k, out_val, out_idx, (hipStream_t)stream);
    return omni_launch_status();
}

// Same, for `nseg` (<= 8) column segments of every row in ONE launch (the per-FPN-level pre-NMS top-k of
// find_top_rpn_proposals): segment s covers elements [seg_off[s], seg_off[s] + seg_n[s]) (host int arrays).
// out_val / out_idx: (rows, nseg, k); indices are relative to the segment start.
int omni_topk_segments(const float* keys, int rows, long long pitch, int estride, int nseg, const int* seg_off,
                       const int* seg_n, int k, float* out_val, int* out_idx, void* stream) {
    if (rows < 0 || nseg <= 0 || nseg > TOPK_MAXSEG || k <= 0 || k > TOPK_MAXK || estride <= 0) return OMNI_ERR_ARG;
    if (rows == 0) return OMNI_OK;
    SegP seg;
    seg.S = nseg;
    for (int i = 0; i < TOPK_MAXSEG; ++i) {
        seg.off[i] = i < nseg ? seg_off[i] : 0;
        seg.n[i] = i < nseg ? seg_n[i] : 0;
        if (seg.off[i] < 0 || seg.n[i] < 0) return OMNI_ERR_ARG;
    }
    int nmax = 0;
    for (int i = 0; i < nseg; ++i) nmax = seg.n[i] > nmax ? seg.n[i] : nmax;
    launch_topk(rows * nseg, nmax, keys, seg, (long)pitch, estride, k, out_val, out_idx, (hipStream_t)stream);
    return omni_launch_status();
}

// Greedy NMS for Q independent problems of up to nmax score-sorted boxes each ((Q, nmax, 4) XYXY).
// counts [nullable] (Q) active boxes per problem; valid [nullable] (Q, nmax) 0 = box takes no part.
// mask_ws: Q * nmax * ceil(nmax/64) 64-bit words of scratch (need not be zeroed: only entries the mask kernel writes are read).
// keep (Q, nmax) int32 out (0/1), every element written.
// scores / masked [both nullable, together] (Q, nmax): masked = keep ? scores : -inf, every element written by the scan itself
// (the input of the post-NMS top-k of the proposal path).
int omni_nms_sorted_masked(const float* boxes, const int* counts, const int* valid, int Q, int nmax, float iou_thr,
                           unsigned long long* mask_ws, int* keep, const float* scores, float* masked, void* stream) {
    if (Q < 0 || nmax < 0 || nmax > 8192 || (scores == nullptr) != (masked == nullptr)) return OMNI_ERR_ARG;
    if (Q == 0 || nmax == 0) return OMNI_OK;
    const int words = (nmax + 63) / 64;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(nms_mask_kernel, dim3(words, (words + 3) / 4, Q), dim3(256), 0, st, boxes, counts, nmax, words, iou_thr,
                       mask_ws);
    if (words > 64)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(nms_scan_kernel<SCAN_WAVES, true>), dim3(Q), dim3(64 * SCAN_WAVES), 0, st,
                           (const unsigned long long*)mask_ws, counts, valid, nmax, words, keep, scores, masked);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(nms_scan_kernel<SCAN_WAVES, false>), dim3(Q), dim3(64 * SCAN_WAVES), 0, st,
                           (const unsigned long long*)mask_ws, counts, valid, nmax, words, keep, scores, masked);
    return omni_launch_status();
}

int omni_nms_sorted(const float* boxes, const int* counts, const int* valid, int Q, int nmax, float iou_thr,
                    unsigned long long* mask_ws, int* keep, void* stream) {
    return omni_nms_sorted_masked(boxes, counts, valid, Q, nmax, iou_thr, mask_ws, keep, nullptr, nullptr, stream);
}

}  // extern "C"
