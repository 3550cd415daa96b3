// augment.hip -- the training augmentations of the input pipeline on the device: INPUT.CROP (detectron2 RandomCrop in front of
// ResizeShortestEdge) and INPUT.COLOR_JITTER (brightness / contrast / saturation).
//
// A random crop makes every (input size, output size) pair of the resampling new, so Pillow's coefficient rows (precompute_coeffs +
// normalize_coeffs_8bpc, Resample.c -- kernels/resize.py::pil_bilinear_coeffs on the host) are built here, one thread per output index,
// in double precision with the host's order of operations: bit-equal tables, no host loop and no upload per image.  The two
// resampling passes are resize.hip's arithmetic reading a WINDOW of the source through its pitch: the crop costs no pass over the
// source and no copy.  The jitter is defined in integers (12 fractional bits per weight) so that it is the same on every device and
// on the host: one read of the image for the contrast mean, one read + one write for the three steps together.
#include <device_rt.h>

// the coefficient rows must round like the host's separate multiplies and adds: no fused multiply-add anywhere in this file
#pragma clang fp contract(off)

namespace {

// ---- Pillow's bilinear coefficient rows ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double triangle(int x, int xmin, double center, double ss) {
    double t = (x + xmin - center + 0.5) * ss;
    t = t < 0 ? -t : t;
    return t < 1.0 ? 1.0 - t : 0.0;
}

// bounds (out_size, 2) = [first, count], kk (out_size, ksize) in 22-bit fixed point.  The row is evaluated twice (sum, then normalise
// and convert) instead of being kept: ksize grows with the down-scale factor and a per-thread array would live in scratch.
__global__ void __launch_bounds__(256) pil_coeffs_kernel(int in_size, int out_size, int* __restrict__ bounds, int* __restrict__ kk, int ksize) {
    const int xx = blockIdx.x * blockDim.x + threadIdx.x;
    if (xx >= out_size) return;
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * filterscale;
    const double ss = 1.0 / filterscale;
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    if (xmax > ksize) xmax = ksize;                 // never taken for a ksize the entry accepted; keeps the row inside its storage
    if (xmax < 0) xmax = 0;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += triangle(x, xmin, center, ss);
    int* k = kk + (long)xx * ksize;
    for (int x = 0; x < xmax; ++x) {
        double w = triangle(x, xmin, center, ss);
        if (ww != 0.0) w /= ww;
        const double v = w * (double)(1 << 22);
        k[x] = w < 0 ? (int)(v - 0.5) : (int)(v + 0.5);
    }
    for (int x = xmax; x < ksize; ++x) k[x] = 0;
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = xmax;
}

// ---- windowed resampling --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned char clip8(int v) {
    v >>= 22;                       // PRECISION_BITS = 32 - 8 - 2
    return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// `win` points at the window's first pixel; its rows are `pitch` bytes apart, its planes `plane` bytes.

// horizontal pass: window (P, rows, cw) -> dst (P, rows, WO) contiguous, output columns mirrored under `flip`
__global__ void __launch_bounds__(256) crop_h_kernel(const unsigned char* __restrict__ win, unsigned char* __restrict__ dst,
                                                      const int* __restrict__ bounds, const int* __restrict__ kk, int ksize, int planes,
                                                      int rows, long pitch, long plane, int WO, int flip) {
    const long total = (long)planes * rows * WO;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int xx = (int)(i % WO);
        const long row = i / WO;
        const int y = (int)(row % rows), p = (int)(row / rows);
        const int xmin = bounds[2 * xx], cnt = bounds[2 * xx + 1];
        const unsigned char* s = win + p * plane + y * pitch + xmin;
        const int* k = kk + (long)xx * ksize;
        int ss = 1 << 21;
        for (int x = 0; x < cnt; ++x) ss += (int)s[x] * k[x];
        dst[row * WO + (flip ? WO - 1 - xx : xx)] = clip8(ss);
    }
}

// vertical pass: window (P, rows of the table, WO) -> dst (P, HO, WO) contiguous
__global__ void __launch_bounds__(256) crop_v_kernel(const unsigned char* __restrict__ win, unsigned char* __restrict__ dst,
                                                      const int* __restrict__ bounds, const int* __restrict__ kk, int ksize, int planes,
                                                      long pitch, long plane, int HO, int WO) {
    const long total = (long)planes * HO * WO;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % WO);
        const long r = i / WO;
        const int yy = (int)(r % HO), p = (int)(r / HO);
        const int ymin = bounds[2 * yy], cnt = bounds[2 * yy + 1];
        const unsigned char* s = win + p * plane + ymin * pitch + x;
        const int* k = kk + (long)yy * ksize;
        int ss = 1 << 21;
        for (int y = 0; y < cnt; ++y) ss += (int)s[y * pitch] * k[y];
        dst[i] = clip8(ss);
    }
}

// identity size: window (P, rows, cols) -> dst (P, rows, cols) contiguous, copied or mirrored
__global__ void __launch_bounds__(256) crop_copy_kernel(const unsigned char* __restrict__ win, unsigned char* __restrict__ dst, int planes,
                                                         int rows, int cols, long pitch, long plane, int flip) {
    const long total = (long)planes * rows * cols;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % cols);
        const long row = i / cols;
        const int y = (int)(row % rows), p = (int)(row / rows);
        dst[i] = win[p * plane + y * pitch + (flip ? cols - 1 - x : x)];
    }
}

inline unsigned grid_for(long n) {               // resize.hip's rule
    long g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

// ---- integer colour jitter --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__device__ __forceinline__ int brighten(int v, int wb) { return clamp255((wb * v + 2048) >> 12); }
// w * 256 * v + (4096 - w) * m8, rounded: |terms| <= 16384 * 65280 + 2^19 < 2^31 for w in [0, 16384], v <= 255, m8 <= 65280
__device__ __forceinline__ int blend(int v, int m8, int w) { return clamp255((w * 256 * v + (4096 - w) * m8 + (1 << 19)) >> 20); }

constexpr int JITTER_MAX_BLOCKS = 2048;          // kernels/augment.py::JITTER_GRID_THREADS = 2048 * 256

// S = sum of the brightened values: 64-bit per thread, wave shuffle, LDS over the four waves, one 64-bit atomic per workgroup.
// Integer addition is associative: two runs give the same bits whatever the order of the atomics.
__global__ void __launch_bounds__(256) jitter_sum_kernel(const unsigned char* __restrict__ img, long n, int wb, unsigned long long* __restrict__ sum) {
    __shared__ unsigned long long part[4];
    unsigned long long acc = 0;
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x, nthr = (long)gridDim.x * blockDim.x;
    long head = (long)((4 - ((uintptr_t)img & 3)) & 3);          // bytes in front of the first aligned dword
    if (head > n) head = n;
    const long n4 = (n - head) / 4;
    const unsigned* body = reinterpret_cast<const unsigned*>(img + head);
    for (long i = gid; i < n4; i += nthr) {
        const unsigned q = body[i];
        acc += (unsigned)(brighten((int)(q & 255u), wb) + brighten((int)((q >> 8) & 255u), wb) + brighten((int)((q >> 16) & 255u), wb) +
                          brighten((int)(q >> 24), wb));
    }
    for (long i = gid; i < head; i += nthr) acc += (unsigned)brighten(img[i], wb);
    for (long i = head + 4 * n4 + gid; i < n; i += nthr) acc += (unsigned)brighten(img[i], wb);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(sum, part[0] + part[1] + part[2] + part[3]);
}

// the three steps on one pixel held in registers; planes are `hw` bytes apart, red is plane c_red, green plane 1
__global__ void __launch_bounds__(256) jitter_apply_kernel(unsigned char* __restrict__ img, long hw, int wb, int wc, int ws, int c_red,
                                                            const unsigned long long* __restrict__ sum) {
    int m8 = 0;                                   // wc == 4096: its factor is 0 and the sum was never taken
    if (wc != 4096) {
        const unsigned long long n = 3ull * (unsigned long long)hw;
        m8 = (int)((256ull * *sum + n / 2) / n);
    }
    unsigned char* pr = img + c_red * hw;
    unsigned char* pg = img + hw;
    unsigned char* pb = img + (2 - c_red) * hw;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += (long)gridDim.x * blockDim.x) {
        int r = blend(brighten(pr[i], wb), m8, wc), g = blend(brighten(pg[i], wb), m8, wc), b = blend(brighten(pb[i], wb), m8, wc);
        const int g8 = 77 * r + 150 * g + 29 * b;
        pr[i] = (unsigned char)blend(r, g8, ws);
        pg[i] = (unsigned char)blend(g, g8, ws);
        pb[i] = (unsigned char)blend(b, g8, ws);
    }
}

inline unsigned jitter_grid(long n) {
    long g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > JITTER_MAX_BLOCKS ? JITTER_MAX_BLOCKS : g));
}

}  // namespace

extern "C" {

int omni_pil_bilinear_coeffs(int in_size, int out_size, int* bounds, int* kk, int ksize, void* stream) {
    if (in_size <= 0 || out_size <= 0 || !bounds || !kk) return OMNI_ERR_ARG;
    const double scale = (double)in_size / (double)out_size;
    if (ksize != 2 * (int)ceil(scale < 1.0 ? 1.0 : scale) + 1) return OMNI_ERR_ARG;
    hipLaunchKernelGGL(pil_coeffs_kernel, dim3((unsigned)((out_size + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in_size, out_size,
                       bounds, kk, ksize);
    return omni_launch_status();
}

int omni_crop_resize_u8(const unsigned char* src, unsigned char* dst, unsigned char* tmp, int planes, int H, int W, int x0, int y0, int ch,
                        int cw, int HO, int WO, const int* bounds_h, const int* kk_h, int ksize_h, const int* bounds_v, const int* kk_v,
                        int ksize_v, int flip, void* stream) {
    if (!src || !dst || planes <= 0 || H <= 0 || W <= 0 || ch <= 0 || cw <= 0 || HO <= 0 || WO <= 0) return OMNI_ERR_ARG;
    if (x0 < 0 || y0 < 0 || x0 > W - cw || y0 > H - ch) return OMNI_ERR_ARG;
    const bool need_h = cw != WO, need_v = ch != HO;
    if ((need_h && (!bounds_h || !kk_h || ksize_h <= 0)) || (need_v && (!bounds_v || !kk_v || ksize_v <= 0))) return OMNI_ERR_ARG;
    if (need_v && (need_h || flip) && !tmp) return OMNI_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const unsigned char* win = src + (long)y0 * W + x0;
    long pitch = W, plane = (long)H * W;
    if (need_h || flip || !need_v) {              // first pass, into tmp when a vertical pass follows
        unsigned char* out = need_v ? tmp : dst;
        if (need_h)
            hipLaunchKernelGGL(crop_h_kernel, dim3(grid_for((long)planes * ch * WO)), dim3(256), 0, st, win, out, bounds_h, kk_h, ksize_h,
                               planes, ch, pitch, plane, WO, flip);
        else
            hipLaunchKernelGGL(crop_copy_kernel, dim3(grid_for((long)planes * ch * cw)), dim3(256), 0, st, win, out, planes, ch, cw, pitch,
                               plane, flip);
        win = out, pitch = WO, plane = (long)ch * WO;
    }
    if (need_v)
        hipLaunchKernelGGL(crop_v_kernel, dim3(grid_for((long)planes * HO * WO)), dim3(256), 0, st, win, dst, bounds_v, kk_v, ksize_v, planes,
                           pitch, plane, HO, WO);
    return omni_launch_status();
}

int omni_color_jitter_u8(unsigned char* img, int H, int W, int wb, int wc, int ws, int c_red, unsigned long long* sum, void* stream) {
    if (!img || !sum || H <= 0 || W <= 0 || (c_red != 0 && c_red != 2)) return OMNI_ERR_ARG;
    if (wb < 0 || wb > 16384 || wc < 0 || wc > 16384 || ws < 0 || ws > 16384) return OMNI_ERR_ARG;
    if (wb == 4096 && wc == 4096 && ws == 4096) return OMNI_OK;
    hipStream_t st = (hipStream_t)stream;
    const long hw = (long)H * W;
    if (wc != 4096) {
        omni_memset_async(sum, 0, sizeof(unsigned long long), st);
        hipLaunchKernelGGL(jitter_sum_kernel, dim3(jitter_grid((3 * hw + 3) / 4)), dim3(256), 0, st, img, 3 * hw, wb, sum);
    }
    hipLaunchKernelGGL(jitter_apply_kernel, dim3(jitter_grid(hw)), dim3(256), 0, st, img, hw, wb, wc, ws, c_red, sum);
    return omni_launch_status();
}

}  // extern "C"
