// warp.hip -- INPUT.CAMERA_ROTATION on the device: a projective warp of a uint8 image.  A rotation Q of the camera about its optical centre
// moves every pixel by the homography K Q K^-1; the mapper hands the inverse map (output pixel -> source pixel) to this file, which
// samples the source bilinearly.  The definition (include/omni3d_hip.h) is ONE double-precision projective map per pixel, each
// product and sum rounded on its own, followed by integers only: 8 fractional bits per blend weight, one rounding at the end.  The host
// (`warp_homography_u8_host`) and every device therefore give the same bytes.  The nine doubles and the fill bytes travel in the kernel
// arguments: no table, no upload.  One thread owns a pixel, computes its map once and writes every plane; the gathers are byte loads,
// which neighbouring lanes issue to neighbouring bytes at the small angles this is used at.
#include <device_rt.h>

#include <math.h>

// every product and sum of the map is rounded on its own, on the host and on the device: no fused multiply-add anywhere in this file
#pragma clang fp contract(off)

namespace {

constexpr int WARP_MAX_PLANES = 4;
constexpr int WARP_MAX_BLOCKS = 2048;            // kernels/augment.py::WARP_GRID_THREADS = 2048 * 256

struct WarpMap {
    double m[9];                                 // row-major: output pixel -> source pixel
    unsigned char fill[WARP_MAX_PLANES];
};

__global__ void __launch_bounds__(256) warp_homography_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int planes,
                                                               int H, int W, int HO, int WO, WarpMap wm) {
    const long total = (long)HO * WO, plane_in = (long)H * W;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int j = (int)(idx % WO), i = (int)(idx / WO);
        const double xd = j + 0.5, yd = i + 0.5;
        const double X = (wm.m[0] * xd + wm.m[1] * yd) + wm.m[2];
        const double Y = (wm.m[3] * xd + wm.m[4] * yd) + wm.m[5];
        const double D = (wm.m[6] * xd + wm.m[7] * yd) + wm.m[8];
        const double r = 1.0 / D;
        const double u = X * r, v = Y * r;
        if (!(u >= 0.0 && u <= (double)W && v >= 0.0 && v <= (double)H)) {      // outside the source, or NaN
            for (int p = 0; p < planes; ++p) dst[p * total + idx] = wm.fill[p];
            continue;
        }
        const double su = u - 0.5, sv = v - 0.5;
        const double fx = floor(su), fy = floor(sv);
        const int a = (int)((su - fx) * 256.0 + 0.5), b = (int)((sv - fy) * 256.0 + 0.5);      // both in [0, 256]
        int x0 = (int)fx, y0 = (int)fy;          // in [-1, W - 1] and [-1, H - 1]
        int x1 = x0 + 1, y1 = y0 + 1;
        x0 = x0 < 0 ? 0 : x0, y0 = y0 < 0 ? 0 : y0;                  // edge replication
        x1 = x1 > W - 1 ? W - 1 : x1, y1 = y1 > H - 1 ? H - 1 : y1;
        const long o00 = (long)y0 * W + x0, o01 = (long)y0 * W + x1, o10 = (long)y1 * W + x0, o11 = (long)y1 * W + x1;
        for (int p = 0; p < planes; ++p) {
            const unsigned char* s = src + p * plane_in;
            const int top = (int)s[o00] * (256 - a) + (int)s[o01] * a;
            const int bot = (int)s[o10] * (256 - a) + (int)s[o11] * a;
            dst[p * total + idx] = (unsigned char)((top * (256 - b) + bot * b + 32768) >> 16);     // <= 255 * 65536 + 32768 < 2^31
        }
    }
}

inline unsigned warp_grid(long n) {
    long g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > WARP_MAX_BLOCKS ? WARP_MAX_BLOCKS : g));
}

}  // namespace

extern "C" {

int omni_warp_homography_u8(const unsigned char* src, unsigned char* dst, int planes, int H, int W, int HO, int WO, const double* m,
                            const unsigned char* fill, void* stream) {
    if (!src || !dst || !m || !fill) return OMNI_ERR_ARG;
    if (planes <= 0 || planes > WARP_MAX_PLANES || H <= 0 || W <= 0 || HO <= 0 || WO <= 0) return OMNI_ERR_ARG;
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + (uintptr_t)planes * H * W, d0 = (uintptr_t)dst, d1 = d0 + (uintptr_t)planes * HO * WO;
    if (s0 < d1 && d0 < s1) return OMNI_ERR_ARG;
    WarpMap wm;
    for (int k = 0; k < 9; ++k) {
        if (!isfinite(m[k])) return OMNI_ERR_ARG;
        wm.m[k] = m[k];
    }
    // the denominator is affine in the pixel: positive at the four corners of the output rectangle, positive all over it
    const double cx[2] = {0.0, (double)WO}, cy[2] = {0.0, (double)HO};
    for (int c = 0; c < 4; ++c) {
        const double D = (m[6] * cx[c & 1] + m[7] * cy[c >> 1]) + m[8];
        if (!(D > 0.0)) return OMNI_ERR_ARG;
    }
    for (int p = 0; p < WARP_MAX_PLANES; ++p) wm.fill[p] = p < planes ? fill[p] : 0;
    hipLaunchKernelGGL(warp_homography_kernel, dim3(warp_grid((long)HO * WO)), dim3(256), 0, (hipStream_t)stream, src, dst, planes, H, W, HO, WO,
                       wm);
    return omni_launch_status();
}

}  // extern "C"
