// shapes.hip -- the two drawing primitives the segment kernel of render.hip cannot express: area fills blended in list order
// (`draw_transparent_polygon`, `cv2.circle`, `draw_transparent_square`; cubercnn/vis/vis.py:540-568, 684-703) and the ground
// plane of the novel view (vis.py:389-490).  Both follow omni_draw_segments: one 256-thread workgroup per 16 x 16 pixel tile,
// every pixel gathers what covers it (no scatter, no atomics, so two runs give the same bits), the sample point of pixel (x, y)
// is (x + 0.5, y + 0.5).
//   fill_shapes_kernel  rows staged through LDS in chunks of 64, culled per tile by their bounding rectangle; a pixel walks the
//                       list in order and blends every covering shape onto its own three bytes, held in registers
//   ground_grid_kernel  the pixel ray is cast onto the plane y = y0 of the scene; the pixel is inked when it lies within half a
//                       line width of the image of one of the two grid lines of each family next to the point hit.  The image
//                       of a grid line is the cross product of a projected point of it and its projected direction; thread 0
//                       works these out in double and hands them to the workgroup through LDS.
#include <device_rt.h>
#include "cuboid_cast.h"      // TILE, CHUNK, pixel_ray

namespace {

constexpr int SHP = 13;        // floats per shape row
constexpr int GPAR = 24;       // floats of the ground grid's per-launch constants

__device__ __forceinline__ bool is_finite(float v) { return fabsf(v) < __int_as_float(0x7f800000); }      // false for a NaN

// the edge a -> b crosses the half line from p towards +x: half-open in y, the side taken from the edge function (no division)
__device__ __forceinline__ bool crosses(float ax, float ay, float bx, float by, float px, float py) {
    const float e = (bx - ax) * (py - ay) - (by - ay) * (px - ax);
    return ay <= py ? (by > py && e > 0.0f) : (by <= py && e < 0.0f);
}

// floor(v * blend + (1 - blend) * c) in double with one rounding per operation: numpy's float64 expression stored into uint8
__device__ __forceinline__ unsigned char blend_u8(unsigned char v, double blend, double c) {
#pragma clang fp contract(off)
    const double r = floor((double)v * blend + (1.0 - blend) * c);
    return (unsigned char)fmin(fmax(r, 0.0), 255.0);
}

__global__ void __launch_bounds__(256) fill_shapes_kernel(const float* __restrict__ shape, int S, unsigned char* __restrict__ image,
                                                           int H, int W) {
    __shared__ float s_shape[CHUNK * SHP];
    __shared__ int s_on[CHUNK];
    const int t = threadIdx.x;
    const int tx0 = blockIdx.x * TILE, ty0 = blockIdx.y * TILE;
    const int x = tx0 + (t & 15), y = ty0 + (t >> 4);
    const float px = (float)x + 0.5f, py = (float)y + 0.5f;
    const bool inside = x < W && y < H;
    const long plane = (long)H * W, i = (long)y * W + x;
    unsigned char v0 = 0, v1 = 0, v2 = 0;
    if (inside) { v0 = image[i]; v1 = image[plane + i]; v2 = image[2 * plane + i]; }
    bool touched = false;
    for (int c0 = 0; c0 < S; c0 += CHUNK) {
        const int n = min(CHUNK, S - c0);
        if (t < CHUNK) {
            int on = 0;
            if (t < n) {
                const float* g = shape + (long)SHP * (c0 + t);
                float* d = s_shape + SHP * t;
                bool ok = true;
#pragma unroll
                for (int k = 0; k < SHP; ++k) { d[k] = g[k]; ok = ok && is_finite(g[k]); }
                float x0, x1, y0, y1;
                if (g[0] == 0.0f) {
                    x0 = fminf(fminf(g[1], g[3]), fminf(g[5], g[7])); x1 = fmaxf(fmaxf(g[1], g[3]), fmaxf(g[5], g[7]));
                    y0 = fminf(fminf(g[2], g[4]), fminf(g[6], g[8])); y1 = fmaxf(fmaxf(g[2], g[4]), fmaxf(g[6], g[8]));
                } else {
                    x0 = g[1] - g[3]; x1 = g[1] + g[3]; y0 = g[2] - g[3]; y1 = g[2] + g[3];
                    ok = ok && g[0] == 1.0f && g[3] >= 0.0f;                 // an unknown kind or a negative radius covers nothing
                }
                // bounding rectangle against the pixel centres of the tile
                on = ok && x0 <= (float)(tx0 + TILE) && x1 >= (float)tx0 && y0 <= (float)(ty0 + TILE) && y1 >= (float)ty0;
            }
            s_on[t] = on;
        }
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            if (!s_on[j]) continue;                  // the same decision in every thread of the workgroup
            const float* g = s_shape + SHP * j;
            bool in;
            if (g[0] == 0.0f) {                      // even-odd: an odd number of edges crossed on the way to +x
                in = crosses(g[1], g[2], g[3], g[4], px, py) != crosses(g[3], g[4], g[5], g[6], px, py);
                in = in != crosses(g[5], g[6], g[7], g[8], px, py);
                in = in != crosses(g[7], g[8], g[1], g[2], px, py);
            } else {
                const float qx = px - g[1], qy = py - g[2], d2 = qx * qx + qy * qy, ri = fmaxf(g[4], 0.0f);
                in = d2 <= g[3] * g[3] && d2 >= ri * ri;
            }
            if (in) {
                const double blend = (double)g[9];
                v0 = blend_u8(v0, blend, (double)g[10]);
                v1 = blend_u8(v1, blend, (double)g[11]);
                v2 = blend_u8(v2, blend, (double)g[12]);
                touched = true;
            }
        }
        __syncthreads();
    }
    if (touched && inside) { image[i] = v0; image[plane + i] = v1; image[2 * plane + i] = v2; }
}

__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// K v for the upper triangular K of pixel_ray
__device__ __forceinline__ void project3(const float* __restrict__ K, const double* v, double* o) {
    o[0] = (double)K[0] * v[0] + (double)K[1] * v[1] + (double)K[2] * v[2];
    o[1] = (double)K[4] * v[1] + (double)K[5] * v[2];
    o[2] = v[2];
}

// the pixel centre lies within `half` pixels of the image line u + k v (homogeneous): (l . q)^2 <= half^2 (l_x^2 + l_y^2)
__device__ __forceinline__ bool on_line(const float* u, const float* v, float sign, float k, float px, float py, float half) {
    const float lx = u[0] + sign * k * v[0], ly = u[1] + sign * k * v[1], lz = u[2] + sign * k * v[2];
    const float d = lx * px + ly * py + lz;
    return d * d <= half * half * (lx * lx + ly * ly);
}

__global__ void __launch_bounds__(256) ground_grid_kernel(unsigned char* __restrict__ image, const int* __restrict__ index,
                                                           const float* __restrict__ K, const float* __restrict__ A,
                                                           const float* __restrict__ tr, float y0, int x_start, int x_end, int z_start,
                                                           int z_end, float near, float half, int bg, int fg, int H, int W) {
    // a0, a1, a2: the columns of A (the scene axes in view space); c = y0 + a1 . t; a0 . t, a2 . t; u, v, u2: the image of the line
    // X = k is u + k v, that of Z = k is u2 - k v
    __shared__ float s_p[GPAR];
    if (threadIdx.x == 0) {
        double a0[3], a1[3], a2[3], c0[3], ka0[3], ka2[3], kc0[3], u[3], v[3], u2[3];
        double a0t = 0.0, a1t = 0.0, a2t = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            a0[r] = (double)A[3 * r]; a1[r] = (double)A[3 * r + 1]; a2[r] = (double)A[3 * r + 2];
            a0t += a0[r] * (double)tr[r]; a1t += a1[r] * (double)tr[r]; a2t += a2[r] * (double)tr[r];
            c0[r] = (double)y0 * a1[r] + (double)tr[r];              // the view-space image of the scene point (0, y0, 0)
        }
        project3(K, a0, ka0);
        project3(K, a2, ka2);
        project3(K, c0, kc0);
        cross3(kc0, ka2, u);
        cross3(ka0, ka2, v);
        cross3(kc0, ka0, u2);
        double big = 0.0;                                            // one common scale keeps the squares far from overflow
#pragma unroll
        for (int r = 0; r < 3; ++r) big = fmax(big, fmax(fabs(u[r]), fmax(fabs(v[r]), fabs(u2[r]))));
        const double sc = big > 0.0 ? 1.0 / big : 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            s_p[r] = (float)a0[r]; s_p[3 + r] = (float)a1[r]; s_p[6 + r] = (float)a2[r];
            s_p[12 + r] = (float)(u[r] * sc); s_p[15 + r] = (float)(v[r] * sc); s_p[18 + r] = (float)(u2[r] * sc);
        }
        s_p[9] = (float)((double)y0 + a1t); s_p[10] = (float)a0t; s_p[11] = (float)a2t;
    }
    __syncthreads();
    const int t = threadIdx.x;
    const int x = blockIdx.x * TILE + (t & 15), y = blockIdx.y * TILE + (t >> 4);
    if (x >= W || y >= H) return;
    const long plane = (long)H * W, i = (long)y * W + x;
    if (index != nullptr && index[i] >= 0) return;                   // a box covers the pixel: its bytes stay
    const float px = (float)x + 0.5f, py = (float)y + 0.5f;
    float dx, dy;
    pixel_ray(K, x, y, dx, dy);
    bool ink = false;
    // the depth s of the plane along the ray (d_z = 1): a1 . (s d - t) = y0.  Behind the camera (above the horizon), parallel
    // (s infinite: X, Z below are not numbers and fail every comparison) or in front of `near`: background.
    const float s = s_p[9] / (s_p[3] * dx + s_p[4] * dy + s_p[5]);
    if (s > 0.0f && s >= near && x_end - x_start >= 2 && z_end - z_start >= 2) {
        const float X = s * (s_p[0] * dx + s_p[1] * dy + s_p[2]) - s_p[10];
        const float Z = s * (s_p[6] * dx + s_p[7] * dy + s_p[8]) - s_p[11];
        if (X >= (float)x_start && X <= (float)(x_end - 1) && Z >= (float)z_start && Z <= (float)(z_end - 1)) {
            // the drawn lines next to the point: k = floor and floor + 1, where k <= end - 2
            const int kx = (int)floorf(X), kz = (int)floorf(Z);
            ink = (kx <= x_end - 2 && on_line(s_p + 12, s_p + 15, 1.0f, (float)kx, px, py, half)) ||
                  (kx + 1 <= x_end - 2 && on_line(s_p + 12, s_p + 15, 1.0f, (float)(kx + 1), px, py, half)) ||
                  (kz <= z_end - 2 && on_line(s_p + 18, s_p + 15, -1.0f, (float)kz, px, py, half)) ||
                  (kz + 1 <= z_end - 2 && on_line(s_p + 18, s_p + 15, -1.0f, (float)(kz + 1), px, py, half));
        }
    }
    const int c = ink ? fg : bg;
    image[i] = (unsigned char)((c >> 16) & 255);
    image[plane + i] = (unsigned char)((c >> 8) & 255);
    image[2 * plane + i] = (unsigned char)(c & 255);
}

}  // namespace

extern "C" {

int omni_fill_shapes(const float* shape, int S, unsigned char* image, int H, int W, void* stream) {
    if (S < 0 || H <= 0 || W <= 0) return OMNI_ERR_ARG;
    if (S == 0) return OMNI_OK;
    hipLaunchKernelGGL(fill_shapes_kernel, dim3((W + TILE - 1) / TILE, (H + TILE - 1) / TILE), dim3(256), 0, (hipStream_t)stream,
                       shape, S, image, H, W);
    return omni_launch_status();
}

int omni_ground_grid(unsigned char* image, const int* index, const float* K, const float* A, const float* t, float y0, int x_start,
                     int x_end, int z_start, int z_end, float near, float thickness, int bg_rgb, int line_rgb, int H, int W,
                     void* stream) {
    if (H <= 0 || W <= 0 || !(near > 0.0f) || !(thickness >= 0.0f) || (bg_rgb >> 24) != 0 || (line_rgb >> 24) != 0) return OMNI_ERR_ARG;
    // whole numbers up to 2^24 are exact in the kernel's float arithmetic
    if (x_start < -(1 << 24) || x_end > (1 << 24) || z_start < -(1 << 24) || z_end > (1 << 24)) return OMNI_ERR_ARG;
    hipLaunchKernelGGL(ground_grid_kernel, dim3((W + TILE - 1) / TILE, (H + TILE - 1) / TILE), dim3(256), 0, (hipStream_t)stream,
                       image, index, K, A, t, y0, x_start, x_end, z_start, z_end, near, 0.5f * thickness, bg_rgb, line_rgb, H, W);
    return omni_launch_status();
}

}  // extern "C"
