// render.hip -- drawing predicted cuboids on the device: the reference renders them with pytorch3d's mesh rasteriser (hard
// rasterisation, faces_per_pixel = 1; cubercnn/util/math_util.py:707-743 `render_depth_map` / `estimate_visibility`,
// cubercnn/vis/vis.py:262-383 `draw_scene_view`) and paints the box edges with OpenCV (`cv2.line`, vis.py:593-626).
//
// A cuboid needs no triangle rasteriser: the ray through a pixel is clipped against the three slabs of the box in the box
// frame, which gives the entry and the exit point, the face each of them lies on and the camera depth of both in a dozen
// flops.  Three kernels, all pixel-parallel gathers (one 256-thread workgroup per 16 x 16 pixel tile, boxes / segments staged
// through LDS in chunks of 64 and culled per tile by their bounding rectangle):
//   cuboid_depth_kernel   nearest hit per pixel (depth, box, face) + per-box pixel counts (integer atomics only)
//   scene_compose_kernel  ambient + diffuse shading of the hit face under a point light at the camera, blended onto the image
//   draw_segments_kernel  thick line segments: every pixel takes the last segment whose capsule holds its centre
// Conventions (stated departures from pytorch3d / OpenCV): the sample point of pixel (x, y) is (x + 0.5, y + 0.5); depth is the
// camera-space z of the true ray / surface intersection (the reference interpolates z in screen space, perspective_correct =
// False); segment end points are kept at sub-pixel precision.
#include <device_rt.h>
#include "cuboid_cast.h"      // TILE, CHUNK, REC, pixel_ray, clamp_to_int, slab, stage_box, cast_box

namespace {

// face number (get_cuboid_verts_faces: 0 front -w/2, 1 right +l/2, 2 left -l/2, 3 back +w/2, 4 top -h/2, 5 bottom +h/2) of
// the side of box-frame axis `axis` (0: length, 1: height, 2: width) at the negative / positive end
__device__ __forceinline__ int face_of(int axis, bool positive) {
    return axis == 0 ? (positive ? 1 : 2) : (axis == 1 ? (positive ? 5 : 4) : (positive ? 3 : 0));
}

__global__ void __launch_bounds__(256) cuboid_depth_kernel(const float* __restrict__ box3d, const float* __restrict__ R,
                                                            const float* __restrict__ K, int N, int H, int W, float zplane,
                                                            float* __restrict__ depth, int* __restrict__ index,
                                                            int* __restrict__ face, int* __restrict__ area, int* __restrict__ visible) {
    __shared__ float s_rec[CHUNK * REC];
    __shared__ int s_on[CHUNK];       // the box's rectangle meets this tile
    __shared__ int s_cnt[CHUNK];      // pixels of this tile per box of the chunk
    const int t = threadIdx.x, lane = t & 63;
    const int tx0 = blockIdx.x * TILE, ty0 = blockIdx.y * TILE;
    const int tx1 = min(tx0 + TILE, W) - 1, ty1 = min(ty0 + TILE, H) - 1;
    const int x = tx0 + (t & 15), y = ty0 + (t >> 4);
    const bool inside = x < W && y < H;
    float dx, dy;
    pixel_ray(K, x, y, dx, dy);
    const float inf = __int_as_float(0x7f800000);
    float best = inf;
    int bi = -1, bf = -1;
    for (int c0 = 0; c0 < N; c0 += CHUNK) {
        const int n = min(CHUNK, N - c0);
        if (t < CHUNK) {
            s_cnt[t] = 0;
            s_on[t] = t < n ? stage_box(box3d + 6L * (c0 + t), R + 9L * (c0 + t), K, zplane, W, H, tx0, ty0, tx1, ty1, s_rec + t * REC) : 0;
        }
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            if (!s_on[j]) continue;                  // the same decision in every thread of the workgroup
            // first surface point at or behind the near plane: the entry, or the exit when the entry lies in front of the plane
            float th, la;
            int ax;
            bool entry;
            const bool hit = cast_box(s_rec + j * REC, dx, dy, zplane, th, ax, la, entry) && inside;
            const unsigned long long m = __ballot(hit);
            if (lane == 0 && m) atomicAdd(&s_cnt[j], (int)__popcll(m));
            if (hit && th < best) {                  // boxes come in index order: equal depths stay with the lower index
                best = th;
                bi = c0 + j;
                bf = face_of(ax, (la > 0.0f) != entry);
            }
        }
        __syncthreads();
        if (t < n && s_cnt[t] > 0) atomicAdd(&area[c0 + t], s_cnt[t]);
    }
    if (inside) {
        const long i = (long)y * W + x;
        depth[i] = best;
        index[i] = bi;
        face[i] = bf;
    }
    // pixels won per box: LDS counters per chunk, then one integer atomic per box and tile
    for (int c0 = 0; c0 < N; c0 += CHUNK) {
        if (t < CHUNK) s_cnt[t] = 0;
        __syncthreads();
        if (inside && bi >= c0 && bi < c0 + CHUNK) atomicAdd(&s_cnt[bi - c0], 1);
        __syncthreads();
        if (t < CHUNK && c0 + t < N && s_cnt[t] > 0) atomicAdd(&visible[c0 + t], s_cnt[t]);
    }
}

__device__ __forceinline__ unsigned char round_u8(float v) {
    return (unsigned char)fminf(fmaxf(floorf(v + 0.5f), 0.0f), 255.0f);
}

// Ambient 0.5 + diffuse 0.3 * max(0, n . l) of pytorch3d's PointLights defaults under SoftPhongShader, light at the camera
// origin; the specular term (0.2 * (r . v)^64) is left out.  n: outward normal of the hit face, turned towards the camera when
// the face is seen from inside (exit hit); l: unit vector from the hit point to the light = -d / |d|.
__global__ void __launch_bounds__(256) scene_compose_kernel(const int* __restrict__ index, const int* __restrict__ face,
                                                             const float* __restrict__ R, const float* __restrict__ K,
                                                             const float* __restrict__ color, int N, int H, int W, float blend,
                                                             unsigned char* __restrict__ image) {
    const long plane = (long)H * W;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < plane; i += (long)gridDim.x * blockDim.x) {
        const int b = index[i];
        if (b < 0 || b >= N) continue;
        const int f = face[i];
        const int axis = (f == 1 || f == 2) ? 0 : ((f == 4 || f == 5) ? 1 : 2);
        const float sgn = (f == 1 || f == 3 || f == 5) ? 1.0f : -1.0f;
        const float* r = R + 9L * b;
        float nx = sgn * r[axis], ny = sgn * r[3 + axis], nz = sgn * r[6 + axis];
        float dx, dy;
        pixel_ray(K, (int)(i % W), (int)(i / W), dx, dy);
        if (nx * dx + ny * dy + nz > 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
        const float nl = -(nx * dx + ny * dy + nz) / sqrtf(dx * dx + dy * dy + 1.0f);
        const float shade = 0.5f + 0.3f * fmaxf(nl, 0.0f);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float s = fminf(color[3L * b + c] * 255.0f * shade, 255.0f);
            image[c * plane + i] = round_u8(s * blend + (float)image[c * plane + i] * (1.0f - blend));
        }
    }
}

__global__ void __launch_bounds__(256) draw_segments_kernel(const float* __restrict__ seg, int S, unsigned char* __restrict__ image,
                                                             int H, int W) {
    __shared__ float s_seg[CHUNK * 8];
    __shared__ int s_on[CHUNK];
    const int t = threadIdx.x;
    const int tx0 = blockIdx.x * TILE, ty0 = blockIdx.y * TILE;
    const int x = tx0 + (t & 15), y = ty0 + (t >> 4);
    const float px = (float)x + 0.5f, py = (float)y + 0.5f;
    int last = -1;
    for (int c0 = 0; c0 < S; c0 += CHUNK) {
        const int n = min(CHUNK, S - c0);
        if (t < CHUNK) {
            int on = 0;
            if (t < n) {
                const float* g = seg + 8L * (c0 + t);
                float* d = s_seg + 8 * t;
#pragma unroll
                for (int k = 0; k < 8; ++k) d[k] = g[k];
                const float rad = 0.5f * g[4];
                // capsule rectangle against the pixel centres of the tile; written so that a NaN anywhere drops the segment
                on = fminf(g[0], g[2]) - rad <= (float)(tx0 + TILE) && fmaxf(g[0], g[2]) + rad >= (float)tx0 &&
                     fminf(g[1], g[3]) - rad <= (float)(ty0 + TILE) && fmaxf(g[1], g[3]) + rad >= (float)ty0 && rad >= 0.0f;
            }
            s_on[t] = on;
        }
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            if (!s_on[j]) continue;
            const float* g = s_seg + 8 * j;
            const float ex = g[2] - g[0], ey = g[3] - g[1], qx = px - g[0], qy = py - g[1];
            const float len2 = ex * ex + ey * ey;
            const float u = len2 > 0.0f ? fminf(fmaxf((qx * ex + qy * ey) / len2, 0.0f), 1.0f) : 0.0f;
            const float fx = qx - u * ex, fy = qy - u * ey, rad = 0.5f * g[4];
            if (fx * fx + fy * fy <= rad * rad) last = c0 + j;
        }
        __syncthreads();
    }
    if (last >= 0 && x < W && y < H) {
        const long plane = (long)H * W, i = (long)y * W + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) image[c * plane + i] = round_u8(seg[8L * last + 5 + c]);
    }
}

inline unsigned grid_for(long n) {
    long g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

}  // namespace

extern "C" {

int omni_cuboid_depth(const float* box3d, const float* R, const float* K, int N, int H, int W, float zplane, float* depth,
                      int* index, int* face, int* area, int* visible, void* stream) {
    if (N < 0 || H <= 0 || W <= 0 || !(zplane > 0.0f)) return OMNI_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (N > 0) {
        omni_memset_async(area, 0, sizeof(int) * (size_t)N, st);
        omni_memset_async(visible, 0, sizeof(int) * (size_t)N, st);
    }
    hipLaunchKernelGGL(cuboid_depth_kernel, dim3((W + TILE - 1) / TILE, (H + TILE - 1) / TILE), dim3(256), 0, st, box3d, R, K, N, H,
                       W, zplane, depth, index, face, area, visible);
    return omni_launch_status();
}

int omni_scene_compose(const int* index, const int* face, const float* R, const float* K, const float* color, int N, int H, int W,
                       float blend_weight, unsigned char* image, void* stream) {
    if (N < 0 || H <= 0 || W <= 0 || !(blend_weight >= 0.0f && blend_weight <= 1.0f)) return OMNI_ERR_ARG;
    if (N == 0) return OMNI_OK;
    hipLaunchKernelGGL(scene_compose_kernel, dim3(grid_for((long)H * W)), dim3(256), 0, (hipStream_t)stream, index, face, R, K, color,
                       N, H, W, blend_weight, image);
    return omni_launch_status();
}

int omni_draw_segments(const float* seg, int S, unsigned char* image, int H, int W, void* stream) {
    if (S < 0 || H <= 0 || W <= 0) return OMNI_ERR_ARG;
    if (S == 0) return OMNI_OK;
    hipLaunchKernelGGL(draw_segments_kernel, dim3((W + TILE - 1) / TILE, (H + TILE - 1) / TILE), dim3(256), 0, (hipStream_t)stream,
                       seg, S, image, H, W);
    return omni_launch_status();
}

}  // extern "C"
