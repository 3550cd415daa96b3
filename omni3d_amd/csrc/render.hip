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

namespace {

constexpr int TILE = 16;       // pixels per tile edge: 256 threads = 4 waves of 4 rows x 16 columns
constexpr int CHUNK = 64;      // boxes / segments staged in LDS at a time
constexpr int REC = 16;        // floats per box record: R^T (9), ray origin in the box frame (3), half extents (3), pad

// direction (dx, dy, 1) of the ray through the centre of pixel (x, y): K (dx, dy, 1)^T = (x + 0.5, y + 0.5, 1)^T
__device__ __forceinline__ void pixel_ray(const float* __restrict__ K, int x, int y, float& dx, float& dy) {
    dy = ((float)y + 0.5f - K[5]) / K[4];
    dx = ((float)x + 0.5f - K[2] - K[1] * dy) / K[0];
}

// clamps before the conversion: a projection may be anything, +-inf included
__device__ __forceinline__ int clamp_to_int(float v, int lo, int hi) {
    return (int)fminf(fmaxf(v, (float)lo), (float)hi);
}

// one slab of the ray / box test: the ray o + t * l against |coordinate| <= h.  Narrows [tn, tf] and remembers which axis
// bounds it; a ray parallel to the slab either misses the box or leaves the interval as it is.
__device__ __forceinline__ bool slab(float o, float l, float h, int axis, float& tn, float& tf, int& an, int& af) {
    if (l == 0.0f) return fabsf(o) <= h;
    const float inv = 1.0f / l;
    const float ta = (-h - o) * inv, tb = (h - o) * inv;
    const float lo = fminf(ta, tb), hi = fmaxf(ta, tb);
    if (lo > tn) { tn = lo; an = axis; }
    if (hi < tf) { tf = hi; af = axis; }
    return true;
}

// face number (get_cuboid_verts_faces: 0 front -w/2, 1 right +l/2, 2 left -l/2, 3 back +w/2, 4 top -h/2, 5 bottom +h/2) of
// the side of box-frame axis `axis` (0: length, 1: height, 2: width) at the negative / positive end
__device__ __forceinline__ int face_of(int axis, bool positive) {
    return axis == 0 ? (positive ? 1 : 2) : (axis == 1 ? (positive ? 5 : 4) : (positive ? 3 : 0));
}

// box record `rec` + whether the box can touch the tile [tx0, tx1] x [ty0, ty1] (rectangle of the projected corners, one pixel
// of slack; the whole view when a corner is in front of the near plane; nothing when all of them are)
__device__ __forceinline__ int stage_box(const float* __restrict__ b, const float* __restrict__ r, const float* __restrict__ K,
                                         float zplane, int W, int H, int tx0, int ty0, int tx1, int ty1, float* rec) {
    const float cx = b[0], cy = b[1], cz = b[2];
    const float hx = 0.5f * b[5], hy = 0.5f * b[4], hz = 0.5f * b[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float r0 = r[a], r1 = r[3 + a], r2 = r[6 + a];            // column a of R = box axis a in camera space
        rec[3 * a] = r0; rec[3 * a + 1] = r1; rec[3 * a + 2] = r2;
        rec[9 + a] = -(r0 * cx + r1 * cy + r2 * cz);                    // the camera centre in the box frame
    }
    rec[12] = hx; rec[13] = hy; rec[14] = hz; rec[15] = 0.0f;
    float zmin = __int_as_float(0x7f800000), zmax = -zmin, umin = zmin, umax = -zmin, vmin = zmin, vmax = -zmin;
    const float znear = fmaxf(zplane, 1e-4f);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float sx = (k & 1) ? hx : -hx, sy = (k & 2) ? hy : -hy, sz = (k & 4) ? hz : -hz;
        const float px = cx + r[0] * sx + r[1] * sy + r[2] * sz;
        const float py = cy + r[3] * sx + r[4] * sy + r[5] * sz;
        const float pz = cz + r[6] * sx + r[7] * sy + r[8] * sz;
        zmin = fminf(zmin, pz); zmax = fmaxf(zmax, pz);
        const float iz = 1.0f / fmaxf(pz, znear);
        const float u = (K[0] * px + K[1] * py) * iz + K[2], v = K[4] * py * iz + K[5];
        umin = fminf(umin, u); umax = fmaxf(umax, u); vmin = fminf(vmin, v); vmax = fmaxf(vmax, v);
    }
    if (!(zmax >= zplane)) return 0;                 // wholly in front of the near plane (or not a number): covers nothing
    if (zmin < znear) return 1;                      // straddles the near plane / holds the camera: any pixel may see it
    const int x0 = clamp_to_int(floorf(umin) - 1.0f, -1, W), x1 = clamp_to_int(ceilf(umax) + 1.0f, -1, W);
    const int y0 = clamp_to_int(floorf(vmin) - 1.0f, -1, H), y1 = clamp_to_int(ceilf(vmax) + 1.0f, -1, H);
    return x0 <= tx1 && x1 >= tx0 && y0 <= ty1 && y1 >= ty0;
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
            const float* r = s_rec + j * REC;
            const float lx = r[0] * dx + r[1] * dy + r[2], ly = r[3] * dx + r[4] * dy + r[5], lz = r[6] * dx + r[7] * dy + r[8];
            float tn = -inf, tf = inf;
            int an = 0, af = 0;
            bool ok = slab(r[9], lx, r[12], 0, tn, tf, an, af);
            ok = slab(r[10], ly, r[13], 1, tn, tf, an, af) && ok;
            ok = slab(r[11], lz, r[14], 2, tn, tf, an, af) && ok;
            // d_z = 1: the ray parameter IS the camera depth.  First surface point at or behind the near plane: the entry, or the
            // exit when the entry lies in front of the plane (camera inside the box, box across the plane)
            const bool entry = tn >= zplane;
            const bool hit = inside && ok && tn <= tf && tf >= zplane;
            const float th = entry ? tn : tf;
            const int ax = entry ? an : af;
            const float la = ax == 0 ? lx : (ax == 1 ? ly : lz);
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
