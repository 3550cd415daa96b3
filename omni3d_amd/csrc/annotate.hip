// annotate.hip -- the derived fields of an Omni3D annotation (bbox3D_cam, bbox2D_proj, bbox2D_trunc, truncation, behind_camera,
// visibility) for every box of every image of a dataset, two launches in all.  The reference derives them box by box and image by
// image on the host: `get_cuboid_verts` / `convert_3d_box_to_2d` / `estimate_truncation` (cubercnn/util/math_util.py:221-259,
// 498-577, 745-758) and `estimate_visibility` (math_util.py:728-743, one mesh rasterisation per image).
//
// Rows are ragged by image: the boxes of image i are rows box_off[i] .. box_off[i + 1] - 1; K (I,9) and size (I,2) = [W, H] hold
// the intrinsics and the frame of every image.
//   box_annotate_kernel       one thread per box: the eight vertices, their projection, the 2D box of the projection with the
//                             vertices behind min_z moved to an image corner, its part inside the frame and the truncation (float64
//                             from the float32 box).  No LDS, no atomics, no dependence on any other thread.
//   visibility_ragged_kernel  the `area` / `visible` counters of cuboid_depth_kernel (render.hip) for all images at once: one
//                             256-thread workgroup per 16 x 16 tile of the concatenated tile list of all images; the workgroup
//                             finds its image by a search in tile_off and casts the pixel rays against the boxes of that image with
//                             the functions of cuboid_cast.h.  No depth, index or face map is written.  Integer atomics only.
#include <device_rt.h>
#include "cuboid_cast.h"

namespace {

// the last row r of off[0 .. n - 1] with off[r] <= v (off never decreases, off[0] <= v)
__device__ __forceinline__ int last_not_above(const int* __restrict__ off, int n, int v) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// torch.min / torch.max over a row: a NaN, once met, stays
__device__ __forceinline__ void row_min_max(float v, float& lo, float& hi) {
    if (lo == lo && (v < lo || v != v)) lo = v;
    if (hi == hi && (v > hi || v != v)) hi = v;
}

__global__ void __launch_bounds__(256) box_annotate_kernel(const float* __restrict__ box3d, const float* __restrict__ R,
                                                            const int* __restrict__ box_off, const float* __restrict__ Ks,
                                                            const int* __restrict__ size, int I, int N, float min_z,
                                                            float* __restrict__ verts3d, float* __restrict__ verts2d,
                                                            float* __restrict__ proj, float* __restrict__ trunc,
                                                            double* __restrict__ truncation, unsigned char* __restrict__ behind,
                                                            unsigned char* __restrict__ fully_behind) {
    const long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const int img = last_not_above(box_off, I, (int)n);
    const float* K = Ks + 9L * img;
    const float* b = box3d + 6L * n;
    const float* r = R + 9L * n;
    const float xmax = (float)(size[2L * img] - 1), ymax = (float)(size[2L * img + 1] - 1);
    const float cx = b[0], cy = b[1], cz = b[2];
    const float hx = 0.5f * b[5], hy = 0.5f * b[4], hz = 0.5f * b[3];      // box frame: x length, y height, z width
    const float inf = __int_as_float(0x7f800000);
    float x1 = inf, y1 = inf, x2 = -inf, y2 = -inf;
    int n_behind = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        // vertex order of get_cuboid_verts_faces: x -++- -++-, y --++ --++, z ---- ++++
        const float sx = ((k + 1) & 2) ? hx : -hx, sy = (k & 2) ? hy : -hy, sz = (k & 4) ? hz : -hz;
        const float px = (r[0] * sx + r[1] * sy + r[2] * sz) + cx;
        const float py = (r[3] * sx + r[4] * sy + r[5] * sz) + cy;
        const float pz = (r[6] * sx + r[7] * sy + r[8] * sz) + cz;
        const float w = K[6] * px + K[7] * py + K[8] * pz;
        float u = (K[0] * px + K[1] * py + K[2] * pz) / w;
        float v = (K[3] * px + K[4] * py + K[5] * pz) / w;
        float* o3 = verts3d + 24L * n + 3 * k;
        float* o2 = verts2d + 24L * n + 3 * k;
        o3[0] = px; o3[1] = py; o3[2] = pz;
        o2[0] = u; o2[1] = v; o2[2] = w;
        if (w <= min_z) {                            // behind: the image corner its camera-space x and y point to; strict signs
            ++n_behind;
            if (px != 0.0f && py != 0.0f && px == px && py == py) {
                u = px > 0.0f ? xmax : 0.0f;
                v = py > 0.0f ? ymax : 0.0f;
            }
        }
        row_min_max(u, x1, x2);
        row_min_max(v, y1, y2);
    }
    const bool all_behind = n_behind == 8;
    behind[n] = n_behind > 0;
    fully_behind[n] = all_behind;
    float* p = proj + 4L * n;
    p[0] = x1; p[1] = y1; p[2] = x2; p[3] = y2;
    // the part inside [0, W - 1] x [0, H - 1]; the marker -1 where there is none (the comparison also drops a NaN)
    const float tx1 = fmaxf(x1, 0.0f), ty1 = fmaxf(y1, 0.0f), tx2 = fminf(x2, xmax), ty2 = fminf(y2, ymax);
    const bool some = !all_behind && x1 == x1 && y1 == y1 && x2 == x2 && y2 == y2 && tx2 > tx1 && ty2 > ty1;
    float* q = trunc + 4L * n;
    q[0] = some ? tx1 : -1.0f; q[1] = some ? ty1 : -1.0f; q[2] = some ? tx2 : -1.0f; q[3] = some ? ty2 : -1.0f;
    // 1 - area(proj ^ frame) / area(proj) in float64 from the float32 box: 0 / 0 (a box of no area) is NaN, as in the reference
    const double ax1 = x1, ay1 = y1, ax2 = x2, ay2 = y2;
    const double iw = fmax(fmin(ax2, (double)xmax) - fmax(ax1, 0.0), 0.0), ih = fmax(fmin(ay2, (double)ymax) - fmax(ay1, 0.0), 0.0);
    const double area = (ax2 - ax1) * (ay2 - ay1);
    truncation[n] = all_behind ? 1.0 : 1.0 - (iw * ih) / area;
}

__global__ void __launch_bounds__(256) visibility_ragged_kernel(const float* __restrict__ box3d, const float* __restrict__ R,
                                                                 const int* __restrict__ box_off, const float* __restrict__ Ks,
                                                                 const int* __restrict__ size, const int* __restrict__ tile_off,
                                                                 int I, float zplane, int* __restrict__ area,
                                                                 int* __restrict__ visible) {
    __shared__ float s_rec[CHUNK * REC];
    __shared__ int s_on[CHUNK];       // the box's rectangle meets this tile
    __shared__ int s_cnt[CHUNK];      // pixels of this tile per box of the chunk
    const int t = threadIdx.x, lane = t & 63;
    const int tile = blockIdx.x;
    const int img = last_not_above(tile_off, I, tile);             // the same image in every thread of the workgroup
    const int W = size[2L * img], H = size[2L * img + 1];
    const int tiles_x = (W + TILE - 1) / TILE, local = tile - tile_off[img];
    const int b0 = box_off[img], N = box_off[img + 1] - b0;
    const float* K = Ks + 9L * img;
    box3d += 6L * b0; R += 9L * b0; area += b0; visible += b0;     // from here on: cuboid_depth_kernel on the boxes of this image
    const int tx0 = (local % tiles_x) * TILE, ty0 = (local / tiles_x) * TILE;
    const int tx1 = min(tx0 + TILE, W) - 1, ty1 = min(ty0 + TILE, H) - 1;
    const int x = tx0 + (t & 15), y = ty0 + (t >> 4);
    const bool inside = x < W && y < H;
    float dx, dy;
    pixel_ray(K, x, y, dx, dy);
    float best = __int_as_float(0x7f800000);
    int bi = -1;
    for (int c0 = 0; c0 < N; c0 += CHUNK) {
        const int n = min(CHUNK, N - c0);
        if (t < CHUNK) {
            s_cnt[t] = 0;
            s_on[t] = t < n ? stage_box(box3d + 6L * (c0 + t), R + 9L * (c0 + t), K, zplane, W, H, tx0, ty0, tx1, ty1, s_rec + t * REC) : 0;
        }
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            if (!s_on[j]) continue;                  // the same decision in every thread of the workgroup
            float th, la;
            int ax;
            bool entry;
            const bool hit = cast_box(s_rec + j * REC, dx, dy, zplane, th, ax, la, entry) && inside;
            const unsigned long long m = __ballot(hit);
            if (lane == 0 && m) atomicAdd(&s_cnt[j], (int)__popcll(m));
            if (hit && th < best) {                  // boxes come in index order: equal depths stay with the lower index
                best = th;
                bi = c0 + j;
            }
        }
        __syncthreads();
        if (t < n && s_cnt[t] > 0) atomicAdd(&area[c0 + t], s_cnt[t]);
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

}  // namespace

extern "C" {

int omni_box_annotate(const float* box3d, const float* R, const int* box_off, const float* K, const int* size, int I, int N,
                      float min_z, float* verts3d, float* verts2d, float* proj, float* trunc, double* truncation,
                      unsigned char* behind, unsigned char* fully_behind, void* stream) {
    if (I < 0 || N < 0 || (I == 0 && N > 0)) return OMNI_ERR_ARG;
    if (N == 0) return OMNI_OK;
    hipLaunchKernelGGL(box_annotate_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, box3d, R, box_off, K,
                       size, I, N, min_z, verts3d, verts2d, proj, trunc, truncation, behind, fully_behind);
    return omni_launch_status();
}

int omni_visibility_ragged(const float* box3d, const float* R, const int* box_off, const float* K, const int* size,
                           const int* tile_off, int I, int N, int tiles, float zplane, int* area, int* visible, void* stream) {
    if (I < 0 || N < 0 || tiles < 0 || (I == 0 && (N > 0 || tiles > 0)) || !(zplane > 0.0f)) return OMNI_ERR_ARG;
    if (N == 0) return OMNI_OK;
    hipStream_t st = (hipStream_t)stream;
    omni_memset_async(area, 0, sizeof(int) * (size_t)N, st);
    omni_memset_async(visible, 0, sizeof(int) * (size_t)N, st);
    if (tiles == 0) return OMNI_OK;
    hipLaunchKernelGGL(visibility_ragged_kernel, dim3((unsigned)tiles), dim3(256), 0, st, box3d, R, box_off, K, size, tile_off, I,
                       zplane, area, visible);
    return omni_launch_status();
}

}  // extern "C"
