// cuboid_cast.h -- the ray / cuboid test shared by render.hip (omni_cuboid_depth: one image) and annotate.hip
// (omni_visibility_ragged: every image of a dataset): the ray through a pixel centre is clipped against the three slabs of a box in
// the box frame.  One 256-thread workgroup per 16 x 16 pixel tile, boxes staged through LDS in chunks of 64 as 16-float records and
// culled per tile by the rectangle of their projected corners.  Device functions only; both files must take every decision from
// these, so that their pixel counts agree.
#pragma once
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

// the hit test of one staged box record `r` against the ray (dx, dy, 1).  d_z = 1: the ray parameter IS the camera depth.  A hit
// is a surface point at or behind the near plane; `th` is the depth of the first one: the entry, or the exit when the entry lies
// in front of the plane (camera inside the box, box across the plane).  `ax` is the box-frame axis of the face hit, `la` the ray
// direction along it, `entry` whether the hit is the entry point.
__device__ __forceinline__ bool cast_box(const float* r, float dx, float dy, float zplane, float& th, int& ax, float& la,
                                         bool& entry) {
    const float inf = __int_as_float(0x7f800000);
    const float lx = r[0] * dx + r[1] * dy + r[2], ly = r[3] * dx + r[4] * dy + r[5], lz = r[6] * dx + r[7] * dy + r[8];
    float tn = -inf, tf = inf;
    int an = 0, af = 0;
    bool ok = slab(r[9], lx, r[12], 0, tn, tf, an, af);
    ok = slab(r[10], ly, r[13], 1, tn, tf, an, af) && ok;
    ok = slab(r[11], lz, r[14], 2, tn, tf, an, af) && ok;
    entry = tn >= zplane;
    th = entry ? tn : tf;
    ax = entry ? an : af;
    la = ax == 0 ? lx : (ax == 1 ? ly : lz);
    return ok && tn <= tf && tf >= zplane;
}

}  // namespace
