// cuboid_exact.h -- the exact IoU3D of two cuboids, in double, as device functions: shared by csrc/iou3d_exact.hip (omni_cuboid_fit,
// omni_iou3d_exact_pairs) and by the pair-matrix launch of omni_nms3d_exact in csrc/nms3d.hip.  Every file that includes it switches multiply-add
// contraction off before it includes this header, so the host emulator and the device do the same arithmetic.
//
//   cuboid_fit       eight float32 corners in the order of boxgen.UNIT -> the cuboid they are taken for: centre = vertex mean, axis k =
//                    mean of the four edges parallel to it (dimension = its norm), the axes orthonormalised (x, then y by Gram-Schmidt,
//                    then z = +-(x cross y) on the side of the measured z).  Float32-rounded corners are not coplanar to better than
//                    1e-6 of the coordinate magnitude; without the fit the twelve "faces" do not bound a solid and two identical
//                    boxes score above 1.  Invalid: a non-finite vertex, a dimension <= eps_dim, or a vertex further than
//                    fit_tol x the largest dimension from its fitted corner (no cuboid at all).
//   cuboid_pair_iou  disjoint bounding spheres: exactly 0.  Otherwise the boundary of A ^ B is the part of A's six faces inside B plus
//                    the part of B's six faces inside A, and V = 1/3 sum (n . p0) area over those pieces, n outward, p0 measured from
//                    A's centre.  Every face is handled in the frame of its own box (centre at the origin, axes = coordinates), so a
//                    face is a rectangle in two coordinates and the other box is six half-planes there: Sutherland-Hodgman, ping-pong
//                    between two lists of <= 10 vertices.  The lists are indexed at run time, so they live in per-thread LDS slices
//                    [slot][thread] of doubles (a private array would go to scratch): ds_read_b64 takes the lanes of a 32-lane half
//                    from 64 distinct banks, ds_write_b64 a 16-lane group from 32; 320 B per thread.
//                    All coordinates are relative to one of the two centres before any product is formed.
//                    Two conventions.  Snap: a signed distance with |d| <= 1e-12 x (the largest coordinate of either box about A's
//                    centre) is 0 -- four orders of magnitude above double rounding, four below float32 input granularity.
//                    Closed / open: B's faces are clipped by A's OPEN half-spaces (d < 0 is inside); A's faces by B's half-spaces
//                    CLOSED (d <= 0) where the two outward normals point the same way and open where they oppose.  A shared face
//                    plane is then counted exactly once when the boxes lie on the same side of it and not at all when they touch
//                    across it.
//                    The axis loops keep constant indices by renaming: after each pass the coordinates (or the other box's axes)
//                    are rotated by one place, three passes restore them.  No atomics, no dependence on another thread.
#pragma once

constexpr int CX_CAP = 10;                     // a rectangle clipped by six half-planes: 4 + 6 vertices
constexpr double CX_SNAP = 1e-12;
constexpr double CX_EPS_DIM = 1e-8;            // defaults of omni_nms3d_exact (include/omni3d_hip.h): conditions on the input, not tuned
constexpr double CX_FIT_TOL = 1e-3;

struct CxBox {
    double c[3];                               // centre
    double x[3][3];                            // x[k]: unit axis k
    double d[3];                               // dimensions
};

__device__ __forceinline__ bool cx_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// v: 24 floats.  Returns the validity; the fields of an invalid box are 0.
__device__ __forceinline__ bool cuboid_fit(const float* __restrict__ v, double eps_dim, double fit_tol, CxBox& o) {
    double p[8][3];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float f = v[3 * k + a];
            ok = ok && cx_finite(f);
            p[k][a] = ok ? (double)f : 0.0;
        }
    double e[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        o.c[a] = 0.125 * (((p[0][a] + p[1][a]) + (p[2][a] + p[3][a])) + ((p[4][a] + p[5][a]) + (p[6][a] + p[7][a])));
        e[0][a] = 0.25 * (((p[1][a] - p[0][a]) + (p[2][a] - p[3][a])) + ((p[5][a] - p[4][a]) + (p[6][a] - p[7][a])));
        e[1][a] = 0.25 * (((p[3][a] - p[0][a]) + (p[2][a] - p[1][a])) + ((p[7][a] - p[4][a]) + (p[6][a] - p[5][a])));
        e[2][a] = 0.25 * (((p[4][a] - p[0][a]) + (p[5][a] - p[1][a])) + ((p[6][a] - p[2][a]) + (p[7][a] - p[3][a])));
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o.d[k] = sqrt(e[k][0] * e[k][0] + e[k][1] * e[k][1] + e[k][2] * e[k][2]);
        ok = ok && o.d[k] > eps_dim;
    }
    const double i0 = ok ? 1.0 / o.d[0] : 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) o.x[0][a] = e[0][a] * i0;
    const double along = e[1][0] * o.x[0][0] + e[1][1] * o.x[0][1] + e[1][2] * o.x[0][2];
    double y[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) y[a] = e[1][a] - along * o.x[0][a];
    const double ny = sqrt(y[0] * y[0] + y[1] * y[1] + y[2] * y[2]);
    ok = ok && ny > eps_dim;
    const double i1 = ok ? 1.0 / ny : 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) o.x[1][a] = y[a] * i1;
    o.x[2][0] = o.x[0][1] * o.x[1][2] - o.x[0][2] * o.x[1][1];
    o.x[2][1] = o.x[0][2] * o.x[1][0] - o.x[0][0] * o.x[1][2];
    o.x[2][2] = o.x[0][0] * o.x[1][1] - o.x[0][1] * o.x[1][0];
    const double side = o.x[2][0] * e[2][0] + o.x[2][1] * e[2][1] + o.x[2][2] * e[2][2];
    const double flip = side < 0.0 ? -1.0 : 1.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) o.x[2][a] *= flip;
    // the largest distance of a vertex from its fitted corner
    double worst = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const double s0 = (k == 1 || k == 2 || k == 5 || k == 6) ? 0.5 : -0.5;
        const double s1 = (k == 2 || k == 3 || k == 6 || k == 7) ? 0.5 : -0.5;
        const double s2 = k >= 4 ? 0.5 : -0.5;
        double r2 = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double q = o.c[a] + ((s0 * o.d[0]) * o.x[0][a] + (s1 * o.d[1]) * o.x[1][a] + (s2 * o.d[2]) * o.x[2][a]);
            r2 += (p[k][a] - q) * (p[k][a] - q);
        }
        worst = fmax(worst, r2);
    }
    const double lim = fit_tol * fmax(o.d[0], fmax(o.d[1], o.d[2]));
    ok = ok && worst <= lim * lim;
    if (!ok) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            o.c[a] = 0.0; o.d[a] = 0.0;
            o.x[0][a] = 0.0; o.x[1][a] = 0.0; o.x[2][a] = 0.0;
        }
    }
    return ok;
}

__device__ __forceinline__ double cx_snap(double d, double snap) { return fabs(d) <= snap ? 0.0 : d; }

// 3 x the volume that the faces of one box (half extents h, centre at the origin, axes = coordinates) contribute: the other box has
// its centre at c, unit axes e[k] and half extents g in these coordinates.  FIRST: the faces are A's (closed where the normals agree,
// weight = distance of the face from A's centre); otherwise B's (open; A's centre lies at c).  L0, L1: this thread's two vertex lists,
// element (vertex i, coordinate j) at [(2 i + j) * T].
template <bool FIRST, int T>
__device__ __forceinline__ double cx_faces(double h0, double h1, double h2, double c0, double c1, double c2, double e00, double e01,
                                           double e02, double e10, double e11, double e12, double e20, double e21, double e22, double g0,
                                           double g1, double g2, double snap, double* L0, double* L1) {
    double sum = 0.0;
    for (int ax = 0; ax < 3; ++ax) {                               // the faces orthogonal to coordinate 0 of the current naming
        for (int sg = 0; sg < 2; ++sg) {
            const double s = sg ? -1.0 : 1.0;
            const double x0 = s * h0 - c0;                         // the face plane, and below its rectangle, about the other centre
            double* src = L0;
            double* dst = L1;
            src[0 * T] = -h1 - c1; src[1 * T] = -h2 - c2;
            src[2 * T] = h1 - c1;  src[3 * T] = -h2 - c2;
            src[4 * T] = h1 - c1;  src[5 * T] = h2 - c2;
            src[6 * T] = -h1 - c1; src[7 * T] = h2 - c2;
            int n = 4;
            for (int k = 0; k < 3; ++k) {                          // the slab of the other box's axis 0 of the current naming
                for (int hs = 0; hs < 2; ++hs) {
                    const double u = hs ? -1.0 : 1.0;
                    const bool closed = FIRST && (s * u) * e00 > 0.0;
                    const double off = e00 * x0;
                    int m = 0;
                    if (n > 0) {
                        double qx = src[(2 * (n - 1)) * T], qy = src[(2 * (n - 1) + 1) * T];
                        double dq = cx_snap(u * (off + (e01 * qx + e02 * qy)) - g0, snap);
                        bool iq = closed ? dq <= 0.0 : dq < 0.0;
                        for (int i = 0; i < n; ++i) {
                            const double px = src[(2 * i) * T], py = src[(2 * i + 1) * T];
                            const double dp = cx_snap(u * (off + (e01 * px + e02 * py)) - g0, snap);
                            const bool ip = closed ? dp <= 0.0 : dp < 0.0;
                            if (ip != iq && m < CX_CAP) {
                                const double f = dq / (dq - dp);
                                dst[(2 * m) * T] = qx + f * (px - qx);
                                dst[(2 * m + 1) * T] = qy + f * (py - qy);
                                ++m;
                            }
                            if (ip && m < CX_CAP) {
                                dst[(2 * m) * T] = px;
                                dst[(2 * m + 1) * T] = py;
                                ++m;
                            }
                            qx = px; qy = py; dq = dp; iq = ip;
                        }
                    }
                    n = m;
                    double* sw = src; src = dst; dst = sw;
                }
                const double t0 = e00, t1 = e01, t2 = e02, tg = g0;  // the other box's axes move up one place
                e00 = e10; e01 = e11; e02 = e12; g0 = g1;
                e10 = e20; e11 = e21; e12 = e22; g1 = g2;
                e20 = t0; e21 = t1; e22 = t2; g2 = tg;
            }
            double area = 0.0;
            if (n >= 3) {
                const double rx = src[0], ry = src[T];
                for (int i = 1; i + 1 < n; ++i)
                    area += (src[(2 * i) * T] - rx) * (src[(2 * i + 3) * T] - ry) - (src[(2 * i + 1) * T] - ry) * (src[(2 * i + 2) * T] - rx);
                area = fmax(0.5 * area, 0.0);
            }
            sum += (FIRST ? h0 : h0 - s * c0) * area;
        }
        const double th = h0, tc = c0, ta = e00, tb = e10, te = e20;  // the coordinates move up one place
        h0 = h1; h1 = h2; h2 = th;
        c0 = c1; c1 = c2; c2 = tc;
        e00 = e01; e01 = e02; e02 = ta;
        e10 = e11; e11 = e12; e12 = tb;
        e20 = e21; e21 = e22; e22 = te;
    }
    return sum;
}

// two VALID fitted boxes -> intersection volume and IoU in [0, 1]; L0, L1 as in cx_faces
template <int T>
__device__ __forceinline__ void cuboid_pair_iou(const CxBox& A, const CxBox& B, double* L0, double* L1, float& vol, float& iou) {
    vol = 0.0f;
    iou = 0.0f;
    const double t0 = B.c[0] - A.c[0], t1 = B.c[1] - A.c[1], t2 = B.c[2] - A.c[2];
    const double ha0 = 0.5 * A.d[0], ha1 = 0.5 * A.d[1], ha2 = 0.5 * A.d[2], hb0 = 0.5 * B.d[0], hb1 = 0.5 * B.d[1], hb2 = 0.5 * B.d[2];
    const double ra = sqrt(ha0 * ha0 + ha1 * ha1 + ha2 * ha2), rb = sqrt(hb0 * hb0 + hb1 * hb1 + hb2 * hb2);
    if (t0 * t0 + t1 * t1 + t2 * t2 > (ra + rb) * (ra + rb)) return;
    double e[3][3], ta[3], tb[3];                                  // e[k][a] = B's axis k . A's axis a
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int a = 0; a < 3; ++a) e[k][a] = B.x[k][0] * A.x[a][0] + B.x[k][1] * A.x[a][1] + B.x[k][2] * A.x[a][2];
        ta[k] = A.x[k][0] * t0 + A.x[k][1] * t1 + A.x[k][2] * t2;            // B's centre in A's frame
        tb[k] = -(B.x[k][0] * t0 + B.x[k][1] * t1 + B.x[k][2] * t2);         // A's centre in B's frame
    }
    double big = fmax(ha0, fmax(ha1, ha2));
#pragma unroll
    for (int a = 0; a < 3; ++a) big = fmax(big, fabs(ta[a]) + (fabs(e[0][a]) * hb0 + fabs(e[1][a]) * hb1 + fabs(e[2][a]) * hb2));
    const double snap = CX_SNAP * big;
    const double sa = cx_faces<true, T>(ha0, ha1, ha2, ta[0], ta[1], ta[2], e[0][0], e[0][1], e[0][2], e[1][0], e[1][1], e[1][2], e[2][0],
                                        e[2][1], e[2][2], hb0, hb1, hb2, snap, L0, L1);
    const double sb = cx_faces<false, T>(hb0, hb1, hb2, tb[0], tb[1], tb[2], e[0][0], e[1][0], e[2][0], e[0][1], e[1][1], e[2][1], e[0][2],
                                         e[1][2], e[2][2], ha0, ha1, ha2, snap, L0, L1);
    const double va = A.d[0] * A.d[1] * A.d[2], vb = B.d[0] * B.d[1] * B.d[2];
    const double V = fmin(fmax((sa + sb) / 3.0, 0.0), fmin(va, vb));
    const double uni = va + vb - V;
    const double r = uni > 0.0 ? V / uni : 0.0;
    vol = (float)V;
    iou = (float)fmin(fmax(r, 0.0), 1.0);
}
