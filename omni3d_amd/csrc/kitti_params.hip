// kitti_params.hip -- cuboid corners to the KITTI object benchmark's box parameters (h, w, l, location, rotation_y, alpha): the
// geometry behind AOS (csrc/eval_kitti.hip) and behind the label files of cubercnn/data/kitti_format.py.
//
// The heading convention rests on the corner order of `omni_cuboid_corners` (the reference's get_cuboid_verts_faces): the length l
// runs along local x, h along y, w along z, and v1 - v0 is the length axis, v3 - v0 the height axis, v4 - v0 the width axis.  With
// R = Ry(ry) the length axis is l (cos ry, 0, -sin ry): KITTI's rotation_y.  For a general up vector u the ground plane is spanned by
// a = camera x less its part along u, normalised, and b = u x a (u = (0, -1, 0): a = (1, 0, 0), b = (0, 0, 1)).
//   omni_kitti_box_params   one thread per box, double arithmetic on the float32 corners, no LDS, no atomics
#include <device_rt.h>

namespace {

struct KittiBasis { double u[3], a[3], b[3]; };

__device__ __forceinline__ double kp_dot(const double* p, const double* q) { return p[0] * q[0] + p[1] * q[1] + p[2] * q[2]; }

__global__ void __launch_bounds__(256) kitti_box_params_kernel(const float* __restrict__ corners, int n, KittiBasis B, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* v = corners + 24ll * i;
    double* o = out + 9ll * i;
    bool finite = true;
    double c[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double x = (double)v[3 * k + a];
            finite = finite && isfinite(x);
            c[a] += x;                                   // corners 0 .. 7 in order
        }
    }
    double e[3], eh[3], ew[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        c[a] *= 0.125;
        e[a] = (double)v[3 + a] - (double)v[a];
        eh[a] = (double)v[9 + a] - (double)v[a];
        ew[a] = (double)v[12 + a] - (double)v[a];
    }
    const double l = sqrt(kp_dot(e, e)), h = sqrt(kp_dot(eh, eh)), w = sqrt(kp_dot(ew, ew));
    if (!(finite && l > 0.0 && h > 0.0 && w > 0.0)) {
        const double nan = __builtin_nan("");
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = nan;
        o[8] = 0.0;
        return;
    }
    // + 0.0 / 0.0 -: no negative zero reaches atan2, so a heading without a ground-plane component gives atan2(0, 0) = 0
    const double ry = atan2(0.0 - kp_dot(e, B.b), kp_dot(e, B.a) + 0.0);
    double alpha = ry - atan2(kp_dot(c, B.a), kp_dot(c, B.b));
    const double pi = 3.14159265358979323846;
    if (alpha > pi) alpha -= 2.0 * pi;
    if (alpha <= -pi) alpha += 2.0 * pi;
    o[0] = h; o[1] = w; o[2] = l;
    o[3] = c[0] - 0.5 * h * B.u[0];                      // the centre of the bottom face
    o[4] = c[1] - 0.5 * h * B.u[1];
    o[5] = c[2] - 0.5 * h * B.u[2];
    o[6] = ry; o[7] = alpha; o[8] = 1.0;
}

}  // namespace

extern "C" {

int omni_kitti_box_params(const float* corners, int n, double up_x, double up_y, double up_z, double* out, void* stream) {
    if (n < 0) return OMNI_ERR_ARG;
    KittiBasis B;
    const double nu = sqrt(up_x * up_x + up_y * up_y + up_z * up_z);
    if (!(nu > 0.0) || !(nu < INFINITY)) return OMNI_ERR_ARG;
    B.u[0] = up_x / nu; B.u[1] = up_y / nu; B.u[2] = up_z / nu;
    // camera x less its part along u
    B.a[0] = 1.0 - B.u[0] * B.u[0]; B.a[1] = -B.u[0] * B.u[1]; B.a[2] = -B.u[0] * B.u[2];
    const double na = sqrt(B.a[0] * B.a[0] + B.a[1] * B.a[1] + B.a[2] * B.a[2]);
    if (!(na > 1e-12)) return OMNI_ERR_ARG;               // up parallel to camera x
    for (int k = 0; k < 3; ++k) B.a[k] /= na;
    B.b[0] = B.u[1] * B.a[2] - B.u[2] * B.a[1];
    B.b[1] = B.u[2] * B.a[0] - B.u[0] * B.a[2];
    B.b[2] = B.u[0] * B.a[1] - B.u[1] * B.a[0];
    if (n == 0) return OMNI_OK;
    hipLaunchKernelGGL(kitti_box_params_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, corners, n, B, out);
    return omni_launch_status();
}

}  // extern "C"
