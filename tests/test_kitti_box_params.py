"""`kernels.kitti.box_params` (csrc/kitti_params.hip): cuboid corners -> KITTI's h, w, l, location, rotation_y, alpha, valid.

Bars.  The kernel computes in double on the float32 corners, so a float64 numpy evaluation of the same formulas ON THE SAME FLOAT32
CORNERS is the reference: lengths and location within 1e-12 relative, angles within 1e-12 rad after wrapping (double atan2 and sqrt
of two implementations differ by a few ulps at magnitude <= pi; 1e-12 is thousands of ulps).  For yaw-only boxes the generating
angle comes back within 8 * 2^-24 * max|coordinate| / l: the heading is the direction of e = v1 - v0, |e| = l; each of the four
float32 coordinates of v0 and v1 that enter it is off by at most one rounding of relative size 2^-24 (the sums that make a
coordinate are dominated by the centre, at least 8 m away here), and a displacement d of e turns it by at most |d| / l."""
import numpy as np
import pytest
import torch

from omni3d_amd import boxgen

PI = np.pi


def _ry(a):
    c, s = np.cos(a), np.sin(a)
    z, o = np.zeros_like(a), np.ones_like(a)
    return np.stack([c, z, s, z, o, z, -s, z, c], -1).reshape(-1, 3, 3)


def _wrap(d):
    return (d + PI) % (2 * PI) - PI


def _exact(corners32, up=(0.0, -1.0, 0.0)):
    """the formulas of include/omni3d_hip.h in float64 numpy, the corner sum in the kernel's order"""
    v = np.asarray(corners32, np.float32).astype(np.float64)
    u = np.asarray(up, np.float64)
    u = u / np.linalg.norm(u)
    a = np.array([1.0, 0.0, 0.0]) - u[0] * u
    a = a / np.linalg.norm(a)
    b = np.cross(u, a)
    c = np.zeros((len(v), 3))
    for k in range(8):
        c = c + v[:, k]
    c = c * 0.125
    e = v[:, 1] - v[:, 0]
    l, h, w = (np.linalg.norm(v[:, k] - v[:, 0], axis=1) for k in (1, 3, 4))
    with np.errstate(invalid="ignore"):                 # the rows of non-finite boxes are overwritten below
        ry = np.arctan2(-(e @ b) + 0.0, e @ a + 0.0)
        alpha = ry - np.arctan2(c @ a, c @ b)
        alpha = np.where(alpha > PI, alpha - 2 * PI, alpha)
        alpha = np.where(alpha <= -PI, alpha + 2 * PI, alpha)
        loc = c - 0.5 * h[:, None] * u
        out = np.column_stack([h, w, l, loc, ry, alpha, np.ones(len(v))])
        bad = ~np.isfinite(v).all(axis=(1, 2)) | ~(l > 0) | ~(h > 0) | ~(w > 0)
    out[bad, :8], out[bad, 8] = np.nan, 0.0
    return out


def _compare(got, want):
    assert got.shape == want.shape and np.array_equal(got[:, 8], want[:, 8])
    ok = want[:, 8] == 1
    assert np.isnan(got[~ok, :8]).all()
    g, w = got[ok], want[ok]
    rel = np.abs(g[:, :6] - w[:, :6]) / np.abs(w[:, :6]).clip(min=1e-300)
    rel = np.where(w[:, :6] == g[:, :6], 0.0, rel)
    ang = np.abs(_wrap(g[:, 6:8] - w[:, 6:8]))
    print("box_params: max relative error of lengths / location %.3g, max angle error %.3g rad" % (rel.max(initial=0), ang.max(initial=0)))
    assert rel.max(initial=0) <= 1e-12 and ang.max(initial=0) <= 1e-12
    assert ((g[:, 7] > -PI) & (g[:, 7] <= PI)).all()


def _cuboids(dev, n=300, seed=3):
    """n random cuboids through `det.cuboid_corners`: the first half yaw-only, the rest freely rotated -> (corners (n, 8, 3) float32
    on dev, the yaw of the first half, their l)"""
    from omni3d_amd.kernels import det
    rng = np.random.default_rng(seed)
    z = rng.uniform(8, 80, n)
    centre = np.stack([rng.uniform(-0.6, 0.6, n) * z, rng.uniform(-3, 3, n), z], 1)
    whl = rng.uniform(0.3, 6.0, (n, 3))
    yaw = rng.uniform(-PI, PI, n // 2)
    R = np.concatenate([_ry(yaw), boxgen.rand_rot(rng, n - n // 2)])
    box = torch.from_numpy(np.concatenate([centre, whl], 1).astype(np.float32)).to(dev)
    return det.cuboid_corners(box, torch.from_numpy(R.reshape(n, 9).astype(np.float32)).to(dev)), yaw, whl[:n // 2, 2]


def _run_random(dev):
    from omni3d_amd.kernels import kitti
    corners, yaw, l = _cuboids(dev)
    c32 = corners.cpu().numpy()
    assert len(c32) == 300 and np.abs(c32).max() > 60                   # more than one workgroup of 256; centres far out
    got = kitti.box_params(corners).cpu().numpy()
    _compare(got, _exact(c32))
    assert got[:, 8].all()
    # the generating yaw of the yaw-only half, within the float32 rounding of the two corners over the edge length
    n = len(yaw)
    bound = 8 * 2.0 ** -24 * np.abs(c32[:n]).max(axis=(1, 2)) / l
    err = np.abs(_wrap(got[:n, 6] - yaw))
    print("yaw recovered within %.3g of its bound at worst" % (err / bound).max())
    assert (err <= bound).all()
    # location: the centre of the bottom face, y down
    centre = c32[:n].astype(np.float64).mean(axis=1)
    assert np.abs(got[:n, 3:6] - (centre + np.column_stack([np.zeros(n), got[:n, 0] / 2, np.zeros(n)]))).max() <= 1e-9
    # another up vector, compared in full; and the batch sizes around one thread, one wave and one workgroup
    _compare(kitti.box_params(corners, (0.0, 0.0, 1.0)).cpu().numpy(), _exact(c32, (0.0, 0.0, 1.0)))
    _compare(kitti.box_params(corners, (0.3, -2.0, 0.1)).cpu().numpy(), _exact(c32, (0.3, -2.0, 0.1)))
    for k in (0, 1, 65, 257):
        out = kitti.box_params(corners[:k].contiguous())
        assert out.shape == (k, 9) and out.dtype == torch.float64 and np.array_equal(out.cpu().numpy(), got[:k])


def test_random_cuboids_emulated(emu_lib):
    _run_random("cpu")


@pytest.mark.gpu
def test_random_cuboids_gpu(hip_lib):
    _run_random("cuda")


def _run_fixed(dev):
    from omni3d_amd.kernels import kitti
    # Ry(pi / 2) at (0, 1, 10), l, h, w = 4, 2, 1: the length axis is (cos, 0, -sin) = (0, 0, -1); every corner is exact in float32
    R = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])
    hand = boxgen.corners(np.array([[0.0, 1.0, 10.0]]), np.array([[4.0, 2.0, 1.0]]), R[None])
    assert np.array_equal(hand[0, 1] - hand[0, 0], [0, 0, -4]) and np.array_equal(hand[0, 3] - hand[0, 0], [0, 2, 0])
    out = kitti.box_params(torch.from_numpy(hand).to(dev)).cpu().numpy()[0]
    want = [2.0, 1.0, 4.0, 0.0, 2.0, 10.0, PI / 2, PI / 2, 1.0]          # h w l, x y z (the bottom face: y + h / 2), rotation_y, alpha, valid
    assert np.abs(out - want).max() <= 1e-15, out
    # the same box seen at 45 degrees to the right: alpha = rotation_y - atan2(x, z)
    moved = hand + np.float32([10.0, 0.0, 0.0])
    out = kitti.box_params(torch.from_numpy(moved).to(dev)).cpu().numpy()[0]
    assert abs(out[6] - PI / 2) <= 1e-15 and abs(out[7] - PI / 4) <= 1e-15
    # alpha wraps into (-pi, pi]: heading -3 pi / 4 (length axis (-1, 0, 1) / sqrt 2), seen at +45 degrees -> -pi, which wraps to +pi
    s = np.sqrt(0.5)
    turned = boxgen.corners(np.array([[10.0, 1.0, 10.0]]), np.array([[4.0, 2.0, 1.0]]), np.array([[[-s, 0, -s], [0, 1, 0], [s, 0, -s]]]))
    out = kitti.box_params(torch.from_numpy(turned).to(dev)).cpu().numpy()[0]
    assert abs(out[6] + 3 * PI / 4) <= 1e-7 and abs(abs(out[7]) - PI) <= 1e-7 and -PI < out[7] <= PI
    # a heading without a ground-plane component (the length axis points up): atan2(0, 0) = 0
    upright = boxgen.corners(np.array([[0.0, 1.0, 10.0]]), np.array([[4.0, 2.0, 1.0]]), np.array([[[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]]))
    out = kitti.box_params(torch.from_numpy(upright).to(dev)).cpu().numpy()[0]
    assert out[6] == 0.0 and out[8] == 1.0
    # non-finite corners and a zero edge: valid 0, NaN elsewhere; the neighbours are untouched
    bad = np.repeat(hand, 5, axis=0)
    bad[1, 6, 2] = np.nan
    bad[2, 0, 0] = np.inf
    bad[3, 1] = bad[3, 0]                                                # l = 0
    out = kitti.box_params(torch.from_numpy(bad).to(dev)).cpu().numpy()
    assert out[:, 8].tolist() == [1, 0, 0, 0, 1] and np.isnan(out[1:4, :8]).all() and np.abs(out[[0, 4]] - want).max() <= 1e-15
    _compare(out, _exact(bad))
    # arguments
    t = torch.from_numpy(hand).to(dev)
    for up in ((1.0, 0.0, 0.0), (-2.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, float("nan"), 0.0), (0.0, 1.0)):
        with pytest.raises(ValueError, match="up"):
            kitti.box_params(t, up)
    for wrong in (t.double(), t.reshape(1, 24), t.expand(2, 8, 3).transpose(1, 2), hand):
        with pytest.raises(ValueError, match="corners"):
            kitti.box_params(wrong)


def test_fixed_cases_emulated(emu_lib):
    _run_fixed("cpu")


@pytest.mark.gpu
def test_fixed_cases_gpu(hip_lib):
    _run_fixed("cuda")
