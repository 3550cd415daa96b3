"""Writes tests/golden/box_annotate.npz: the inputs of `kernels.annotate.box_annotate` (about 400 boxes over 9 images, ragged) and
what the reference's own `get_cuboid_verts`, `convert_3d_box_to_2d(..., XYWH=False)` and `estimate_truncation`
(cubercnn/util/math_util.py, imported unchanged through oracle/ref_harness.py, CPU) return for them.  Needs the reference checkout.
    python tools/make_annotate_golden.py

The boxes: ordinary ones, boxes partly and wholly outside the frame, boxes with 1 .. 7 vertices at z <= min_z in each of the four
sign quadrants of (x, y), boxes wholly behind the camera, one image without a box, and one hand-placed box of zero width whose
projection has no area.  A candidate is rejected (and counted) when, in float64 on the float32 inputs, any vertex has
|z - min_z| < 1e-4 or any vertex at z <= min_z has |x| or |y| below 1e-4: every decision the kernel takes is then unambiguous."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MIN_Z, MARGIN = 0.20, 1e-4
SIZES = ((33, 17), (50, 40), (16, 16), (640, 480), (30, 20), (47, 31), (100, 75), (21, 37), (65, 49))     # (W, H); nothing a multiple of 16 but the third
EMPTY_IMAGE, FLAT_IMAGE = 4, 2
PATH = os.path.join(ROOT, "tests", "golden", "box_annotate.npz")
SX = np.array([-1, 1, 1, -1, -1, 1, 1, -1]) * 0.5
SY = np.array([-1, -1, 1, 1, -1, -1, 1, 1]) * 0.5
SZ = np.array([-1, -1, -1, -1, 1, 1, 1, 1]) * 0.5


def intrinsics(i, W, H):
    if i == FLAT_IMAGE:                   # powers of two: the projection of x = 0 is the principal point exactly, in any precision
        return np.array([[16.0, 0.0, 8.0], [0.0, 16.0, 8.0], [0.0, 0.0, 1.0]])
    return np.array([[0.9 * W + 0.3, 0.0, 0.5 * W + 0.7], [0.0, 0.9 * W - 0.4, 0.5 * H - 0.9], [0.0, 0.0, 1.0]])


def rot(a, b, c):
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def verts64(box, R):
    """float64 vertices (8,3) of the float32 inputs, in the order of get_cuboid_verts_faces"""
    box, R = np.asarray(box, np.float32).astype(np.float64), np.asarray(R, np.float32).astype(np.float64).reshape(3, 3)
    local = np.stack((box[5] * SX, box[4] * SY, box[3] * SZ))
    return (R @ local).T + box[:3]


def unambiguous(box, R):
    v = verts64(box, R)
    if (np.abs(v[:, 2] - MIN_Z) < MARGIN).any():
        return False
    b = v[:, 2] <= MIN_Z
    return not ((np.abs(v[b, 0]) < MARGIN) | (np.abs(v[b, 1]) < MARGIN)).any()


def make_inputs(seed=5):
    """-> dict of float32 / int32 arrays + the number of rejected candidates"""
    rs = np.random.RandomState(seed)
    boxes, rots, counts, Ks, rejected = [], [], [], [], 0
    for i, (W, H) in enumerate(SIZES):
        K = intrinsics(i, W, H)
        Ks.append(K)
        group = []

        def at(u, v, z):
            return [(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z]

        def take(box, R):
            nonlocal rejected
            if unambiguous(box, R):
                group.append((box, R))
                return True
            rejected += 1
            return False

        def any_rot():
            return rot(rs.uniform(-np.pi, np.pi), rs.uniform(-0.6, 0.6), rs.uniform(-0.6, 0.6))

        if i != EMPTY_IMAGE:
            while len(group) < 16:                                      # ordinary: the centre inside the frame
                z = rs.uniform(2.0, 10.0)
                take(at(rs.uniform(0.2 * W, 0.8 * W), rs.uniform(0.2 * H, 0.8 * H), z) + list(rs.uniform(0.1, 0.25, 3) * z), any_rot())
            while len(group) < 26:                                      # across the border
                z = rs.uniform(2.0, 10.0)
                u, v = (rs.choice([0.0, W - 1.0]), rs.uniform(0, H)) if rs.rand() < 0.5 else (rs.uniform(0, W), rs.choice([0.0, H - 1.0]))
                take(at(u, v, z) + list(rs.uniform(0.2, 0.5, 3) * z), any_rot())
            while len(group) < 30:                                      # wholly outside
                z = rs.uniform(2.0, 10.0)
                take(at(rs.choice([-2.0, 3.0]) * W, rs.choice([-2.0, 3.0]) * H, z) + list(rs.uniform(0.1, 0.3, 3) * z), any_rot())
            while len(group) < 34:                                      # wholly behind the camera
                take([rs.uniform(-2, 2), rs.uniform(-2, 2), rs.uniform(-6.0, -2.0)] + list(rs.uniform(0.3, 1.5, 3)), any_rot())
            # 1 .. 7 vertices behind min_z, all vertices in one sign quadrant of (x, y)
            want = {(k, qx, qy) for k in range(1, 8) for qx in (-1, 1) for qy in (-1, 1)} if i in (0, 3) else \
                   {(k, qx, qy) for k in (1 + i % 7, 1 + (i + 3) % 7) for qx in (-1, 1) for qy in (-1, 1)}
            while want:
                qx, qy = rs.choice([-1, 1]), rs.choice([-1, 1])
                box = [qx * rs.uniform(3.0, 6.0), qy * rs.uniform(3.0, 6.0), rs.uniform(-0.8, 1.2)] + list(rs.uniform(0.5, 2.0, 3))
                R = rot(rs.uniform(-np.pi, np.pi), rs.uniform(-1.0, 1.0), rs.uniform(-1.0, 1.0))
                v = verts64(box, R)
                key = (int((v[:, 2] <= MIN_Z).sum()), qx, qy)
                if key in want and (np.sign(v[:, 0]) == qx).all() and (np.sign(v[:, 1]) == qy).all() and take(box, R):
                    want.discard(key)
            if i == FLAT_IMAGE:                                         # width 0, turned so that the flat side faces the camera edge-on
                flat = ([0.0, 0.25, 4.0, 0.0, 1.0, 2.0], np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]]))
                assert unambiguous(*flat)
                group.append(flat)
        counts.append(len(group))
        boxes += [g[0] for g in group]
        rots += [g[1] for g in group]
    return dict(box3d=np.asarray(boxes, np.float32).reshape(-1, 6), R=np.asarray(rots, np.float32).reshape(-1, 9),
                box_off=np.concatenate(([0], np.cumsum(counts))).astype(np.int32), K=np.asarray(Ks, np.float32).reshape(-1, 9),
                size=np.asarray(SIZES, np.int32), min_z=np.float32(MIN_Z), rejected=np.int32(rejected))


def record(inp):
    """the reference's results for the inputs: ref_verts3d / ref_verts2d (N,8,3), ref_proj (N,4) XYXY, ref_behind / ref_fully (N,) bool,
    ref_truncation (N,) float64"""
    from oracle import ref_harness
    ref_harness.install()
    from cubercnn.util import math_util as RM                             # the reference's file
    N = len(inp["box3d"])
    out = dict(ref_verts3d=np.zeros((N, 8, 3), np.float32), ref_verts2d=np.zeros((N, 8, 3), np.float32), ref_proj=np.zeros((N, 4), np.float32),
               ref_behind=np.zeros(N, bool), ref_fully=np.zeros(N, bool), ref_truncation=np.zeros(N, np.float64))
    for i, (W, H) in enumerate(inp["size"].tolist()):
        a, b = int(inp["box_off"][i]), int(inp["box_off"][i + 1])
        if a == b:
            continue
        K = torch.from_numpy(inp["K"][i].reshape(3, 3).copy())
        box, R = torch.from_numpy(inp["box3d"][a:b].copy()), torch.from_numpy(inp["R"][a:b].reshape(-1, 3, 3).copy())
        v2, v3 = RM.get_cuboid_verts(K, box, R)
        out["ref_verts2d"][a:b], out["ref_verts3d"][a:b] = v2.numpy(), v3.numpy()
        p, behind, fully = RM.convert_3d_box_to_2d(K, box, R, W, H, XYWH=False, min_z=float(inp["min_z"]))
        out["ref_proj"][a:b], out["ref_behind"][a:b], out["ref_fully"][a:b] = p.numpy(), behind.numpy(), fully.numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            for n in range(a, b):
                out["ref_truncation"][n] = RM.estimate_truncation(K, box[n - a], R[n - a], W, H)
    return out


def main():
    inp = make_inputs()
    out = record(inp)
    np.savez_compressed(PATH, **inp, **out)
    n_b = out["ref_behind"].sum()
    print("%s: %d boxes over %d images, %d candidates rejected; behind %d, fully behind %d, truncation NaN %d, in (0, 1) %d, == 1 %d, %d bytes"
          % (os.path.relpath(PATH, ROOT), len(inp["box3d"]), len(inp["size"]), int(inp["rejected"]), n_b, out["ref_fully"].sum(),
             np.isnan(out["ref_truncation"]).sum(), ((out["ref_truncation"] > 0) & (out["ref_truncation"] < 1)).sum(),
             (out["ref_truncation"] == 1).sum(), os.path.getsize(PATH)))


if __name__ == "__main__":
    main()
