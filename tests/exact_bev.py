"""The bird's-eye-view IoU of two cuboids written from its definition, in the floating-point type given (float64 = the reference
of tests/test_bev_iou.py and tests/test_bev_eval.py; float32 = the same steps in the kernels' precision, to show without any kernel
that the inputs sit well inside the tolerance).

Footprint: the convex hull (Andrew's monotone chain, pop while cross <= 0, so duplicate and collinear points go) of the eight
corners' coordinates (v.e1, v.e2) in the plane orthogonal to the up vector, counter-clockwise; its area by the shoelace formula
relative to its own first vertex.  A box is invalid when a vertex is not finite or the area is <= eps_area.
IoU: 0 for a pair with an invalid box or with disjoint bounding rectangles; otherwise both polygons are moved to the first vertex of
the first one (the local origin), the first is clipped by every edge of the second (Sutherland-Hodgman), the shoelace area of the
result is taken and IoU = inter / (a1 + a2 - inter), clamped to [0, 1].  `local_origin=False` skips the move (to measure what it buys).
"""
import numpy as np

from omni3d_amd.kernels.bev import plane_basis

UP = (0.0, -1.0, 0.0)


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def _shoelace(pts, T):
    """area of a counter-clockwise polygon relative to its own first vertex"""
    s = T(0)
    for i in range(1, len(pts) - 1):
        s = s + _cross(pts[0], pts[i], pts[i + 1])
    return T(0.5) * s


def footprint(box, up=UP, eps_area=1e-8, dtype=np.float64):
    """box (8,3) -> (hull: list of (x, y) of `dtype`, counter-clockwise; area).  ([], 0) for an invalid box."""
    T = dtype
    box = np.asarray(box)
    if not np.isfinite(box).all():
        return [], T(0)
    e1, e2 = plane_basis(up)
    b, e1, e2 = box.astype(T), e1.astype(T), e2.astype(T)
    pts = sorted({(T(v[0] * e1[0] + v[1] * e1[1] + v[2] * e1[2]), T(v[0] * e2[0] + v[1] * e2[1] + v[2] * e2[2])) for v in b})
    if len(pts) < 3:
        return [], T(0)
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and _cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and _cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    hull = lower[:-1] + upper[:-1]
    if len(hull) < 3:
        return [], T(0)
    area = _shoelace(hull, T)
    if not (np.isfinite(area) and area > T(eps_area)):
        return [], T(0)
    return hull, area


def _clip(subject, a, b, T):
    """the part of the polygon `subject` on the left of the directed line a -> b"""
    dx, dy = b[0] - a[0], b[1] - a[1]
    out = []
    q = subject[-1]
    dq = dx * (q[1] - a[1]) - dy * (q[0] - a[0])
    for c in subject:
        dc = dx * (c[1] - a[1]) - dy * (c[0] - a[0])
        if (dc >= 0) != (dq >= 0):
            s = dq / (dq - dc)
            out.append((q[0] + s * (c[0] - q[0]), q[1] + s * (c[1] - q[1])))
        if dc >= 0:
            out.append(c)
        q, dq = c, dc
    return out


def iou_footprints(fp1, fp2, dtype=np.float64, local_origin=True):
    """(hull, area) x (hull, area) -> IoU as a `dtype` scalar"""
    T = dtype
    (P, a1), (Q, a2) = fp1, fp2
    if not P or not Q:
        return T(0)
    if (max(p[0] for p in P) < min(q[0] for q in Q) or max(q[0] for q in Q) < min(p[0] for p in P)
            or max(p[1] for p in P) < min(q[1] for q in Q) or max(q[1] for q in Q) < min(p[1] for p in P)):
        return T(0)
    o = P[0] if local_origin else (T(0), T(0))
    P = [(p[0] - o[0], p[1] - o[1]) for p in P]
    Q = [(q[0] - o[0], q[1] - o[1]) for q in Q]
    for j in range(len(Q)):
        P = _clip(P, Q[j - 1], Q[j], T)
        if not P:
            break
    inter = max(_shoelace(P, T), T(0)) if len(P) >= 3 else T(0)
    union = a1 + a2 - inter
    r = inter / union if union > 0 else T(0)
    return min(max(r, T(0)), T(1))


def bev_iou(box1, box2, up=UP, eps_area=1e-8, dtype=np.float64, local_origin=True):
    return iou_footprints(footprint(box1, up, eps_area, dtype), footprint(box2, up, eps_area, dtype), dtype, local_origin)


def footprints(boxes, up=UP, eps_area=1e-8, dtype=np.float64):
    return [footprint(b, up, eps_area, dtype) for b in boxes]


def bev_iou_pairs(fps1, fps2, idx1, idx2, dtype=np.float64, local_origin=True):
    return np.array([iou_footprints(fps1[i], fps2[j], dtype, local_origin) for i, j in zip(idx1, idx2)], dtype=dtype)
