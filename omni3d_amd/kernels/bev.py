"""Launchers of csrc/bev_iou.hip: the IoU of cuboids in the bird's-eye view, i.e. of their footprints on the ground plane (the
matching criterion of AP-BEV).  The reference has no counterpart: ``bev_overlap(boxes_dt, boxes_gt) -> ious`` stands next to
``iou3d.box3d_overlap``, and the arguments are checked by `kernels/_args.py`.

A footprint set is the tuple ``(poly (N,8,2) float32, count (N,) int32, area (N,) float32)`` of `bev_footprints`: the convex hull of
the eight corners projected along `up`, counter-clockwise, `count` 0 for an invalid box (a non-finite vertex or area <= eps_area).
"""
import numpy as np
import torch

from .. import lib as _lib
from . import _args
from ._args import empty as _empty      # a name of this module: the tests poison the outputs through it

UP = (0.0, -1.0, 0.0)              # camera y points down


def plane_basis(up=UP):
    """The fixed rule that turns an up vector into the orthonormal basis (e1, e2) of the ground plane, in float64: e1 is the
    coordinate axis x (z when `up` is within 45 degrees of x) minus its part along `up`, normalised; e2 = up x e1.
    up = (0, -1, 0) gives exactly e1 = (1, 0, 0), e2 = (0, 0, 1).  The IoU does not depend on this choice."""
    u = _args.up_vector(up)
    u = u / np.linalg.norm(u)
    a = np.array([0.0, 0.0, 1.0]) if abs(u[0]) > np.sqrt(0.5) else np.array([1.0, 0.0, 0.0])
    e1 = a - np.dot(a, u) * u
    e1 = e1 / np.linalg.norm(e1)
    e2 = np.cross(u, e1)
    return e1 + 0.0, e2 + 0.0           # + 0.0: no negative zeros


def bev_footprints(boxes, up=UP, eps_area=1e-8, counts=None):
    """boxes (N,8,3) float32 contiguous corner lists (any corner order) -> (poly (N,8,2), count (N,) int32, area (N,)).
    counts: optional int32 (1,) tensor the number of invalid boxes is added to.  ValueError on a wrong shape / dtype / stride /
    argument before anything is launched; N == 0 launches nothing."""
    N = _args.corners(boxes, "boxes")
    if not float(eps_area) >= 0.0:
        raise ValueError("eps_area must be >= 0")
    _args.counter(counts, boxes)
    e1, e2 = plane_basis(up)
    L = _lib.check_device(boxes, counts)
    poly, count, area = _empty((N, 8, 2), torch.float32, boxes), _empty((N,), torch.int32, boxes), _empty((N,), torch.float32, boxes)
    if N > 0:
        L.call("omni_bev_footprint", _lib.ptr(boxes), N, *[float(v) for v in e1], *[float(v) for v in e2], float(eps_area),
               _lib.ptr(poly), _lib.ptr(count), _lib.ptr(area), _lib.ptr(counts), _lib.stream_of(boxes))
    return poly, count, area


FOOTPRINTS = (("poly", torch.float32, (8, 2)), ("count", torch.int32, ()), ("area", torch.float32, ()))


def bev_iou_pairs(fp1, fp2, idx1, idx2):
    """iou[p] = BEV IoU of footprint idx1[p] of fp1 and footprint idx2[p] of fp2 -> (P,) float32.  idx1 / idx2: 1-D integer tensors
    of equal length (int32 on the device; other integer types are converted).  Exactly 0 for a pair with an invalid footprint or
    with disjoint bounding rectangles; two calls give the same bits; P == 0 launches nothing."""
    n1, n2 = (_args.box_set(fp, name, "bev_footprints", FOOTPRINTS) for fp, name in ((fp1, "fp1"), (fp2, "fp2")))
    tensors = (*fp1, *fp2, idx1, idx2)
    idx1, idx2 = _args.pair_index(idx1, idx2)
    _args.one_device(tensors)
    L = _lib.check_device(*tensors)
    P = idx1.numel()
    iou = _empty((P,), torch.float32, idx1)
    if P > 0:
        L.call("omni_bev_iou_pairs", *[_lib.ptr(t) for t in fp1], n1, *[_lib.ptr(t) for t in fp2], n2, _lib.ptr(idx1), _lib.ptr(idx2), P,
               _lib.ptr(iou), _lib.stream_of(idx1))
    return iou


def bev_overlap(boxes_dt, boxes_gt, up=UP, eps_area=1e-8):
    """(N,8,3), (M,8,3) corner lists -> (N,M) BEV IoU; the rows and columns of invalid boxes are 0."""
    fp1, fp2 = bev_footprints(boxes_dt, up, eps_area), bev_footprints(boxes_gt, up, eps_area)
    N, M = boxes_dt.shape[0], boxes_gt.shape[0]
    return bev_iou_pairs(fp1, fp2, *_args.all_pairs(N, M, boxes_dt.device)).view(N, M)
