"""Launchers of csrc/bev_iou.hip: the IoU of cuboids in the bird's-eye view, i.e. of their footprints on the ground plane (the
matching criterion of AP-BEV).  The reference has no counterpart; the interface follows `kernels/iou3d.py`:
``bev_overlap(boxes_dt, boxes_gt) -> ious`` next to ``box3d_overlap``.

A footprint set is the tuple ``(poly (N,8,2) float32, count (N,) int32, area (N,) float32)`` of `bev_footprints`: the convex hull of
the eight corners projected along `up`, counter-clockwise, `count` 0 for an invalid box (a non-finite vertex or area <= eps_area).
"""
import numpy as np
import torch

from .. import lib as _lib
from .iou3d import _check_boxes

UP = (0.0, -1.0, 0.0)              # camera y points down


def _empty(shape, dtype, like):
    return torch.empty(shape, dtype=dtype, device=like.device)


def plane_basis(up=UP):
    """The fixed rule that turns an up vector into the orthonormal basis (e1, e2) of the ground plane, in float64: e1 is the
    coordinate axis x (z when `up` is within 45 degrees of x) minus its part along `up`, normalised; e2 = up x e1.
    up = (0, -1, 0) gives exactly e1 = (1, 0, 0), e2 = (0, 0, 1).  The IoU does not depend on this choice."""
    u = np.asarray(up, dtype=np.float64).reshape(-1)
    if u.shape != (3,) or not np.isfinite(u).all() or not np.linalg.norm(u) > 0:
        raise ValueError("up must be three finite numbers, not all zero")
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
    if not isinstance(boxes, torch.Tensor):
        raise ValueError("boxes must be a tensor")
    _check_boxes(boxes, "boxes")
    if not boxes.is_contiguous():
        raise ValueError("boxes must be contiguous")
    if not float(eps_area) >= 0.0:
        raise ValueError("eps_area must be >= 0")
    if counts is not None and (counts.dtype != torch.int32 or counts.numel() != 1 or counts.device != boxes.device):
        raise ValueError("counts must be one int32 on the boxes' device")
    e1, e2 = plane_basis(up)
    L = _lib.check_device(boxes, counts)
    N = boxes.shape[0]
    poly, count, area = _empty((N, 8, 2), torch.float32, boxes), _empty((N,), torch.int32, boxes), _empty((N,), torch.float32, boxes)
    if N > 0:
        L.call("omni_bev_footprint", _lib.ptr(boxes), N, *[float(v) for v in e1], *[float(v) for v in e2], float(eps_area),
               _lib.ptr(poly), _lib.ptr(count), _lib.ptr(area), _lib.ptr(counts), _lib.stream_of(boxes))
    return poly, count, area


def _check_footprints(fp, name):
    if not isinstance(fp, (tuple, list)) or len(fp) != 3 or not all(isinstance(t, torch.Tensor) for t in fp):
        raise ValueError(f"{name} must be the (poly, count, area) of bev_footprints")
    poly, count, area = fp
    n = poly.shape[0] if poly.dim() else -1
    if poly.shape != (n, 8, 2) or poly.dtype != torch.float32:
        raise ValueError(f"{name}: poly must be float32 of shape (N, 8, 2), got {tuple(poly.shape)}")
    if count.shape != (n,) or count.dtype != torch.int32:
        raise ValueError(f"{name}: count must be int32 of shape ({n},)")
    if area.shape != (n,) or area.dtype != torch.float32:
        raise ValueError(f"{name}: area must be float32 of shape ({n},)")
    if not all(t.is_contiguous() for t in fp):
        raise ValueError(f"{name} must be contiguous")
    return n


def bev_iou_pairs(fp1, fp2, idx1, idx2):
    """iou[p] = BEV IoU of footprint idx1[p] of fp1 and footprint idx2[p] of fp2 -> (P,) float32.  idx1 / idx2: 1-D integer tensors
    of equal length (int32 on the device; other integer types are converted).  Exactly 0 for a pair with an invalid footprint or
    with disjoint bounding rectangles; two calls give the same bits; P == 0 launches nothing."""
    n1, n2 = _check_footprints(fp1, "fp1"), _check_footprints(fp2, "fp2")
    for i in (idx1, idx2):
        if not isinstance(i, torch.Tensor) or i.dim() != 1 or i.dtype not in (torch.int32, torch.int64):
            raise ValueError("idx1 / idx2 must be 1-D int32 or int64 tensors")
    if idx1.shape != idx2.shape:
        raise ValueError("idx1 / idx2 must be of equal length")
    tensors = (*fp1, *fp2, idx1, idx2)
    if len({t.device for t in tensors}) != 1:
        raise ValueError("all inputs must live on one device")
    idx1, idx2 = idx1.to(torch.int32).contiguous(), idx2.to(torch.int32).contiguous()
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
    N, M, dev = boxes_dt.shape[0], boxes_gt.shape[0], boxes_dt.device
    idx1 = torch.arange(N, dtype=torch.int32, device=dev).repeat_interleave(M)
    idx2 = torch.arange(M, dtype=torch.int32, device=dev).repeat(N)
    return bev_iou_pairs(fp1, fp2, idx1, idx2).view(N, M)
