"""Launchers of csrc/tp_errors.hip: the translation, scale and orientation error of a pair of cuboids, and their averages along the
recall curve (the ATE / ASE / AOE of the nuScenes protocol).  The reference has no counterpart; the interface follows
`kernels/iou3d.py`: a box set is the tuple ``(centre, axes, dims, valid)`` of `iou3d.cuboid_fit`.

Errors of a pair (box 1 = detection, box 2 = ground truth), all float64:
  trans   the Euclidean distance of the fitted centres; with a unit vector `up`, the distance in the ground plane orthogonal to it,
          ``sqrt(max(0, |d|^2 - (d.up)^2))`` (nuScenes' definition; ``up = (0, -1, 0)`` for level outdoor cameras)
  scale   ``1 - inter / (V1 + V2 - inter)``, ``inter = prod_k min(dims1[k], dims2[k])``: one minus the IoU of the two boxes after
          aligning centre and orientation; axis k is paired with axis k
  orient  the geodesic angle of ``R = R1 R2^T`` (the fitted axes as columns), in [0, pi] radians, by
          ``atan2(0.5 |(R32-R23, R13-R31, R21-R12)|, 0.5 (trace R - 1))``.  No symmetry folding: the same solid with its corners
          listed from the opposite side scores pi (nuScenes scores yaw with period 2 pi; here it is the full rotation).
"""
import numpy as np
import torch

from .. import lib as _lib
from .iou3d import _check_fit, cuboid_fit


def _empty(shape, dtype, like):
    return torch.empty(shape, dtype=dtype, device=like.device)


def unit_up(up):
    """None -> (0, 0, 0), the full 3D distance; three finite numbers, not all zero -> the unit vector along them, in float64"""
    if up is None:
        return (0.0, 0.0, 0.0)
    u = np.asarray(up, dtype=np.float64).reshape(-1)
    if u.shape != (3,) or not np.isfinite(u).all() or not np.linalg.norm(u) > 0:
        raise ValueError("up must be None or three finite numbers, not all zero")
    u = u / np.linalg.norm(u)
    return tuple(float(v) for v in u)


def pair_errors(fit1, fit2, idx1, idx2, up=None):
    """err (P, 3) float64 = (trans, scale, orient) of fitted cuboid idx1[p] of fit1 against idx2[p] of fit2 (the tuples of
    `cuboid_fit`).  idx1 / idx2: 1-D int32 or int64 tensors of equal length.  (+inf, NaN, NaN) for a pair with an invalid box or an
    index outside its set; two calls give the same bits; P == 0 launches nothing.  ValueError on a wrong argument before anything is
    launched."""
    n1, n2 = _check_fit(fit1, "fit1"), _check_fit(fit2, "fit2")
    for i in (idx1, idx2):
        if not isinstance(i, torch.Tensor) or i.dim() != 1 or i.dtype not in (torch.int32, torch.int64):
            raise ValueError("idx1 / idx2 must be 1-D int32 or int64 tensors")
    if idx1.shape != idx2.shape:
        raise ValueError("idx1 / idx2 must be of equal length")
    u = unit_up(up)
    tensors = (*fit1, *fit2, idx1, idx2)
    if len({t.device for t in tensors}) != 1:
        raise ValueError("all inputs must live on one device")
    idx1, idx2 = idx1.to(torch.int32).contiguous(), idx2.to(torch.int32).contiguous()
    L = _lib.check_device(*tensors)
    P = idx1.numel()
    err = _empty((P, 3), torch.float64, idx1)
    if P > 0:
        L.call("omni_pair_errors", *[_lib.ptr(t) for t in fit1], n1, *[_lib.ptr(t) for t in fit2], n2, _lib.ptr(idx1), _lib.ptr(idx2), P,
               *u, _lib.ptr(err), _lib.stream_of(idx1))
    return err


def box3d_errors(boxes_dt, boxes_gt, up=None):
    """(N,8,3), (M,8,3) float32 corner lists in the order of `boxgen.UNIT` -> (N, M, 3) float64 errors of every pair, both sides fitted
    by `cuboid_fit` with its default eps_dim and fit_tol; the rows and columns of invalid boxes are (+inf, NaN, NaN)."""
    fit1, fit2 = cuboid_fit(boxes_dt), cuboid_fit(boxes_gt)
    N, M, dev = boxes_dt.shape[0], boxes_gt.shape[0], boxes_dt.device
    idx1 = torch.arange(N, dtype=torch.int32, device=dev).repeat_interleave(M)
    idx2 = torch.arange(M, dtype=torch.int32, device=dev).repeat(N)
    return pair_errors(fit1, fit2, idx1, idx2, up).view(N, M, 3)


def _check(t, name, dtype, shape):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be a {dtype} tensor of shape {tuple(shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def tp_errors(order, cat_off, dt_match, dt_ignore, pair_row, err, npig, has_e, rec_thrs, min_recall=0.1):
    """The true-positive errors along the recall curve, one wave per (category, depth range) -> (tp_err (K, A, 3) float64,
    tp_count (K, A) int32).

    order (N,) int32 / cat_off (K+1,) int32: the merge order of `Omni3Deval.accumulate` (detections by category, descending score);
    dt_match (A, sumD) int32 / dt_ignore (A, sumD) uint8: the tables of `evaluate_groups` at one threshold; pair_row (sumD,) int64:
    the row of `err` (P, 3) float64 of the pair (detection, ground truth 0 of its group); npig (K, A) int32 the number of non-ignored
    ground truths, has_e (K,) int32, rec_thrs (R,) float64 ascending.
    A detection with dt_match >= 0 and dt_ignore == 0 is a true positive; at the c-th one m_c is the mean of each error over the first
    c; the threshold r_j takes m_c when r_j >= min_recall and (c-1)/npig < r_j <= c/npig; tp_err is the mean of the values taken: -1
    where npig == 0 or has_e == 0, 1.0 where ground truths exist but no threshold took a value.  Two calls give the same bits."""
    _check(cat_off, "cat_off", torch.int32, (cat_off.numel() if isinstance(cat_off, torch.Tensor) else 0,))
    K = cat_off.numel() - 1
    if K < 0:
        raise ValueError("cat_off must hold K + 1 offsets")
    _check(order, "order", torch.int32, (order.numel() if isinstance(order, torch.Tensor) else 0,))
    if not isinstance(dt_match, torch.Tensor) or dt_match.dim() != 2 or dt_match.shape[0] < 1:
        raise ValueError("dt_match must have shape (A, sumD) with A >= 1")
    A, sumD = dt_match.shape
    _check(dt_match, "dt_match", torch.int32, (A, sumD))
    _check(dt_ignore, "dt_ignore", torch.uint8, (A, sumD))
    _check(pair_row, "pair_row", torch.int64, (sumD,))
    if not isinstance(err, torch.Tensor) or err.dim() != 2:
        raise ValueError("err must have shape (P, 3)")
    _check(err, "err", torch.float64, (err.shape[0], 3))
    _check(npig, "npig", torch.int32, (K, A))
    _check(has_e, "has_e", torch.int32, (K,))
    if not isinstance(rec_thrs, torch.Tensor) or rec_thrs.dim() != 1 or rec_thrs.numel() < 1:
        raise ValueError("rec_thrs must be 1-D and not empty")
    _check(rec_thrs, "rec_thrs", torch.float64, (rec_thrs.numel(),))
    if not 0.0 <= float(min_recall) <= 1.0:
        raise ValueError("min_recall must lie in [0, 1]")
    tensors = (order, cat_off, dt_match, dt_ignore, pair_row, err, npig, has_e, rec_thrs)
    if len({t.device for t in tensors}) != 1:
        raise ValueError("all inputs must live on one device")
    off = cat_off.tolist()
    if off[0] != 0 or off[-1] != order.numel() or any(b < a for a, b in zip(off, off[1:])):
        raise ValueError("cat_off must ascend from 0 to len(order)")
    L = _lib.check_device(*tensors)
    tp_err = torch.full((K, A, 3), -1.0, dtype=torch.float64, device=order.device)
    tp_count = torch.zeros((K, A), dtype=torch.int32, device=order.device)
    if K > 0:
        L.call("omni_eval_tp_errors", _lib.ptr(order), _lib.ptr(cat_off), _lib.ptr(dt_match), _lib.ptr(dt_ignore), _lib.ptr(pair_row),
               _lib.ptr(err), err.shape[0], _lib.ptr(npig), _lib.ptr(has_e), _lib.ptr(rec_thrs), float(min_recall), K, A, rec_thrs.numel(),
               sumD, _lib.ptr(tp_err), _lib.ptr(tp_count), _lib.stream_of(order))
    return tp_err, tp_count
