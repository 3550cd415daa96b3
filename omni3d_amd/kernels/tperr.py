"""Launchers of csrc/tp_errors.hip: the translation, scale and orientation error of a pair of cuboids, and their averages along the
recall curve (the ATE / ASE / AOE of the nuScenes protocol).  The reference has no counterpart; a box set is the tuple
``(centre, axes, dims, valid)`` of `iou3d.cuboid_fit`, and the arguments are checked by `kernels/_args.py`.

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
from . import _args
from ._args import empty as _empty      # a name of this module: the tests poison the outputs through it
from .iou3d import check_fit, cuboid_fit


def unit_up(up):
    """None -> (0, 0, 0), the full 3D distance; three finite numbers, not all zero -> the unit vector along them, in float64"""
    if up is None:
        return (0.0, 0.0, 0.0)
    u = _args.up_vector(up)
    u = u / np.linalg.norm(u)
    return tuple(float(v) for v in u)


def pair_errors(fit1, fit2, idx1, idx2, up=None):
    """err (P, 3) float64 = (trans, scale, orient) of fitted cuboid idx1[p] of fit1 against idx2[p] of fit2 (the tuples of
    `cuboid_fit`).  idx1 / idx2: 1-D int32 or int64 tensors of equal length.  (+inf, NaN, NaN) for a pair with an invalid box or an
    index outside its set; two calls give the same bits; P == 0 launches nothing.  ValueError on a wrong argument before anything is
    launched."""
    n1, n2 = check_fit(fit1, "fit1"), check_fit(fit2, "fit2")
    tensors = (*fit1, *fit2, idx1, idx2)
    idx1, idx2 = _args.pair_index(idx1, idx2)
    u = unit_up(up)
    _args.one_device(tensors)
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
    N, M = boxes_dt.shape[0], boxes_gt.shape[0]
    return pair_errors(fit1, fit2, *_args.all_pairs(N, M, boxes_dt.device), up).view(N, M, 3)


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
    K, A, _, R, sumD, _ = _args.merge_order(order, cat_off, dt_match, dt_ignore, rec_thrs, per_threshold=False)
    _args.tensor(pair_row, "pair_row", torch.int64, (sumD,))
    P = _args.tensor(err, "err", torch.float64, (None, 3))[0]
    _args.tensor(npig, "npig", torch.int32, (K, A))
    _args.tensor(has_e, "has_e", torch.int32, (K,))
    if not 0.0 <= float(min_recall) <= 1.0:
        raise ValueError("min_recall must lie in [0, 1]")
    tensors = (order, cat_off, dt_match, dt_ignore, pair_row, err, npig, has_e, rec_thrs)
    _args.one_device(tensors)
    L = _lib.check_device(*tensors)
    tp_err = torch.full((K, A, 3), -1.0, dtype=torch.float64, device=order.device)
    tp_count = torch.zeros((K, A), dtype=torch.int32, device=order.device)
    if K > 0:
        L.call("omni_eval_tp_errors", _lib.ptr(order), _lib.ptr(cat_off), _lib.ptr(dt_match), _lib.ptr(dt_ignore), _lib.ptr(pair_row),
               _lib.ptr(err), P, _lib.ptr(npig), _lib.ptr(has_e), _lib.ptr(rec_thrs), float(min_recall), K, A, R, sumD,
               _lib.ptr(tp_err), _lib.ptr(tp_count), _lib.stream_of(order))
    return tp_err, tp_count
