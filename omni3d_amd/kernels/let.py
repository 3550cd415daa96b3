"""Launchers of csrc/let_iou.hip: the longitudinal-error-tolerant IoU3D of a detection and a ground truth, and the longitudinal
precision along the recall curve (LET-3D-AP / LET-3D-APL, Hung et al. 2022, the camera-only metric of the Waymo Open Dataset).  The
reference has no counterpart; the arguments are checked by `kernels/_args.py`: a box set is the tuple ``(centre, axes, dims, valid)`` of
`iou3d.cuboid_fit`, box 1 = detection (fitted centre P), box 2 = ground truth (fitted centre G), the sensor at the origin.

Of a pair:
  lon   float64  ``(G - P) . u`` with ``u = P / |P|``: the signed longitudinal error, positive when the detection is too near
  aff   float64  ``1 - min(|lon| / T, 1)`` with ``T = max(tol_frac |G|, tol_min)``: the longitudinal affinity in [0, 1]
  iou   float32  the exact IoU3D of the ground truth and the detection moved to ``P + lon u``, the point of its line of sight closest
                 to G, when aff > 0; exactly 0 when aff == 0
(0, 0, NaN) for a gated pair: an invalid box on either side, an index outside its set, or ``|P| <= 1e-8``.
"""
import math

import torch

from .. import lib as _lib
from . import _args
from ._args import empty as _empty      # a name of this module: the tests poison the outputs through it
from .iou3d import check_fit, cuboid_fit

TOL_FRAC, TOL_MIN = 0.1, 0.5       # Waymo's values: a convention, not tuned here


def check_tolerance(tol_frac, tol_min):
    """-> (tol_frac, tol_min) as floats; ValueError unless tol_frac is finite and >= 0 and tol_min finite and > 0"""
    try:
        f, m = float(tol_frac), float(tol_min)
    except (TypeError, ValueError):
        raise ValueError("tol_frac and tol_min must be numbers") from None
    if not (math.isfinite(f) and f >= 0.0):
        raise ValueError("tol_frac must be finite and >= 0")
    if not (math.isfinite(m) and m > 0.0):
        raise ValueError("tol_min must be finite and > 0")
    return f, m


def let_pairs(fit1, fit2, idx1, idx2, tol_frac=TOL_FRAC, tol_min=TOL_MIN):
    """(iou (P,) float32, aff (P,) float64, lon (P,) float64) of fitted detection idx1[p] of fit1 against fitted ground truth idx2[p]
    of fit2 (the tuples of `cuboid_fit`).  idx1 / idx2: 1-D int32 or int64 tensors of equal length.  (0, 0, NaN) for a gated pair;
    NaN never leaves through iou or aff; two calls give the same bits; P == 0 launches nothing.  ValueError on a wrong argument
    before anything is launched."""
    n1, n2 = check_fit(fit1, "fit1"), check_fit(fit2, "fit2")
    tensors = (*fit1, *fit2, idx1, idx2)
    idx1, idx2 = _args.pair_index(idx1, idx2)
    tol_frac, tol_min = check_tolerance(tol_frac, tol_min)
    _args.one_device(tensors)
    L = _lib.check_device(*tensors)
    P = idx1.numel()
    iou, aff, lon = _empty((P,), torch.float32, idx1), _empty((P,), torch.float64, idx1), _empty((P,), torch.float64, idx1)
    if P > 0:
        L.call("omni_let_pairs", *[_lib.ptr(t) for t in fit1], n1, *[_lib.ptr(t) for t in fit2], n2, _lib.ptr(idx1), _lib.ptr(idx2), P,
               tol_frac, tol_min, _lib.ptr(iou), _lib.ptr(aff), _lib.ptr(lon), _lib.stream_of(idx1))
    return iou, aff, lon


def box3d_let(boxes_dt, boxes_gt, tol_frac=TOL_FRAC, tol_min=TOL_MIN):
    """(N,8,3), (M,8,3) float32 corner lists in the order of `boxgen.UNIT` -> (iou, aff, lon), each (N, M), of every pair, both sides
    fitted by `cuboid_fit` with its default eps_dim and fit_tol; the rows and columns of invalid boxes are (0, 0, NaN)."""
    check_tolerance(tol_frac, tol_min)
    fit1, fit2 = cuboid_fit(boxes_dt), cuboid_fit(boxes_gt)
    N, M = boxes_dt.shape[0], boxes_gt.shape[0]
    iou, aff, lon = let_pairs(fit1, fit2, *_args.all_pairs(N, M, boxes_dt.device), tol_frac, tol_min)
    return iou.view(N, M), aff.view(N, M), lon.view(N, M)


def accumulate_let(order, cat_off, rank, dt_match, dt_ignore, pair_row, aff, lon, npig, has_e, rec_thrs, max_dets):
    """The longitudinal precision along the recall curve, one wave per (category, depth range, maxDets, threshold) ->
    (precision_l (T, R, K, A, M), tp_affinity (T, K, A, M), tp_lon (T, K, A, M)), all float64.

    order (N,) int32 / cat_off (K+1,) int32 / rank (sumD,) int32: the merge order of `Omni3Deval.accumulate` (detections by category,
    descending score) and the rank of a detection inside its (image, category) list; dt_match (A, T, sumD) int32 / dt_ignore
    (A, T, sumD) uint8: the tables of `evaluate_groups`; pair_row (sumD,) int64: the row of `aff` / `lon` (P,) float64 of the pair
    (detection, ground truth 0 of its group); npig (K, A) int32 the number of non-ignored ground truths, has_e (K,) int32, rec_thrs
    (R,) float64 ascending, max_dets (M,) int32.
    A detection with rank < max_dets[m] is included; one with dt_match >= 0 and dt_ignore == 0 is a true positive, its pair is row
    pair_row[d] + dt_match[a, t, d].  At a list position prec_L = (sum of aff over the true positives so far) / (tp + fp + eps);
    precision_l is prec_L made monotone from the right and sampled at rec_thrs as `precision` is, -1 in the same cells (npig == 0 or
    has_e == 0); tp_affinity / tp_lon are the means of aff / lon over the true positives, -1 without one.  Two calls give the same
    bits."""
    K, A, T, R, sumD, _ = _args.merge_order(order, cat_off, dt_match, dt_ignore, rec_thrs)
    _args.tensor(rank, "rank", torch.int32, (sumD,))
    _args.tensor(pair_row, "pair_row", torch.int64, (sumD,))
    P = _args.tensor(aff, "aff", torch.float64, (None,))[0]
    _args.tensor(lon, "lon", torch.float64, (P,))
    _args.tensor(npig, "npig", torch.int32, (K, A))
    _args.tensor(has_e, "has_e", torch.int32, (K,))
    M = _args.nonempty(max_dets, "max_dets", torch.int32)
    tensors = (order, cat_off, rank, dt_match, dt_ignore, pair_row, aff, lon, npig, has_e, rec_thrs, max_dets)
    _args.one_device(tensors)
    L = _lib.check_device(*tensors)
    dev = order.device
    prec_l = torch.full((T, R, K, A, M), -1.0, dtype=torch.float64, device=dev)
    tp_aff = torch.full((T, K, A, M), -1.0, dtype=torch.float64, device=dev)
    tp_lon = torch.full((T, K, A, M), -1.0, dtype=torch.float64, device=dev)
    if K > 0:
        L.call("omni_eval_accumulate_let", _lib.ptr(order), _lib.ptr(cat_off), _lib.ptr(rank), _lib.ptr(dt_match), _lib.ptr(dt_ignore),
               _lib.ptr(pair_row), _lib.ptr(aff), _lib.ptr(lon), P, _lib.ptr(npig), _lib.ptr(has_e), _lib.ptr(rec_thrs), _lib.ptr(max_dets),
               K, A, M, T, R, sumD, _lib.ptr(prec_l), _lib.ptr(tp_aff), _lib.ptr(tp_lon), _lib.stream_of(order))
    return prec_l, tp_aff, tp_lon
