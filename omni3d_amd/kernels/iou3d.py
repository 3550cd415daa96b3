"""IoU3D launchers.  Mirrors the reference interface
``box3d_overlap(boxes_dt, boxes_gt, eps_coplanar=1e-4, eps_nonzero=1e-8) -> ious``
(/root/reference/cubercnn/evaluation/omni3d_evaluation.py:106-166) and pytorch3d's
``_C.iou_box3d(boxes1, boxes2) -> (vol, iou)`` (call site omni3d_evaluation.py:155).
"""
import torch

from .. import lib as _lib
from . import _args
from ._args import empty as _empty      # a name of this module: the tests poison the outputs through it


def _check_boxes(b, name):
    if b.dim() != 3 or b.shape[1] != 8 or b.shape[2] != 3:
        raise ValueError(f"{name} must have shape (B, 8, 3), got {tuple(b.shape)}")
    if b.dtype != torch.float32:
        raise ValueError(f"{name} must be float32")


def iou_box3d(boxes1, boxes2, valid1=None):
    """(N,8,3),(M,8,3) -> (vol (N,M), iou (N,M)); optional int32 mask of valid rows."""
    _check_boxes(boxes1, "boxes1")
    _check_boxes(boxes2, "boxes2")
    boxes1, boxes2 = boxes1.contiguous(), boxes2.contiguous()
    L = _lib.check_device(boxes1, boxes2, valid1)
    N, M = boxes1.shape[0], boxes2.shape[0]
    vol = torch.empty((N, M), dtype=torch.float32, device=boxes1.device)
    iou = torch.empty((N, M), dtype=torch.float32, device=boxes1.device)
    overflow = torch.zeros(1, dtype=torch.int32, device=boxes1.device)
    L.call("omni_iou_box3d", _lib.ptr(boxes1), N, _lib.ptr(boxes2), M, _lib.ptr(valid1), _lib.ptr(vol), _lib.ptr(iou),
           _lib.ptr(overflow), _lib.stream_of(boxes1))
    return vol, iou


def iou_box3d_pairs(boxes1, boxes2, idx1, idx2, valid1=None, lanes_per_pair=0):
    """Ragged / paired form: iou[p] = IoU3D(boxes1[idx1[p]], boxes2[idx2[p]]).  lanes_per_pair: launch variant of
    omni_iou_box3d_pairs_algo (64 / 32 / 16 lanes per pair, + 1000 = small LDS lists with a retry pass; 0 = production choice);
    every variant gives the same result."""
    _check_boxes(boxes1, "boxes1")
    _check_boxes(boxes2, "boxes2")
    boxes1, boxes2 = boxes1.contiguous(), boxes2.contiguous()
    idx1 = idx1.to(torch.int32).contiguous()
    idx2 = idx2.to(torch.int32).contiguous()
    if idx1.shape != idx2.shape or idx1.dim() != 1:
        raise ValueError("idx1/idx2 must be 1-D and of equal length")
    L = _lib.check_device(boxes1, boxes2, idx1, idx2, valid1)
    P = idx1.numel()
    vol = torch.empty(P, dtype=torch.float32, device=boxes1.device)
    iou = torch.empty(P, dtype=torch.float32, device=boxes1.device)
    overflow = torch.zeros(1, dtype=torch.int32, device=boxes1.device)
    if lanes_per_pair:
        L.call("omni_iou_box3d_pairs_algo", _lib.ptr(boxes1), _lib.ptr(boxes2), _lib.ptr(idx1), _lib.ptr(idx2), P,
               _lib.ptr(valid1), _lib.ptr(vol), _lib.ptr(iou), _lib.ptr(overflow), int(lanes_per_pair), _lib.stream_of(boxes1))
    else:
        L.call("omni_iou_box3d_pairs", _lib.ptr(boxes1), _lib.ptr(boxes2), _lib.ptr(idx1), _lib.ptr(idx2), P,
               _lib.ptr(valid1), _lib.ptr(vol), _lib.ptr(iou), _lib.ptr(overflow), _lib.stream_of(boxes1))
    return vol, iou


def box3d_validity(boxes, eps_coplanar=1e-4, eps_nonzero=1e-8):
    """-> (valid int32 (N,), counts int32 (2,) = [#non-coplanar, #zero-area])."""
    _check_boxes(boxes, "boxes")
    boxes = boxes.contiguous()
    L = _lib.check_device(boxes)
    N = boxes.shape[0]
    valid = torch.empty(N, dtype=torch.int32, device=boxes.device)
    counts = torch.zeros(2, dtype=torch.int32, device=boxes.device)
    L.call("omni_box3d_validity", _lib.ptr(boxes), N, float(eps_coplanar), float(eps_nonzero), _lib.ptr(valid),
           _lib.ptr(counts), _lib.stream_of(boxes))
    return valid, counts


def box3d_overlap(boxes_dt, boxes_gt, eps_coplanar=1e-4, eps_nonzero=1e-8, warn=True):
    """Drop-in for the reference's ``box3d_overlap``: (N,8,3),(M,8,3) -> iou (N,M) with the rows
    of non-coplanar / zero-area detection boxes zeroed (and the same warnings printed)."""
    valid, counts = box3d_validity(boxes_dt, eps_coplanar, eps_nonzero)
    _, iou = iou_box3d(boxes_dt, boxes_gt, valid1=valid)
    if warn:
        c = counts.tolist()
        if c[0] > 0:
            print('Warning: skipping {:d} non-coplanar boxes at eval.'.format(int(c[0])))
        if c[1] > 0:
            print('Warning: skipping {:d} zero volume boxes at eval.'.format(int(c[1])))
    return iou


# ---- exact geometry (csrc/cuboid_exact.h, csrc/iou3d_exact.hip) --------------------------------------------------------------------

def cuboid_fit(boxes, eps_dim=1e-8, fit_tol=1e-3, counts=None):
    """boxes (N,8,3) float32 contiguous corner lists in the order of `boxgen.UNIT` -> the fitted cuboids ``(centre (N,3), axes (N,3,3),
    dims (N,3), valid (N,) int32)``, the first three float64: centre = vertex mean, axes[n, k] = unit axis k (mean of the four parallel
    edges, orthonormalised), dims = the norms of the mean edges.  A box is invalid (valid 0, the rest 0) when a vertex is not finite, a
    dimension is <= eps_dim, or a vertex lies further than fit_tol x the largest dimension from its fitted corner.  counts: optional
    int32 (1,) tensor the number of invalid boxes is added to.  ValueError on a wrong shape / dtype / stride / argument before
    anything is launched; N == 0 launches nothing."""
    N = _args.corners(boxes, "boxes")
    if not float(eps_dim) >= 0.0 or not float(fit_tol) >= 0.0 or float(eps_dim) == float("inf") or float(fit_tol) == float("inf"):
        raise ValueError("eps_dim and fit_tol must be finite and >= 0")
    _args.counter(counts, boxes)
    L = _lib.check_device(boxes, counts)
    centre, axes, dims = _empty((N, 3), torch.float64, boxes), _empty((N, 3, 3), torch.float64, boxes), _empty((N, 3), torch.float64, boxes)
    valid = _empty((N,), torch.int32, boxes)
    if N > 0:
        L.call("omni_cuboid_fit", _lib.ptr(boxes), N, float(eps_dim), float(fit_tol), _lib.ptr(centre), _lib.ptr(axes), _lib.ptr(dims),
               _lib.ptr(valid), _lib.ptr(counts), _lib.stream_of(boxes))
    return centre, axes, dims, valid


FIT = (("centre", torch.float64, (3,)), ("axes", torch.float64, (3, 3)), ("dims", torch.float64, (3,)), ("valid", torch.int32, ()))


def check_fit(fit, name):
    """fit is the tuple of `cuboid_fit`, contiguous -> its number of boxes; ValueError otherwise"""
    return _args.box_set(fit, name, "cuboid_fit", FIT)


def iou_fitted_pairs(fit1, fit2, idx1, idx2):
    """(vol, iou), each (P,) float32: the exact intersection volume and IoU3D of fitted cuboid idx1[p] of fit1 and idx2[p] of fit2
    (the tuples of `cuboid_fit`).  idx1 / idx2: 1-D int32 or int64 tensors of equal length.  Exactly 0 for a pair with an invalid box,
    an index outside its set or disjoint bounding spheres; never NaN; two calls give the same bits; P == 0 launches nothing."""
    n1, n2 = check_fit(fit1, "fit1"), check_fit(fit2, "fit2")
    tensors = (*fit1, *fit2, idx1, idx2)
    idx1, idx2 = _args.pair_index(idx1, idx2)
    _args.one_device(tensors)
    L = _lib.check_device(*tensors)
    P = idx1.numel()
    vol, iou = _empty((P,), torch.float32, idx1), _empty((P,), torch.float32, idx1)
    if P > 0:
        L.call("omni_iou3d_exact_pairs", *[_lib.ptr(t) for t in fit1], n1, *[_lib.ptr(t) for t in fit2], n2, _lib.ptr(idx1), _lib.ptr(idx2),
               P, _lib.ptr(vol), _lib.ptr(iou), _lib.stream_of(idx1))
    return vol, iou


def iou_box3d_exact_pairs(boxes1, boxes2, idx1, idx2, eps_dim=1e-8, fit_tol=1e-3):
    """Ragged / paired form of `iou_box3d_exact`: (vol, iou)[p] for boxes1[idx1[p]] and boxes2[idx2[p]].  Two fits and one pair launch."""
    return iou_fitted_pairs(cuboid_fit(boxes1, eps_dim, fit_tol), cuboid_fit(boxes2, eps_dim, fit_tol), idx1, idx2)


def iou_box3d_exact(boxes1, boxes2, eps_dim=1e-8, fit_tol=1e-3):
    """(N,8,3), (M,8,3) float32 corner lists -> (vol (N,M), iou (N,M)) float32 from exact geometry in double: the IoU3D of the cuboids
    fitted to the corners (`cuboid_fit`), right whatever the relative pose of the two boxes.  The rows and columns of invalid boxes
    are exactly 0."""
    fit1, fit2 = cuboid_fit(boxes1, eps_dim, fit_tol), cuboid_fit(boxes2, eps_dim, fit_tol)
    N, M = boxes1.shape[0], boxes2.shape[0]
    vol, iou = iou_fitted_pairs(fit1, fit2, *_args.all_pairs(N, M, boxes1.device))
    return vol.view(N, M), iou.view(N, M)


def box3d_overlap_exact(boxes_dt, boxes_gt):
    """(N,8,3), (M,8,3) -> iou (N,M): the IoU3D of the two sets from exact geometry (`iou_box3d_exact`), next to `box3d_overlap`.
    `Omni3Deval` does NOT use it: AP3D is only comparable with the reference's numbers when it is matched with the reference's own
    pair algorithm, near-planar rule included, so the evaluator keeps `box3d_overlap`.  This one is for consumers that need the
    overlap itself, such as TEST.NMS_3D.IOU_TYPE "exact"."""
    return iou_box3d_exact(boxes_dt, boxes_gt)[1]
