"""The pair passes of the evaluator: `box3d_overlap` (reference cubercnn/evaluation/omni3d_evaluation.py:106-166) on the IoU3D kernel,
and the batched form the evaluator needs: `Omni3Deval.evaluate` calls `computeIoU` once per (image, category) group from a Python dict
comprehension (:1339-1343, :1357-1431), i.e. thousands of tiny `box3d_overlap` calls; `box3d_overlap_groups` takes all groups at once --
one validity launch + one ragged pairs launch + one readback.  `bev_overlap_groups`, `dist_errors_groups` and `let_overlap_groups` are
the same pass for the similarities of the modes "BEV", "DIST" and "LET" (one skeleton, `_pairs_pass`); `evaluate_groups` is the greedy
matching on whatever similarity they gave."""
import numpy as np
import torch

from ...kernels import bev, iou3d, let, tperr

BEV_UP = bev.UP            # camera y points down: the ground plane of the outdoor splits


def box3d_overlap(boxes_dt: torch.Tensor, boxes_gt: torch.Tensor, eps_coplanar: float = 1e-4, eps_nonzero: float = 1e-8) -> torch.Tensor:
    """(N,8,3), (M,8,3) corner lists -> (N,M) IoU; rows of non-coplanar / zero-area detections are 0."""
    dev = boxes_dt.device
    if not boxes_dt.is_cuda:   # the reference forces this path to the CPU (MAX_DTS_CROSS_GTS_FOR_IOU3D = 0); here it is a GPU op
        dev = torch.device("cuda")
    out = iou3d.box3d_overlap(boxes_dt.to(dev).float(), boxes_gt.to(dev).float(), eps_coplanar, eps_nonzero)
    return out.to(boxes_dt.device)


def _ragged_pairs(dt_sizes, gt_sizes):
    """the pair list of all groups, row-major inside each group (host index arithmetic on the group table):
    -> (row of the detection (P,), row of the ground truth (P,), offsets of the groups' pairs (groups + 1,))"""
    counts = dt_sizes * gt_sizes
    pair_off = np.concatenate([[0], np.cumsum(counts)])
    P = int(pair_off[-1])
    gid = np.repeat(np.arange(len(counts)), counts)
    local = np.arange(P) - pair_off[gid]
    ng = np.maximum(gt_sizes[gid], 1)
    dt_off = np.concatenate([[0], np.cumsum(dt_sizes)])[:-1]
    gt_off = np.concatenate([[0], np.cumsum(gt_sizes)])[:-1]
    return (dt_off[gid] + local // ng).astype(np.int64), (gt_off[gid] + local % ng).astype(np.int64), pair_off


def _pair_index(pairs, device):
    """the two row lists of `_ragged_pairs` as int64 index tensors on `device`"""
    return torch.from_numpy(pairs[0]).to(device), torch.from_numpy(pairs[1]).to(device)


def _group_pairs(boxes_dt, boxes_gt, dt_sizes, gt_sizes, pairs=None):
    """what the four `*_groups` passes share: the checked group table, the boxes on the device the kernels run on, the ragged pair list
    (`pairs` = what `_ragged_pairs` gave for these sizes, when the caller has it already) uploaded once as int32"""
    dt_sizes = np.asarray(dt_sizes, dtype=np.int64)
    gt_sizes = np.asarray(gt_sizes, dtype=np.int64)
    if dt_sizes.shape != gt_sizes.shape or dt_sizes.ndim != 1:
        raise ValueError("dt_sizes / gt_sizes must be 1-D and of equal length")
    if int(dt_sizes.sum()) != boxes_dt.shape[0] or int(gt_sizes.sum()) != boxes_gt.shape[0]:
        raise ValueError("group sizes do not add up to the number of boxes")
    dev = boxes_dt.device if boxes_dt.is_cuda else torch.device("cuda")
    if not boxes_dt.is_cuda and iou3d._lib.get().emulated:      # host-emulated kernels in the GPU-less test suite
        dev = boxes_dt.device
    dt, gt = boxes_dt.to(dev).float().contiguous(), boxes_gt.to(dev).float().contiguous()
    i1, i2, pair_off = _ragged_pairs(dt_sizes, gt_sizes) if pairs is None else pairs
    idx1, idx2 = torch.from_numpy(i1.astype(np.int32)).to(dev), torch.from_numpy(i2.astype(np.int32)).to(dev)
    return dt_sizes, gt_sizes, dt, gt, idx1, idx2, pair_off


def _group_views(flat, dt_sizes, gt_sizes, pair_off, *tail):
    return [flat[pair_off[g]:pair_off[g + 1]].view(int(dt_sizes[g]), int(gt_sizes[g]), *tail) for g in range(len(dt_sizes))]


def _pairs_pass(boxes_dt, boxes_gt, dt_sizes, gt_sizes, pairs, empty, launch, warn=False, skipped=None, check=None):
    """The skeleton of the four `*_groups` passes: `_group_pairs`; `check()` refuses a bad argument of the pass whether or not there is
    a pair; without a pair `empty(device)`, else `launch(dt, gt, idx1, idx2, bad)`, where `bad` is None or, when `warn` and the pass
    names what it skips (`skipped`), a device counter of the detections it skipped, reported in the warning after the launches.
    -> (what `empty` / `launch` gave, (dt_sizes, gt_sizes, pair_off) for `_group_views`)"""
    dt_sizes, gt_sizes, dt, gt, idx1, idx2, pair_off = _group_pairs(boxes_dt, boxes_gt, dt_sizes, gt_sizes, pairs)
    if check is not None:
        check()
    if int(pair_off[-1]) == 0:
        out = empty(dt.device)
    else:
        bad = torch.zeros(1, dtype=torch.int32, device=dt.device) if warn and skipped else None
        out = launch(dt, gt, idx1, idx2, bad)
        if bad is not None and int(bad) > 0:
            print('Warning: skipping {:d} {} at eval.'.format(int(bad), skipped))
    return out, (dt_sizes, gt_sizes, pair_off)


def box3d_overlap_groups(boxes_dt, boxes_gt, dt_sizes, gt_sizes, eps_coplanar: float = 1e-4, eps_nonzero: float = 1e-8, warn=False, pairs=None):
    """All (image, category) groups of an evaluation in one pass.

    boxes_dt (sum(dt_sizes), 8, 3) / boxes_gt (sum(gt_sizes), 8, 3): the groups' detection (already score-sorted and cut to
    maxDets, :1374-1377) and ground-truth corner lists, concatenated in group order; dt_sizes / gt_sizes: per-group counts; pairs:
    None, or what `_ragged_pairs(dt_sizes, gt_sizes)` gave (a caller that has the pair list passes it on, here and in the three
    passes below).
    -> list of (Nd_g, Ng_g) float32 IoU matrices (views of one flat device tensor, in group order; empty groups give
    empty matrices), each equal to `box3d_overlap(dt_g, gt_g)` of the reference."""
    def launch(dt, gt, idx1, idx2, _):
        valid, vcounts = iou3d.box3d_validity(dt, eps_coplanar, eps_nonzero)
        _, flat = iou3d.iou_box3d_pairs(dt, gt, idx1, idx2, valid1=valid)
        if warn:
            c = vcounts.tolist()
            if c[0] > 0:
                print('Warning: skipping {:d} non-coplanar boxes at eval.'.format(int(c[0])))
            if c[1] > 0:
                print('Warning: skipping {:d} zero volume boxes at eval.'.format(int(c[1])))
        return flat

    flat, table = _pairs_pass(boxes_dt, boxes_gt, dt_sizes, gt_sizes, pairs, lambda dev: torch.zeros(0, dtype=torch.float32, device=dev), launch)
    return _group_views(flat, *table)


def bev_overlap_groups(boxes_dt, boxes_gt, dt_sizes, gt_sizes, up=BEV_UP, eps_area: float = 1e-8, warn=False, pairs=None):
    """`box3d_overlap_groups` with the IoU of the boxes' footprints on the ground plane orthogonal to `up` (csrc/bev_iou.hip) in
    place of IoU3D: the same arguments, the same return layout (views of one flat device tensor in group order).  Two footprint
    launches, one pairs launch.  A box with a non-finite vertex or a footprint area <= eps_area overlaps nothing, on either side."""
    flat, table = _pairs_pass(
        boxes_dt, boxes_gt, dt_sizes, gt_sizes, pairs, lambda dev: torch.zeros(0, dtype=torch.float32, device=dev),
        lambda dt, gt, idx1, idx2, bad: bev.bev_iou_pairs(bev.bev_footprints(dt, up, eps_area, counts=bad), bev.bev_footprints(gt, up, eps_area),
                                                          idx1, idx2),
        warn, "boxes without a footprint")
    return _group_views(flat, *table)


def dist_errors_groups(boxes_dt, boxes_gt, dt_sizes, gt_sizes, up=None, warn=False, pairs=None):
    """The pair errors of the centre-distance protocol for all (image, category) groups in one pass: the arguments of
    `box3d_overlap_groups`, `up` as in `kernels.tperr` (None = the full 3D distance).  Both sides are fitted by `cuboid_fit` with its
    default eps_dim and fit_tol (two launches), then one pairs launch (csrc/tp_errors.hip).
    -> (flat (P, 3) float64 device tensor of (trans, scale, orient) in group order, row-major inside a group; the list of its
    per-group views (Nd_g, Ng_g, 3)).  A pair with an invalid box on either side is (+inf, NaN, NaN): it matches nothing."""
    flat, table = _pairs_pass(
        boxes_dt, boxes_gt, dt_sizes, gt_sizes, pairs, lambda dev: torch.zeros((0, 3), dtype=torch.float64, device=dev),
        lambda dt, gt, idx1, idx2, bad: tperr.pair_errors(iou3d.cuboid_fit(dt, counts=bad), iou3d.cuboid_fit(gt), idx1, idx2, up),
        warn, "boxes that are no cuboid", check=lambda: tperr.unit_up(up))
    return flat, _group_views(flat, *table, 3)


def let_overlap_groups(boxes_dt, boxes_gt, dt_sizes, gt_sizes, tol_frac=let.TOL_FRAC, tol_min=let.TOL_MIN, warn=False, pairs=None):
    """The longitudinal-error-tolerant IoU3D, affinity and longitudinal error of `kernels.let` for all (image, category) groups in one
    pass: the arguments of `box3d_overlap_groups` plus the tolerance T = max(tol_frac |G|, tol_min).  Both sides are fitted by
    `cuboid_fit` with its default eps_dim and fit_tol (two launches), then one pairs launch (csrc/let_iou.hip).
    -> (iou (P,) float32, aff (P,) float64, lon (P,) float64: flat device tensors in group order, row-major inside a group; the list
    of the per-group views (Nd_g, Ng_g) of iou).  A gated pair (an invalid box on either side, a detection on the sensor) is
    (0, 0, NaN): it matches nothing."""
    (iou, aff, lon), table = _pairs_pass(
        boxes_dt, boxes_gt, dt_sizes, gt_sizes, pairs,
        lambda dev: tuple(torch.zeros(0, dtype=t, device=dev) for t in (torch.float32, torch.float64, torch.float64)),
        lambda dt, gt, idx1, idx2, bad: let.let_pairs(iou3d.cuboid_fit(dt, counts=bad), iou3d.cuboid_fit(gt), idx1, idx2, tol_frac, tol_min),
        warn, "boxes that are no cuboid", check=lambda: let.check_tolerance(tol_frac, tol_min))
    return iou, aff, lon, _group_views(iou, *table)


def _xywh_iou(bd, bg):
    """row-wise IoU of two (P, 4) lists of xywh boxes (pycocotools bbIou, iscrowd = 0)"""
    iw = (torch.min(bd[:, 0] + bd[:, 2], bg[:, 0] + bg[:, 2]) - torch.max(bd[:, 0], bg[:, 0])).clamp(min=0)
    ih = (torch.min(bd[:, 1] + bd[:, 3], bg[:, 1] + bg[:, 3]) - torch.max(bd[:, 1], bg[:, 1])).clamp(min=0)
    inter = iw * ih
    return inter / (bd[:, 2] * bd[:, 3] + bg[:, 2] * bg[:, 3] - inter)


def evaluate_groups(ious_flat, dt_sizes, gt_sizes, gt_ignore, gt_range, dt_range, area_ranges, iou_thrs):
    """The greedy matching of `Omni3Deval.evaluateImg` (:1433-1551, 3D mode, eval_prox off) for every (image, category)
    group x depth range x IoU threshold in one launch (the reference loops over them in Python, :1346-1351).

    ious_flat: the concatenated (D_g, G_g) matrices (e.g. torch.cat of box3d_overlap_groups' views), detections in descending
    score order and cut to maxDets; dt_sizes / gt_sizes: per-group counts; gt_ignore (sumG) int `ignore3D`; gt_range (sumG),
    dt_range (sumD) float `depth`; area_ranges (A, 2); iou_thrs (T,).
    -> dict of device tensors: dt_match (A,T,sumD) index of the matched gt inside its group (original order) or -1,
       gt_match (A,T,sumG) index of the matched dt or -1, dt_ignore (A,T,sumD) uint8, gt_order (A,sumG) the stable
       ignore-last order, gt_ignore (A,sumG) uint8 `_ignore` per original gt."""
    L = iou3d._lib.get()
    dev = ious_flat.device
    dt_sizes, gt_sizes = np.asarray(dt_sizes, dtype=np.int64), np.asarray(gt_sizes, dtype=np.int64)
    ng, sumD, sumG = len(dt_sizes), int(dt_sizes.sum()), int(gt_sizes.sum())
    A, T = len(area_ranges), len(iou_thrs)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)      # noqa: E731
    iou_off = torch.from_numpy(np.concatenate([[0], np.cumsum(dt_sizes * gt_sizes)])[:-1].astype(np.int64)).to(dev)
    dt_off, gt_off = i32(np.concatenate([[0], np.cumsum(dt_sizes)])), i32(np.concatenate([[0], np.cumsum(gt_sizes)]))
    areas = torch.tensor(np.asarray(area_ranges, dtype=np.float32)).to(dev).contiguous()
    thrs = torch.tensor(np.asarray(iou_thrs, dtype=np.float64)).to(dev).contiguous()
    out = {"dt_match": torch.empty((A, T, sumD), dtype=torch.int32, device=dev), "gt_match": torch.empty((A, T, sumG), dtype=torch.int32, device=dev),
           "dt_ignore": torch.empty((A, T, sumD), dtype=torch.uint8, device=dev), "gt_order": torch.empty((A, sumG), dtype=torch.int32, device=dev),
           "gt_ignore": torch.empty((A, sumG), dtype=torch.uint8, device=dev)}
    if ng == 0:
        return out
    ious_flat = ious_flat.float().contiguous()
    gt_ignore, gt_range, dt_range = gt_ignore.to(torch.int32).contiguous(), gt_range.float().contiguous(), dt_range.float().contiguous()
    iou3d._lib.check_device(ious_flat, gt_ignore, gt_range, dt_range)
    _p = iou3d._lib.ptr
    L.call("omni_eval_match", _p(ious_flat), _p(iou_off), _p(dt_off), _p(gt_off), _p(gt_ignore), _p(gt_range), _p(dt_range), _p(areas),
           _p(thrs), ng, A, T, sumD, sumG, int(gt_sizes.max()) if ng else 0, _p(out["dt_match"]), _p(out["gt_match"]),
           _p(out["dt_ignore"]), _p(out["gt_order"]), _p(out["gt_ignore"]), iou3d._lib.stream_of(ious_flat))
    return out
