"""`box3d_overlap` (reference cubercnn/evaluation/omni3d_evaluation.py:106-166) on the IoU3D kernel, and the batched
form the evaluator needs: `Omni3Deval.evaluate` calls `computeIoU` once per (image, category) group from a Python dict
comprehension (:1339-1343, :1357-1431), i.e. thousands of tiny `box3d_overlap` calls; `box3d_overlap_groups` takes all
groups at once -- one validity launch + one ragged pairs launch + one readback.  `Omni3Deval` runs the COCO-style greedy
matching and the precision / recall accumulation around it on the device as well; `Omni3DEvaluator` / `Omni3DEvaluationHelper`
are the per-split drivers `tools/train_net.py:do_test` uses.

Extension without a counterpart in the reference: mode "BEV" = the 3D protocol with the IoU of the cuboids' footprints on the ground
plane (`bev_overlap_groups`, csrc/bev_iou.hip) in place of IoU3D, i.e. the AP-BEV of the outdoor benchmarks; `eval_bev` switches it
on in the two drivers, off by default.

A second one: mode "DIST" = the centre-distance protocol of nuScenes (`dist_errors_groups`, csrc/tp_errors.hip): detections are matched
by the distance of the fitted centres, and the matched pairs are scored for translation, scale and orientation error along the recall
curve (ATE / ASE / AOE); `eval_dist` switches it on in the two drivers, off by default.  See `Omni3Deval`.

A third one: mode "LET" = the longitudinal-error-tolerant metrics of the Waymo camera-only benchmark (`let_overlap_groups`,
csrc/let_iou.hip): a detection may slide along its own line of sight onto the ground truth within a tolerance that grows with range, the
exact IoU3D of the slid box decides the match (LET-AP), and a second table scales precision by how little sliding was needed (LET-APL);
`eval_let` switches it on in the two drivers, off by default.  See `Omni3Deval`.

A fourth one, for every mode: `Omni3Deval.bootstrap` / `bootstrap_compare` = image-level bootstrap confidence intervals of AP / AR and
the paired comparison of two prediction sets.  The match tables of evaluate() are kept and all replicates are accumulated in one launch
from integer image multiplicities (`kernels.bootstrap`, csrc/eval_bootstrap.hip); `bootstrap` switches it on in the two drivers, off by
default.  See `Omni3Deval.bootstrap`."""
import copy
import datetime
import json
import logging
import os

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


def _group_pairs(boxes_dt, boxes_gt, dt_sizes, gt_sizes):
    """what `box3d_overlap_groups` and `bev_overlap_groups` share: the checked group table, the boxes on the device the kernels
    run on, the ragged pair list uploaded once as int32"""
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
    i1, i2, pair_off = _ragged_pairs(dt_sizes, gt_sizes)
    idx1, idx2 = torch.from_numpy(i1.astype(np.int32)).to(dev), torch.from_numpy(i2.astype(np.int32)).to(dev)
    return dt_sizes, gt_sizes, dt, gt, idx1, idx2, pair_off


def _group_views(flat, dt_sizes, gt_sizes, pair_off):
    return [flat[pair_off[g]:pair_off[g + 1]].view(int(dt_sizes[g]), int(gt_sizes[g])) for g in range(len(dt_sizes))]


def box3d_overlap_groups(boxes_dt, boxes_gt, dt_sizes, gt_sizes, eps_coplanar: float = 1e-4, eps_nonzero: float = 1e-8, warn=False):
    """All (image, category) groups of an evaluation in one pass.

    boxes_dt (sum(dt_sizes), 8, 3) / boxes_gt (sum(gt_sizes), 8, 3): the groups' detection (already score-sorted and cut to
    maxDets, :1374-1377) and ground-truth corner lists, concatenated in group order; dt_sizes / gt_sizes: per-group counts.
    -> list of (Nd_g, Ng_g) float32 IoU matrices (views of one flat device tensor, in group order; empty groups give
    empty matrices), each equal to `box3d_overlap(dt_g, gt_g)` of the reference."""
    dt_sizes, gt_sizes, dt, gt, idx1, idx2, pair_off = _group_pairs(boxes_dt, boxes_gt, dt_sizes, gt_sizes)
    if int(pair_off[-1]) == 0:
        flat = torch.zeros(0, dtype=torch.float32, device=dt.device)
    else:
        valid, vcounts = iou3d.box3d_validity(dt, eps_coplanar, eps_nonzero)
        _, flat = iou3d.iou_box3d_pairs(dt, gt, idx1, idx2, valid1=valid)
        if warn:
            c = vcounts.tolist()
            if c[0] > 0:
                print('Warning: skipping {:d} non-coplanar boxes at eval.'.format(int(c[0])))
            if c[1] > 0:
                print('Warning: skipping {:d} zero volume boxes at eval.'.format(int(c[1])))
    return _group_views(flat, dt_sizes, gt_sizes, pair_off)


def bev_overlap_groups(boxes_dt, boxes_gt, dt_sizes, gt_sizes, up=BEV_UP, eps_area: float = 1e-8, warn=False):
    """`box3d_overlap_groups` with the IoU of the boxes' footprints on the ground plane orthogonal to `up` (csrc/bev_iou.hip) in
    place of IoU3D: the same arguments, the same return layout (views of one flat device tensor in group order).  Two footprint
    launches, one pairs launch.  A box with a non-finite vertex or a footprint area <= eps_area overlaps nothing, on either side."""
    dt_sizes, gt_sizes, dt, gt, idx1, idx2, pair_off = _group_pairs(boxes_dt, boxes_gt, dt_sizes, gt_sizes)
    if int(pair_off[-1]) == 0:
        flat = torch.zeros(0, dtype=torch.float32, device=dt.device)
    else:
        bad = torch.zeros(1, dtype=torch.int32, device=dt.device) if warn else None
        flat = bev.bev_iou_pairs(bev.bev_footprints(dt, up, eps_area, counts=bad), bev.bev_footprints(gt, up, eps_area), idx1, idx2)
        if warn and int(bad) > 0:
            print('Warning: skipping {:d} boxes without a footprint at eval.'.format(int(bad)))
    return _group_views(flat, dt_sizes, gt_sizes, pair_off)


def dist_errors_groups(boxes_dt, boxes_gt, dt_sizes, gt_sizes, up=None, warn=False):
    """The pair errors of the centre-distance protocol for all (image, category) groups in one pass: the arguments of
    `box3d_overlap_groups`, `up` as in `kernels.tperr` (None = the full 3D distance).  Both sides are fitted by `cuboid_fit` with its
    default eps_dim and fit_tol (two launches), then one pairs launch (csrc/tp_errors.hip).
    -> (flat (P, 3) float64 device tensor of (trans, scale, orient) in group order, row-major inside a group; the list of its
    per-group views (Nd_g, Ng_g, 3)).  A pair with an invalid box on either side is (+inf, NaN, NaN): it matches nothing."""
    dt_sizes, gt_sizes, dt, gt, idx1, idx2, pair_off = _group_pairs(boxes_dt, boxes_gt, dt_sizes, gt_sizes)
    tperr.unit_up(up)                                              # a bad `up` is refused whether or not there is a pair
    if int(pair_off[-1]) == 0:
        flat = torch.zeros((0, 3), dtype=torch.float64, device=dt.device)
    else:
        bad = torch.zeros(1, dtype=torch.int32, device=dt.device) if warn else None
        flat = tperr.pair_errors(iou3d.cuboid_fit(dt, counts=bad), iou3d.cuboid_fit(gt), idx1, idx2, up)
        if warn and int(bad) > 0:
            print('Warning: skipping {:d} boxes that are no cuboid at eval.'.format(int(bad)))
    views = [flat[pair_off[g]:pair_off[g + 1]].view(int(dt_sizes[g]), int(gt_sizes[g]), 3) for g in range(len(dt_sizes))]
    return flat, views


def let_overlap_groups(boxes_dt, boxes_gt, dt_sizes, gt_sizes, tol_frac=let.TOL_FRAC, tol_min=let.TOL_MIN, warn=False):
    """The longitudinal-error-tolerant IoU3D, affinity and longitudinal error of `kernels.let` for all (image, category) groups in one
    pass: the arguments of `box3d_overlap_groups` plus the tolerance T = max(tol_frac |G|, tol_min).  Both sides are fitted by
    `cuboid_fit` with its default eps_dim and fit_tol (two launches), then one pairs launch (csrc/let_iou.hip).
    -> (iou (P,) float32, aff (P,) float64, lon (P,) float64: flat device tensors in group order, row-major inside a group; the list
    of the per-group views (Nd_g, Ng_g) of iou).  A gated pair (an invalid box on either side, a detection on the sensor) is
    (0, 0, NaN): it matches nothing."""
    dt_sizes, gt_sizes, dt, gt, idx1, idx2, pair_off = _group_pairs(boxes_dt, boxes_gt, dt_sizes, gt_sizes)
    tol_frac, tol_min = let.check_tolerance(tol_frac, tol_min)    # a bad tolerance is refused whether or not there is a pair
    if int(pair_off[-1]) == 0:
        iou = torch.zeros(0, dtype=torch.float32, device=dt.device)
        aff, lon = torch.zeros(0, dtype=torch.float64, device=dt.device), torch.zeros(0, dtype=torch.float64, device=dt.device)
    else:
        bad = torch.zeros(1, dtype=torch.int32, device=dt.device) if warn else None
        iou, aff, lon = let.let_pairs(iou3d.cuboid_fit(dt, counts=bad), iou3d.cuboid_fit(gt), idx1, idx2, tol_frac, tol_min)
        if warn and int(bad) > 0:
            print('Warning: skipping {:d} boxes that are no cuboid at eval.'.format(int(bad)))
    return iou, aff, lon, _group_views(iou, dt_sizes, gt_sizes, pair_off)


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


# =====================================================================================================================
# the headline slots of summarize(), shared with the bootstrap
# =====================================================================================================================
def _stat_thresholds(mode):
    return [0.5, 0.75, 0.95] if mode == "2D" else [0.5, 1.0, 2.0] if mode == "DIST" else [0.15, 0.25, 0.50]


def _stat_slots(p, mode):
    """the 13 `stats` of summarize() as (ap, iouThr, areaRng label, maxDets): AP overall, at three thresholds, in three ranges; AR at
    the three maxDets and in three ranges"""
    thres, L, md = _stat_thresholds(mode), p.areaRngLbl, p.maxDets
    return [(1, None, "all", 100)] + [(1, thres[i], "all", md[2]) for i in range(3)] + [(1, None, L[1 + i], md[2]) for i in range(3)] \
        + [(0, None, "all", md[i]) for i in range(3)] + [(0, None, L[1 + i], md[2]) for i in range(3)]


def _slot_indices(p, mode, ap, iouThr, areaRng, maxDets):
    """-> (indices of the thresholds or None = all, of the ranges, of the maxDets) one slot of summarize() averages over"""
    shown = p.distThrs if mode == "DIST" else p.iouThrs            # DIST: thresholds are named, and looked up, in metres
    aind = [i for i, a in enumerate(p.areaRngLbl) if a == areaRng]
    mind = [i for i, m in enumerate(p.maxDets) if m == maxDets]
    tind = None
    if iouThr is not None:
        tind = np.where(np.isclose(iouThr, np.asarray(shown).astype(float)))[0] if ap == 1 else np.where(iouThr == np.asarray(shown))[0]
    return tind, aind, mind


BOOTSTRAP_CHUNK = 256       # replicates per launch of `Omni3Deval.bootstrap`


def _check_confidence(confidence):
    try:
        c = float(confidence)
    except (TypeError, ValueError):
        raise ValueError("confidence must be a number") from None
    if not 0.0 < c < 1.0:
        raise ValueError("confidence must lie in (0, 1)")
    return c


def bootstrap_weights(img_ids, n=1000, seed=0, weights=None, strata=None):
    """The (n, I) int32 replicate table of `Omni3Deval.bootstrap`: `weights` checked (columns in the order of img_ids), or n rows drawn
    by np.random.default_rng(seed), one multinomial per stratum in sorted label order."""
    I = len(img_ids)
    if weights is not None:
        w = np.asarray(weights)
        if w.ndim != 2 or w.shape[0] < 1 or w.shape[1] != I:
            raise ValueError("weights must have shape (n, %d): one column per image of params.imgIds" % I)
        if not np.issubdtype(w.dtype, np.integer):
            if not np.issubdtype(w.dtype, np.floating) or not np.isfinite(w).all() or (w != np.round(w)).any():
                raise ValueError("weights must be integers")
        if (w < 0).any():
            raise ValueError("weights must be >= 0")
        if w.size and w.max() > np.iinfo(np.int32).max:
            raise ValueError("weights must fit 32 bits")
        return np.ascontiguousarray(w.astype(np.int32))
    if int(n) != n or n < 1:
        raise ValueError("n must be a positive integer")
    if strata is None:
        labels = [0] * I
    else:
        try:
            labels = [strata[i] for i in img_ids]
        except KeyError as e:
            raise ValueError("strata has no label for image %r" % (e.args[0],)) from None
    g = np.random.default_rng(seed)
    w = np.zeros((int(n), I), np.int32)
    for label in sorted(set(labels)):
        cols = np.flatnonzero(np.array([lb == label for lb in labels], dtype=bool))
        w[:, cols] = g.multinomial(len(cols), np.full(len(cols), 1.0 / len(cols)), size=int(n))
    return w


def _replicate_summary(values, confidence):
    """values (n, S), -1 = no value -> mean, se (ddof=1), ci (S, 2), n_valid over the replicates with a value, per column"""
    S = values.shape[1]
    mean, se, ci, n_valid = np.full(S, np.nan), np.full(S, np.nan), np.full((S, 2), np.nan), np.zeros(S, np.int64)
    for j in range(S):
        v = values[:, j][values[:, j] > -1]
        n_valid[j] = v.size
        if v.size:
            mean[j] = v.mean()
            ci[j] = np.quantile(v, [(1.0 - confidence) / 2.0, (1.0 + confidence) / 2.0])
        if v.size > 1:
            se[j] = v.std(ddof=1)
    return mean, se, ci, n_valid


def _masked_mean(vals, axes):
    """mean over `axes` of the entries > -1, -1 where there is none"""
    valid = vals > -1
    cnt = valid.sum(axis=axes)
    tot = np.where(valid, vals, 0.0).sum(axis=axes)
    return np.where(cnt > 0, tot / np.maximum(cnt, 1), -1.0)


def _bootstrap_stats(p, mode, ap, ar):
    """ap, ar (n, T, K, A, M) -> (n, 13): the slots of summarize() per replicate.  `one()` averages a slot's (T', R, K) block of
    `precision` over the entries > -1, and for fixed (k, a) all (t, r) hold a value or none does: the mean over the valid (t, k) of the
    R-means is the same number."""
    out = np.full((ap.shape[0], 13), -1.0)
    for i, (is_ap, iouThr, areaRng, maxDets) in enumerate(_stat_slots(p, mode)):
        tind, aind, mind = _slot_indices(p, mode, is_ap, iouThr, areaRng, maxDets)
        s = ap if is_ap == 1 else ar
        if tind is not None:
            s = s[:, tind]
        if len(aind) and len(mind) and s.shape[1]:
            out[:, i] = _masked_mean(s[:, :, :, aind[0], mind[0]], (1, 2))
    return out


def _bootstrap_result(p, mode, W, ap, ar, confidence):
    """the dict of `Omni3Deval.bootstrap` from the tables of [the all-ones replicate] + W"""
    stats = _bootstrap_stats(p, mode, ap, ar)
    mean, se, ci, n_valid = _replicate_summary(stats[1:], confidence)
    aall = p.areaRngLbl.index("all") if "all" in p.areaRngLbl else 0
    cat = _masked_mean(ap[:, :, :, aall, -1], (1,))                                   # (n + 1, K)
    cmean, cse, cci, cn = _replicate_summary(cat[1:], confidence)
    return {"weights": W, "ap": ap[1:], "ar": ar[1:], "stats": stats[1:], "point": stats[0], "mean": mean, "se": se, "ci": ci,
            "n_valid": n_valid, "confidence": confidence,
            "per_category": {"point": cat[0], "values": cat[1:], "mean": cmean, "se": cse, "ci": cci, "n_valid": cn}}


def bootstrap_compare(ev_a, ev_b, n=1000, seed=0, confidence=0.95, weights=None, strata=None, chunk=None):
    """Paired bootstrap of two prediction sets on the same images: both `Omni3Deval` must have been evaluated with equal imgIds, catIds,
    areaRng, maxDets, iouThrs and recThrs (ValueError otherwise).  ONE weight table (given, or drawn as in `Omni3Deval.bootstrap`) is
    used for both, so every replicate compares the two on the same resampled test set.
    -> dict: `a`, `b` the two `bootstrap` dicts; `delta` (n, 13) = a - b per stats slot, NaN where either side has no value;
    `delta_point` (13,); `delta_ci` (13, 2) the percentile interval and `p_le0` (13,) the share of the replicates with delta <= 0,
    both over the replicates valid on both sides (NaN without any); `n_valid` (13,); `per_category`: the same (`delta` (n, K),
    `delta_point`, `delta_ci`, `p_le0`, `n_valid`) for the per-category AP."""
    for ev in (ev_a, ev_b):
        if ev._dev is None:
            raise Exception("Please run evaluate() first")
    pa, pb = ev_a._paramsEval, ev_b._paramsEval
    same = list(pa.imgIds) == list(pb.imgIds) and list(pa.catIds) == list(pb.catIds) and list(pa.maxDets) == list(pb.maxDets) \
        and np.array_equal(np.asarray(pa.areaRng, dtype=np.float64), np.asarray(pb.areaRng, dtype=np.float64)) \
        and np.array_equal(np.asarray(ev_a.params.iouThrs), np.asarray(ev_b.params.iouThrs)) \
        and np.array_equal(np.asarray(ev_a.params.recThrs), np.asarray(ev_b.params.recThrs))
    if not same:
        raise ValueError("the two evaluations differ in imgIds, catIds, areaRng, maxDets, iouThrs or recThrs")
    confidence = _check_confidence(confidence)
    W = bootstrap_weights(pa.imgIds, n, seed, weights, strata)
    a = ev_a.bootstrap(confidence=confidence, weights=W, chunk=chunk)
    b = ev_b.bootstrap(confidence=confidence, weights=W, chunk=chunk)

    def paired(va, vb, pa_, pb_):
        both = (va > -1) & (vb > -1)
        delta = np.where(both, va - vb, np.nan)
        S = va.shape[1]
        dci, ple0, nv = np.full((S, 2), np.nan), np.full(S, np.nan), both.sum(axis=0)
        for j in range(S):
            v = delta[both[:, j], j]
            if v.size:
                dci[j] = np.quantile(v, [(1.0 - confidence) / 2.0, (1.0 + confidence) / 2.0])
                ple0[j] = float((v <= 0).mean())
        return {"delta": delta, "delta_point": np.where((pa_ > -1) & (pb_ > -1), pa_ - pb_, np.nan), "delta_ci": dci, "p_le0": ple0,
                "n_valid": nv}

    out = {"a": a, "b": b, "weights": W, "confidence": confidence}
    out.update(paired(a["stats"], b["stats"], a["point"], b["point"]))
    out["per_category"] = paired(a["per_category"]["values"], b["per_category"]["values"], a["per_category"]["point"], b["per_category"]["point"])
    return out


# =====================================================================================================================
# Omni3Deval: evaluate -> accumulate -> summarize on the device (reference :1019-1704)
# =====================================================================================================================
class Omni3DParams:
    """omni3d_evaluation.py:1019-1088"""

    def setDet2DParams(self):
        self.imgIds, self.catIds = [], []
        self.iouThrs = np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1, endpoint=True)
        self.recThrs = np.linspace(0.0, 1.00, int(np.round((1.00 - 0.0) / 0.01)) + 1, endpoint=True)
        self.maxDets = [1, 10, 100]
        self.areaRng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
        self.areaRngLbl = ["all", "small", "medium", "large"]
        self.useCats = 1

    def setDet3DParams(self):
        self.imgIds, self.catIds = [], []
        self.iouThrs = np.linspace(0.05, 0.5, int(np.round((0.5 - 0.05) / 0.05)) + 1, endpoint=True)
        self.recThrs = np.linspace(0.0, 1.00, int(np.round((1.00 - 0.0) / 0.01)) + 1, endpoint=True)
        self.maxDets = [1, 10, 100]
        self.areaRng = [[0, 1e5], [0, 10], [10, 35], [35, 1e5]]
        self.areaRngLbl = ["all", "near", "medium", "far"]
        self.useCats = 1

    def setDetDistParams(self):
        """the 3D protocol's depth ranges and maxDets; a match needs dist <= d for d in distThrs (metres).  iouThrs holds the
        thresholds mapped to the similarity 1 / (1 + dist) the matching kernel compares (`Omni3Deval.evaluate` refreshes it from
        distThrs); the TP errors are taken at tpDist along the recall thresholds >= minRecall"""
        self.setDet3DParams()
        self.distThrs = np.array([0.5, 1.0, 2.0, 4.0])
        self.tpDist = 2.0
        self.minRecall = 0.1
        self.iouThrs = 1.0 / (1.0 + self.distThrs)

    def setDetLetParams(self):
        """the 3D protocol (thresholds on the longitudinal-error-tolerant IoU3D, depth ranges, maxDets); a detection may slide along
        its line of sight by up to max(lonTolFrac x range of the ground truth, lonTolMin metres)"""
        self.setDet3DParams()
        self.lonTolFrac = let.TOL_FRAC
        self.lonTolMin = let.TOL_MIN

    def __init__(self, mode="2D"):
        if mode == "2D":
            self.setDet2DParams()
        elif mode in ("3D", "BEV"):            # BEV: the 3D protocol (thresholds, depth ranges), so AP-BEV compares with AP3D
            self.setDet3DParams()
        elif mode == "DIST":
            self.setDetDistParams()
        elif mode == "LET":
            self.setDetLetParams()
        else:
            raise Exception("mode %s not supported" % (mode))
        self.iouType = "bbox"
        self.mode = mode
        self.proximity_thresh = 0.3


class AnnotationIndex:
    """The four COCO-API calls Omni3Deval makes (getImgIds / getCatIds / getAnnIds / loadAnns) over a plain list of
    annotation dicts -- pycocotools is not needed for the scoped path."""

    def __init__(self, anns, img_ids=None, cat_ids=None):
        self.anns = {}
        for i, a in enumerate(anns):
            a.setdefault("id", i + 1)
            self.anns[a["id"]] = a
        self._imgs = sorted(set(img_ids) if img_ids is not None else {a["image_id"] for a in anns})
        self._cats = sorted(set(cat_ids) if cat_ids is not None else {a["category_id"] for a in anns})

    def getImgIds(self):
        return list(self._imgs)

    def getCatIds(self):
        return list(self._cats)

    def getAnnIds(self, imgIds=(), catIds=()):
        imgs, cats = set(imgIds), set(catIds)
        return [i for i, a in self.anns.items() if (not imgs or a["image_id"] in imgs) and (not cats or a["category_id"] in cats)]

    def loadAnns(self, ids):
        return [self.anns[i] for i in ids]


class Omni3Deval:
    """`Omni3Deval(cocoGt, cocoDt, mode=...)` with the reference's evaluate() / accumulate() / summarize() and result layout
    (`eval['precision']` [T,R,K,A,M], `eval['recall']` [T,K,A,M], `eval['scores']`, `stats` (13,)).

    evaluate(): all (image, category) groups at once -- one IoU pass (`box3d_overlap_groups` in 3D, `bev_overlap_groups` with the
    up vector `up` in BEV -- which otherwise is the 3D mode: `bbox3D`, `ignore3D`, `depth` --, a vectorised box IoU in 2D) and one greedy-matching launch for every group x range x threshold (`evaluate_groups`, csrc/eval_match.hip);
    accumulate(): one launch for every (category, range, maxDets, threshold) (`omni_eval_accumulate`).  The reference runs
    these as Python loops over dict-of-list structures (:1339-1351, :1230-1301).

    eval_prox (proximity evaluation for non-exhaustively annotated datasets, :1419-1429, :1499, :1534-1536): a detection may
    only match ground truths whose 2D box overlaps its own by more than `params.proximity_thresh`, and a detection with no
    ground truth in proximity is ignored.  True / False like the reference, or a collection of image ids (extension: the
    helper evaluates the union of several datasets of which only some use proximity evaluation).

    Mode "DIST" (extension, the centre-distance protocol of nuScenes; `up` = None or the up vector of the ground plane).
    Boxes: both sides are the eight `bbox3D` corners in the order of `boxgen.UNIT`, fitted by `cuboid_fit` (default eps_dim, fit_tol);
    an invalid box on either side has distance +inf and matches nothing.
    Distance: the Euclidean distance of the fitted centres; with `up`, the distance in the ground plane orthogonal to it (nuScenes'
    definition; (0, -1, 0) for level outdoor cameras).  The default is the full 3D distance: Omni3D has no world frame and indoor
    cameras are pitched.
    Matching: the 3D protocol (depth ranges, `ignore3D`, maxDets, eval_prox; `evaluate_groups` unchanged) on the similarity
    s = 1 / (1 + dist), computed in double and stored as float32 (0 for +inf), against the thresholds 1 / (1 + d), d in
    `params.distThrs` (default 0.5, 1, 2, 4 m); `params.iouThrs` holds the mapped thresholds.  Departures from nuScenes: a match needs
    dist <= d (nuScenes: <), and AP is this evaluator's 101-point AP averaged over the distance thresholds, without nuScenes' 10 %
    recall and precision clipping.
    TP metrics: at `params.tpDist` (default 2.0, one of distThrs) and the largest maxDets, per category and depth range: the
    category's detections in the merge order of accumulate(), the ignored ones skipped; at the c-th true positive m_c = the mean of
    (trans, scale, orient) of `kernels.tperr` over the first c; the recall threshold r_j of `params.recThrs` takes m_c when r_j >=
    `params.minRecall` (default 0.1) and (c-1)/npig < r_j <= c/npig; the metric is the mean of the values taken, -1 without ground
    truth or evaluated image, 1.0 when no threshold took a value (nuScenes' rule).  Departure: nuScenes interpolates over confidence,
    this is the step rule above.  accumulate() fills `eval['tp_errors']` (K, A, 3) and `eval['tp_count']` (K, A); summarize() keeps
    the `stats` layout (slots 1..3: AP at 0.5, 1 and 2 m, looked up in distThrs), appends mATE / mASE / mAOE = the means over the
    categories with a value > -1 at range "all", and sets `tp_stats`.  No composite score: NDS needs velocity and attribute errors
    one image does not give.

    Mode "LET" (extension, LET-3D-AP / LET-3D-APL of Hung et al. 2022, the Waymo camera-only metric: is the detector wrong, or only
    wrong in depth?).  Boxes as in mode "DIST": the eight `bbox3D` corners in the order of `boxgen.UNIT`, in camera coordinates, both
    sides fitted by `cuboid_fit`; the sensor origin is the camera centre.
    Pair: for a detection with fitted centre P and a ground truth with fitted centre G, u = P / |P| is the line of sight, lon =
    (G - P) . u the signed longitudinal error (positive: predicted too near), T = max(lonTolFrac |G|, lonTolMin) (defaults 0.10 and
    0.5 m, Waymo's values), aff = 1 - min(|lon| / T, 1) the longitudinal affinity; the aligned box is the detection with its centre
    moved to P + lon u, the point of its ray closest to G; let_iou = the exact cuboid IoU3D (csrc/cuboid_exact.h, in double, stored
    as float32) of the aligned box and the ground truth when aff > 0, exactly 0 when aff == 0.  An invalid box on either side or a
    detection on the sensor (|P| <= 1e-8) gives (0, 0, NaN) and matches nothing.
    Matching: the 3D protocol (iouThrs 0.05 .. 0.5, depth ranges, `ignore3D`, maxDets, eval_prox; `evaluate_groups` unchanged) on
    let_iou; LET-AP is this evaluator's 101-point AP on those matches (`eval['precision']`, `stats`).  Departures from Waymo: Waymo
    matches bipartitely on the longitudinal affinity, this is the greedy COCO matching by descending score on let_iou;
    Waymo thresholds at one IoU per class and bins by difficulty level, here the ten IoU thresholds and the depth ranges of AP3D
    apply; the exact IoU3D decides, not the pair algorithm AP3D keeps for comparability (a slid box is a near-aligned near-duplicate,
    where that algorithm is off by up to 0.3).
    LET-APL: on the same lists and recall axis the precision at a list position is (sum of aff over the true positives so far) /
    (tp + fp + eps), aff of the pair (detection, its matched ground truth); made monotone from the right and sampled at recThrs like
    precision: `eval['precision_l']` (T, R, K, A, M), -1 where precision is, never above precision.  `eval['tp_affinity']` and
    `eval['tp_lon']` (T, K, A, M): the mean aff and the mean signed lon (metres; its sign tells whether a category is predicted
    systematically near or far) of the true positives among the included detections, -1 without one.  summarize() keeps the `stats`
    layout, sets `stats_l` (7,) = LET-APL overall, at 0.15 / 0.25 / 0.50, near / medium / far, and `let_stats` (2,) = mean affinity
    and mean signed longitudinal error at range "all", the largest maxDets and IoU 0.25, as means over the categories with a true
    positive (-1 without any), and prints those lines too."""

    def __init__(self, cocoGt=None, cocoDt=None, iouType="bbox", mode="2D", eval_prox=False, up=None):
        if mode not in ["2D", "3D", "BEV", "DIST", "LET"]:
            raise Exception("mode %s not supported" % (mode))
        self.mode, self.eval_prox = mode, eval_prox
        if mode == "DIST":                     # None: the full 3D distance
            self.up = None if up is None else tperr.unit_up(up)
        else:                                  # the ground plane of mode BEV
            self.up = tuple(float(v) for v in (BEV_UP if up is None else up))
        self.cocoGt, self.cocoDt = cocoGt, cocoDt
        self.params = Omni3DParams(mode)
        self.eval, self.stats, self._dev = {}, [], None
        if cocoGt is not None:
            self.params.imgIds = sorted(cocoGt.getImgIds())
            self.params.catIds = sorted(cocoGt.getCatIds())

    # ---- evaluate (:1315-1357 + computeIoU :1359-1431 + evaluateImg :1433-1551) ----------------------------------------
    def evaluate(self, device=None):
        p = self.params
        p.imgIds = list(np.unique(p.imgIds))
        p.catIds = list(np.unique(p.catIds)) if p.useCats else p.catIds
        p.maxDets = sorted(p.maxDets)
        if not p.useCats:
            raise NotImplementedError("useCats = 0 is not built on the device path")
        gts = self.cocoGt.loadAnns(self.cocoGt.getAnnIds(imgIds=p.imgIds, catIds=p.catIds))
        dts = self.cocoDt.loadAnns(self.cocoDt.getAnnIds(imgIds=p.imgIds, catIds=p.catIds))
        flag = "ignore2D" if self.mode == "2D" else "ignore3D"
        g_by, d_by = {}, {}
        for g in gts:
            g[flag] = g[flag] if flag in g else 0
            g_by.setdefault((g["image_id"], g["category_id"]), []).append(g)
        for d in dts:
            d_by.setdefault((d["image_id"], d["category_id"]), []).append(d)
        if self.mode == "DIST":
            p.distThrs = np.asarray(p.distThrs, dtype=np.float64).reshape(-1)
            if not (np.isfinite(p.distThrs).all() and (p.distThrs >= 0).all()):
                raise ValueError("distThrs must be finite and >= 0")
            if not np.any(p.distThrs == float(p.tpDist)):
                raise ValueError("tpDist %r is not one of distThrs %r" % (p.tpDist, p.distThrs.tolist()))
            if not 0.0 <= float(p.minRecall) <= 1.0:
                raise ValueError("minRecall must lie in [0, 1]")
            p.iouThrs = 1.0 / (1.0 + p.distThrs)
        if self.mode == "LET":
            try:
                p.lonTolFrac, p.lonTolMin = let.check_tolerance(p.lonTolFrac, p.lonTolMin)
            except ValueError:
                raise ValueError("lonTolFrac must be finite and >= 0, lonTolMin finite and > 0") from None
        maxDet = p.maxDets[-1]
        # group table in (category, image) order = the order evalImgs / accumulate walk (:1346-1351, :1230-1241)
        groups = []
        for ki, cat in enumerate(p.catIds):
            for ii, img in enumerate(p.imgIds):
                g, d = g_by.get((img, cat), []), d_by.get((img, cat), [])
                if not g and not d:
                    continue
                order = np.argsort([-x["score"] for x in d], kind="mergesort")
                groups.append((ki, ii, g, [d[i] for i in order[:maxDet]]))
        key = "bbox" if self.mode == "2D" else "bbox3D"
        rng_key = "area" if self.mode == "2D" else "depth"
        dt_sizes = np.array([len(gr[3]) for gr in groups], dtype=np.int64)
        gt_sizes = np.array([len(gr[2]) for gr in groups], dtype=np.int64)
        all_d = [x for gr in groups for x in gr[3]]
        all_g = [x for gr in groups for x in gr[2]]
        if device is None:
            device = torch.device("cpu") if iou3d._lib.get().emulated else torch.device("cuda")
        f32 = lambda v, shape: torch.tensor(np.asarray(v, dtype=np.float32).reshape(shape)).to(device)      # noqa: E731
        if self.mode != "2D":
            b_d, b_g = f32([x[key] for x in all_d], (-1, 8, 3)), f32([x[key] for x in all_g], (-1, 8, 3))
            if self.mode == "DIST":
                pair_err, _ = dist_errors_groups(b_d, b_g, dt_sizes, gt_sizes, up=self.up, warn=True)
                flat = (1.0 / (1.0 + pair_err[:, 0])).float()                 # in double; +inf -> 0
            elif self.mode == "LET":
                flat, pair_aff, pair_lon, _ = let_overlap_groups(b_d, b_g, dt_sizes, gt_sizes, p.lonTolFrac, p.lonTolMin, warn=True)
            else:
                mats = box3d_overlap_groups(b_d, b_g, dt_sizes, gt_sizes) if self.mode == "3D" else bev_overlap_groups(b_d, b_g, dt_sizes, gt_sizes, up=self.up)
                flat = torch.cat([m.reshape(-1) for m in mats]) if mats else torch.zeros(0, device=device)
        else:
            i1, i2, _ = _ragged_pairs(dt_sizes, gt_sizes)
            bd, bg = f32([x[key] for x in all_d], (-1, 4))[torch.from_numpy(i1).to(device)], f32([x[key] for x in all_g], (-1, 4))[torch.from_numpy(i2).to(device)]
            iw = (torch.min(bd[:, 0] + bd[:, 2], bg[:, 0] + bg[:, 2]) - torch.max(bd[:, 0], bg[:, 0])).clamp(min=0)
            ih = (torch.min(bd[:, 1] + bd[:, 3], bg[:, 1] + bg[:, 3]) - torch.max(bd[:, 1], bg[:, 1])).clamp(min=0)
            inter = iw * ih
            flat = inter / (bd[:, 2] * bd[:, 3] + bg[:, 2] * bg[:, 3] - inter)                  # pycocotools bbIou, iscrowd = 0
        far = None
        if self.eval_prox is not False and self.eval_prox is not None and len(all_d) and len(all_g):
            i1, i2, _ = _ragged_pairs(dt_sizes, gt_sizes)
            t1, t2 = torch.from_numpy(i1).to(device), torch.from_numpy(i2).to(device)
            if self.mode == "2D":
                iou2d = flat
            else:
                bd, bg = f32([x["bbox"] for x in all_d], (-1, 4))[t1], f32([x["bbox"] for x in all_g], (-1, 4))[t2]
                iw = (torch.min(bd[:, 0] + bd[:, 2], bg[:, 0] + bg[:, 2]) - torch.max(bd[:, 0], bg[:, 0])).clamp(min=0)
                ih = (torch.min(bd[:, 1] + bd[:, 3], bg[:, 1] + bg[:, 3]) - torch.max(bd[:, 1], bg[:, 1])).clamp(min=0)
                iou2d = iw * ih / (bd[:, 2] * bd[:, 3] + bg[:, 2] * bg[:, 3] - iw * ih)
            prox = iou2d > p.proximity_thresh
            if self.eval_prox is not True:            # only the images named
                chosen = set(self.eval_prox)
                applies = np.repeat(np.array([p.imgIds[gr[1]] in chosen for gr in groups], dtype=bool), dt_sizes)
                t_app = torch.from_numpy(applies).to(device)
                prox = prox | ~t_app[t1]
            else:
                t_app = torch.ones(len(all_d), dtype=torch.bool, device=device)
            flat = torch.where(prox, flat, torch.full_like(flat, -1.0))      # a pair out of proximity can never be a match
            near = torch.zeros(len(all_d), dtype=torch.int32, device=device).index_add_(0, t1, prox.to(torch.int32)) > 0
            has_gt = torch.from_numpy(np.repeat(gt_sizes > 0, dt_sizes)).to(device)
            far = ~near & has_gt & t_app
        m = evaluate_groups(flat, dt_sizes, gt_sizes, torch.tensor([int(x[flag]) for x in all_g], dtype=torch.int32, device=device),
                            f32([x[rng_key] for x in all_g], (-1,)), f32([x[rng_key] for x in all_d], (-1,)), p.areaRng, p.iouThrs)
        if far is not None:
            m["dt_ignore"] = (m["dt_ignore"].bool() | far.view(1, 1, -1)).to(m["dt_ignore"].dtype)
        self._dev = {"groups": groups, "dt_sizes": dt_sizes, "gt_sizes": gt_sizes, "match": m, "device": device,
                     "scores": np.array([x["score"] for x in all_d], dtype=np.float64),
                     "dt_ids": np.array([x.get("id", 0) for x in all_d]), "gt_ids": np.array([x.get("id", 0) for x in all_g])}
        if self.mode == "DIST":
            self._dev["pair_err"] = pair_err
        if self.mode == "LET":
            self._dev["pair_aff"], self._dev["pair_lon"] = pair_aff, pair_lon
        self._paramsEval = copy.deepcopy(self.params)
        self._evalImgs = None

    @property
    def evalImgs(self):
        """the reference's per-(category, range, image) list of dicts (:1541-1551), materialised on demand from the device
        results -- accumulate() does not need it"""
        if self._evalImgs is None and self._dev is not None:
            p, d = self._paramsEval, self._dev
            m = {k: v.cpu().numpy() for k, v in d["match"].items()}
            doff, goff = np.concatenate([[0], np.cumsum(d["dt_sizes"])]), np.concatenate([[0], np.cumsum(d["gt_sizes"])])
            where = {(ki, ii): n for n, (ki, ii, _, _) in enumerate(d["groups"])}
            out = []
            for ki, cat in enumerate(p.catIds):
                for ai, aRng in enumerate(p.areaRng):
                    for ii, img in enumerate(p.imgIds):
                        n = where.get((ki, ii))
                        if n is None:
                            out.append(None)
                            continue
                        ds, gs = slice(doff[n], doff[n + 1]), slice(goff[n], goff[n + 1])
                        order = m["gt_order"][ai, gs]
                        gids, dids = d["gt_ids"][gs], d["dt_ids"][ds]
                        dtm = m["dt_match"][ai][:, ds]
                        gtm = m["gt_match"][ai][:, gs][:, order]
                        out.append({"image_id": img, "category_id": cat, "aRng": aRng, "maxDet": p.maxDets[-1],
                                    "dtIds": list(dids), "gtIds": list(gids[order]),
                                    "dtMatches": np.where(dtm >= 0, gids[np.clip(dtm, 0, None)] if len(gids) else 0, 0).astype(np.float64),
                                    "gtMatches": np.where(gtm >= 0, dids[np.clip(gtm, 0, None)] if len(dids) else 0, 0).astype(np.float64),
                                    "dtScores": list(d["scores"][ds]), "gtIgnore": m["gt_ignore"][ai, gs][order].astype(np.float64),
                                    "dtIgnore": m["dt_ignore"][ai][:, ds].astype(bool)})
            self._evalImgs = out
        return self._evalImgs

    def _merge_tables(self, K, A):
        """the host tables accumulate() and bootstrap() hand to the device: the merge order, the rank of a detection in its image's
        list, the ground-truth counts; per (image, category) group its category, image index and non-ignored ground truths per range"""
        d = self._dev
        groups, dt_sizes, gt_sizes = d["groups"], d["dt_sizes"], d["gt_sizes"]
        sumD = int(dt_sizes.sum())
        cat_of_group = np.array([g[0] for g in groups], dtype=np.int64)
        det_cat = np.repeat(cat_of_group, dt_sizes)
        det_rank = np.concatenate([np.arange(n) for n in dt_sizes]).astype(np.int32) if len(groups) else np.zeros(0, np.int32)
        # merge order: stable by -score inside a category, categories ascending; ties keep (image, in-image) order (:1250-1253)
        order = np.lexsort((np.arange(sumD), -d["scores"], det_cat)).astype(np.int32) if sumD else np.zeros(0, np.int32)
        cat_off = np.concatenate([[0], np.cumsum(np.bincount(det_cat, minlength=K))]).astype(np.int32)
        gt_ig = d["match"]["gt_ignore"].cpu().numpy()                                   # (A, sumG)
        gcat = np.repeat(cat_of_group, gt_sizes)
        npig = np.zeros((K, A), np.int32)
        for a in range(A):
            npig[:, a] = np.bincount(gcat[gt_ig[a] == 0], minlength=K)
        has_e = np.bincount(cat_of_group, minlength=K).astype(np.int32).clip(max=1)
        return {"cat_of_group": cat_of_group, "det_rank": det_rank, "order": order, "cat_off": cat_off, "gt_ig": gt_ig, "npig": npig,
                "has_e": has_e}

    # ---- accumulate (:1172-1313) --------------------------------------------------------------------------------------
    def accumulate(self, p=None):
        assert self._dev is not None, "Please run evaluate() first"
        if p is None:
            p = self.params
        pe, d = self._paramsEval, self._dev
        if list(p.catIds) != list(pe.catIds) or list(map(tuple, p.areaRng)) != list(map(tuple, pe.areaRng)) or list(p.maxDets) != list(pe.maxDets) \
                or list(p.imgIds) != list(pe.imgIds):
            raise NotImplementedError("accumulate() with parameters other than evaluate()'s is not built on the device path")
        T, R, K, A, M = len(p.iouThrs), len(p.recThrs), len(p.catIds), len(p.areaRng), len(p.maxDets)
        dev = d["device"]
        dt_sizes, gt_sizes = d["dt_sizes"], d["gt_sizes"]
        sumD = int(dt_sizes.sum())
        tb = self._merge_tables(K, A)
        det_rank, order, cat_off, npig, has_e = tb["det_rank"], tb["order"], tb["cat_off"], tb["npig"], tb["has_e"]
        tod = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)               # noqa: E731
        prec = torch.full((T, R, K, A, M), -1.0, dtype=torch.float64, device=dev)
        rec = torch.full((T, K, A, M), -1.0, dtype=torch.float64, device=dev)
        scr = torch.full((T, R, K, A, M), -1.0, dtype=torch.float64, device=dev)
        L = iou3d._lib.get()
        _p = iou3d._lib.ptr
        t_order, t_off, t_rank, t_sc = tod(order), tod(cat_off), tod(det_rank), tod(d["scores"])
        t_npig, t_has, t_thr, t_md = tod(npig), tod(has_e), tod(np.asarray(p.recThrs, dtype=np.float64)), tod(np.asarray(p.maxDets, dtype=np.int32))
        dm, dg = d["match"]["dt_match"].contiguous(), d["match"]["dt_ignore"].contiguous()
        L.call("omni_eval_accumulate", _p(t_order), _p(t_off), _p(t_rank), _p(t_sc), _p(dm), _p(dg), _p(t_npig), _p(t_has), _p(t_thr),
               _p(t_md), K, A, M, T, R, sumD, _p(prec), _p(rec), _p(scr), iou3d._lib.stream_of(prec))
        self.eval = {"params": p, "counts": [T, R, K, A, M], "date": datetime.datetime.now().strftime("%Y-%m-%d %H:%M:%S"),
                     "precision": prec.cpu().numpy(), "recall": rec.cpu().numpy(), "scores": scr.cpu().numpy()}
        if self.mode == "DIST":
            # the lists were cut to the largest maxDets in evaluate(): every detection takes part
            ti = int(np.flatnonzero(np.asarray(pe.distThrs) == float(pe.tpDist))[0])
            pair_off = np.concatenate([[0], np.cumsum(dt_sizes * gt_sizes)])[:-1]
            pair_row = np.repeat(pair_off, dt_sizes) + det_rank.astype(np.int64) * np.repeat(gt_sizes, dt_sizes)
            tp_err, tp_cnt = tperr.tp_errors(t_order, t_off, dm[:, ti].contiguous(), dg[:, ti].contiguous(), tod(pair_row.astype(np.int64)),
                                             d["pair_err"], t_npig, t_has, t_thr, float(pe.minRecall))
            self.eval["tp_errors"], self.eval["tp_count"] = tp_err.cpu().numpy(), tp_cnt.cpu().numpy()
        if self.mode == "LET":
            pair_off = np.concatenate([[0], np.cumsum(dt_sizes * gt_sizes)])[:-1]
            pair_row = np.repeat(pair_off, dt_sizes) + det_rank.astype(np.int64) * np.repeat(gt_sizes, dt_sizes)
            prec_l, tp_aff, tp_lon = let.accumulate_let(t_order, t_off, t_rank, dm, dg, tod(pair_row.astype(np.int64)), d["pair_aff"],
                                                        d["pair_lon"], t_npig, t_has, t_thr, t_md)
            self.eval["precision_l"], self.eval["tp_affinity"], self.eval["tp_lon"] = prec_l.cpu().numpy(), tp_aff.cpu().numpy(), tp_lon.cpu().numpy()

    # ---- summarize (:1553-1704) ---------------------------------------------------------------------------------------
    def summarize(self):
        if not self.eval:
            raise Exception("Please run accumulate() first")
        p, ev, mode = self.params, self.eval, self.mode
        lines = []

        def one(ap=1, iouThr=None, areaRng="all", maxDets=100, table="precision"):
            fmt = (" {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}" if mode == "2D"
                   else " {:<18} {} @[ dist={:<9}| depth={:>6s} | maxDets={:>3d} ] = {:0.3f}" if mode == "DIST"
                   else " {:<18} {} @[ IoU={:<9} | depth={:>6s} | maxDets={:>3d} ] = {:0.3f}")
            shown = p.distThrs if mode == "DIST" else p.iouThrs            # DIST: thresholds are named, and looked up, in metres
            iouStr = "{:0.2f}:{:0.2f}".format(shown[0], shown[-1]) if iouThr is None else "{:0.2f}".format(iouThr)
            tind, aind, mind = _slot_indices(p, mode, ap, iouThr, areaRng, maxDets)
            s = ev[table] if ap == 1 else ev["recall"]
            if tind is not None:
                s = s[tind]
            s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
            mean_s = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
            name, short = ("Average Recall", "(AR)") if ap != 1 else ("Average Precision", "(AP)") if table == "precision" else ("Longitudinal Prec.", "(APL)")
            lines.append("mode={} ".format(mode) + fmt.format(name, short, iouStr, areaRng, maxDets, mean_s))
            return mean_s

        thres = _stat_thresholds(mode)
        L, md = p.areaRngLbl, p.maxDets
        stats = np.zeros((13,))
        for i, (ap, iouThr, areaRng, maxDets) in enumerate(_stat_slots(p, mode)):
            stats[i] = one(ap, iouThr=iouThr, areaRng=areaRng, maxDets=maxDets)
        self.stats = stats
        if mode == "DIST":
            aall = p.areaRngLbl.index("all")
            self.tp_stats = np.full((3,), -1.0)
            for j, (name, short) in enumerate((("Translation Error", "(mATE)"), ("Scale Error", "(mASE)"), ("Orientation Error", "(mAOE)"))):
                v = ev["tp_errors"][:, aall, j]
                self.tp_stats[j] = np.mean(v[v > -1]) if (v > -1).any() else -1.0
                lines.append("mode={} ".format(mode) + " {:<18} {} @[ dist={:<9}| depth={:>6s} | maxDets={:>3d} ] = {:0.3f}".format(
                    name, short, "{:0.2f}".format(float(p.tpDist)), "all", md[-1], self.tp_stats[j]))
        if mode == "LET":
            stats_l = np.zeros((7,))
            stats_l[0] = one(1, table="precision_l")
            for i in range(3):
                stats_l[1 + i] = one(1, iouThr=thres[i], maxDets=md[2], table="precision_l")
            for i in range(3):
                stats_l[4 + i] = one(1, areaRng=L[1 + i], maxDets=md[2], table="precision_l")
            self.stats_l = stats_l
            aall, ti = p.areaRngLbl.index("all"), np.where(np.isclose(_LET_TP_IOU, np.asarray(p.iouThrs).astype(float)))[0]
            self.let_stats = np.full((2,), -1.0)
            for j, (name, short, key) in enumerate((("Long. Affinity", "(mAFF)", "tp_affinity"), ("Long. Error [m]", "(mLON)", "tp_lon"))):
                if len(ti):                                             # tp_lon is signed: the affinity says where there is a value
                    has = ev["tp_affinity"][ti[0], :, aall, -1] > -1
                    if has.any():
                        self.let_stats[j] = np.mean(ev[key][ti[0], :, aall, -1][has])
                lines.append("mode={} ".format(mode) + " {:<18} {} @[ IoU={:<9} | depth={:>6s} | maxDets={:>3d} ] = {:0.3f}".format(
                    name, short, "{:0.2f}".format(_LET_TP_IOU), "all", md[-1], self.let_stats[j]))
        return "\n".join(lines)

    def __str__(self):
        self.summarize()

    # ---- bootstrap (extension) ----------------------------------------------------------------------------------------
    def _bootstrap_tables(self, weights, chunk=None):
        """weights (n, I) int32 -> (ap, ar) (n, T, K, A, M) float64 on the host: `kernels.bootstrap` on the tables of evaluate(),
        `chunk` rows of `weights` at a time"""
        from ...kernels import bootstrap as kb
        p, pe, d = self.params, self._paramsEval, self._dev
        if list(p.catIds) != list(pe.catIds) or list(map(tuple, p.areaRng)) != list(map(tuple, pe.areaRng)) or list(p.maxDets) != list(pe.maxDets) \
                or list(p.imgIds) != list(pe.imgIds):
            raise NotImplementedError("bootstrap() with parameters other than evaluate()'s is not built on the device path")
        chunk = BOOTSTRAP_CHUNK if chunk is None else int(chunk)
        if chunk < 1:
            raise ValueError("chunk must be >= 1")
        T, K, A, M = len(p.iouThrs), len(p.catIds), len(p.areaRng), len(p.maxDets)
        dev, groups, dt_sizes, gt_sizes = d["device"], d["groups"], d["dt_sizes"], d["gt_sizes"]
        tb = self._merge_tables(K, A)
        G = len(groups)
        grp_img = np.array([g[1] for g in groups], dtype=np.int32)
        grp_off = np.concatenate([[0], np.cumsum(np.bincount(tb["cat_of_group"], minlength=K))]).astype(np.int32)
        gid = np.repeat(np.arange(G), gt_sizes)
        grp_npig = np.zeros((G, A), np.int32)
        for a in range(A):
            grp_npig[:, a] = np.bincount(gid[tb["gt_ig"][a] == 0], minlength=G)
        tod = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)               # noqa: E731
        t_order, t_off, t_rank, t_img = tod(tb["order"]), tod(tb["cat_off"]), tod(tb["det_rank"]), tod(np.repeat(grp_img, dt_sizes).astype(np.int32))
        t_goff, t_gimg, t_gnpig = tod(grp_off), tod(grp_img), tod(grp_npig)
        t_thr, t_md = tod(np.asarray(p.recThrs, dtype=np.float64)), tod(np.asarray(p.maxDets, dtype=np.int32))
        dm, dg = d["match"]["dt_match"].contiguous(), d["match"]["dt_ignore"].contiguous()
        n = weights.shape[0]
        ap, ar = np.empty((n, T, K, A, M), np.float64), np.empty((n, T, K, A, M), np.float64)
        for c0 in range(0, n, chunk):
            w = tod(weights[c0:c0 + chunk])
            npig_b, has_e_b = kb.bootstrap_counts(t_goff, t_gimg, t_gnpig, w, sum_gt=int(gt_sizes.sum()))
            a1, a2 = kb.bootstrap_accumulate(t_order, t_off, t_rank, dm, dg, t_img, w, npig_b, has_e_b, t_thr, t_md)
            ap[c0:c0 + chunk], ar[c0:c0 + chunk] = a1.cpu().numpy(), a2.cpu().numpy()
        return ap, ar

    def bootstrap(self, n=1000, seed=0, confidence=0.95, weights=None, strata=None, chunk=None):
        """Image-level bootstrap of the AP / AR this evaluator reports (extension; call after evaluate()): is a difference in AP more
        than the luck of the test set?

        Definition.  A replicate is a vector w of len(params.imgIds) non-negative integers; its result is BY DEFINITION what this
        evaluator returns on the data set in which image i is present w[i] times, each copy with copies of its ground truths and
        detections (w[i] = 0: absent), the copies adjacent in the image order.  evaluate() matches per (image, category), so the match
        tables stay; only accumulate() is redone, for all replicates in one launch (`omni_eval_bootstrap`, csrc/eval_bootstrap.hip): in
        the merge order of accumulate() a detection counts as w consecutive identical entries; npig and "has an evaluated image" are the
        weighted sums over the (image, category) groups; precision at the last copy of a true positive is TP / (FP + TP + eps) on the
        weighted inclusive sums, and it serves the recall thresholds in ((TP - w) / npig, TP / npig].  When several detections of a
        category tie in score this weighted order is the definition (a physically duplicated data set would interleave them).
        Scope: `precision` (as its mean over the recall thresholds) and `recall` of all five modes, which share the match tables.  Out
        of scope: the true-positive errors of mode "DIST" and `precision_l` / the affinity tables of mode "LET".

        weights: explicit replicates, (n, I) integers >= 0, columns in the order of params.imgIds (ValueError otherwise).  Without
        them n rows are drawn: g = np.random.default_rng(seed); the strata in sorted label order; a stratum of n_s images fills its
        columns with g.multinomial(n_s, np.full(n_s, 1 / n_s), size=n), so every row sums to I.  strata: None = one stratum, or a
        mapping image id -> label: images are resampled within their label.  chunk: the replicates go to the device `chunk` rows at a
        time (default BOOTSTRAP_CHUNK = 256: the weight table and the two result tables of a chunk take 256 x (4 I + 16 T K A M)
        bytes there); the result does not depend on it, bit for bit.  ValueError when (number of detections or of ground truths) x
        (largest weight) >= 2^31: the weighted counts are 32-bit.

        -> dict: `weights` (n, I) int32; `ap`, `ar` (n, T, K, A, M) float64, -1 where accumulate() leaves -1; `stats` (n, 13) the
        slots of summarize() per replicate (each the mean over the thresholds and categories with a value of `ap` or `ar`); `point`
        (13,) the same from the all-ones replicate = the data set itself; `mean`, `se` (std, ddof=1) and `n_valid` (13,) over the
        replicates whose slot is > -1, `ci` (13, 2) = np.quantile of those at (1 - confidence) / 2 and (1 + confidence) / 2 (NaN
        without a valid replicate, `se` NaN with fewer than two); `per_category`: a dict of the same (`point`, `values` (n, K),
        `mean`, `se`, `n_valid` (K,), `ci` (K, 2)) for the per-category AP at range "all" and the largest maxDets, averaged over the
        thresholds."""
        if self._dev is None:
            raise Exception("Please run evaluate() first")
        confidence = _check_confidence(confidence)
        W = bootstrap_weights(self._paramsEval.imgIds, n, seed, weights, strata)
        ap, ar = self._bootstrap_tables(np.concatenate([np.ones((1, W.shape[1]), np.int32), W]), chunk)      # row 0: the point estimate
        return _bootstrap_result(self.params, self.mode, W, ap, ar, confidence)


# =====================================================================================================================
# prediction plumbing around it (f-3): instances -> COCO-style records, the inference loop, the evaluator object
# =====================================================================================================================
def instances_to_coco_json(instances, img_id):
    """omni3d_evaluation.py:970-1013.  The reference converts each field with its own `.tolist()` after a per-field device
    copy and averages the corner depths one box at a time in numpy; here one host copy per field and a vectorised depth."""
    n = len(instances)
    if n == 0:
        return []
    cpu = instances.to("cpu") if instances.pred_boxes.tensor.is_cuda else instances
    xyxy = cpu.pred_boxes.tensor.numpy()
    boxes = np.concatenate([xyxy[:, :2], xyxy[:, 2:] - xyxy[:, :2]], axis=1).tolist()          # XYXY_ABS -> XYWH_ABS
    scores, classes = cpu.scores.tolist(), cpu.pred_classes.tolist()
    if cpu.has("pred_bbox3D"):
        b3 = cpu.pred_bbox3D.numpy()
        depth = b3[:, :, 2].mean(axis=1).tolist()
        bbox3D, center_cam, center_2D = b3.tolist(), cpu.pred_center_cam.tolist(), cpu.pred_center_2D.tolist()
        dimensions, pose = cpu.pred_dimensions.tolist(), cpu.pred_pose.tolist()
    else:
        bbox3D, center_cam, center_2D = np.ones([n, 8, 3]).tolist(), np.ones([n, 3]).tolist(), np.ones([n, 2]).tolist()
        dimensions, pose, depth = np.ones([n, 3]).tolist(), np.ones([n, 3, 3]).tolist(), [1.0] * n
    return [{"image_id": img_id, "category_id": classes[k], "bbox": boxes[k], "score": scores[k], "depth": depth[k], "bbox3D": bbox3D[k],
             "center_cam": center_cam[k], "center_2D": center_2D[k], "dimensions": dimensions[k], "pose": pose[k]} for k in range(n)]


def inference_on_dataset(model, data_loader):
    """omni3d_evaluation.py:522-640 without the timing / logging: model in eval mode over the loader -> list of
    {'image_id', 'K', 'width', 'height', 'instances': [COCO-style records]}"""
    was_training = model.training
    model.eval()
    out = []
    with torch.no_grad():
        for inputs in data_loader:
            outputs = model(inputs)
            for inp, o in zip(inputs, outputs):
                out.append({"image_id": inp["image_id"], "K": inp["K"], "width": inp["width"], "height": inp["height"],
                            "instances": instances_to_coco_json(o["instances"], inp["image_id"])})
    model.train(was_training)
    return out


_METRICS = {"2D": ["AP", "AP50", "AP75", "AP95", "APs", "APm", "APl"], "3D": ["AP", "AP15", "AP25", "AP50", "APn", "APm", "APf"]}
_METRICS["BEV"] = _METRICS["3D"]
_METRICS["DIST"] = ["AP", "AP@0.5m", "AP@1m", "AP@2m", "APn", "APm", "APf"]
_METRICS["LET"] = _METRICS["3D"]
_LET_TP_IOU = 0.25                         # the threshold at which summarize() reports mean affinity and longitudinal error
_TP_NAMES = ("ATE", "ASE", "AOE")          # metres, 1 - IoU of the aligned boxes, radians: not scaled by 100


def _derive_results(ev, mode, class_names):
    """omni3d_evaluation.py:765-846: the seven headline numbers (x100, NaN when undefined) + per-category AP ('AP-<name>': mean
    of the precision table over thresholds and recall points at area 'all', maxDets 100)"""
    res = {name: float(ev.stats[i] * 100 if ev.stats[i] >= 0 else "nan") for i, name in enumerate(_METRICS[mode])}
    if mode == "DIST":
        res.update({"m" + n: float(ev.tp_stats[j] if ev.tp_stats[j] > -1 else "nan") for j, n in enumerate(_TP_NAMES)})
    if mode == "LET":                      # the same seven slots on the longitudinal precision, and the two diagnostics (not x100)
        res.update({name.replace("AP", "APL", 1): float(ev.stats_l[i] * 100 if ev.stats_l[i] >= 0 else "nan") for i, name in enumerate(_METRICS[mode])})
        res["mAFF"] = float(ev.let_stats[0] if ev.let_stats[0] > -1 else "nan")
        res["mLON"] = float(ev.let_stats[1] if ev.let_stats[0] > -1 else "nan")
    if class_names is None or len(class_names) <= 1:
        return res
    prec = ev.eval["precision"]
    assert len(class_names) == prec.shape[2], (len(class_names), prec.shape)
    for k, name in enumerate(class_names):
        vals = prec[:, :, k, 0, -1]
        vals = vals[vals > -1]
        res["AP-" + name] = float(np.mean(vals) * 100) if vals.size else float("nan")
        if mode == "DIST":
            tp = ev.eval["tp_errors"][k, 0]
            res.update({n + "-" + name: float(tp[j] if tp[j] > -1 else "nan") for j, n in enumerate(_TP_NAMES)})
        if mode == "LET":
            vals = ev.eval["precision_l"][:, :, k, 0, -1]
            vals = vals[vals > -1]
            res["APL-" + name] = float(np.mean(vals) * 100) if vals.size else float("nan")
    return res


def _dist_up(up):
    """None, or the unit vector along three finite numbers (ValueError otherwise)"""
    return None if up is None else tperr.unit_up(up)


_DIST_KEYS = ("distThrs", "tpDist", "minRecall")


def _dist_params(params):
    """None or a dict with some of distThrs / tpDist / minRecall -> a checked copy"""
    if params is None:
        return {}
    if not isinstance(params, dict) or set(params) - set(_DIST_KEYS):
        raise ValueError("dist_params must be a dict with keys out of %r" % (_DIST_KEYS,))
    out = dict(params)
    if "distThrs" in out:
        out["distThrs"] = [float(v) for v in out["distThrs"]]
    thrs = out.get("distThrs", Omni3DParams("DIST").distThrs.tolist())
    if float(out.get("tpDist", Omni3DParams("DIST").tpDist)) not in thrs:
        raise ValueError("tpDist must be one of distThrs")
    return out


_LET_KEYS = ("lonTolFrac", "lonTolMin")


def _let_params(params):
    """None or a dict with some of lonTolFrac / lonTolMin -> a checked copy"""
    if params is None:
        return {}
    if not isinstance(params, dict) or set(params) - set(_LET_KEYS):
        raise ValueError("let_params must be a dict with keys out of %r" % (_LET_KEYS,))
    frac, tmin = let.check_tolerance(params.get("lonTolFrac", let.TOL_FRAC), params.get("lonTolMin", let.TOL_MIN))
    return {k: v for k, v in (("lonTolFrac", frac), ("lonTolMin", tmin)) if k in params}


_BOOTSTRAP_KEYS = ("n", "seed", "confidence")


def _bootstrap_params(params):
    """None (off) or a dict with some of n / seed / confidence -> None or the checked, completed dict"""
    if params is None:
        return None
    if not isinstance(params, dict) or set(params) - set(_BOOTSTRAP_KEYS):
        raise ValueError("bootstrap must be None or a dict with keys out of %r" % (_BOOTSTRAP_KEYS,))
    n, seed = params.get("n", 1000), params.get("seed", 0)
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError("bootstrap n must be a positive integer")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or seed < 0:
        raise ValueError("bootstrap seed must be a non-negative integer")
    return {"n": int(n), "seed": int(seed), "confidence": _check_confidence(params.get("confidence", 0.95))}


def _bootstrap_ci(ev, mode, class_names, params, strata=None):
    """the percentile intervals of `ev.bootstrap(**params, strata=strata)` in the layout of `_derive_results`: the seven headline
    numbers and 'AP-<name>' per category, each (lo, hi) x 100 (NaN, NaN without a valid replicate)"""
    bs = ev.bootstrap(strata=strata, **params)
    pair = lambda row: (float(row[0] * 100), float(row[1] * 100))                      # noqa: E731
    res = {name: pair(bs["ci"][i]) for i, name in enumerate(_METRICS[mode])}
    if class_names is not None and len(class_names) > 1:
        assert len(class_names) == bs["per_category"]["ci"].shape[0], (len(class_names), bs["per_category"]["ci"].shape)
        res.update({"AP-" + name: pair(bs["per_category"]["ci"][k]) for k, name in enumerate(class_names)})
    return res


def _make_eval(gt, dt, mode, eval_prox, bev_up, dist_up, dist_params, let_params=None):
    """the Omni3Deval of one pass of the drivers: `up` is the BEV ground plane, except in mode DIST, which has its own"""
    ev = Omni3Deval(gt, dt, mode=mode, eval_prox=eval_prox, up=dist_up if mode == "DIST" else bev_up)
    if mode == "DIST":
        for key, value in dist_params.items():
            setattr(ev.params, key, np.asarray(value, dtype=np.float64) if key == "distThrs" else float(value))
    if mode == "LET":
        for key, value in (let_params or {}).items():
            setattr(ev.params, key, float(value))
    return ev


class Omni3DEvaluator:
    """Per-dataset evaluator (reference :643-935, a detectron2 COCOEvaluator subclass).

    Reference form: `Omni3DEvaluator(dataset_name, output_dir=..., filter_settings=..., only_2d=..., eval_prox=..., distributed=...)`
    -- the ground truth is the dataset's registered annotation file read through `Omni3D([json_file], filter_settings)`;
    predictions are per-image dicts {'image_id', 'K', 'width', 'height', 'instances': [records with CONTIGUOUS category ids]}.
    `evaluate()` maps the categories back to dataset ids, keeps the dataset's own categories, writes
    `omni_instances_results.json`, runs Omni3Deval in 2D (and 3D) and returns {'bbox_2D': {...}, 'bbox_3D': {...},
    'log_str_2D', 'log_str_3D', 'bbox_*_merge'} ('*_merge' = what the helper needs to score the union of several datasets; the
    reference caches per-image match tables under '*_evals_per_cat_area' for the same purpose).

    Short form (in-memory ground truth): `Omni3DEvaluator(gt_annotations, img_ids, cat_ids, only_2d)` with
    `process(inputs, outputs)` taking model outputs -> {'bbox': {'AP2D', 'AP3D', 'omni_eval_*'}}.

    eval_bev (extension, off by default; `bev_up` = the up vector of the ground plane in the camera frame): unless only_2d, a third
    pass in mode 'BEV' adds 'bbox_BEV', 'log_str_BEV', 'bbox_BEV_merge' (short form: 'APBEV', 'omni_eval_BEV'); nothing else changes.

    eval_dist (extension, off by default; `dist_up` = None for the full 3D distance or the up vector of the ground plane; `dist_params`
    = optional dict of `distThrs` / `tpDist` / `minRecall` set on the pass's params): unless only_2d, one more pass in mode 'DIST'
    after 3D and BEV adds 'bbox_DIST' (the headline APs, 'AP-<name>', 'ATE-<name>', 'ASE-<name>', 'AOE-<name>', 'mATE', 'mASE',
    'mAOE'), 'log_str_DIST', 'bbox_DIST_merge' (short form: 'APDIST', 'omni_eval_DIST'); nothing else changes.

    eval_let (extension, off by default; `let_params` = optional dict of `lonTolFrac` / `lonTolMin` set on the pass's params): unless
    only_2d, one more pass in mode 'LET' after 3D, BEV and DIST adds 'bbox_LET' (LET-AP in the headline slots of the 3D protocol,
    LET-APL as 'APL', 'APL15', ..., 'AP-<name>', 'APL-<name>', 'mAFF', 'mLON'), 'log_str_LET', 'bbox_LET_merge' (short form: 'APLET',
    'omni_eval_LET'); nothing else changes.

    bootstrap (extension, off by default; None or a dict with some of `n` (1000), `seed` (0), `confidence` (0.95)): every evaluated
    mode also gets 'bbox_<mode>_ci': the image-level bootstrap percentile intervals (`Omni3Deval.bootstrap`) of the seven headline
    numbers of 'bbox_<mode>' and of 'AP-<name>' per category, each (lo, hi) x 100 (short form: 'AP<mode>_ci'); nothing else changes."""

    def __init__(self, dataset_name, tasks=None, distributed=True, output_dir=None, *, max_dets_per_image=None, use_fast_impl=False,
                 eval_prox=False, only_2d=False, filter_settings=None, img_ids=None, cat_ids=None, eval_bev=False, bev_up=BEV_UP,
                 eval_dist=False, dist_up=None, dist_params=None, eval_let=False, let_params=None, bootstrap=None):
        self._only_2d, self._eval_prox, self._output_dir, self._distributed = only_2d, eval_prox, output_dir, distributed
        self._bootstrap = _bootstrap_params(bootstrap)
        self._eval_let, self._let_params = bool(eval_let), _let_params(let_params)
        self._eval_bev, self._bev_up = bool(eval_bev), tuple(float(v) for v in bev_up)
        self._eval_dist, self._dist_up, self._dist_params = bool(eval_dist), _dist_up(dist_up), _dist_params(dist_params)
        if not isinstance(dataset_name, str):                   # short form: (gt_annotations, img_ids, cat_ids, only_2d)
            self._gt, self._omni_api = dataset_name, None
            self._img_ids = tasks if tasks is not None else img_ids
            self._cat_ids = cat_ids if isinstance(distributed, bool) else distributed
            if output_dir is not None and not isinstance(output_dir, str):
                self._only_2d, self._output_dir = bool(output_dir), None
            self.reset()
            return
        from ...d2.data import MetadataCatalog
        from ..data.datasets import Omni3D
        self._filter_settings = filter_settings if filter_settings is not None else {}
        self._metadata = MetadataCatalog.get(dataset_name)
        self._omni_api = Omni3D([self._metadata.json_file], self._filter_settings)
        self._do_evaluation = "annotations" in self._omni_api.dataset
        self.reset()

    def reset(self):
        self._predictions = []
        self._results = {}

    def process(self, inputs, outputs):
        for inp, o in zip(inputs, outputs):
            recs = o["instances"] if isinstance(o["instances"], list) else instances_to_coco_json(o["instances"], inp["image_id"])
            if self._omni_api is None:
                self._predictions.extend(recs)
            else:
                pred = {"image_id": inp["image_id"], "K": inp["K"], "width": inp["width"], "height": inp["height"], "instances": recs}
                if "p2" in inp:
                    pred["p2"] = inp["p2"]
                self._predictions.append(pred)

    def _modes(self):
        """2D, 3D unless only_2d, and -- extensions the reference does not have, off by default -- BEV, DIST and LET after them"""
        return ["2D"] if self._only_2d else ["2D", "3D"] + (["BEV"] if self._eval_bev else []) + (["DIST"] if self._eval_dist else []) \
            + (["LET"] if self._eval_let else [])

    def _make_eval(self, gt, dt, mode, eval_prox=False):
        return _make_eval(gt, dt, mode, eval_prox, self._bev_up, self._dist_up, self._dist_params, self._let_params)

    def _evaluate_short(self):
        res = {}
        for mode in self._modes():
            ev = self._make_eval(AnnotationIndex(copy.deepcopy(self._gt), self._img_ids, self._cat_ids),
                                 AnnotationIndex(copy.deepcopy(self._predictions), self._img_ids, self._cat_ids), mode)
            ev.evaluate()
            ev.accumulate()
            ev.summarize()
            res["AP" + mode] = float(ev.stats[0] * 100)
            res["omni_eval_" + mode] = ev
            if self._bootstrap is not None:
                res["AP" + mode + "_ci"] = _bootstrap_ci(ev, mode, None, self._bootstrap)["AP"]
        return {"bbox": res}

    def evaluate(self, img_ids=None):
        if self._omni_api is None:
            return self._evaluate_short()
        from ...d2.data import MetadataCatalog
        predictions = self._predictions
        if self._distributed:
            from ...d2 import comm
            comm.synchronize()
            gathered = comm.gather(predictions, dst=0)
            predictions = [x for part in gathered for x in part]
            if not comm.is_main_process():
                return {}
        self._results = {}
        if len(predictions) == 0:
            logging.getLogger(__name__).warning("[Omni3DEvaluator] Did not receive valid predictions.")
            return {}
        if self._output_dir:
            os.makedirs(self._output_dir, exist_ok=True)
            torch.save(predictions, os.path.join(self._output_dir, "instances_predictions.pth"))
        model_meta = MetadataCatalog.get("omni3d_model")
        model_classes = model_meta.thing_classes
        # the split's own tables are filled in when its dataset dicts are loaded (load_omni3d_json); without a loader run the
        # model's id table and the categories of the annotation file stand in (they are what the loader would have stored)
        id_map = self._metadata.get("thing_dataset_id_to_contiguous_id") or model_meta.thing_dataset_id_to_contiguous_id
        split_classes = self._metadata.get("thing_classes") or [c["name"] for c in sorted(self._omni_api.dataset["categories"], key=lambda c: c["id"])]
        to_dataset_id = {v: k for k, v in id_map.items()}
        num_classes = len(to_dataset_id)
        kept = []
        for rec in (r for pred in predictions for r in pred["instances"]):
            c = rec["category_id"]
            assert c < num_classes, f"A prediction has class={c}, but the model only has {num_classes} classes"
            if model_classes[c] in split_classes:                         # categories this dataset is annotated for
                r = dict(rec)
                r["category_id"] = to_dataset_id[c]
                kept.append(r)
        if self._output_dir:
            with open(os.path.join(self._output_dir, "omni_instances_results.json"), "w") as f:
                json.dump(kept, f)
        if not self._do_evaluation or len(kept) == 0:
            return copy.deepcopy(self._results)
        omni_dt = self._omni_api.loadRes(kept)
        for mode in self._modes():
            ev = self._make_eval(self._omni_api, omni_dt, mode, self._eval_prox)
            if img_ids is not None:
                ev.params.imgIds = img_ids
            ev.evaluate()
            ev.accumulate()
            self._results["log_str_" + mode] = ev.summarize()
            self._results["bbox_" + mode] = _derive_results(ev, mode, split_classes)
            if self._bootstrap is not None:
                self._results["bbox_" + mode + "_ci"] = _bootstrap_ci(ev, mode, split_classes, self._bootstrap)
            self._results["bbox_" + mode + "_merge"] = {"gt": self._omni_api, "dt": kept, "eval_prox": self._eval_prox,
                                                        "img_ids": list(ev.params.imgIds), "cat_ids": list(ev.params.catIds)}
        return copy.deepcopy({k: v for k, v in self._results.items() if not k.endswith("_merge")}) | \
            {k: v for k, v in self._results.items() if k.endswith("_merge")}


class Omni3DEvaluationHelper:
    """omni3d_evaluation.py:168-520: one `Omni3DEvaluator` per test split, their printed tables, and `summarize_all()` = the
    metrics of the union of all splits (<Concat>) plus the Omni3D / Omni3D_In / Omni3D_Out aggregates.  Needs
    `MetadataCatalog.get('omni3d_model').{thing_classes, thing_dataset_id_to_contiguous_id}`.  The union is scored by one
    evaluation over the concatenated ground truth and detections (images of different splits are disjoint, so this equals the
    reference's concatenation of cached per-image match tables), with proximity evaluation applied to the images of the splits
    that use it.

    bootstrap (extension, off by default; None or the dict `Omni3DEvaluator` takes): every split's result gets 'bbox_<mode>_ci', and
    `results_ci[name]` = {'iters', 'AP2D': (lo, hi), 'AP3D': (lo, hi)}: the bootstrap intervals (x 100) of the evaluator's AP in modes
    2D and 3D, i.e. of the mean of the per-category APs the AP2D / AP3D columns show.  For <Concat> the images are resampled within
    the split they come from (strata), so every replicate keeps the splits' sizes.  The printed tables do not change."""

    def __init__(self, dataset_names, filter_settings, output_folder, iter_label="-", only_2d=False, eval_bev=False, bev_up=BEV_UP,
                 eval_dist=False, dist_up=None, dist_params=None, eval_let=False, let_params=None, bootstrap=None):
        from collections import OrderedDict
        from ...d2.data import MetadataCatalog
        from ..data.datasets import simple_register
        self.dataset_names, self.filter_settings, self.output_folder = list(dataset_names), filter_settings, output_folder
        self.iter_label, self.only_2d = iter_label, only_2d
        self.evaluators, self.results = OrderedDict(), OrderedDict()
        self.results_analysis, self.results_omni3d = OrderedDict(), OrderedDict()
        # extension (off by default): AP in the bird's-eye view per split and for <Concat>, in `results_bev`
        self.eval_bev, self.bev_up, self.results_bev = bool(eval_bev) and not only_2d, tuple(float(v) for v in bev_up), OrderedDict()
        # extension (off by default): centre-distance AP and ATE / ASE / AOE per split and for <Concat>, in `results_dist`
        self.eval_dist, self.dist_up, self.dist_params = bool(eval_dist) and not only_2d, _dist_up(dist_up), _dist_params(dist_params)
        self.results_dist = OrderedDict()
        # extension (off by default): LET-AP / LET-APL and the longitudinal diagnostics per split and for <Concat>, in `results_let`
        self.eval_let, self.let_params, self.results_let = bool(eval_let) and not only_2d, _let_params(let_params), OrderedDict()
        # extension (off by default): bootstrap intervals of AP2D / AP3D per split and for <Concat>, in `results_ci`
        self.bootstrap, self.results_ci = _bootstrap_params(bootstrap), OrderedDict()
        self.overall_imgIds, self.overall_catIds = set(), set()
        self.output_folders = {n: os.path.join(output_folder, n) for n in self.dataset_names}
        for name in self.dataset_names:
            if MetadataCatalog.get(name).get("json_file") is None:
                simple_register(name, filter_settings, filter_empty=False)
            ev = Omni3DEvaluator(name, output_dir=self.output_folders[name], filter_settings=filter_settings, only_2d=only_2d,
                                 eval_prox=("Objectron" in name or "SUNRGBD" in name), distributed=False, eval_bev=self.eval_bev,
                                 bev_up=self.bev_up, eval_dist=self.eval_dist, dist_up=self.dist_up, dist_params=self.dist_params,
                                 eval_let=self.eval_let, let_params=self.let_params, bootstrap=self.bootstrap)
            ev.reset()
            self.evaluators[name] = ev
            self.overall_imgIds.update(ev._omni_api.getImgIds())
            self.overall_catIds.update(ev._omni_api.getCatIds())

    def add_predictions(self, dataset_name, predictions):
        self.evaluators[dataset_name]._predictions += predictions

    def save_predictions(self, dataset_name):
        os.makedirs(self.output_folders[dataset_name], exist_ok=True)
        torch.save(self.evaluators[dataset_name]._predictions, os.path.join(self.output_folders[dataset_name], "instances_predictions.pth"))

    @staticmethod
    def _mean(values):
        values = list(values)
        return float(np.mean(values)) if values else float("nan")

    def _bev_row(self, rb, categories):
        """the row of `results_bev`: APBEV = mean of the per-category APs like AP3D, then the headline columns"""
        return {"iters": self.iter_label, "APBEV": self._mean(rb["AP-" + c] for c in categories if "AP-" + c in rb),
                "APBEV@15": rb["AP15"], "APBEV@25": rb["AP25"], "APBEV@50": rb["AP50"], "APBEV-N": rb["APn"], "APBEV-M": rb["APm"],
                "APBEV-F": rb["APf"]}

    def _dist_row(self, rd, categories):
        """the row of `results_dist`: APDIST = mean of the per-category APs like AP3D, the headline columns, the three mean errors"""
        return {"iters": self.iter_label, "APDIST": self._mean(rd["AP-" + c] for c in categories if "AP-" + c in rd),
                "APDIST@0.5m": rd["AP@0.5m"], "APDIST@1m": rd["AP@1m"], "APDIST@2m": rd["AP@2m"], "APDIST-N": rd["APn"],
                "APDIST-M": rd["APm"], "APDIST-F": rd["APf"], "mATE": rd["mATE"], "mASE": rd["mASE"], "mAOE": rd["mAOE"]}

    def _let_row(self, rl, categories):
        """the row of `results_let`: APLET / APLLET = means of the per-category LET-AP / LET-APL like AP3D, the headline columns of
        both, the mean affinity and the mean signed longitudinal error (metres) of the true positives"""
        return {"iters": self.iter_label, "APLET": self._mean(rl["AP-" + c] for c in categories if "AP-" + c in rl),
                "APLET@15": rl["AP15"], "APLET@25": rl["AP25"], "APLET@50": rl["AP50"], "APLET-N": rl["APn"], "APLET-M": rl["APm"],
                "APLET-F": rl["APf"], "APLLET": self._mean(rl["APL-" + c] for c in categories if "APL-" + c in rl),
                "APLLET@15": rl["APL15"], "APLLET@25": rl["APL25"], "APLLET@50": rl["APL50"], "APLLET-N": rl["APLn"],
                "APLLET-M": rl["APLm"], "APLLET-F": rl["APLf"], "mAFF": rl["mAFF"], "mLON": rl["mLON"]}

    def _ci_row(self, c2, c3):
        """the row of `results_ci`: the intervals of the evaluator's AP in modes 2D and 3D"""
        nan2 = (float("nan"), float("nan"))
        return {"iters": self.iter_label, "AP2D": c2["AP"] if c2 else nan2, "AP3D": c3["AP"] if c3 and not self.only_2d else nan2}

    def _aggregates(self, res2d, res3d, categories):
        nan = float("nan")
        out = {"AP2D": self._mean(res2d["AP-" + c] for c in categories), "AP3D": nan}
        if not self.only_2d:
            out["AP3D"] = self._mean(res3d["AP-" + c] for c in categories)
        return out

    def evaluate(self, dataset_name):
        from ..data.datasets import get_omni3d_categories
        from ..vis import logperf
        log = logging.getLogger(__name__)
        if dataset_name not in self.results:
            self.results[dataset_name] = self.evaluators[dataset_name].evaluate()
        res = self.results[dataset_name]
        tag = "{} iter={} mode=".format(dataset_name, self.iter_label)
        log.info("\n" + res["log_str_2D"].replace("mode=2D", tag + "2D"))
        if not self.only_2d:
            log.info("\n" + res["log_str_3D"].replace("mode=3D", tag + "3D"))
        if self.eval_bev and "log_str_BEV" in res:
            log.info("\n" + res["log_str_BEV"].replace("mode=BEV", tag + "BEV"))
        if self.eval_dist and "log_str_DIST" in res:
            log.info("\n" + res["log_str_DIST"].replace("mode=DIST", tag + "DIST"))
        if self.eval_let and "log_str_LET" in res:
            log.info("\n" + res["log_str_LET"].replace("mode=LET", tag + "LET"))
        names = self.filter_settings["category_names"]
        r2, r3 = res["bbox_2D"], res.get("bbox_3D", {})
        present = {c for c in names if "AP-" + c in r2}
        general = self._aggregates(r2, r3, present)
        omni = {"AP2D": float("nan"), "AP3D": float("nan")}
        split_cats = get_omni3d_categories(dataset_name)
        if len(split_cats - present) == 0:
            omni = self._aggregates(r2, r3, split_cats)
        self.results_omni3d[dataset_name] = {"iters": self.iter_label, **omni}
        extras = {k: (r3[k] if not self.only_2d else float("nan")) for k in ("AP15", "AP25", "AP50", "APn", "APm", "APf")}
        self.results_analysis[dataset_name] = {"iters": self.iter_label, "AP2D": general["AP2D"], "AP3D": general["AP3D"],
                                               "AP3D@15": extras["AP15"], "AP3D@25": extras["AP25"], "AP3D@50": extras["AP50"],
                                               "AP3D-N": extras["APn"], "AP3D-M": extras["APm"], "AP3D-F": extras["APf"]}
        if self.eval_bev and "bbox_BEV" in res:
            self.results_bev[dataset_name] = self._bev_row(res["bbox_BEV"], present)
        if self.eval_dist and "bbox_DIST" in res:
            self.results_dist[dataset_name] = self._dist_row(res["bbox_DIST"], present)
        if self.eval_let and "bbox_LET" in res:
            self.results_let[dataset_name] = self._let_row(res["bbox_LET"], present)
        if self.bootstrap is not None and "bbox_2D_ci" in res:
            self.results_ci[dataset_name] = self._ci_row(res["bbox_2D_ci"], res.get("bbox_3D_ci"))
            log.info("{} iter={} bootstrap {:g} % intervals (n={}): {}".format(dataset_name, self.iter_label, 100 * self.bootstrap["confidence"],
                                                                            self.bootstrap["n"], self.results_ci[dataset_name]))
        logperf.print_ap_category_histogram(dataset_name, self._per_category(r2, r3))

    def _per_category(self, r2, r3):
        from collections import OrderedDict
        out = OrderedDict()
        for c in self.filter_settings["category_names"]:
            a2 = r2.get("AP-" + c, float("nan"))
            a3 = r3.get("AP-" + c, float("nan")) if not self.only_2d else float("nan")
            if not np.isnan(a2) or not np.isnan(a3):
                out[c] = {"AP2D": a2, "AP3D": a3}
        return out

    def summarize_all(self):
        from ...d2.data import MetadataCatalog
        from ..data.datasets import get_omni3d_categories
        from ..vis import logperf
        for name in self.dataset_names:
            if name not in self.results:
                self.evaluate(name)
        meta = MetadataCatalog.get("omni3d_model")
        cat_ids = sorted(self.overall_catIds)
        ordered = [meta.thing_classes[meta.thing_dataset_id_to_contiguous_id[c]] for c in cat_ids]
        categories = set(ordered)
        merged, merged_ci = {}, {}
        for mode in (["2D"] if self.only_2d else ["2D", "3D"] + (["BEV"] if self.eval_bev else []) + (["DIST"] if self.eval_dist else [])
                     + (["LET"] if self.eval_let else [])):
            gts, dts, prox_imgs, strata = [], [], set(), {}
            for name in self.dataset_names:
                rec = self.results[name].get("bbox_" + mode + "_merge")
                if rec is None:
                    continue
                gts += rec["gt"].loadAnns(rec["gt"].getAnnIds(imgIds=rec["img_ids"], catIds=rec["cat_ids"]))
                dts += rec["dt"]
                if rec["eval_prox"]:
                    prox_imgs.update(rec["img_ids"])
                strata.update({i: name for i in rec["img_ids"]})
            ev = _make_eval(AnnotationIndex(copy.deepcopy(gts), self.overall_imgIds, cat_ids),
                            AnnotationIndex(copy.deepcopy(dts), self.overall_imgIds, cat_ids), mode,
                            (prox_imgs if prox_imgs else False), self.bev_up, self.dist_up, self.dist_params, self.let_params)
            ev.evaluate()
            ev.accumulate()
            ev.summarize()
            merged[mode] = _derive_results(ev, mode, ordered if len(ordered) > 1 else None)
            if self.bootstrap is not None and mode in ("2D", "3D"):
                # an image no split lists (it has no prediction record) is a stratum of its own kind
                merged_ci[mode] = _bootstrap_ci(ev, mode, None, self.bootstrap, strata={i: strata.get(i, "") for i in ev.params.imgIds})
            if len(ordered) == 1:       # _derive_results skips the per-category part for a single class
                merged[mode]["AP-" + ordered[0]] = merged[mode]["AP"]
                if mode == "DIST":
                    merged[mode].update({n + "-" + ordered[0]: merged[mode]["m" + n] for n in _TP_NAMES})
                if mode == "LET":
                    merged[mode]["APL-" + ordered[0]] = merged[mode]["APL"]
        r2, r3 = merged["2D"], merged.get("3D", {})
        if "BEV" in merged:
            self.results_bev["<Concat>"] = self._bev_row(merged["BEV"], categories)
        if "DIST" in merged:
            self.results_dist["<Concat>"] = self._dist_row(merged["DIST"], categories)
        if "LET" in merged:
            self.results_let["<Concat>"] = self._let_row(merged["LET"], categories)
        if "2D" in merged_ci:
            self.results_ci["<Concat>"] = self._ci_row(merged_ci["2D"], merged_ci.get("3D"))
        general = self._aggregates(r2, r3, categories)
        extras = {k: (r3[k] if not self.only_2d else float("nan")) for k in ("AP15", "AP25", "AP50", "APn", "APm", "APf")}
        self.results_analysis["<Concat>"] = {"iters": self.iter_label, "AP2D": general["AP2D"], "AP3D": general["AP3D"],
                                             "AP3D@15": extras["AP15"], "AP3D@25": extras["AP25"], "AP3D@50": extras["AP50"],
                                             "AP3D-N": extras["APn"], "AP3D-M": extras["APm"], "AP3D-F": extras["APf"]}
        for label, key in (("Omni3D_Out", "omni3d_out"), ("Omni3D_In", "omni3d_in"), ("Omni3D", "omni3d")):
            want = get_omni3d_categories(key)
            agg = self._aggregates(r2, r3, want) if len(want - categories) == 0 else {"AP2D": float("nan"), "AP3D": float("nan")}
            self.results_omni3d[label] = {"iters": self.iter_label, **agg}
        logperf.print_ap_category_histogram("<Concat>", self._per_category(r2, r3))
        logperf.print_ap_analysis_histogram(self.results_analysis)
        logperf.print_ap_omni_histogram(self.results_omni3d)
        return self.results_analysis, self.results_omni3d
