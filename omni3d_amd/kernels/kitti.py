"""Launchers of csrc/eval_kitti.hip: the KITTI object benchmark's protocol (AP|R40 / AP|R11 per class, difficulty, metric and overlap
set) for `cubercnn.evaluation.kitti.KittiEval`.  The reference has no counterpart; the protocol is stated in include/omni3d_hip.h and,
in float64, in tests/exact_kitti.py.  Device tensors in, device tensors out; the tensor arguments are checked by `kernels/_args.py`.

A `Problem` holds one packed data set (per-image row ranges, per-row quantities, the similarity matrices and the small tables);
`match_tp`, `thresholds`, `match_counts` and `finalize` are the four launches and `run` chains them without a host round trip.

AOS (the benchmark's average orientation similarity; like the rest a reading of the devkit written from memory, stated in float64 by
tests/exact_kitti_aos.py): `match_counts_aos` / `finalize_aos` are pass 2 and the finalize with the orientation sum, `run_aos` chains
the four launches with them.  `box_params` (csrc/kitti_params.hip) turns cuboid corners into KITTI's h, w, l, location, rotation_y and
alpha; it is where the headings of `KittiEval` and the label files of `cubercnn.data.kitti_format` come from.
"""
import numpy as np
import torch

from .. import lib as _lib
from . import _args

MAX_ROWS = 1024            # detections / ground-truth rows of one image (csrc/eval_kitti.hip)
MAX_PTS = 64
NO_TP = float("-inf")      # the mark of `tp_score` for a row without a true positive


def _offsets(sizes, name):
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
    if (sizes < 0).any():
        raise ValueError(f"{name} must not be negative")
    return sizes, np.concatenate([[0], np.cumsum(sizes)])


def _on_device(t, name, dtype, shape, dev):
    _args.shaped(t, name, dtype, shape)
    if t.device != dev:
        raise ValueError(f"{name} must be on {dev}")


class Problem:
    """dt_sizes / gt_sizes / dc_sizes: (I,) detections (in descending score order, stable), ground-truth rows and DontCare regions per
    image.  sim (M, P) float32: per metric the images' (G_i, D_i) row-major matrices, concatenated (P = sum G_i D_i); dc_ov (sum R_i D_i,)
    float32: the images' (R_i, D_i) matrices.  dt_code (sumD,) int32, dt_height / dt_score (sumD,) float64; gt_code (sumG,) int32,
    gt_height / gt_trunc (sumG,) float64, gt_occ (sumG,) int32: all on the device of `sim`.
    Host tables: cls_tab (C, ncodes) ints (0 the class, 1 a neighbour, 2 the class set aside, -1 other), diffs (Dn, 3) (min height, max occlusion, max
    truncation), min_ov (O, C) >= 0, dc_metric (M,) bools.
    ValueError before anything is launched: a wrong shape / dtype / device, a negative min-overlap, more than MAX_ROWS detections or
    ground-truth rows in one image."""

    def __init__(self, dt_sizes, gt_sizes, dc_sizes, sim, dc_ov, dt_code, dt_height, dt_score, gt_code, gt_height, gt_occ, gt_trunc,
                 cls_tab, diffs, min_ov, dc_metric):
        dt_sizes, dt_off = _offsets(dt_sizes, "dt_sizes")
        gt_sizes, gt_off = _offsets(gt_sizes, "gt_sizes")
        dc_sizes, dc_off = _offsets(dc_sizes, "dc_sizes")
        if not (len(dt_sizes) == len(gt_sizes) == len(dc_sizes)):
            raise ValueError("dt_sizes / gt_sizes / dc_sizes must be of equal length")
        self.I, self.sumD, self.sumG = len(dt_sizes), int(dt_off[-1]), int(gt_off[-1])
        self.max_dt, self.max_gt = int(dt_sizes.max(initial=0)), int(gt_sizes.max(initial=0))
        if self.max_dt > MAX_ROWS:
            raise ValueError(f"an image holds {self.max_dt} detections; the matching kernels take at most {MAX_ROWS}")
        if self.max_gt > MAX_ROWS:
            raise ValueError(f"an image holds {self.max_gt} ground-truth rows; the matching kernels take at most {MAX_ROWS}")
        cls_tab, diffs = np.asarray(cls_tab, dtype=np.int32), np.asarray(diffs, dtype=np.float64)
        min_ov, dc_metric = np.asarray(min_ov, dtype=np.float64), np.asarray(dc_metric).astype(np.int32).reshape(-1)
        if cls_tab.ndim != 2 or diffs.ndim != 2 or diffs.shape[1] != 3 or min_ov.ndim != 2 or min_ov.shape[1] != cls_tab.shape[0]:
            raise ValueError("cls_tab must be (C, ncodes), diffs (Dn, 3), min_ov (O, C)")
        if not (min_ov >= 0).all():
            raise ValueError("min-overlaps must be >= 0")
        self.C, self.ncodes, self.Dn, self.O, self.M = cls_tab.shape[0], cls_tab.shape[1], diffs.shape[0], min_ov.shape[0], len(dc_metric)
        self.S = self.C * self.Dn * self.M * self.O
        sim_off, dc_pair_off = np.concatenate([[0], np.cumsum(dt_sizes * gt_sizes)]), np.concatenate([[0], np.cumsum(dt_sizes * dc_sizes)])
        self.P = int(sim_off[-1])
        _args.shaped(sim, "sim", torch.float32, (self.M, self.P))
        dev = self.device = sim.device
        for t, name, dtype, n in ((dc_ov, "dc_ov", torch.float32, int(dc_pair_off[-1])), (dt_code, "dt_code", torch.int32, self.sumD),
                                  (dt_height, "dt_height", torch.float64, self.sumD), (dt_score, "dt_score", torch.float64, self.sumD),
                                  (gt_code, "gt_code", torch.int32, self.sumG), (gt_height, "gt_height", torch.float64, self.sumG),
                                  (gt_occ, "gt_occ", torch.int32, self.sumG), (gt_trunc, "gt_trunc", torch.float64, self.sumG)):
            _on_device(t, name, dtype, (n,), dev)
        self.rows = (dt_code, dt_height, dt_score, gt_code, gt_height, gt_occ, gt_trunc)
        self.sim, self.dc_ov = sim, dc_ov
        self.lib = _lib.check_device(sim, dc_ov, *self.rows)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)      # noqa: E731
        self.sim_off, self.dc_pair_off = up(sim_off[:-1], np.int64), up(dc_pair_off[:-1], np.int64)
        self.dt_off, self.gt_off, self.dc_off = up(dt_off, np.int32), up(gt_off, np.int32), up(dc_off, np.int32)
        self.cls_tab, self.diffs, self.min_ov, self.dc_metric = up(cls_tab, np.int32), up(diffs, np.float64), up(min_ov, np.float64), up(dc_metric, np.int32)

    def _common(self):
        p = _lib.ptr
        return (p(self.sim), self.P, p(self.sim_off), p(self.dt_off), p(self.gt_off), *[p(t) for t in self.rows], p(self.cls_tab), self.ncodes,
                p(self.diffs), p(self.min_ov))

    def _sizes(self):
        return (self.I, self.C, self.Dn, self.M, self.O, self.sumD, self.sumG, self.max_dt, self.max_gt)


def _check_pts(npts):
    npts = int(npts)
    if not 2 <= npts <= MAX_PTS:
        raise ValueError(f"the number of recall sample points must lie in [2, {MAX_PTS}]")
    return npts


def match_tp(pb, out=None):
    """pass 1 -> (tp_score (S, sumG) float64: the score of the row's true positive or NO_TP; n_gt (S,) int32).  `out`: tensors to write
    (tp_score is written in full, n_gt is zeroed here)."""
    tp, n_gt = out if out is not None else (torch.empty((pb.S, pb.sumG), dtype=torch.float64, device=pb.device),
                                            torch.empty((pb.S,), dtype=torch.int32, device=pb.device))
    n_gt.zero_()
    pb.lib.call("omni_kitti_match_tp", *pb._common(), *pb._sizes(), _lib.ptr(tp), _lib.ptr(n_gt), _lib.stream_of(tp))
    return tp, n_gt


def thresholds(pb, tp_score, n_gt, npts=41, out=None):
    """-> (thresholds (S, npts) float64: the scores at the ranks the recall sampling emits, 0 beyond K; K (S,) int32)"""
    npts = _check_pts(npts)
    thr, K = out if out is not None else (torch.empty((pb.S, npts), dtype=torch.float64, device=pb.device),
                                          torch.empty((pb.S,), dtype=torch.int32, device=pb.device))
    pb.lib.call("omni_kitti_thresholds", _lib.ptr(tp_score), _lib.ptr(n_gt), pb.S, pb.sumG, npts, _lib.ptr(thr), _lib.ptr(K), _lib.stream_of(thr))
    return thr, K


def match_counts(pb, thr, K, out=None):
    """pass 2 -> counts (S, npts, 3) int32 (tp, fp, fn), zero for k >= K (`out` is zeroed here)"""
    npts = _check_pts(thr.shape[1])
    counts = out if out is not None else torch.empty((pb.S, npts, 3), dtype=torch.int32, device=pb.device)
    counts.zero_()
    p = _lib.ptr
    pb.lib.call("omni_kitti_match_counts", *pb._common(), p(pb.dc_ov), p(pb.dc_pair_off), p(pb.dc_off), p(pb.dc_metric), p(thr), p(K), npts,
                *pb._sizes(), p(counts), _lib.stream_of(counts))
    return counts


def finalize(pb, counts, K, out=None):
    """-> (precision (S, npts), recall (S, npts), ap (S, 2) = (AP|R40, AP|R11) x 100), float64"""
    npts = _check_pts(counts.shape[1])
    prec, rec, ap = out if out is not None else (torch.empty((pb.S, npts), dtype=torch.float64, device=pb.device),
                                                 torch.empty((pb.S, npts), dtype=torch.float64, device=pb.device),
                                                 torch.empty((pb.S, 2), dtype=torch.float64, device=pb.device))
    pb.lib.call("omni_kitti_finalize", _lib.ptr(counts), _lib.ptr(K), pb.S, npts, _lib.ptr(prec), _lib.ptr(rec), _lib.ptr(ap), _lib.stream_of(ap))
    return prec, rec, ap


def run(pb, npts=41):
    """the four launches on the current stream, nothing read back -> dict of device tensors: tp_score, n_gt, thresholds, K, counts,
    precision, recall, ap"""
    tp, n_gt = match_tp(pb)
    thr, K = thresholds(pb, tp, n_gt, npts)
    counts = match_counts(pb, thr, K)
    prec, rec, ap = finalize(pb, counts, K)
    return {"tp_score": tp, "n_gt": n_gt, "thresholds": thr, "K": K, "counts": counts, "precision": prec, "recall": rec, "ap": ap}


# ---- AOS ---------------------------------------------------------------------------------------------------------------------------
AOS_ONE = 2 ** 40          # the fixed point of `sim_sum`: one true positive with equal headings adds 2^40
AOS_MAX_ROWS = 2 ** 23     # sumG below this: sumG true positives of at most 2^40 each stay below 2^63


def _check_aos(pb, dt_alpha, gt_alpha, aos_metric):
    """the argument check of the AOS launches -> aos_metric as a host int32 array; ValueError before anything is allocated or launched"""
    if pb.sumG >= AOS_MAX_ROWS:
        raise ValueError(f"{pb.sumG} ground-truth rows: the fixed-point orientation sum takes fewer than 2^23")
    _on_device(dt_alpha, "dt_alpha", torch.float64, (pb.sumD,), pb.device)
    _on_device(gt_alpha, "gt_alpha", torch.float64, (pb.sumG,), pb.device)
    aos_metric = np.asarray(aos_metric).astype(np.int32).reshape(-1)
    if len(aos_metric) != pb.M:
        raise ValueError(f"aos_metric must hold one value per metric ({pb.M})")
    return aos_metric


def match_counts_aos(pb, thr, K, dt_alpha, gt_alpha, aos_metric, out=None):
    """pass 2 with the orientation sum -> (counts (S, npts, 3) int32, the bits of `match_counts`; sim_sum (S, npts) int64: over the
    true positives of the slots whose metric has aos_metric[m] != 0, the sum of llrint(2^40 (1 + cos(gt_alpha - dt_alpha)) / 2), a
    non-finite alpha on either side contributing 0).  dt_alpha (sumD,), gt_alpha (sumG,) float64, NaN: no heading.  `out` is zeroed here."""
    aos_metric = _check_aos(pb, dt_alpha, gt_alpha, aos_metric)
    npts = _check_pts(thr.shape[1])
    counts, sim_sum = out if out is not None else (torch.empty((pb.S, npts, 3), dtype=torch.int32, device=pb.device),
                                                   torch.empty((pb.S, npts), dtype=torch.int64, device=pb.device))
    counts.zero_()
    sim_sum.zero_()
    p = _lib.ptr
    _lib.check_device(dt_alpha, gt_alpha)
    metric = torch.from_numpy(aos_metric).to(pb.device)
    pb.lib.call("omni_kitti_match_counts_aos", *pb._common(), p(pb.dc_ov), p(pb.dc_pair_off), p(pb.dc_off), p(pb.dc_metric), p(thr), p(K), npts,
                *pb._sizes(), p(dt_alpha), p(gt_alpha), p(metric), p(counts), p(sim_sum), _lib.stream_of(counts))
    return counts, sim_sum


def finalize_aos(pb, counts, sim_sum, K, aos_metric, out=None):
    """-> (aos (S, npts): sim_sum 2^-40 / (tp + fp), made monotone from the right like precision; aos_ap (S, 2) = (AOS|R40, AOS|R11)
    x 100), float64; NaN for the slots of a metric with aos_metric[m] == 0"""
    npts = _check_pts(counts.shape[1])
    aos_metric = np.asarray(aos_metric).astype(np.int32).reshape(-1)
    if len(aos_metric) != pb.M:
        raise ValueError(f"aos_metric must hold one value per metric ({pb.M})")
    _on_device(sim_sum, "sim_sum", torch.int64, (pb.S, npts), counts.device)
    aos, aos_ap = out if out is not None else (torch.empty((pb.S, npts), dtype=torch.float64, device=pb.device),
                                               torch.empty((pb.S, 2), dtype=torch.float64, device=pb.device))
    metric = torch.from_numpy(aos_metric).to(pb.device)
    pb.lib.call("omni_kitti_finalize_aos", _lib.ptr(counts), _lib.ptr(sim_sum), _lib.ptr(K), _lib.ptr(metric), pb.S, pb.M, pb.O, npts,
                _lib.ptr(aos), _lib.ptr(aos_ap), _lib.stream_of(aos))
    return aos, aos_ap


def run_aos(pb, dt_alpha, gt_alpha, aos_metric, npts=41):
    """`run` with AOS: five launches on the current stream, nothing read back -> the dict of `run` (the same bits) plus sim_sum, aos,
    aos_ap"""
    _check_aos(pb, dt_alpha, gt_alpha, aos_metric)
    tp, n_gt = match_tp(pb)
    thr, K = thresholds(pb, tp, n_gt, npts)
    counts, sim_sum = match_counts_aos(pb, thr, K, dt_alpha, gt_alpha, aos_metric)
    prec, rec, ap = finalize(pb, counts, K)
    aos, aos_ap = finalize_aos(pb, counts, sim_sum, K, aos_metric)
    return {"tp_score": tp, "n_gt": n_gt, "thresholds": thr, "K": K, "counts": counts, "precision": prec, "recall": rec, "ap": ap,
            "sim_sum": sim_sum, "aos": aos, "aos_ap": aos_ap}


# ---- cuboid corners -> KITTI's box parameters -----------------------------------------------------------------------------------
UP = (0.0, -1.0, 0.0)              # camera y points down


def check_up(up):
    """-> the up vector as three floats; ValueError for one that is not three finite numbers, of zero length or parallel to camera x
    (the ground-plane axis a = camera x less its part along up would vanish)"""
    u = _args.up_vector(up)
    n = u / np.linalg.norm(u)
    if not np.linalg.norm(np.array([1.0, 0.0, 0.0]) - n[0] * n) > 1e-12:
        raise ValueError("up must not be parallel to camera x: the heading is measured from camera x in the ground plane")
    return tuple(float(v) for v in u)


def box_params(corners, up=UP):
    """corners (N, 8, 3) float32 contiguous, in the corner order of `det.cuboid_corners` (v1 - v0 the length axis, v3 - v0 the height
    axis, v4 - v0 the width axis) -> (N, 9) float64: h, w, l, x, y, z, rotation_y, alpha, valid.  (x, y, z) is the centre of the bottom
    face, c - (h / 2) up; rotation_y = atan2(-e.b, e.a) for e = v1 - v0 in the ground-plane basis (a, b) of `up` (up = (0, -1, 0):
    a = camera x, b = camera z), which is KITTI's rotation_y for R = Ry(ry); a heading without a ground-plane component gives
    atan2(0, 0) = 0.  alpha = rotation_y - atan2(c.a, c.b) in (-pi, pi].  valid = 0, and NaN elsewhere, for a box with a non-finite
    corner or a zero edge.  One launch; N == 0 launches nothing."""
    n = _args.corners(corners, "corners")
    up = check_up(up)
    L = _lib.check_device(corners)
    out = torch.empty((n, 9), dtype=torch.float64, device=corners.device)
    if n > 0:
        L.call("omni_kitti_box_params", _lib.ptr(corners), n, *up, _lib.ptr(out), _lib.stream_of(corners))
    return out
