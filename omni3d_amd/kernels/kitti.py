"""Launchers of csrc/eval_kitti.hip: the KITTI object benchmark's protocol (AP|R40 / AP|R11 per class, difficulty, metric and overlap
set) for `cubercnn.evaluation.kitti.KittiEval`.  The reference has no counterpart; the protocol is stated in include/omni3d_hip.h and,
in float64, in tests/exact_kitti.py.  The interface follows `kernels/accumulate.py`: device tensors in, device tensors out.

A `Problem` holds one packed data set (per-image row ranges, per-row quantities, the similarity matrices and the small tables);
`match_tp`, `thresholds`, `match_counts` and `finalize` are the four launches and `run` chains them without a host round trip.
"""
import numpy as np
import torch

from .. import lib as _lib

MAX_ROWS = 1024            # detections / ground-truth rows of one image (csrc/eval_kitti.hip)
MAX_PTS = 64
NO_TP = float("-inf")      # the mark of `tp_score` for a row without a true positive


def _offsets(sizes, name):
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
    if (sizes < 0).any():
        raise ValueError(f"{name} must not be negative")
    return sizes, np.concatenate([[0], np.cumsum(sizes)])


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
        if not isinstance(sim, torch.Tensor) or sim.dtype != torch.float32 or tuple(sim.shape) != (self.M, self.P):
            raise ValueError(f"sim must be float32 of shape ({self.M}, {self.P})")
        dev = self.device = sim.device
        for t, name, dtype, n in ((dc_ov, "dc_ov", torch.float32, int(dc_pair_off[-1])), (dt_code, "dt_code", torch.int32, self.sumD),
                                  (dt_height, "dt_height", torch.float64, self.sumD), (dt_score, "dt_score", torch.float64, self.sumD),
                                  (gt_code, "gt_code", torch.int32, self.sumG), (gt_height, "gt_height", torch.float64, self.sumG),
                                  (gt_occ, "gt_occ", torch.int32, self.sumG), (gt_trunc, "gt_trunc", torch.float64, self.sumG)):
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != (n,) or t.device != dev:
                raise ValueError(f"{name} must be {dtype} of shape ({n},) on {dev}")
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
