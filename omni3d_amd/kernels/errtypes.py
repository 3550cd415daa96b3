"""Launcher of csrc/eval_errors.hip: the error type of every detection and the Miss flag of every ground truth of a data set, after
TIDE (Bolya et al., ECCV 2020).  The reference has no counterpart; the arguments are checked by `kernels/_args.py`.  `Omni3Deval.errors`
documents the definitions in full; the codes are the constants below.
"""
import numpy as np
import torch

from .. import lib as _lib
from . import _args

TP, IGN, CLS, LOC, BOTH, DUPE, BKG = range(7)          # the codes of `type`
FP_TYPES = (CLS, LOC, BOTH, DUPE, BKG)                 # the false-positive codes, in TIDE's order
MAX_GT = 1024                                          # ground truths per image (the LDS capacity of error_types_kernel)


def error_types(sim, dt_off, gt_off, dt_cat, dt_matched, dt_ignore, dt_score, gt_cat, gt_matched, gt_ignore, t_fg, t_bg):
    """-> dict of device tensors: `type` (sumD,) int8, `attr` (sumD,) int32 the global row of the attributed ground truth or -1, `smax`
    (sumD, 3) float32 = (s_free, s_used, s_other), `win_loc` / `win_cls` (sumD,) uint8, `gt_missed` (sumG,) uint8.

    Rows are ragged by image over all categories: dt_off / gt_off (I+1,) int32 ascending from 0 to sumD / sumG; sim float32, the (D_i,
    G_i) row-major similarity matrices of the images one after another; dt_cat (sumD,) int32, dt_matched / dt_ignore (sumD,) uint8,
    dt_score (sumD,) float64; gt_cat (sumG,) int32, gt_matched / gt_ignore (sumG,) uint8: the outcome of the greedy matching at one
    (range, threshold); 0 < t_bg < t_fg.  ValueError on a wrong argument, and on an image with more than MAX_GT ground truths, before
    anything is launched: nothing is truncated.  One launch; two calls give the same bits."""
    do, go = np.asarray(_args.offsets(dt_off, "dt_off"), np.int64), np.asarray(_args.offsets(gt_off, "gt_off"), np.int64)
    if len(do) != len(go):
        raise ValueError("dt_off / gt_off must hold I + 1 offsets each")
    I = len(do) - 1
    sumD, sumG = int(do[-1]), int(go[-1])
    for t, name, dtype, n in ((dt_cat, "dt_cat", torch.int32, sumD), (dt_matched, "dt_matched", torch.uint8, sumD),
                              (dt_ignore, "dt_ignore", torch.uint8, sumD), (dt_score, "dt_score", torch.float64, sumD),
                              (gt_cat, "gt_cat", torch.int32, sumG), (gt_matched, "gt_matched", torch.uint8, sumG),
                              (gt_ignore, "gt_ignore", torch.uint8, sumG)):
        _args.tensor(t, name, dtype, (n,))
    sim_off = np.concatenate([[0], np.cumsum(np.diff(do) * np.diff(go))]).astype(np.int64)
    _args.tensor(sim, "sim", torch.float32, (int(sim_off[-1]),))
    t_fg, t_bg = float(t_fg), float(t_bg)
    if not 0.0 < t_bg < t_fg:
        raise ValueError("the thresholds must satisfy 0 < t_bg < t_fg")
    max_gt = int(np.diff(go).max()) if I else 0
    if max_gt > MAX_GT:
        raise ValueError("an image holds %d ground truths, the capacity is %d" % (max_gt, MAX_GT))
    tensors = (sim, dt_off, gt_off, dt_cat, dt_matched, dt_ignore, dt_score, gt_cat, gt_matched, gt_ignore)
    _args.one_device(tensors)
    L = _lib.check_device(*tensors)
    dev = sim.device
    out = {"type": torch.empty(sumD, dtype=torch.int8, device=dev), "attr": torch.empty(sumD, dtype=torch.int32, device=dev),
           "smax": torch.empty((sumD, 3), dtype=torch.float32, device=dev), "win_loc": torch.empty(sumD, dtype=torch.uint8, device=dev),
           "win_cls": torch.empty(sumD, dtype=torch.uint8, device=dev), "gt_missed": torch.empty(sumG, dtype=torch.uint8, device=dev)}
    if I > 0:
        t_off = torch.from_numpy(sim_off).to(dev)
        L.call("omni_eval_error_types", _lib.ptr(sim), _lib.ptr(t_off), _lib.ptr(dt_off), _lib.ptr(gt_off), _lib.ptr(dt_cat), _lib.ptr(dt_matched),
               _lib.ptr(dt_ignore), _lib.ptr(dt_score), _lib.ptr(gt_cat), _lib.ptr(gt_matched), _lib.ptr(gt_ignore), t_fg, t_bg, I, sumD, sumG,
               max_gt, *[_lib.ptr(out[k]) for k in ("type", "attr", "smax", "win_loc", "win_cls", "gt_missed")], _lib.stream_of(sim))
    return out
