"""Launchers of the accumulation of `Omni3Deval.accumulate`: `omni_eval_accumulate` (csrc/eval_match.hip, one 64-lane wave per
(category, range, maxDets, threshold) list) and `omni_eval_accumulate_par` (csrc/eval_accumulate_par.hip, the same tables bit for bit
from many workgroups per list, in three plain launches).  The interface follows `kernels/bootstrap.py`.

The parallel form is for the one long list of a class-agnostic evaluation (`params.useCats = 0`); with K categories the lists are short
and there are K x A x M x T of them, which the one-wave kernel serves well.
"""
import torch

from .. import lib as _lib
from .tperr import _check

# PAR_MIN_LIST: the smallest list length tested by tools/bench_accumulate_par.py at which the median of the parallel form is not above that of
# omni_eval_accumulate; PAR_BLOCK: the fastest tested block at 10^6 elements (profiles/accumulate_par_timing.txt)
PAR_MIN_LIST = 10000
PAR_BLOCK = 1024


def workspace_bytes(K, A, M, T, sumD, block):
    """the bytes `omni_eval_accumulate_par` needs of its caller (the size query of the ABI)"""
    import ctypes
    n = ctypes.c_longlong(0)
    _lib.get().call("omni_eval_accumulate_par_workspace", int(K), int(A), int(M), int(T), int(sumD), int(block), ctypes.addressof(n))
    return int(n.value)


def accumulate(order, cat_off, rank, score, dt_match, dt_ignore, npig, has_e, rec_thrs, max_dets, parallel=None, block=None):
    """-> (precision (T, R, K, A, M), recall (T, K, A, M), scores (T, R, K, A, M)) float64: the tables of the reference's accumulate(),
    -1 where a category has no evaluated image or no ground truth in the range.

    order (N,) int32: all detections by (category, descending score), stable; cat_off (K+1,) int32: the categories' ranges of `order`;
    rank (sumD,) int32: the position of a detection in its group's score-sorted list; score (sumD,) float64; dt_match (A, T, sumD) int32 /
    dt_ignore (A, T, sumD) uint8: the tables of `evaluate_groups`; npig (K, A) int32; has_e (K,) int32; rec_thrs (R,) float64 ascending;
    max_dets (M,) int32.
    parallel: None = the parallel form when the longest list holds at least PAR_MIN_LIST detections, True / False force one; block: the
    list elements per workgroup of the parallel form, a multiple of 64 (default PAR_BLOCK).  Both forms give the same bits."""
    _check(cat_off, "cat_off", torch.int32, (cat_off.numel() if isinstance(cat_off, torch.Tensor) else 0,))
    K = cat_off.numel() - 1
    if K < 0:
        raise ValueError("cat_off must hold K + 1 offsets")
    _check(order, "order", torch.int32, (order.numel() if isinstance(order, torch.Tensor) else 0,))
    if not isinstance(dt_match, torch.Tensor) or dt_match.dim() != 3 or dt_match.shape[0] < 1 or dt_match.shape[1] < 1:
        raise ValueError("dt_match must have shape (A, T, sumD) with A >= 1 and T >= 1")
    A, T, sumD = dt_match.shape
    _check(dt_match, "dt_match", torch.int32, (A, T, sumD))
    _check(dt_ignore, "dt_ignore", torch.uint8, (A, T, sumD))
    _check(rank, "rank", torch.int32, (sumD,))
    _check(score, "score", torch.float64, (sumD,))
    _check(npig, "npig", torch.int32, (K, A))
    _check(has_e, "has_e", torch.int32, (K,))
    if not isinstance(rec_thrs, torch.Tensor) or rec_thrs.dim() != 1 or rec_thrs.numel() < 1:
        raise ValueError("rec_thrs must be 1-D and not empty")
    _check(rec_thrs, "rec_thrs", torch.float64, (rec_thrs.numel(),))
    if not isinstance(max_dets, torch.Tensor) or max_dets.dim() != 1 or max_dets.numel() < 1:
        raise ValueError("max_dets must be 1-D and not empty")
    _check(max_dets, "max_dets", torch.int32, (max_dets.numel(),))
    tensors = (order, cat_off, rank, score, dt_match, dt_ignore, npig, has_e, rec_thrs, max_dets)
    if len({t.device for t in tensors}) != 1:
        raise ValueError("all inputs must live on one device")
    off = cat_off.tolist()
    if off[0] != 0 or off[-1] != order.numel() or any(b < a for a, b in zip(off, off[1:])):
        raise ValueError("cat_off must ascend from 0 to len(order)")
    if order.numel() > sumD:
        raise ValueError("order must not be longer than the sumD detections")
    if order.numel() and (int(order.min()) < 0 or int(order.max()) >= sumD):
        raise ValueError("order must index the sumD detections")
    block = PAR_BLOCK if block is None else int(block)
    if block < 64 or block % 64:
        raise ValueError("block must be a positive multiple of 64")
    longest = max((b - a for a, b in zip(off, off[1:])), default=0)
    if parallel is None:
        parallel = longest >= PAR_MIN_LIST
    L = _lib.check_device(*tensors)
    R, M, dev = rec_thrs.numel(), max_dets.numel(), order.device
    prec = torch.full((T, R, K, A, M), -1.0, dtype=torch.float64, device=dev)
    rec = torch.full((T, K, A, M), -1.0, dtype=torch.float64, device=dev)
    scr = torch.full((T, R, K, A, M), -1.0, dtype=torch.float64, device=dev)
    p = _lib.ptr
    args = (p(order), p(cat_off), p(rank), p(score), p(dt_match), p(dt_ignore), p(npig), p(has_e), p(rec_thrs), p(max_dets), K, A, M, T, R, sumD)
    if K == 0:
        return prec, rec, scr
    if parallel:
        nbytes = workspace_bytes(K, A, M, T, sumD, block)
        ws = torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device=dev)
        L.call("omni_eval_accumulate_par", *args, block, p(ws), nbytes, p(prec), p(rec), p(scr), _lib.stream_of(prec))
    else:
        L.call("omni_eval_accumulate", *args, p(prec), p(rec), p(scr), _lib.stream_of(prec))
    return prec, rec, scr
