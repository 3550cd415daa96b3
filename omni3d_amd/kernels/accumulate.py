"""Launchers of the accumulation of `Omni3Deval.accumulate`: `omni_eval_accumulate` (csrc/eval_match.hip, one 64-lane wave per
(category, range, maxDets, threshold) list) and `omni_eval_accumulate_par` (csrc/eval_accumulate_par.hip, the same tables bit for bit
from many workgroups per list, in three plain launches).  The arguments are checked by `kernels/_args.py`.

The parallel form is for the one long list of a class-agnostic evaluation (`params.useCats = 0`); with K categories the lists are short
and there are K x A x M x T of them, which the one-wave kernel serves well.
"""
import torch

from .. import lib as _lib
from . import _args

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
    K, A, T, R, sumD, off = _args.merge_order(order, cat_off, dt_match, dt_ignore, rec_thrs)
    _args.tensor(rank, "rank", torch.int32, (sumD,))
    _args.tensor(score, "score", torch.float64, (sumD,))
    _args.tensor(npig, "npig", torch.int32, (K, A))
    _args.tensor(has_e, "has_e", torch.int32, (K,))
    M = _args.nonempty(max_dets, "max_dets", torch.int32)
    tensors = (order, cat_off, rank, score, dt_match, dt_ignore, npig, has_e, rec_thrs, max_dets)
    _args.one_device(tensors)
    if order.numel() > sumD:
        raise ValueError("order must not be longer than the sumD detections")
    block = PAR_BLOCK if block is None else int(block)
    if block < 64 or block % 64:
        raise ValueError("block must be a positive multiple of 64")
    longest = max((b - a for a, b in zip(off, off[1:])), default=0)
    if parallel is None:
        parallel = longest >= PAR_MIN_LIST
    L = _lib.check_device(*tensors)
    dev = order.device
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
