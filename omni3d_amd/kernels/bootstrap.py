"""Launchers of csrc/eval_bootstrap.hip: AP and recall of B image-level bootstrap replicates from the one set of match tables of an
evaluation.  The reference has no counterpart; the arguments are checked by `kernels/_args.py`.

A replicate is a row of `weights` (B, I) int32: how many times each of the I evaluated images is present.  Its result is by definition
what `omni_eval_accumulate` gives on the data set in which image i is present weights[b, i] times, copies adjacent in the image order;
`Omni3Deval.bootstrap` documents the definition in full.

Overflow rule: the weighted counts are 32-bit.  `bootstrap_counts` raises ValueError when (number of ground truths) x (largest weight)
>= 2^31, `bootstrap_accumulate` when (number of detections) x (largest weight) >= 2^31; the library refuses the same with OMNI_ERR_ARG.
"""
import torch

from .. import lib as _lib
from . import _args

COUNT_LIMIT = 1 << 31
MAX_IMAGES = 1 << 29


def check_weights(weights):
    """weights (B, I) int32, contiguous, B >= 1, no negative entry -> its largest entry (0 for I == 0)"""
    if not isinstance(weights, torch.Tensor) or weights.dim() != 2 or weights.dtype != torch.int32 or weights.shape[0] < 1:
        raise ValueError("weights must be an int32 tensor of shape (B, I) with B >= 1")
    if not weights.is_contiguous():
        raise ValueError("weights must be contiguous")
    if weights.shape[1] >= MAX_IMAGES:
        raise ValueError("more than 2^29 - 1 images")
    if weights.numel() == 0:
        return 0
    lo, hi = int(weights.min()), int(weights.max())
    if lo < 0:
        raise ValueError("weights must be >= 0")
    return hi


def bootstrap_counts(grp_off, grp_img, grp_npig, weights, sum_gt=None):
    """-> (npig_b (B, K, A) int32, has_e_b (B, K) int32): the number of non-ignored ground truths per category and range, and whether
    any evaluated image holds the category, of every replicate.

    grp_off (K+1,) int32 / grp_img (G,) int32 / grp_npig (G, A) int32: the (image, category) groups of the evaluation in (category,
    image) order: their ranges per category, the index of a group's image in [0, I), its non-ignored ground truths per range; sum_gt:
    an upper bound of the column sums of grp_npig (default: the largest of them)."""
    K = _args.offset_count(grp_off, "grp_off")
    G = _args.tensor(grp_img, "grp_img", torch.int32, (None,))[0]
    A = _args.tensor(grp_npig, "grp_npig", torch.int32, (G, None))[1]
    if A < 1:
        raise ValueError("grp_npig must have shape (G, A) with A >= 1")
    wmax = check_weights(weights)
    B, I = weights.shape
    tensors = (grp_off, grp_img, grp_npig, weights)
    _args.one_device(tensors)
    _args.offsets(grp_off, "grp_off", G)
    if G and (int(grp_npig.min()) < 0 or int(grp_img.min()) < 0 or int(grp_img.max()) >= I):
        raise ValueError("grp_npig must be >= 0 and grp_img must index the I images")
    if sum_gt is None:
        sum_gt = int(grp_npig.sum(dim=0).max()) if G else 0
    if int(sum_gt) * wmax >= COUNT_LIMIT:
        raise ValueError("weighted ground-truth counts would reach 2^31: %d ground truths x weight %d" % (sum_gt, wmax))
    L = _lib.check_device(*tensors)
    npig_b = torch.zeros((B, K, A), dtype=torch.int32, device=weights.device)
    has_e_b = torch.zeros((B, K), dtype=torch.int32, device=weights.device)
    if K > 0:
        L.call("omni_eval_bootstrap_counts", _lib.ptr(grp_off), _lib.ptr(grp_img), _lib.ptr(grp_npig), _lib.ptr(weights), wmax, K, A, G,
               int(sum_gt), B, I, _lib.ptr(npig_b), _lib.ptr(has_e_b), _lib.stream_of(weights))
    return npig_b, has_e_b


def bootstrap_accumulate(order, cat_off, rank, dt_match, dt_ignore, det_img, weights, npig_b, has_e_b, rec_thrs, max_dets):
    """-> (ap (B, T, K, A, M), ar (B, T, K, A, M)) float64: per replicate the mean over the R recall thresholds of the `precision` table
    `omni_eval_accumulate` would give, and its `recall`; -1 where that writes nothing (has_e_b 0 or npig_b 0).

    order (N,) int32 / cat_off (K+1,) int32 / rank (sumD,) int32 / dt_match (A, T, sumD) int32 / dt_ignore (A, T, sumD) uint8 / rec_thrs
    (R,) float64 / max_dets (M,) int32: as for `kernels.let.accumulate_let`; det_img (sumD,) int32: the index of a detection's image in
    [0, I); weights (B, I) int32 >= 0; npig_b (B, K, A) / has_e_b (B, K) int32 from `bootstrap_counts`.  One launch; two calls, and any
    split of the rows of `weights` over several calls, give the same bits."""
    K, A, T, R, sumD, _ = _args.merge_order(order, cat_off, dt_match, dt_ignore, rec_thrs)
    _args.tensor(rank, "rank", torch.int32, (sumD,))
    _args.tensor(det_img, "det_img", torch.int32, (sumD,))
    wmax = check_weights(weights)
    B, I = weights.shape
    _args.tensor(npig_b, "npig_b", torch.int32, (B, K, A))
    _args.tensor(has_e_b, "has_e_b", torch.int32, (B, K))
    M = _args.nonempty(max_dets, "max_dets", torch.int32)
    tensors = (order, cat_off, rank, dt_match, dt_ignore, det_img, weights, npig_b, has_e_b, rec_thrs, max_dets)
    _args.one_device(tensors)
    if sumD * wmax >= COUNT_LIMIT:
        raise ValueError("weighted detection counts would reach 2^31: %d detections x weight %d" % (sumD, wmax))
    L = _lib.check_device(*tensors)
    dev = weights.device
    ap = torch.full((B, T, K, A, M), -1.0, dtype=torch.float64, device=dev)
    ar = torch.full((B, T, K, A, M), -1.0, dtype=torch.float64, device=dev)
    if K > 0:
        L.call("omni_eval_bootstrap", _lib.ptr(order), _lib.ptr(cat_off), _lib.ptr(rank), _lib.ptr(dt_match), _lib.ptr(dt_ignore),
               _lib.ptr(det_img), _lib.ptr(weights), wmax, _lib.ptr(npig_b), _lib.ptr(has_e_b), _lib.ptr(rec_thrs), _lib.ptr(max_dets),
               K, A, M, T, R, sumD, B, I, _lib.ptr(ap), _lib.ptr(ar), _lib.stream_of(weights))
    return ap, ar
