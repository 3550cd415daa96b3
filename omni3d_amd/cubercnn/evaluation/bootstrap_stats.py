"""Image-level bootstrap of the evaluator's AP / AR (`Omni3Deval.bootstrap`, `bootstrap_compare`): the replicate tables, the
statistics over the replicates and the layout the drivers report them in, with the headline slots of summarize() they share.  The match
tables of evaluate() are kept and all replicates are accumulated in one launch from integer image multiplicities (`kernels.bootstrap`,
csrc/eval_bootstrap.hip); that part is `Omni3Deval._bootstrap_tables`."""
import numpy as np

from .modes import _METRICS, _slot_indices, _stat_slots


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
