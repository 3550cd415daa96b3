"""The error decomposition of the evaluator (`Omni3Deval.errors` / `summarize_errors`): what the AP of a mode is lost to, after TIDE
(Bolya et al., ECCV 2020).  The image-level similarity is one more pass of the mode's own `similarity` over image groups, the
classification and the contests are one launch (`kernels.errtypes`, csrc/eval_errors.hip), every oracle is an unchanged
`omni_eval_accumulate` on a copy of the match tables of evaluate().  `Omni3Deval.errors` documents the definitions."""
import numpy as np
import torch

from ...kernels import errtypes, iou3d, tperr
from .modes import Mode3D
from .pairs import _ragged_pairs

ERROR_TYPES = ("Cls", "Loc", "Both", "Dupe", "Bkg", "Miss")          # the columns of `counts`
ORACLES = ERROR_TYPES + ("FP", "FN")                                   # the rows of `ap_fixed` / `dap`
_FP_CODES = (errtypes.CLS, errtypes.LOC, errtypes.BOTH, errtypes.DUPE, errtypes.BKG)
_ERROR_KEYS = ("t_fg", "t_bg")


def _error_params(params):
    """None (off) or a dict with some of t_fg / t_bg -> None or a checked copy; they apply to the modes of the 3D protocol, mode 2D
    keeps its own defaults"""
    if params is None:
        return None
    if not isinstance(params, dict) or set(params) - set(_ERROR_KEYS):
        raise ValueError("errors must be None or a dict with keys out of %r" % (_ERROR_KEYS,))
    out = {}
    for key in ("t_fg", "t_bg"):
        if params.get(key) is not None:
            v = float(params[key])
            if not 0.0 < v < 1.0:
                raise ValueError("errors: %s must lie in (0, 1)" % key)
            out[key] = v
    if "t_fg" in out and "t_bg" in out and not out["t_bg"] < out["t_fg"]:
        raise ValueError("errors: t_bg must be below t_fg")
    return out


def _accumulate_ap(t, dt_match, dt_ignore, order, cat_off, npig):
    """one unchanged omni_eval_accumulate with T = A = M = 1 -> AP (K,) float64 on the host: the mean of precision over the recall
    thresholds, -1 where accumulate() leaves -1"""
    L, _p = iou3d._lib.get(), iou3d._lib.ptr
    K, R, sumD, dev = t["K"], t["rec_thrs"].numel(), t["sumD"], t["rec_thrs"].device
    prec = torch.full((1, R, K, 1, 1), -1.0, dtype=torch.float64, device=dev)
    rec = torch.full((1, K, 1, 1), -1.0, dtype=torch.float64, device=dev)
    scr = torch.full((1, R, K, 1, 1), -1.0, dtype=torch.float64, device=dev)
    dt_match, dt_ignore, npig = dt_match.to(torch.int32).contiguous(), dt_ignore.to(torch.uint8).contiguous(), npig.to(torch.int32).contiguous()
    L.call("omni_eval_accumulate", _p(order), _p(cat_off), _p(t["rank"]), _p(t["scores"]), _p(dt_match), _p(dt_ignore), _p(npig), _p(t["has_e"]),
           _p(t["rec_thrs"]), _p(t["max_dets"]), K, 1, 1, 1, R, sumD, _p(prec), _p(rec), _p(scr), iou3d._lib.stream_of(prec))
    pr = np.ascontiguousarray(prec[0, :, :, 0, 0].cpu().numpy())                      # (R, K); the mean is numpy's, like summarize()'s
    return np.where((pr > -1).all(axis=0), pr.mean(axis=0), -1.0)


def error_analysis(ev, t_fg=None, t_bg=None, area="all"):
    """`Omni3Deval.errors`: see there"""
    if ev._dev is None:
        raise Exception("Please run evaluate() first")
    M, p, d = ev._mode, ev.params, ev._dev
    if M.error_thrs is None:
        raise ValueError("mode %s matches by distance: a background overlap has no meaning there, errors() is not defined" % M.name)
    ev._check_same_params(p, "errors()")
    t_fg = M.error_thrs[0] if t_fg is None else float(t_fg)
    t_bg = M.error_thrs[1] if t_bg is None else float(t_bg)
    thrs = np.asarray(p.iouThrs, dtype=np.float64)
    ti = np.flatnonzero(np.isclose(t_fg, thrs))
    if not len(ti):
        raise ValueError("t_fg %r is not one of params.iouThrs %r: the analysis reuses the match tables of evaluate()" % (t_fg, thrs.tolist()))
    ti = int(ti[0])
    if not 0.0 < t_bg < t_fg:
        raise ValueError("the thresholds must satisfy 0 < t_bg < t_fg")
    if area not in p.areaRngLbl:
        raise ValueError("area %r is not one of params.areaRngLbl %r" % (area, p.areaRngLbl))
    ai = p.areaRngLbl.index(area)
    K, A, I = len(p.catIds), len(p.areaRng), len(p.imgIds)
    groups, dt_sizes, gt_sizes, dev, m = d["groups"], d["dt_sizes"], d["gt_sizes"], d["device"], d["match"]
    sumD, sumG = int(dt_sizes.sum()), int(gt_sizes.sum())
    tb = ev._merge_tables(K, A)
    tod = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)               # noqa: E731
    # ---- the image groups: a stable sort of the (category, image) groups by image keeps the category-major order inside an image ----
    grp_cat, grp_img = tb["cat_of_group"], np.array([g[1] for g in groups], dtype=np.int64)
    det_cat, gt_cat = np.repeat(grp_cat, dt_sizes), np.repeat(grp_cat, gt_sizes)
    perm_d = np.argsort(np.repeat(grp_img, dt_sizes), kind="stable")
    perm_g = np.argsort(np.repeat(grp_img, gt_sizes), kind="stable")
    D_i = np.bincount(np.repeat(grp_img, dt_sizes), minlength=I).astype(np.int64)
    G_i = np.bincount(np.repeat(grp_img, gt_sizes), minlength=I).astype(np.int64)
    all_d, all_g = [x for gr in groups for x in gr[3]], [x for gr in groups for x in gr[2]]
    f32 = lambda v: torch.tensor(np.asarray(v, dtype=np.float32).reshape(M.box_shape)).to(dev)      # noqa: E731
    b_d, b_g = f32([all_d[i][M.box_key] for i in perm_d]), f32([all_g[i][M.box_key] for i in perm_g])
    sim, _ = M.similarity(ev, b_d, b_g, D_i, G_i, _ragged_pairs(D_i, G_i))          # the raw similarity, also under eval_prox
    t_pd, t_pg = tod(perm_d), tod(perm_g)
    dtm, dti = m["dt_match"][ai, ti] >= 0, m["dt_ignore"][ai, ti] != 0               # (sumD,) in the order of evaluate()
    gtm, gig = m["gt_match"][ai, ti] >= 0, m["gt_ignore"][ai] != 0
    t_dcat, t_gcat, t_sc = tod(det_cat.astype(np.int32)), tod(gt_cat.astype(np.int32)), tod(d["scores"])
    i32off = lambda s: tod(np.concatenate([[0], np.cumsum(s)]).astype(np.int32))     # noqa: E731
    u8 = lambda x: x.to(torch.uint8).contiguous()                                    # noqa: E731
    out = errtypes.error_types(sim.float().contiguous(), i32off(D_i), i32off(G_i), t_dcat[t_pd].contiguous(), u8(dtm[t_pd]), u8(dti[t_pd]),
                               t_sc[t_pd].contiguous(), t_gcat[t_pg].contiguous(), u8(gtm[t_pg]), u8(gig[t_pg]), float(thrs[ti]), t_bg)

    def back(x, perm, n):                    # image-major rows -> the order of evaluate()
        y = torch.empty((n,) + tuple(x.shape[1:]), dtype=x.dtype, device=dev)
        y[perm] = x
        return y
    typ = back(out["type"], t_pd, sumD)
    attr_img = out["attr"].long()
    attr = back(torch.where(attr_img >= 0, t_pg[attr_img.clamp(min=0)] if sumG else attr_img, attr_img), t_pd, sumD)
    smax, win_loc, win_cls = back(out["smax"], t_pd, sumD), back(out["win_loc"], t_pd, sumD) != 0, back(out["win_cls"], t_pd, sumD) != 0
    missed = back(out["gt_missed"], t_pg, sumG) != 0
    # ---- the oracles: each alone on a copy of the tables at (range, t_fg, the largest maxDets), then the unchanged accumulation ----
    t = {"K": K, "sumD": sumD, "rank": tod(np.zeros(sumD, np.int32)), "scores": t_sc, "has_e": tod(tb["has_e"]),
         "rec_thrs": tod(np.asarray(p.recThrs, dtype=np.float64)), "max_dets": tod(np.asarray(p.maxDets[-1:], dtype=np.int32))}
    order, cat_off, npig = tod(tb["order"]), tod(tb["cat_off"]), tod(tb["npig"][:, ai].astype(np.int32))
    match = lambda hit: torch.where(hit, 0, -1)                                      # noqa: E731  (accumulate reads dt_match >= 0)
    is_fp = torch.zeros(sumD, dtype=torch.bool, device=dev)
    for code in _FP_CODES:
        is_fp |= typ == code
    bins = lambda rows: torch.bincount(t_gcat[rows].long(), minlength=K).to(torch.int32)           # noqa: E731
    ap = _accumulate_ap(t, match(dtm), dti, order, cat_off, npig)
    fixed = np.zeros((len(ORACLES), K))
    # Cls: the winner moves to the merged list of the ground truth's category; the merge order is rebuilt like `_merge_tables` builds it
    h_win, h_attr = win_cls.cpu().numpy(), attr.cpu().numpy()
    moved = np.where(h_win, gt_cat[np.clip(h_attr, 0, None)] if sumG else 0, det_cat)
    order_c = np.lexsort((np.arange(sumD), -d["scores"], moved)).astype(np.int32) if sumD else np.zeros(0, np.int32)
    off_c = np.concatenate([[0], np.cumsum(np.bincount(moved, minlength=K))]).astype(np.int32)
    fixed[0] = _accumulate_ap(t, match(dtm | win_cls), dti | ((typ == errtypes.CLS) & ~win_cls), tod(order_c), tod(off_c), npig)
    fixed[1] = _accumulate_ap(t, match(dtm | win_loc), dti | ((typ == errtypes.LOC) & ~win_loc), order, cat_off, npig)
    for j, code in ((2, errtypes.BOTH), (3, errtypes.DUPE), (4, errtypes.BKG)):
        fixed[j] = _accumulate_ap(t, match(dtm), dti | (typ == code), order, cat_off, npig)
    fixed[5] = _accumulate_ap(t, match(dtm), dti, order, cat_off, npig - bins(missed))
    fixed[6] = _accumulate_ap(t, match(dtm), dti | is_fp, order, cat_off, npig)
    fixed[7] = _accumulate_ap(t, match(dtm), dti, order, cat_off, bins(gtm & ~gig))
    both = (fixed > -1) & (ap > -1)
    dap = np.where(both, fixed - ap, np.nan)
    h_typ, h_missed = typ.cpu().numpy(), missed.cpu().numpy()
    counts = np.stack([np.bincount(det_cat[h_typ == code], minlength=K) for code in _FP_CODES] + [np.bincount(gt_cat[h_missed], minlength=K)],
                      axis=1).astype(np.int64)
    res = {"t_fg": t_fg, "t_bg": t_bg, "area": area, "names": ORACLES, "type": h_typ, "dt_ids": d["dt_ids"],
           "attributed_gt": np.where(h_attr >= 0, d["gt_ids"][np.clip(h_attr, 0, None)] if sumG else -1, -1),
           "s_free": smax[:, 0].cpu().numpy(), "s_used": smax[:, 1].cpu().numpy(), "s_other": smax[:, 2].cpu().numpy(),
           "missed_gt_ids": d["gt_ids"][h_missed], "counts": counts, "counts_total": counts.sum(axis=0), "ap": ap, "ap_fixed": fixed, "dap": dap,
           "dap_mean": np.array([np.nanmean(r) if np.isfinite(r).any() else np.nan for r in dap]),
           "dropped": ((ap > -1) & (fixed == -1)).sum(axis=1).astype(np.int64), "loc_errors": None, "loc_errors_mean": None, "loc_skipped": 0}
    if M.loc_errors:
        # whether "poor box" means depth, size or rotation: the pair errors of the Loc detections and their attributed ground truths
        rows = torch.nonzero(out["type"] == errtypes.LOC).reshape(-1)                # image-major rows, like b_d / b_g
        err = tperr.pair_errors(iou3d.cuboid_fit(b_d.contiguous()), iou3d.cuboid_fit(b_g.contiguous()), rows.to(torch.int32),
                                out["attr"][rows].contiguous()).cpu().numpy()
        cats, ok = det_cat[perm_d][rows.cpu().numpy()], np.isfinite(err[:, 0]) if len(err) else np.zeros(0, bool)
        loc = np.full((K, 3), np.nan)
        for k in np.unique(cats[ok]):
            loc[k] = err[ok & (cats == k)].mean(axis=0)
        has = np.isfinite(loc[:, 0])
        res.update(loc_errors=loc, loc_errors_mean=loc[has].mean(axis=0) if has.any() else np.full(3, np.nan), loc_skipped=int((~ok).sum()))
    return res


def error_lines(M, p, res):
    """one line per type in the style of `Mode.line`: the type, its count, dAP x 100; then the `loc_errors` line"""
    head = "mode={}  Error {:<5} (dAP) @[ IoU={:0.2f}/{:0.2f} | {}={:>6s} | maxDets={:>3d} | n={:>6} ] = {:0.3f}"
    what = "area" if M.range_key == "area" else "depth"
    lines = []
    for j, name in enumerate(ORACLES):
        n = int(res["counts_total"][j]) if j < len(ERROR_TYPES) else "-"
        lines.append(head.format(M.name, name, res["t_fg"], res["t_bg"], what, res["area"], p.maxDets[-1], n, 100 * res["dap_mean"][j]))
    if res["loc_errors"] is not None:
        e = res["loc_errors_mean"]
        lines.append("mode={}  Loc pairs: translation {:0.3f} m | 1 - aligned IoU {:0.3f} | orientation {:0.3f} rad | left out {:d}".format(
            M.name, e[0], e[1], e[2], res["loc_skipped"]))
    return lines


def error_summary(ev, params):
    """the drivers' `bbox_<mode>_errors`: counts, dAP x 100 (the means over the categories) and the mean Loc pair errors of one evaluated
    mode; None for a mode without the analysis (DIST).  `params` from `_error_params`; t_fg / t_bg go to the 3D-protocol modes only"""
    M = ev._mode
    if M.error_thrs is None:
        return None
    res = ev.errors(**(params if isinstance(M, Mode3D) else {}))
    nan = lambda v: float(v) if np.isfinite(v) else float("nan")                     # noqa: E731
    return {"t_fg": res["t_fg"], "t_bg": res["t_bg"], "counts": {n: int(c) for n, c in zip(ERROR_TYPES, res["counts_total"])},
            "dAP": {n: nan(100 * v) for n, v in zip(ORACLES, res["dap_mean"])},
            "loc_errors": None if res["loc_errors"] is None else {n: nan(v) for n, v in zip(("trans", "scale", "orient"), res["loc_errors_mean"])}}
