"""The error decomposition of `Omni3Deval.errors` written from its definition, in float64, numpy and Python loops: the reference of
tests/test_error_types.py (`classify`, one image) and tests/test_error_analysis.py (`analyse`, the whole pipeline).  Uses no kernel and
imports nothing from omni3d_amd but `boxgen` (through the other exact_* modules): the similarity is `exact_iou3d.iou3d` (Qhull) in mode
3D, `exact_let._iou2d` in 2D, `exact_bev.bev_iou` in BEV and `exact_let.let_pair` in LET; the matching is `exact_let.match_group`, the
accumulation `exact_let.accumulate`, the pair errors `exact_tp_errors.errors`.

Definitions (after TIDE, Bolya et al., ECCV 2020).  Per image, all detections (category-major, descending score inside a category, each
category's list cut to the largest maxDets) against all ground truths (category-major).  Candidates: the ground truths that are not
ignored at the range.  TP: matched and not ignored.  IGN: ignored.  Every other detection, of category c: s_free / s_used / s_other = its
largest similarity to an unmatched / a matched candidate of category c / a candidate of another category (-inf for an empty set, the
LATER row among equal values); Loc if s_free >= t_bg, else Cls if s_other >= t_fg, else Dupe if s_used >= t_fg, else Bkg if all three <
t_bg, else Both.  Attributed ground truth: the arg-max of the deciding set (Loc, Cls, Dupe), -1 otherwise.  Miss: an unmatched candidate
that is the attributed ground truth of no Loc or Cls detection.
Oracles, each alone on a copy of the tables, then the unchanged accumulation: Loc / Cls: among the detections of that type attributed to
one ground truth the highest score wins (the lower row among equal scores) and becomes a true positive -- under Cls in the ground
truth's category, and only when the ground truth is unmatched --, the others are removed (ignored); Both / Dupe / Bkg: removed; Miss:
npig loses the missed ground truths; FP: every false positive removed; FN: npig = the matched candidates."""
import math

import numpy as np

import exact_bev
import exact_iou3d
import exact_let as XL
from exact_tp_errors import errors as pair_error
from exact_tp_errors import fit

TP, IGN, CLS, LOC, BOTH, DUPE, BKG = range(7)
ORACLES = ("Cls", "Loc", "Both", "Dupe", "Bkg", "Miss", "FP", "FN")
AREA_2D = ((0 ** 2, 1e5 ** 2), (0 ** 2, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e5 ** 2))
MODES = {   # similarity of two records, key of the ignore flag, of the range value, ranges, thresholds, default (t_fg, t_bg)
    "2D": ("ignore2D", "area", AREA_2D, np.linspace(0.5, 0.95, 10), (0.5, 0.1)),
    "3D": ("ignore3D", "depth", XL.AREA_RNG, XL.IOU_THRS, (0.25, 0.05)),
    "BEV": ("ignore3D", "depth", XL.AREA_RNG, XL.IOU_THRS, (0.25, 0.05)),
    "LET": ("ignore3D", "depth", XL.AREA_RNG, XL.IOU_THRS, (0.25, 0.05)),
}


def _box(x):
    return np.array(x["bbox3D"], np.float32).astype(np.float64)


def similarity(mode, d, g):
    """one detection record against one ground-truth record, float64"""
    if mode == "2D":
        return XL._iou2d(d["bbox"], g["bbox"])
    if mode == "BEV":
        return float(exact_bev.bev_iou(_box(d), _box(g)))
    fd, fg = fit(np.array(d["bbox3D"], np.float32)), fit(np.array(g["bbox3D"], np.float32))
    if mode == "LET":
        return float(XL.let_pair(fd, fg)[0])
    if np.linalg.norm(fd[0] - fg[0]) > 0.5 * (np.linalg.norm(fd[2]) + np.linalg.norm(fg[2])):
        return 0.0                                      # disjoint bounding spheres: nothing for Qhull to intersect
    return float(min(max(exact_iou3d.iou3d(_box(d), _box(g))[1], 0.0), 1.0))


def classify(sim, dt_cat, dt_matched, dt_ignore, dt_score, gt_cat, gt_matched, gt_ignore, t_fg, t_bg):
    """One image.  sim (D, G) float64; the other arguments are sequences over its detections / ground truths.
    -> dict: type (D,), attr (D,) row of the attributed ground truth or -1, smax (D, 3) = (s_free, s_used, s_other), win_loc / win_cls
    (D,) bool, missed (G,) bool"""
    sim = np.asarray(sim, np.float64).reshape(len(dt_cat), len(gt_cat))
    D, G = sim.shape
    typ, attr, smax = np.zeros(D, np.int64), np.full(D, -1, np.int64), np.full((D, 3), -math.inf)
    for d in range(D):
        best, arg = [-math.inf] * 3, [-1] * 3
        for g in range(G):
            if gt_ignore[g]:
                continue
            s = 2 if gt_cat[g] != dt_cat[d] else (1 if gt_matched[g] else 0)
            if sim[d, g] >= best[s]:
                best[s], arg[s] = sim[d, g], g
        smax[d] = best
        f, u, o = best
        if dt_ignore[d]:
            typ[d] = IGN
        elif dt_matched[d]:
            typ[d] = TP
        elif f >= t_bg:
            typ[d], attr[d] = LOC, arg[0]
        elif o >= t_fg:
            typ[d], attr[d] = CLS, arg[2]
        elif u >= t_fg:
            typ[d], attr[d] = DUPE, arg[1]
        elif max(f, u, o) < t_bg:
            typ[d] = BKG
        else:
            typ[d] = BOTH
    win = {LOC: np.zeros(D, bool), CLS: np.zeros(D, bool)}
    claimed = np.zeros(G, bool)
    for code in (LOC, CLS):
        for g in range(G):
            rows = [d for d in range(D) if typ[d] == code and attr[d] == g]
            if not rows:
                continue
            claimed[g] = True
            top = max(dt_score[d] for d in rows)
            winner = min(d for d in rows if dt_score[d] == top)
            win[code][winner] = code == LOC or not gt_matched[g]
    missed = np.array([not gt_ignore[g] and not gt_matched[g] and not claimed[g] for g in range(G)], bool)
    return {"type": typ, "attr": attr, "smax": smax, "win_loc": win[LOC], "win_cls": win[CLS], "missed": missed}


def _merge_order(det_cat, scores):
    n = len(scores)
    return np.lexsort((np.arange(n), -np.asarray(scores, np.float64), det_cat)).astype(np.int64) if n else np.zeros(0, np.int64)


def analyse(gts, dts, img_ids, cat_ids, mode="3D", t_fg=None, t_bg=None, area=0, max_det=100, rec_thrs=None):
    """The whole analysis on plain record lists -> dict in the detection order of the evaluator ((category, image) groups, descending
    score inside a group): type, attributed_gt (annotation id or -1), dt_ids, missed_gt_ids, counts (K, 6), dropped (8,), ap (K,),
    ap_fixed / dap (8, K), dap_mean (8,), loc_errors (K, 3) or None, loc_pairs; and for the checks of the test: `images` (per image:
    sim, the rows' categories and flags, the classification), `scores`, `det_cat`, `npig`, `tp` (true positives per category)."""
    flag, rkey, ranges, thrs, defaults = MODES[mode]
    t_fg = defaults[0] if t_fg is None else t_fg
    t_bg = defaults[1] if t_bg is None else t_bg
    rec_thrs = np.linspace(0.0, 1.0, 101) if rec_thrs is None else np.asarray(rec_thrs, np.float64)
    lo, hi = ranges[area]
    K = len(cat_ids)
    groups = []
    for k, cat in enumerate(cat_ids):
        for img in img_ids:
            g = [x for x in gts if x["image_id"] == img and x["category_id"] == cat]
            d = [x for x in dts if x["image_id"] == img and x["category_id"] == cat]
            if not g and not d:
                continue
            order = np.argsort([-x["score"] for x in d], kind="mergesort")
            groups.append((k, img, g, [d[i] for i in order[:max_det]]))
    dsz, gsz = [len(gr[3]) for gr in groups], [len(gr[2]) for gr in groups]
    doff, goff = np.concatenate([[0], np.cumsum(dsz)]).astype(np.int64), np.concatenate([[0], np.cumsum(gsz)]).astype(np.int64)
    sumD, sumG = int(doff[-1]), int(goff[-1])
    all_d, all_g = [x for gr in groups for x in gr[3]], [x for gr in groups for x in gr[2]]
    det_cat = np.repeat([gr[0] for gr in groups], dsz).astype(np.int64)
    gcat = np.repeat([gr[0] for gr in groups], gsz).astype(np.int64)
    scores = np.array([x["score"] for x in all_d], np.float64)
    dtm, dti, gtm, gig = np.zeros(sumD, bool), np.zeros(sumD, bool), np.zeros(sumG, bool), np.zeros(sumG, bool)
    typ, attr = np.zeros(sumD, np.int64), np.full(sumD, -1, np.int64)
    win_loc, win_cls, missed = np.zeros(sumD, bool), np.zeros(sumD, bool), np.zeros(sumG, bool)
    images = []
    for img in img_ids:
        mine = [n for n, gr in enumerate(groups) if gr[1] == img]
        drow = np.concatenate([np.arange(doff[n], doff[n + 1]) for n in mine] + [np.zeros(0, np.int64)]).astype(np.int64)
        grow = np.concatenate([np.arange(goff[n], goff[n + 1]) for n in mine] + [np.zeros(0, np.int64)]).astype(np.int64)
        sim = np.array([[similarity(mode, all_d[i], all_g[j]) for j in grow] for i in drow], np.float64).reshape(len(drow), len(grow))
        for n in mine:                                  # the greedy matching of every group of the image at (range, t_fg)
            di, gi = np.searchsorted(drow, doff[n]), np.searchsorted(grow, goff[n])
            _, _, g, d = groups[n]
            block = sim[di:di + len(d), gi:gi + len(g)]
            m, ig, g_ig = XL.match_group(block, [x.get(flag, 0) for x in g], [x[rkey] for x in g], [x[rkey] for x in d], lo, hi, t_fg)
            dtm[doff[n]:doff[n + 1]], dti[doff[n]:doff[n + 1]], gig[goff[n]:goff[n + 1]] = m >= 0, ig, g_ig
            gtm[goff[n] + m[m >= 0]] = True
        c = classify(sim, det_cat[drow], dtm[drow], dti[drow], scores[drow], gcat[grow], gtm[grow], gig[grow], t_fg, t_bg)
        typ[drow], win_loc[drow], win_cls[drow], missed[grow] = c["type"], c["win_loc"], c["win_cls"], c["missed"]
        attr[drow] = np.where(c["attr"] >= 0, grow[np.clip(c["attr"], 0, None)] if len(grow) else -1, -1)
        images.append({"sim": sim, "drow": drow, "grow": grow, "dt_cat": det_cat[drow], "gt_cat": gcat[grow], "gt_matched": gtm[grow],
                       "gt_ignore": gig[grow], **c})
    # ---- the oracles ----
    npig = np.bincount(gcat[~gig], minlength=K).astype(np.int64)
    has_e = np.bincount([gr[0] for gr in groups], minlength=K).clip(max=1)
    fp = np.isin(typ, (CLS, LOC, BOTH, DUPE, BKG))

    def ap_of(matched, ignored, cats, counts):
        order = _merge_order(cats, scores)
        cat_off = np.concatenate([[0], np.cumsum(np.bincount(cats, minlength=K))]).astype(np.int64)
        res = XL.accumulate(order, cat_off, np.zeros(sumD, np.int64), np.where(matched, 0, -1).reshape(1, 1, -1), ignored.reshape(1, 1, -1),
                            np.zeros(sumD, np.int64), np.zeros(1), np.zeros(1), counts.reshape(K, 1), has_e, rec_thrs, [max_det])
        p = res["precision"][0, :, :, 0, 0]
        return np.array([p[:, k].mean() if (p[:, k] > -1).all() else -1.0 for k in range(K)])

    ap = ap_of(dtm, dti, det_cat, npig)
    fixed = np.zeros((8, K))
    fixed[1] = ap_of(dtm | win_loc, dti | ((typ == LOC) & ~win_loc), det_cat, npig)
    moved = np.where(win_cls, gcat[np.clip(attr, 0, None)] if sumG else 0, det_cat)
    fixed[0] = ap_of(dtm | win_cls, dti | ((typ == CLS) & ~win_cls), moved, npig)
    for j, code in ((2, BOTH), (3, DUPE), (4, BKG)):
        fixed[j] = ap_of(dtm, dti | (typ == code), det_cat, npig)
    fixed[5] = ap_of(dtm, dti, det_cat, npig - np.bincount(gcat[missed], minlength=K))
    fixed[6] = ap_of(dtm, dti | fp, det_cat, npig)
    fixed[7] = ap_of(dtm, dti, det_cat, np.bincount(gcat[gtm & ~gig], minlength=K))
    both = (fixed > -1) & (ap > -1)
    dap = np.where(both, fixed - ap, np.nan)
    counts = np.stack([np.bincount(det_cat[typ == code], minlength=K) for code in (CLS, LOC, BOTH, DUPE, BKG)]
                      + [np.bincount(gcat[missed], minlength=K)], axis=1)
    gt_ids, dt_ids = np.array([x["id"] for x in all_g], np.int64), np.array([x["id"] for x in all_d], np.int64)
    loc_errors, loc_pairs = None, []
    if mode != "2D":
        loc_errors = np.full((K, 3), np.nan)
        rows = [[] for _ in range(K)]
        for d in np.flatnonzero(typ == LOC):
            e = pair_error(fit(np.array(all_d[d]["bbox3D"], np.float32)), fit(np.array(all_g[attr[d]]["bbox3D"], np.float32)))
            loc_pairs.append((int(d), int(attr[d]), e))
            if math.isfinite(e[0]):
                rows[det_cat[d]].append(e)
        for k in range(K):
            if rows[k]:
                loc_errors[k] = np.mean(np.array(rows[k]), axis=0)
    return {"t_fg": t_fg, "t_bg": t_bg, "type": typ, "attributed_gt": np.where(attr >= 0, gt_ids[np.clip(attr, 0, None)] if sumG else -1, -1),
            "dt_ids": dt_ids, "missed_gt_ids": gt_ids[missed], "counts": counts, "ap": ap, "ap_fixed": fixed, "dap": dap,
            "dap_mean": np.array([np.nanmean(r) if np.isfinite(r).any() else np.nan for r in dap]),
            "dropped": ((ap > -1) & (fixed == -1)).sum(axis=1), "loc_errors": loc_errors, "loc_pairs": loc_pairs, "images": images,
            "scores": scores, "det_cat": det_cat, "npig": npig, "tp": np.bincount(det_cat[dtm & ~dti], minlength=K), "win_loc": win_loc,
            "win_cls": win_cls, "attr_row": attr, "gt_cat": gcat, "gt_matched": gtm, "gt_ignore": gig, "thrs": thrs}
