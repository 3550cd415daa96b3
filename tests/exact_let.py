"""The longitudinal-error-tolerant metrics (LET-3D-AP / LET-3D-APL, Hung et al. 2022) written from their definition, in float64, numpy
and Python loops: the reference of tests/test_let_iou.py and tests/test_let_eval.py.  Uses no kernel: the fit is `exact_tp_errors.fit`,
the IoU `exact_iou3d.iou3d` (Qhull) on corners rebuilt from the fits.

Pair (detection with fitted centre P, ground truth with fitted centre G, the sensor at the origin): u = P / |P|, lon = (G - P) . u,
T = max(tol_frac |G|, tol_min), aff = 1 - min(|lon| / T, 1); the aligned box is the detection's fit with its centre at P + lon u;
let_iou = IoU3D(aligned box, fitted ground truth) as float32 when aff > 0, 0 when aff == 0.  Gated (0, 0, NaN): an invalid box, an index
outside its set, |P| <= eps_dim.
Matching (the rules in the header of csrc/eval_match.hip): per (image, category) group, depth range and IoU threshold, the detections
in descending score order, cut to the largest maxDets; a ground truth is ignored when flagged or outside the depth range; a detection
takes the unmatched non-ignored ground truth with the LARGEST let_iou >= min(t, 1 - 1e-10), the later one among equals, an ignored one
only when no non-ignored one qualifies; it is ignored when its match is, or when unmatched and outside the depth range.  Proximity
evaluation: a pair whose 2D boxes overlap by no more than proximity_thresh can not match, and a detection of a group with ground truths
none of which is in proximity is ignored.
Accumulation: the COCO tables of `Omni3Deval.accumulate` (precision [T,R,K,A,M], recall [T,K,A,M]) and, on the same lists,
precision_l: at a list position prec_L = (sum of aff over the true positives so far) / (tp + fp + spacing(1)), made monotone from the
right and sampled at the recall thresholds like precision; tp_affinity / tp_lon [T,K,A,M]: the means of aff / lon over the true
positives of the included detections, -1 without one."""
import math

import numpy as np

import exact_iou3d
from exact_tp_errors import SIGNS, fit

GATED = (0.0, 0.0, math.nan)
IOU_THRS = np.linspace(0.05, 0.5, 10)
AREA_RNG = ((0, 1e5), (0, 10), (10, 35), (35, 1e5))


def corners(c, X, d):
    """the eight corners of a fitted cuboid in the order of boxgen.UNIT, float64"""
    return c + (SIGNS * 0.5 * d) @ X


def let_pair(fd, fg, tol_frac=0.1, tol_min=0.5, eps_dim=1e-8, iou=True):
    """two fits (detection, ground truth) -> (let_iou, aff, lon); iou=False leaves let_iou None where it would need Qhull"""
    if fd is None or fg is None:
        return GATED
    (P, Xd, dd), (G, Xg, dg) = fd, fg
    rng = math.sqrt(float(np.dot(P, P)))
    if not rng > eps_dim:
        return GATED
    u = P / rng
    lon = float(np.dot(G - P, u))
    T = max(tol_frac * math.sqrt(float(np.dot(G, G))), tol_min)
    aff = 1.0 - min(abs(lon) / T, 1.0)
    if not aff > 0.0:
        return 0.0, 0.0, lon
    if not iou:
        return None, aff, lon
    if np.linalg.norm(P + lon * u - G) > 0.5 * (np.linalg.norm(dd) + np.linalg.norm(dg)):
        return 0.0, aff, lon                            # disjoint bounding spheres: nothing for Qhull to intersect
    r = exact_iou3d.iou3d(corners(P + lon * u, Xd, dd), corners(G, Xg, dg))[1]
    return float(np.float32(min(max(r, 0.0), 1.0))), aff, lon


def let_pairs(boxes1, boxes2, idx1, idx2, tol_frac=0.1, tol_min=0.5, iou=True):
    """-> (iou (P,), aff (P,), lon (P,)) float64 (iou holds float32 values)"""
    f1, f2 = [fit(b) for b in boxes1], [fit(b) for b in boxes2]
    out = np.empty((len(idx1), 3), np.float64)
    for p, (i, j) in enumerate(zip(idx1, idx2)):
        ok = 0 <= i < len(f1) and 0 <= j < len(f2)
        r = let_pair(f1[i], f2[j], tol_frac, tol_min, iou=iou) if ok else GATED
        out[p] = (math.nan if r[0] is None else r[0], r[1], r[2])
    return out[:, 0], out[:, 1], out[:, 2]


def plain_iou(boxes1, boxes2):
    """the exact IoU3D of the fitted pairs without the alignment (0 with an invalid box): what the alignment is compared with"""
    out = np.zeros(len(boxes1))
    for p, (a, b) in enumerate(zip(boxes1, boxes2)):
        fa, fb = fit(a), fit(b)
        if fa is not None and fb is not None and np.linalg.norm(fa[0] - fb[0]) < 0.5 * (np.linalg.norm(fa[2]) + np.linalg.norm(fb[2])):
            out[p] = exact_iou3d.iou3d(corners(*fa), corners(*fb))[1]
    return out


def match_group(iou, gt_flag, gt_depth, dt_depth, lo, hi, thr):
    """iou (D, G) with the detections in score order -> (dt_match (D,) index of the gt or -1, dt_ignore (D,) bool, gt_ignore (G,))"""
    D, G = iou.shape
    lo, hi = np.float32(lo), np.float32(hi)
    g_ig = np.array([bool(gt_flag[g]) or np.float32(gt_depth[g]) < lo or np.float32(gt_depth[g]) > hi for g in range(G)], bool)
    thr = min(float(thr), 1 - 1e-10)
    taken = np.zeros(G, bool)
    dtm, dti = np.full(D, -1, np.int64), np.zeros(D, bool)
    for d in range(D):
        m = -1
        for ignored in (False, True):
            best = -1.0
            for g in range(G):
                if g_ig[g] != ignored or taken[g] or not iou[d, g] >= thr:
                    continue
                if iou[d, g] >= best:
                    best, m = iou[d, g], g
            if m >= 0:
                break
        if m >= 0:
            taken[m] = True
            dtm[d], dti[d] = m, g_ig[m]
        else:
            dti[d] = np.float32(dt_depth[d]) < lo or np.float32(dt_depth[d]) > hi
    return dtm, dti, g_ig


def _envelope_sample(pr, rc, rec_thrs):
    pr = list(pr)
    for i in range(len(pr) - 1, 0, -1):
        if pr[i] > pr[i - 1]:
            pr[i - 1] = pr[i]
    q = np.zeros(len(rec_thrs))
    for ri, pi in enumerate(np.searchsorted(rc, rec_thrs, side="left")):
        if pi < len(pr):
            q[ri] = pr[pi]
    return q


def accumulate(order, cat_off, rank, dt_match, dt_ignore, pair_row, aff, lon, npig, has_e, rec_thrs, max_dets, scores=None):
    """numpy arrays in the layout of `kernels.let.accumulate_let` -> dict(precision, precision_l [T,R,K,A,M], recall, tp_affinity,
    tp_lon [T,K,A,M]); with the detections' scores (sumD,) also `scores` [T,R,K,A,M], the score at the sampled position"""
    A, T, _ = dt_match.shape
    K, R, M = len(cat_off) - 1, len(rec_thrs), len(max_dets)
    out = {"precision": -np.ones((T, R, K, A, M)), "precision_l": -np.ones((T, R, K, A, M)), "recall": -np.ones((T, K, A, M)),
           "tp_affinity": -np.ones((T, K, A, M)), "tp_lon": -np.ones((T, K, A, M)), "scores": -np.ones((T, R, K, A, M))}
    for k in range(K):
        if not has_e[k]:
            continue
        lst = np.asarray(order[cat_off[k]:cat_off[k + 1]], np.int64)
        for a in range(A):
            if npig[k, a] == 0:
                continue
            for m, md in enumerate(max_dets):
                sel = lst[rank[lst] < md]
                for t in range(T):
                    dtm, dti = dt_match[a, t, sel], dt_ignore[a, t, sel].astype(bool)
                    is_tp, is_fp = (dtm >= 0) & ~dti, (dtm < 0) & ~dti
                    tp, fp = np.cumsum(is_tp).astype(np.float64), np.cumsum(is_fp).astype(np.float64)
                    w, ln, run = np.zeros(len(sel)), np.zeros(len(sel)), 0.0
                    cw = np.zeros(len(sel))
                    for i in range(len(sel)):
                        if is_tp[i]:
                            row = int(pair_row[sel[i]] + dtm[i])
                            w[i], ln[i] = aff[row], lon[row]
                            run += w[i]
                        cw[i] = run
                    nd = len(sel)
                    rc = tp / npig[k, a]
                    den = fp + tp + np.spacing(1)
                    out["recall"][t, k, a, m] = rc[-1] if nd else 0
                    out["precision"][t, :, k, a, m] = _envelope_sample(tp / den, rc, rec_thrs)
                    out["precision_l"][t, :, k, a, m] = _envelope_sample(cw / den, rc, rec_thrs)
                    if scores is not None:
                        at = np.searchsorted(rc, rec_thrs, side="left")
                        out["scores"][t, :, k, a, m] = [scores[sel[pi]] if pi < nd else 0.0 for pi in at]
                    if is_tp.any():
                        out["tp_affinity"][t, k, a, m] = math.fsum(w[is_tp]) / int(is_tp.sum())
                        out["tp_lon"][t, k, a, m] = math.fsum(ln[is_tp]) / int(is_tp.sum())
    return out


def _iou2d(b1, b2):
    iw = max(min(b1[0] + b1[2], b2[0] + b2[2]) - max(b1[0], b2[0]), 0.0)
    ih = max(min(b1[1] + b1[3], b2[1] + b2[3]) - max(b1[1], b2[1]), 0.0)
    return iw * ih / (b1[2] * b1[3] + b2[2] * b2[3] - iw * ih)


def summarize(res, iou_thrs=IOU_THRS):
    """-> stats (13,) of the 3D protocol on precision / recall, stats_l (7,) the same seven AP slots on precision_l, let_stats (2,)"""
    M = res["precision"].shape[-1]
    it = lambda thr: [t for t, v in enumerate(iou_thrs) if np.isclose(v, thr)]      # noqa: E731

    def ap(table, thr=None, a=0, m=M - 1):
        s = table if thr is None else table[it(thr)]
        s = s[:, :, :, a, m]
        return -1 if not (s > -1).any() else float(np.mean(s[s > -1]))

    def ar(a=0, m=M - 1):
        s = res["recall"][:, :, a, m]
        return -1 if not (s > -1).any() else float(np.mean(s[s > -1]))

    seven = lambda tb: [ap(tb), ap(tb, 0.15), ap(tb, 0.25), ap(tb, 0.5), ap(tb, a=1), ap(tb, a=2), ap(tb, a=3)]      # noqa: E731
    stats = np.array(seven(res["precision"]) + [ar(m=0), ar(m=1), ar(m=2), ar(a=1), ar(a=2), ar(a=3)])
    t25 = it(0.25)[0]
    af, ln = res["tp_affinity"][t25, :, 0, M - 1], res["tp_lon"][t25, :, 0, M - 1]
    has = af > -1
    let_stats = np.array([float(np.mean(af[has])), float(np.mean(ln[has]))]) if has.any() else np.array([-1.0, -1.0])
    return stats, np.array(seven(res["precision_l"])), let_stats


def evaluate(gts, dts, img_ids, cat_ids, tol_frac=0.1, tol_min=0.5, iou_thrs=IOU_THRS, area_rng=AREA_RNG, max_dets=(1, 10, 100),
             rec_thrs=None, eval_prox=False, proximity_thresh=0.3):
    """The whole pipeline on plain record lists.  eval_prox: False, True, or a collection of image ids.  -> dict with `groups`,
    `tables` (per group: iou / aff / lon (D, G), match[a, t] = (dt_match, dt_ignore, gt_ignore)), the tables of `accumulate`, and
    stats / stats_l / let_stats of `summarize`."""
    rec_thrs = np.linspace(0.0, 1.0, 101) if rec_thrs is None else np.asarray(rec_thrs, np.float64)
    T, K, A = len(iou_thrs), len(cat_ids), len(area_rng)
    groups = []                                         # (k, image, gts, dts by descending score cut to the largest maxDets)
    for k, cat in enumerate(cat_ids):
        for img in img_ids:
            g = [x for x in gts if x["image_id"] == img and x["category_id"] == cat]
            d = [x for x in dts if x["image_id"] == img and x["category_id"] == cat]
            if not g and not d:
                continue
            order = np.argsort([-x["score"] for x in d], kind="mergesort")
            groups.append((k, img, g, [d[i] for i in order[:max(max_dets)]]))
    tables = []
    for k, img, g, d in groups:
        fg = [fit(np.array(x["bbox3D"], np.float32)) for x in g]
        fd = [fit(np.array(x["bbox3D"], np.float32)) for x in d]
        trip = np.array([[let_pair(a, b, tol_frac, tol_min) for b in fg] for a in fd], np.float64).reshape(len(d), len(g), 3)
        iou = trip[:, :, 0].copy()
        far = np.zeros(len(d), bool)
        if (eval_prox is True or (eval_prox is not False and img in set(eval_prox))) and len(g) and len(d):
            prox = np.array([[_iou2d(a["bbox"], b["bbox"]) > proximity_thresh for b in g] for a in d], bool)
            iou[~prox] = -1.0
            far = ~prox.any(axis=1)
        res = {}
        for a, (lo, hi) in enumerate(area_rng):
            for t, thr in enumerate(iou_thrs):
                dtm, dti, gig = match_group(iou, [x.get("ignore3D", 0) for x in g], [x["depth"] for x in g], [x["depth"] for x in d], lo, hi, thr)
                res[a, t] = (dtm, dti | far, gig)
        tables.append({"iou": trip[:, :, 0], "aff": trip[:, :, 1], "lon": trip[:, :, 2], "match": res,
                       "scores": np.array([x["score"] for x in d], np.float64)})
    dsz = np.array([len(gr[3]) for gr in groups], np.int64)
    gsz = np.array([len(gr[2]) for gr in groups], np.int64)
    sumD = int(dsz.sum())
    cat_of = np.array([gr[0] for gr in groups], np.int64)
    det_cat = np.repeat(cat_of, dsz)
    scores = np.concatenate([tb["scores"] for tb in tables]) if tables else np.zeros(0)
    rank = np.concatenate([np.arange(n) for n in dsz]) if len(groups) else np.zeros(0, np.int64)
    order = np.concatenate([np.flatnonzero(det_cat == k)[np.argsort(-scores[det_cat == k], kind="mergesort")] for k in range(K)]) \
        if sumD else np.zeros(0, np.int64)
    cat_off = np.concatenate([[0], np.cumsum(np.bincount(det_cat, minlength=K))])
    cat = lambda i: (np.stack([np.stack([np.concatenate([tb["match"][a, t][i] for tb in tables]) for t in range(T)]) for a in range(A)])      # noqa: E731
                     if tables else np.zeros((A, T, 0)))
    dt_match, dt_ignore, gt_ig = cat(0).astype(np.int64), cat(1).astype(bool), cat(2).astype(bool)
    gcat = np.repeat(cat_of, gsz)
    npig = np.stack([np.bincount(gcat[~gt_ig[a, 0]], minlength=K) for a in range(A)], axis=1)
    has_e = np.bincount(cat_of, minlength=K).clip(max=1)
    pair_off = np.concatenate([[0], np.cumsum(dsz * gsz)])[:-1]
    pair_row = np.repeat(pair_off, dsz) + rank * np.repeat(gsz, dsz)
    flat = lambda key: np.concatenate([tb[key].reshape(-1) for tb in tables]) if tables else np.zeros(0)      # noqa: E731
    out = accumulate(order, cat_off, rank, dt_match, dt_ignore, pair_row, flat("aff"), flat("lon"), npig, has_e, rec_thrs, list(max_dets), scores)
    out["stats"], out["stats_l"], out["let_stats"] = summarize(out, iou_thrs)
    out.update({"groups": groups, "tables": tables, "dt_match": dt_match, "dt_ignore": dt_ignore, "let_iou": flat("iou"),
                "aff": flat("aff"), "lon": flat("lon")})
    return out
