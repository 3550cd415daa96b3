"""The KITTI object benchmark's protocol as plain float64 loops: the yardstick of csrc/eval_kitti.hip and of
`cubercnn.evaluation.kitti.KittiEval`.  It is the project's reading of the devkit's `evaluate_object`, written from memory (the devkit
is not part of this repository); similarity matrices come in, nothing here knows about boxes.

Per image a dict: `sim` (D, G) similarities, detection x ground-truth row, detections in descending score order; `score` (D,);
`dt_flag` (D,) and `gt_flag` (G,) as made by `dt_flags` / `gt_flags`; `dc` (D, R) the DontCare overlaps (optional).
"""
import numpy as np

N_SAMPLE_PTS = 41
OCC_CUTS = (0.75, 0.5, 0.25)


def occlusion_level(ann, cuts=OCC_CUTS):
    """the integer `occlusion` key when the annotation has one, else the number of cuts c with visibility <= c (0 when unknown)"""
    if ann.get("occlusion") is not None:
        return int(ann["occlusion"])
    v = float(ann.get("visibility", -1))
    return 0 if v < 0 else sum(1 for c in cuts if v <= c)


def gt_flags(rel, height, occ, trunc, difficulty):
    """rel: 0 the class, 1 a neighbour class, 2 the class but set aside (an `ignore` flag the three bounds do not explain), anything
    else other -> 0 counted, 1 neutral, -1 no candidate"""
    hmin, omax, tmax = difficulty
    out = []
    for r, h, o, t in zip(rel, height, occ, trunc):
        hard = o > omax or t > tmax or h < hmin
        out.append((1 if hard else 0) if r == 0 else 1 if r == 1 or (r == 2 and hard) else -1)
    return np.array(out, dtype=np.int64)


def dt_flags(is_class, height, hmin):
    return np.array([-1 if not c else 1 if h < hmin else 0 for c, h in zip(is_class, height)], dtype=np.int64)


def statistics(img, m, thr, compute_fp, use_dc=True):
    """-> (tp, fp, fn, per ground-truth row the score of its true positive or None)"""
    sim, score, dt_flag, gt_flag = np.asarray(img["sim"], np.float64), img["score"], img["dt_flag"], img["gt_flag"]
    D, G = len(dt_flag), len(gt_flag)
    assigned = [False] * D
    tp = fp = fn = 0
    tp_score = [None] * G

    def usable(d):
        return dt_flag[d] != -1 and not assigned[d] and not (compute_fp and score[d] < thr)

    for g in range(G):
        if gt_flag[g] == -1:
            continue
        chosen, chosen_small, best_sim, best_score = None, False, -np.inf, None
        for d in range(D):
            if not usable(d) or not float(sim[d, g]) > m:
                continue
            if not compute_fp:
                if chosen is None or score[d] > best_score:
                    chosen, best_score = d, score[d]
            elif dt_flag[d] == 0 and (sim[d, g] > best_sim or chosen_small):
                chosen, chosen_small, best_sim = d, False, sim[d, g]
            elif chosen is None and dt_flag[d] == 1:
                chosen, chosen_small = d, True
        if chosen is None:
            fn += gt_flag[g] == 0
        elif gt_flag[g] == 1 or dt_flag[chosen] == 1:
            assigned[chosen] = True
        else:
            tp += 1
            assigned[chosen] = True
            tp_score[g] = score[chosen]
    if compute_fp:
        fp = sum(1 for d in range(D) if usable(d) and dt_flag[d] == 0)
        dc = img.get("dc")
        if use_dc and dc is not None and D > 0:
            dc = np.asarray(dc, np.float64).reshape(D, -1)
            for r in range(dc.shape[1]):
                for d in range(D):
                    if usable(d) and dt_flag[d] == 0 and float(dc[d, r]) > m:
                        assigned[d] = True
                        fp -= 1
    return int(tp), int(fp), int(fn), tp_score


def thresholds(v, n_gt, npts=N_SAMPLE_PTS):
    """the scores the recall sampling keeps (at most npts: the precision table has no more rows)"""
    v = sorted(v, reverse=True)
    out, cur = [], 0.0
    for i in range(len(v)):
        if len(out) == npts:
            break
        l = (i + 1) / n_gt
        r = (i + 2) / n_gt if i < len(v) - 1 else l
        if (r - cur) < (cur - l) and i < len(v) - 1:
            continue
        out.append(v[i])
        cur += 1.0 / (npts - 1)
    return out


def evaluate_slot(images, m, use_dc=True, npts=N_SAMPLE_PTS):
    """one (class, difficulty, metric, overlap set) -> dict: n_gt, tp_score (per image, per row), thresholds, K, counts (npts, 3),
    precision, recall (npts,), ap_r40, ap_r11.  Precision is indexed by THRESHOLD as in the devkit, so fewer than 2 (npts - 1) counted
    ground truths cannot reach 100."""
    n_gt, v, rows = 0, [], []
    for img in images:
        n_gt += int((np.asarray(img["gt_flag"]) == 0).sum())
        s = statistics(img, m, -np.inf, False)[3]
        rows.append(s)
        v += [x for x in s if x is not None]
    thr = thresholds(v, n_gt, npts)
    K = len(thr)
    counts = np.zeros((npts, 3), np.int64)
    for k, t in enumerate(thr):
        for img in images:
            counts[k] += statistics(img, m, t, True, use_dc)[:3]
    prec, rec = np.zeros(npts), np.zeros(npts)
    for k in range(K):
        tp, fp, fn = (float(x) for x in counts[k])
        prec[k] = tp / (tp + fp) if tp + fp > 0 else 0.0
        rec[k] = tp / (tp + fn) if tp + fn > 0 else 0.0
    for k in range(K):
        prec[k] = prec[k:K].max()
    return {"n_gt": n_gt, "tp_score": rows, "thresholds": thr, "K": K, "counts": counts, "precision": prec, "recall": rec,
            "ap_r40": 100.0 * float(np.mean(prec[1:])), "ap_r11": 100.0 * float(np.mean(prec[0::4]))}
