"""The KITTI benchmark's average orientation similarity (AOS) in float64: the yardstick of `omni_kitti_match_counts_aos` /
`omni_kitti_finalize_aos` (csrc/eval_kitti.hip) and of `KittiEval` with `params.aos`.  Like tests/exact_kitti.py it is the project's
reading of the devkit (its `compute_aos` path), written from memory; the devkit is not part of this repository.

Pass 2 is RESTATED here (`statistics_pairs`), not imported, so that it also returns the (ground-truth row, detection) pair of every
true positive; `test_kitti_aos_match.py` shows that its counters equal those of `exact_kitti.statistics`.  The inner search over the
detections is written with numpy, the rules are those of exact_kitti.py: detections below the threshold do not exist; a ground truth
takes the unassigned detection of full height with the largest overlap above the min-overlap (the earliest among equals), and without
one the earliest qualifying detection below the height; both flags 0: a true positive.

Per true positive q = (1 + cos(alpha_gt - alpha_dt)) / 2, 0 when either alpha is not finite; aos[k] = sum q / (tp + fp), then made
monotone from the right and averaged exactly as precision is.  Images are the dicts of exact_kitti.py plus `gt_alpha` (G,) and
`dt_alpha` (D,)."""
import numpy as np

import exact_kitti as X

ONE = 2.0 ** 40            # the fixed point of the kernel's sum


def similarity(ga, da):
    return 0.5 * (1.0 + np.cos(ga - da)) if np.isfinite(ga) and np.isfinite(da) else 0.0


def statistics_pairs(img, m, thr, use_dc=True):
    """pass 2 at one threshold -> (tp, fp, fn, [(ground-truth row, detection) of every true positive])"""
    sim, score = np.asarray(img["sim"], np.float64), np.asarray(img["score"], np.float64)
    dt_flag, gt_flag = np.asarray(img["dt_flag"]), np.asarray(img["gt_flag"])
    D, G = len(dt_flag), len(gt_flag)
    sim = sim.reshape(D, G)
    exists = (dt_flag != -1) & ~(score < thr)
    assigned = np.zeros(D, bool)
    tp = fn = 0
    pairs = []
    for g in range(G):
        if gt_flag[g] == -1:
            continue
        cand = exists & ~assigned & (sim[:, g] > m)
        full = np.nonzero(cand & (dt_flag == 0))[0]
        small = np.nonzero(cand & (dt_flag == 1))[0]
        if len(full):
            chosen = int(full[np.argmax(sim[full, g])])          # argmax: the first of the largest
        elif len(small):
            chosen = int(small[0])
        else:
            fn += int(gt_flag[g] == 0)
            continue
        assigned[chosen] = True
        if gt_flag[g] == 0 and dt_flag[chosen] == 0:
            tp += 1
            pairs.append((g, chosen))
    open_ = exists & ~assigned & (dt_flag == 0)
    fp = int(open_.sum())
    dc = img.get("dc")
    if use_dc and dc is not None and D > 0:
        dc = np.asarray(dc, np.float64).reshape(D, -1)
        fp -= int((open_ & (dc > m).any(axis=1)).sum())
    return tp, fp, fn, pairs


def evaluate_slot_aos(images, m, use_dc=True, npts=X.N_SAMPLE_PTS):
    """-> dict: n_gt, thresholds, K, counts (npts, 3), pairs (per threshold, per image), sim (npts,) the float64 sums of q, sim_fixed
    (npts,) the integer sums of rint(q 2^40), precision, aos (npts,), ap_r40, ap_r11, aos_r40, aos_r11"""
    n_gt, v = 0, []
    for img in images:
        n_gt += int((np.asarray(img["gt_flag"]) == 0).sum())
        v += [x for x in X.statistics(img, m, -np.inf, False)[3] if x is not None]
    thr = X.thresholds(v, n_gt, npts)
    K = len(thr)
    counts, sim, fixed, all_pairs = np.zeros((npts, 3), np.int64), np.zeros(npts), np.zeros(npts, np.int64), []
    for k, t in enumerate(thr):
        per_image = []
        for img in images:
            tp, fp, fn, pairs = statistics_pairs(img, m, t, use_dc)
            counts[k] += (tp, fp, fn)
            for g, d in pairs:
                q = similarity(img["gt_alpha"][g], img["dt_alpha"][d])
                sim[k] += q
                fixed[k] += int(np.rint(q * ONE))
            per_image.append(pairs)
        all_pairs.append(per_image)
    prec, aos = np.zeros(npts), np.zeros(npts)
    for k in range(K):
        tp, fp, _ = (float(x) for x in counts[k])
        prec[k] = tp / (tp + fp) if tp + fp > 0 else 0.0
        aos[k] = sim[k] / (tp + fp) if tp + fp > 0 else 0.0
    for k in range(K):
        prec[k], aos[k] = prec[k:K].max(), aos[k:K].max()
    return {"n_gt": n_gt, "thresholds": thr, "K": K, "counts": counts, "pairs": all_pairs, "sim": sim, "sim_fixed": fixed, "precision": prec,
            "aos": aos, "ap_r40": 100.0 * float(np.mean(prec[1:])), "ap_r11": 100.0 * float(np.mean(prec[0::4])),
            "aos_r40": 100.0 * float(np.mean(aos[1:])), "aos_r11": 100.0 * float(np.mean(aos[0::4]))}
