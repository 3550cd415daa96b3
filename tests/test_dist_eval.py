"""`Omni3Deval(mode="DIST")`, `dist_errors_groups`, the `eval_dist` switch of `Omni3DEvaluator` / `Omni3DEvaluationHelper` and
`config.add_dist_eval_config`: the centre-distance protocol with its ATE / ASE / AOE true-positive errors.

The reference has no such mode, so the yardstick is tests/exact_tp_errors.py: the whole pipeline (fit, errors, greedy matching,
accumulation, TP aggregation) written from the definitions in float64 with Python loops.  Match tables, precision, recall and the AP
stats must be EQUAL to it; `tp_errors`, `tp_stats` and the per-category entries within 2e-9 (the bound of tests/test_tp_errors.py).
Equality can only be asked of inputs on which float32 rounding of the similarity 1 / (1 + dist) decides nothing -- it moves a
distance by at most (1 + d) x 6e-8 --, so, in float64: no pair's distance lies within 1e-4 of a threshold, no two ground truths of a
group that lie within 4 m + 1e-4 of the same detection differ by less than 1e-4 in distance, and no two scores of a category tie.  The
split is generated from the first seed from 1 on that meets this, which `test_reference_alone_meets_the_conditions` asserts on the CPU.
"""
import copy
import functools
import math
import os

import numpy as np
import pytest
import torch

import exact_tp_errors as X
from omni3d_amd import boxgen

N_IMG, N_CAT = 6, 4                 # categories 1..3: the small groups; category 4: about 135 detections over 3 images
DIST_THRS = (0.5, 1.0, 2.0, 4.0)
MARGIN = 1e-4
SEED = 2                            # the first seed from 1 on that meets the conditions (asserted below)
TP_TOL = 2e-9
UPS = (None, (0.0, -1.0, 0.0))


def _ry(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def _rec(img, cat, box, score=None, ignore=0):
    box = np.asarray(box, np.float32)
    with np.errstate(invalid="ignore"):
        depth = float(np.nanmean(box[:, 2]))
    u, v = 64.0 + 40.0 * box[:, 0] / np.maximum(box[:, 2], 0.1), 48.0 + 40.0 * box[:, 1] / np.maximum(box[:, 2], 0.1)
    u, v = np.nan_to_num(u), np.nan_to_num(v)
    bbox = [float(u.min()), float(v.min()), float(u.max() - u.min() + 1.0), float(v.max() - v.min() + 1.0)]
    r = {"image_id": img, "category_id": cat, "bbox3D": box.tolist(), "depth": depth, "bbox": bbox, "area": bbox[2] * bbox[3]}
    if score is None:
        r.update(ignore3D=ignore, ignore2D=0, iscrowd=0)
    else:
        r["score"] = float(score)
    return r


@functools.lru_cache(maxsize=None)
def _split(seed):
    """(ground truths, detections): 6 images x 3 categories with up to 6 ground truths and 12 detections per group, groups without
    detections, without ground truth and with `ignore3D`, depths over all three ranges, one detection with a NaN vertex; category 4
    in images 1..3 with 15 ground truths and 45 detections each.  Detections are copies moved by 0.05 .. 5 m, scaled and turned."""
    rng = np.random.default_rng(seed)
    gts, dts = [], []

    def one_gt():
        c = np.array([rng.uniform(-8, 8), rng.uniform(-1, 1), rng.uniform(3, 60)])
        return c, rng.uniform(0.6, 4.0, 3), boxgen.rand_rot(rng, 1)[0]

    def box(c, d, R):
        return boxgen.corners(np.asarray(c)[None], np.asarray(d)[None], R[None])[0]

    def candidate(img, cat, c, d, R, score):
        step = rng.normal(size=3)
        c2 = c + step / np.linalg.norm(step) * math.exp(rng.uniform(math.log(0.05), math.log(5.0)))
        d2 = d * rng.uniform(0.7, 1.3, 3)
        dts.append(_rec(img, cat, box(c2, d2, R @ _ry(rng.normal(scale=0.3))), score=score))

    for img in range(1, N_IMG + 1):
        for cat in range(1, 4):
            n_gt = int(rng.integers(0, 7)) if (img + cat) % 5 else 0
            n_fp = int(rng.integers(0, 4))
            have_dt = (img + 2 * cat) % 6 != 0
            for _ in range(n_gt):
                c, d, R = one_gt()
                gts.append(_rec(img, cat, box(c, d, R), ignore=int(rng.uniform() < 0.15)))
                for _ in range(int(rng.integers(0, 3)) if have_dt else 0):
                    candidate(img, cat, c, d, R, rng.uniform(0.05, 0.99))
            for _ in range(n_fp if have_dt else 0):
                c, d, R = one_gt()
                dts.append(_rec(img, cat, box(c, d, R), score=rng.uniform(0.05, 0.6)))
    for img in range(1, 4):
        for _ in range(15):
            c, d, R = one_gt()
            gts.append(_rec(img, 4, box(c, d, R), ignore=int(rng.uniform() < 0.1)))
            for _ in range(2):
                candidate(img, 4, c, d, R, rng.uniform(0.05, 0.99))
        for _ in range(15):
            c, d, R = one_gt()
            dts.append(_rec(img, 4, box(c, d, R), score=rng.uniform(0.05, 0.7)))
    bad = np.array(dts[3]["bbox3D"], np.float32)
    bad[2, 0] = np.nan
    dts[3]["bbox3D"] = bad.tolist()
    for k, r in enumerate(gts + dts):
        r["id"] = k + 1
    return gts, dts


def _by_group(recs):
    out = {}
    for r in recs:
        out.setdefault((r["image_id"], r["category_id"]), []).append(r)
    return out


@functools.lru_cache(maxsize=None)
def _conditions(seed):
    """float64 alone -> (smallest distance of a pair's distance to a threshold, smallest difference of two candidate ground truths
    of one detection, number of score ties, facts about the split)"""
    gts, dts = _split(seed)
    G, D = _by_group(gts), _by_group(dts)
    to_thr, apart, dists = math.inf, math.inf, []
    for key in sorted(set(G) | set(D)):
        fg = [X.fit(np.array(x["bbox3D"], np.float32)) for x in G.get(key, [])]
        fd = [X.fit(np.array(x["bbox3D"], np.float32)) for x in D.get(key, [])]
        for a in fd:
            for up in UPS:                                         # both distances the tests evaluate with
                row = [X.errors(a, b, up)[0] for b in fg]
                dists += row if up is None else []
                to_thr = min([to_thr] + [abs(v - t) for v in row for t in DIST_THRS if math.isfinite(v)])
                close = sorted(v for v in row if v <= 4.0 + MARGIN)
                apart = min([apart] + [b - a_ for a_, b in zip(close, close[1:])])
    ties = 0
    for cat in range(1, N_CAT + 1):
        s = [x["score"] for x in dts if x["category_id"] == cat]
        ties += len(s) - len(set(s))
    sizes = [(len(G.get(k, [])), len(D.get(k, []))) for k in sorted(set(G) | set(D))]
    depth = np.array([x["depth"] for x in gts])
    facts = dict(dists=np.array(dists), sizes=sizes, ignore=sum(x["ignore3D"] for x in gts), n4=sum(x["category_id"] == 4 for x in dts),
                 ranges=[int((depth < 10).sum()), int(((depth >= 10) & (depth < 35)).sum()), int((depth >= 35).sum())])
    return to_thr, apart, ties, facts


def _good(seed):
    to_thr, apart, ties, f = _conditions(seed)
    kinds = any(g and not d for g, d in f["sizes"]) and any(d and not g for g, d in f["sizes"])         # no detections / no ground truth
    spread = f["ignore"] >= 2 and min(f["ranges"]) >= 3 and f["n4"] == 135
    d = f["dists"]
    mix = all(((d > lo) & (d <= hi)).sum() >= 10 for lo, hi in ((0, 0.5), (0.5, 1.0), (1.0, 2.0), (2.0, 4.0))) and np.isinf(d).sum() >= 1
    return to_thr >= MARGIN and apart >= MARGIN and ties == 0 and kinds and spread and bool(mix)


def test_reference_alone_meets_the_conditions():
    assert next(s for s in range(1, 50) if _good(s)) == SEED
    gts, dts = _split(SEED)
    assert X.fit(np.array(dts[3]["bbox3D"], np.float32)) is None                                       # the NaN detection


IMGS, CATS = list(range(1, N_IMG + 1)), list(range(1, N_CAT + 1))


@functools.lru_cache(maxsize=None)
def _reference(seed, up=None, cats=tuple(CATS)):
    gts, dts = _split(seed)
    return X.evaluate(gts, dts, IMGS, list(cats), DIST_THRS, up=up)


def _evaluate(gts, dts, imgs=IMGS, cats=CATS, **kw):
    from omni3d_amd.cubercnn.evaluation import omni3d_evaluation as E
    ev = E.Omni3Deval(E.AnnotationIndex(copy.deepcopy(list(gts)), imgs, cats), E.AnnotationIndex(copy.deepcopy(list(dts)), imgs, cats), mode="DIST", **kw)
    ev.evaluate()
    ev.accumulate()
    return ev, ev.summarize()


def _reference_tables(ref, A, T):
    """the reference's per-group tables in the evaluator's layout: dt_match / dt_ignore (A, T, sumD), gt_ignore (A, sumG)"""
    dtm = np.stack([np.stack([np.concatenate([tb["match"][a, t][0] for tb in ref["tables"]]) for t in range(T)]) for a in range(A)])
    dti = np.stack([np.stack([np.concatenate([tb["match"][a, t][1] for tb in ref["tables"]]) for t in range(T)]) for a in range(A)])
    gti = np.stack([np.concatenate([tb["match"][a, 0][2] for tb in ref["tables"]]) for a in range(A)])
    return dtm, dti, gti


def _run_dist_mode(capsys):
    from omni3d_amd.cubercnn.evaluation import omni3d_evaluation as E
    gts, dts = _split(SEED)
    for up in UPS:
        ev, text = _evaluate(gts, dts, up=up)
        ref = _reference(SEED, up)
        assert "Warning: skipping 1 boxes" in capsys.readouterr().out                                  # the NaN detection is reported
        m = {k: v.cpu().numpy() for k, v in ev._dev["match"].items()}
        dtm, dti, gti = _reference_tables(ref, 4, 4)
        assert np.array_equal(m["dt_match"], dtm) and np.array_equal(m["dt_ignore"].astype(bool), dti)
        assert np.array_equal(m["gt_ignore"].astype(bool), gti)
        assert np.array_equal(ev.eval["precision"], ref["precision"]) and np.array_equal(ev.eval["recall"], ref["recall"])
        assert np.array_equal(ev.stats, ref["stats"])
        assert (dtm >= 0).sum() > 200 and 0.02 < ev.stats[0] < 0.98                                   # something is matched, not everything
        assert np.array_equal(ev.eval["tp_count"], ref["tp_count"]) and ev.eval["tp_errors"].shape == (N_CAT, 4, 3)
        assert np.array_equal(ev.eval["tp_errors"] == -1, ref["tp_errors"] == -1)
        worst = float(np.abs(ev.eval["tp_errors"] - ref["tp_errors"]).max())
        print("up %r: |tp_errors - fp64| %.2e" % (up, worst))
        assert worst <= TP_TOL and np.abs(ev.tp_stats - ref["tp_stats"]).max() <= TP_TOL
        assert (ref["tp_errors"][:, 0] > 0).all() and (ref["tp_errors"][:, 0] != 1.0).all()            # every category has real errors
        lines = text.split("\n")
        assert len(lines) == 16 and all(ln.startswith("mode=DIST ") for ln in lines) and "IoU" not in text
        assert "dist=0.50:4.00" in lines[0] and "dist=0.50 " in lines[1] and "dist=1.00 " in lines[2] and "dist=2.00 " in lines[3]
        assert "depth=  near" in lines[4] and "(mATE)" in lines[13] and "(mASE)" in lines[14] and "(mAOE)" in lines[15]
        assert lines[13].endswith("= %0.3f" % ev.tp_stats[0]) and "dist=2.00" in lines[13]
        res = E._derive_results(ev, "DIST", ["c%d" % c for c in CATS])
        assert list(res)[:7] == ["AP", "AP@0.5m", "AP@1m", "AP@2m", "APn", "APm", "APf"] and res["AP@1m"] == ev.stats[2] * 100
        for k, c in enumerate(CATS):
            for j, n in enumerate(("ATE", "ASE", "AOE")):
                assert abs(res["%s-c%d" % (n, c)] - ref["tp_errors"][k, 0, j]) <= TP_TOL
        assert [abs(res["m" + n] - ref["tp_stats"][j]) <= TP_TOL for j, n in enumerate(("ATE", "ASE", "AOE"))] == [True] * 3
    # with the ground plane the distances are smaller: at least as many matches; both differ
    assert not np.array_equal(_reference(SEED, None)["precision"], _reference(SEED, (0.0, -1.0, 0.0))["precision"])
    # thresholds are looked up in distThrs, not by position; tpDist must be one of them
    ev = E.Omni3Deval(E.AnnotationIndex(copy.deepcopy(list(gts)), IMGS, CATS), E.AnnotationIndex(copy.deepcopy(list(dts)), IMGS, CATS), mode="DIST")
    ev.params.distThrs = [4.0, 2.0, 1.0]
    ev.evaluate()
    ev.accumulate()
    ev.summarize()
    full = _reference(SEED, None)
    assert ev.stats[1] == -1 and ev.stats[2] == full["stats"][2] and ev.stats[3] == full["stats"][3]
    assert np.abs(ev.eval["tp_errors"] - full["tp_errors"]).max() <= TP_TOL
    ev.params.tpDist = 3.0
    with pytest.raises(ValueError):
        ev.evaluate()
    p = E.Omni3DParams("DIST")
    assert p.areaRngLbl == E.Omni3DParams("3D").areaRngLbl and p.maxDets == [1, 10, 100] and p.tpDist == 2.0 and p.minRecall == 0.1
    assert list(p.distThrs) == [0.5, 1.0, 2.0, 4.0] and np.array_equal(p.iouThrs, 1.0 / (1.0 + np.array([0.5, 1.0, 2.0, 4.0])))
    assert E.Omni3Deval(mode="DIST").up is None and E.Omni3Deval(mode="BEV").up == (0.0, -1.0, 0.0) and E.Omni3Deval(mode="3D").up == (0.0, -1.0, 0.0)
    with pytest.raises(ValueError):
        E.Omni3Deval(mode="DIST", up=(0.0, 0.0, 0.0))


def test_dist_mode_emulated(emu_lib, capsys):
    _run_dist_mode(capsys)


@pytest.mark.gpu
def test_dist_mode_gpu(hip_lib, capsys):
    _run_dist_mode(capsys)


def _run_prox():
    """eval_prox: no match outside proximity (2D IoU > 0.3), and fewer matches than without it"""
    gts, dts = _split(SEED)
    ev, _ = _evaluate(gts, dts, eval_prox=True)
    plain, _ = _evaluate(gts, dts)
    dtm = ev._dev["match"]["dt_match"].cpu().numpy()
    doff, n = np.concatenate([[0], np.cumsum(ev._dev["dt_sizes"])]), 0
    for gi, (_, _, g, d) in enumerate(ev._dev["groups"]):
        for i, det in enumerate(d):
            for m in set(dtm[:, :, doff[gi] + i].reshape(-1).tolist()) - {-1}:
                (x1, y1, w1, h1), (x2, y2, w2, h2) = det["bbox"], g[m]["bbox"]
                iw, ih = max(min(x1 + w1, x2 + w2) - max(x1, x2), 0.0), max(min(y1 + h1, y2 + h2) - max(y1, y2), 0.0)
                assert iw * ih / (w1 * h1 + w2 * h2 - iw * ih) > 0.3
                n += 1
    assert 20 < n and (dtm >= 0).sum() < (plain._dev["match"]["dt_match"].cpu().numpy() >= 0).sum()


def test_eval_prox_emulated(emu_lib):
    _run_prox()


@pytest.mark.gpu
def test_eval_prox_gpu(hip_lib):
    _run_prox()


# ---- a split small enough to score by hand --------------------------------------------------------------------------------------
SHIFT = (0.1, 0.2, 0.3, 0.4, 0.6, 0.8, 1.2, 1.6, 3.0)       # detection j = ground truth j moved by SHIFT[j] along z
SCALE = (1.0, 1.1, 0.9, 1.2, 1.0, 0.8, 1.25, 1.0, 1.0)      # ... every dimension times SCALE[j]
TURN = (0.0, 0.1, 0.2, 0.05, 0.3, 0.0, 0.15, 0.25, 0.0)     # ... turned by TURN[j] radians about y
# float32 corners: a coordinate of magnitude <= 26 is off by <= 2^-24 x 26 = 1.6e-6, a distance of centres by 2 x that; an axis by
# 2 sqrt(3) x 1.6e-6 / the smallest dimension 1.2, the angle of two boxes after Gram-Schmidt by 4 x that = 1.8e-5
HAND_TOL = 2e-5


def _hand_split():
    dims = np.array([2.0, 1.5, 4.0])
    gts, dts = [], []
    for i in range(10):
        gts.append(_rec(1, 1, boxgen.corners(np.array([[5.0 * (i - 4.5), 0.0, 20.0]]), dims[None], np.eye(3)[None])[0]))
    scores = (0.95, 0.90, 0.85, 0.75, 0.70, 0.65, 0.60, 0.55, 0.50)
    for j in range(9):
        c = np.array([[5.0 * (j - 4.5), 0.0, 20.0 + SHIFT[j]]])
        dts.append(_rec(1, 1, boxgen.corners(c, SCALE[j] * dims[None], _ry(TURN[j])[None])[0], score=scores[j]))
    for x, s in ((0.0, 0.80), (2.5, 0.10)):                  # two false positives 30 m further out: fourth and last by score
        dts.append(_rec(1, 1, boxgen.corners(np.array([[x, 0.0, 50.0]]), dims[None], np.eye(3)[None])[0], score=s))
    for k, r in enumerate(gts + dts):
        r["id"] = k + 1
    return gts, dts


def _run_hand_split():
    gts, dts = _hand_split()
    ev, _ = _evaluate(gts, dts, imgs=[1], cats=[1])
    # by score: T T T F T T T T T T F with T = the nine copies; a copy is a true positive at threshold d when SHIFT[j] <= d.
    # npig = 10, so recall after the c-th true positive is c / 10 and the c-th takes the thresholds in ((c-1)/10, c/10]: ten of the
    # 101 each, except the first, which also takes r = 0 (eleven).
    # d = 0.5: copies 0..3.  T T T F T, then misses.  precision 1, 1, 1, 4/5 -> envelope 1, 1, 1, 0.8; recall 0.4
    ap05 = (31 * 1.0 + 10 * 0.8) / 101
    # d = 1.0: copies 0..5.  T T T F T T T.  precision 1, 1, 1, 4/5, 5/6, 6/7 -> envelope 1, 1, 1, 6/7, 6/7, 6/7; recall 0.6
    ap10 = (31 * 1.0 + 30 * (6 / 7)) / 101
    # d = 2.0: copies 0..7.  precision ..., 7/8, 8/9 -> envelope 1, 1, 1, then 8/9 five times; recall 0.8
    ap20 = (31 * 1.0 + 50 * (8 / 9)) / 101
    # d = 4.0: all nine.  ..., 9/10 -> envelope 1, 1, 1, then 9/10 six times; recall 0.9
    ap40 = (31 * 1.0 + 60 * 0.9) / 101
    want = np.array([ap05, ap10, ap20, ap40])
    got = np.array([np.mean(ev.eval["precision"][t, :, 0, 0, -1]) for t in range(4)])
    assert np.abs(got - want).max() <= 1e-12, (got, want)
    assert abs(ev.stats[0] - want.mean()) <= 1e-12 and np.abs(ev.stats[1:4] - want[:3]).max() <= 1e-12
    assert np.array_equal(ev.eval["recall"][:, 0, 0, -1], [0.4, 0.6, 0.8, 0.9])
    assert ev.stats[4] == -1 and ev.stats[6] == -1                                                # every ground truth is at medium depth
    # TP metrics at d = 2.0: eight true positives; m_c = the mean of the first c errors; the thresholds >= 0.1 in ((c-1)/10, c/10]
    # are r = 0.10 alone for c = 1 and ten for each c = 2..6; np.linspace gives r_70 = 0.7000000000000001 > 7/10, so -- the same doubles
    # as the precision table's searchsorted -- c = 7 takes nine (0.61 .. 0.69) and c = 8 eleven (r_70 .. 0.80): 71 values
    trans = np.array(SHIFT[:8])
    scale = np.array([1.0 - min(f, 1 / f) ** 3 for f in SCALE[:8]])
    orient = np.array(TURN[:8])
    weight = np.array([1, 10, 10, 10, 10, 10, 9, 11])
    for j, e in enumerate((trans, scale, orient)):
        m = np.cumsum(e) / np.arange(1, 9)
        want_j = float((weight * m).sum() / 71)
        assert abs(ev.eval["tp_errors"][0, 0, j] - want_j) <= HAND_TOL, (j, ev.eval["tp_errors"][0, 0], want_j)
        assert abs(ev.tp_stats[j] - want_j) <= HAND_TOL
        assert abs(ev.eval["tp_errors"][0, 2, j] - want_j) <= HAND_TOL                               # range "medium" holds the same boxes
    # ATE written out: m = 0.1, 0.15, 0.2, 0.25, 0.32, 0.4, 3.6/7, 0.65 -> (0.1 + 10 x 1.32 + 9 x 3.6/7 + 11 x 0.65) / 71 = 0.353219...
    assert abs(ev.tp_stats[0] - 0.3532193) <= HAND_TOL
    assert ev.eval["tp_count"].tolist() == [[8, 0, 8, 0]] and (ev.eval["tp_errors"][0, 1] == -1).all() and (ev.eval["tp_errors"][0, 3] == -1).all()
    # the reference pipeline agrees with the hand computation too
    ref = X.evaluate(gts, dts, [1], [1], DIST_THRS)
    assert np.array_equal(ref["precision"], ev.eval["precision"]) and np.abs(ref["tp_errors"] - ev.eval["tp_errors"]).max() <= TP_TOL
    # ground truth but no true positive: the rule of nuScenes, 1.0
    ev2, _ = _evaluate(gts, dts[9:], imgs=[1], cats=[1])
    assert (ev2.eval["tp_errors"][0, 0] == 1.0).all() and ev2.eval["tp_count"][0, 0] == 0


def test_hand_computable_split_emulated(emu_lib):
    _run_hand_split()


@pytest.mark.gpu
def test_hand_computable_split_gpu(hip_lib):
    _run_hand_split()


def _run_groups(dev):
    """dist_errors_groups: the layout of box3d_overlap_groups with a last axis of 3, empty groups, an up vector, errors"""
    from omni3d_amd.cubercnn.evaluation import omni3d_evaluation as E
    rng = np.random.default_rng(3)
    dt, gt, _ = boxgen.omni3d_like_pairs(rng, 12, degenerate_frac=0.0)
    dts, gts = [3, 0, 5, 4, 0], [2, 4, 0, 6, 0]
    tdt, tgt = torch.from_numpy(dt).to(dev), torch.from_numpy(gt).to(dev)
    up = (0.2, -0.9, 0.1)
    flat, views = E.dist_errors_groups(tdt, tgt, dts, gts, up=up)
    assert flat.shape == (3 * 2 + 4 * 6, 3) and flat.dtype == torch.float64
    assert [tuple(m.shape) for m in views] == [(3, 2, 3), (0, 4, 3), (5, 0, 3), (4, 6, 3), (0, 0, 3)]
    assert views[0].untyped_storage().data_ptr() == flat.untyped_storage().data_ptr()                     # views of the flat tensor
    od, og = np.concatenate([[0], np.cumsum(dts)]), np.concatenate([[0], np.cumsum(gts)])
    for n, m in enumerate(views):
        i1, i2 = np.repeat(np.arange(dts[n]), gts[n]), np.tile(np.arange(gts[n]), dts[n])
        want = X.pair_errors(dt[od[n]:od[n + 1]], gt[og[n]:og[n + 1]], i1, i2, up).reshape(dts[n], gts[n], 3)
        assert m.numel() == 0 or float(np.abs(m.cpu().numpy() - want).max()) <= 1e-9
    assert E.dist_errors_groups(tdt[:0], tgt[:0], [], [])[1] == []
    assert [tuple(m.shape) for m in E.dist_errors_groups(tdt[:2], tgt[:0], [2], [0])[1]] == [(2, 0, 3)]
    for bad in (([3, 9], [2, 10, 0]), ([3, 8], [2, 10])):
        with pytest.raises(ValueError):
            E.dist_errors_groups(tdt, tgt, *bad)
    with pytest.raises(ValueError):
        E.dist_errors_groups(tdt, tgt, dts, gts, up=(0.0, 1.0))


def test_errors_groups_emulated(emu_lib):
    _run_groups("cpu")


@pytest.mark.gpu
def test_errors_groups_gpu(hip_lib):
    _run_groups("cuda")


def _run_short_form():
    """categories 1..3 only: the crowded category adds nothing here and its IoU3D pass is slow under the host emulator"""
    from omni3d_amd.cubercnn.evaluation import Omni3DEvaluator
    gts, dts = _split(SEED)
    cats = CATS[:3]
    by_img = {i: [d for d in dts if d["image_id"] == i] for i in IMGS}
    out = []
    for kw in ({}, {"eval_dist": False}, {"eval_dist": True}):
        ev = Omni3DEvaluator(copy.deepcopy(list(gts)), IMGS, cats, False, **kw)
        ev.process([{"image_id": i} for i in IMGS], [{"instances": copy.deepcopy(by_img[i])} for i in IMGS])
        out.append(ev.evaluate()["bbox"])
    none, off, on = out
    assert set(none) == set(off) == {"AP2D", "AP3D", "omni_eval_2D", "omni_eval_3D"}                      # today's keys, exactly
    for k in ("2D", "3D"):
        assert none["AP" + k] == off["AP" + k] == on["AP" + k] and np.array_equal(none["omni_eval_" + k].stats, off["omni_eval_" + k].stats)
        assert np.array_equal(none["omni_eval_" + k].eval["precision"], off["omni_eval_" + k].eval["precision"])
        assert np.array_equal(none["omni_eval_" + k].eval["precision"], on["omni_eval_" + k].eval["precision"])
    assert set(on) == set(off) | {"APDIST", "omni_eval_DIST"}
    ref = _reference(SEED, None, tuple(cats))
    assert on["APDIST"] == float(ref["stats"][0] * 100) and np.abs(on["omni_eval_DIST"].tp_stats - ref["tp_stats"]).max() <= TP_TOL
    assert on["omni_eval_DIST"].up is None and on["omni_eval_3D"].up == (0.0, -1.0, 0.0)
    ev = Omni3DEvaluator(copy.deepcopy(list(gts)), IMGS, cats, False, eval_dist=True, dist_up=(0.0, -2.0, 0.0), dist_params={"tpDist": 1.0})
    made = ev._make_eval(None, None, "DIST")
    assert made.up == (0.0, -1.0, 0.0) and made.params.tpDist == 1.0 and ev._make_eval(None, None, "BEV").up == (0.0, -1.0, 0.0)      # normalised
    ev = Omni3DEvaluator(copy.deepcopy(list(gts)), IMGS, cats, True, eval_dist=True)                      # only_2d wins
    ev.process([{"image_id": i} for i in IMGS], [{"instances": copy.deepcopy(by_img[i])} for i in IMGS])
    assert set(ev.evaluate()["bbox"]) == {"AP2D", "omni_eval_2D"}
    with pytest.raises(ValueError):
        Omni3DEvaluator(copy.deepcopy(list(gts)), IMGS, cats, False, eval_dist=True, dist_params={"tpDist": 3.0})
    with pytest.raises(ValueError):
        Omni3DEvaluator(copy.deepcopy(list(gts)), IMGS, cats, False, eval_dist=True, dist_up=(1.0, 0.0))


def test_evaluator_short_form_emulated(emu_lib):
    _run_short_form()


@pytest.mark.gpu
def test_evaluator_short_form_gpu(hip_lib):
    _run_short_form()


KITTI, IDS = ["pedestrian", "car", "cyclist", "van", "truck"], [31, 3, 20, 12, 7]
SPLITS = ("KITTI_val", "KITTI_test")           # names of a known family: the helper looks up the family's category list


def _run_helper(tmp_path, monkeypatch):
    """two tiny registered splits, the ground truth (moved a little, scaled and turned) fed back as predictions"""
    from omni3d_amd import synthetic
    from omni3d_amd.cubercnn import data
    from omni3d_amd.cubercnn.config import add_dist_eval_config, dist_eval_args, get_cfg_defaults
    from omni3d_amd.cubercnn.evaluation import Omni3DEvaluationHelper
    from omni3d_amd.d2.config import get_cfg
    from omni3d_amd.d2.data import DatasetCatalog, MetadataCatalog
    monkeypatch.chdir(tmp_path)
    saved_model = MetadataCatalog.pop("omni3d_model", None)           # another test's model table: put back at the end
    root = str(tmp_path)
    try:
        synthetic.write_omni3d_stats(root, KITTI, IDS)
        files = [synthetic.write_omni3d_dataset(root, n, KITTI, IDS, num_images=3, height=96, width=128, num_gt=4, seed=7 + k, dataset_id=k,
                                                image_id_base=1000 * (k + 1)) for k, n in enumerate(SPLITS)]
        cfg = get_cfg()
        get_cfg_defaults(cfg)
        cfg.merge_from_file(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "cubercnn_DLA34_FPN.yaml"))
        cfg.merge_from_list(["DATASETS.CATEGORY_NAMES", tuple(KITTI), "MODEL.ROI_HEADS.NUM_CLASSES", len(KITTI)])
        fs = data.get_filter_settings_from_cfg(cfg)
        data.register_and_store_model_metadata(data.Omni3D(files, filter_settings=fs), root, fs)
        fs_test = data.get_filter_settings_from_cfg(cfg)
        fs_test.update(visibility_thres=cfg.TEST.VISIBILITY_THRES, truncation_thres=cfg.TEST.TRUNCATION_THRES, min_height_thres=0.0625, max_depth=1e8)
        id_map = MetadataCatalog.get("omni3d_model").thing_dataset_id_to_contiguous_id
        add_dist_eval_config(cfg)
        cfg.merge_from_list(["TEST.EVAL_DIST.ENABLED", True, "TEST.EVAL_DIST.UP", [0.0, -1.0, 0.0]])
        got = {}
        for tag, kw in (("none", {}), ("off", {"eval_dist": False}), ("on", dist_eval_args(cfg))):
            helper = Omni3DEvaluationHelper(list(SPLITS), fs_test, os.path.join(root, "inference_" + tag), iter_label="3", **kw)
            for name, path in zip(SPLITS, files):
                gt = data.Omni3D([path], filter_settings=copy.deepcopy(fs_test))
                preds = []
                for img_id, im in sorted(gt.imgs.items()):
                    recs = []
                    for k, a in enumerate(gt.imgToAnns[img_id]):
                        if a["ignore"]:
                            continue
                        b3 = np.array(a["bbox3D"], np.float64)
                        c = b3.mean(axis=0)
                        b3 = (b3 - c) * (1.0 + 0.1 * (k % 3)) @ _ry(0.1 * k).T + c + np.array([0.25 * (k % 3), 0.0, 0.1 * k])
                        recs.append({"image_id": img_id, "category_id": id_map[a["category_id"]], "bbox": list(a["bbox"]), "score": 0.9 - 0.01 * k,
                                     "depth": a["depth"], "bbox3D": b3.tolist()})
                    preds.append({"image_id": img_id, "K": im["K"], "width": im["width"], "height": im["height"], "instances": recs})
                helper.add_predictions(name, preds)
            ret = helper.summarize_all()
            got[tag] = (copy.deepcopy(ret), helper)
        (ana0, omni0), h0 = got["none"]
        (ana1, omni1), h1 = got["off"]
        (ana2, omni2), h2 = got["on"]
        assert h0.results_dist == {} and h1.results_dist == {} and h1.eval_dist is False and h2.eval_dist is True
        assert repr(ana0) == repr(ana1) == repr(ana2) and repr(omni0) == repr(omni1) == repr(omni2)      # NaNs compare by their text
        for name in SPLITS:                                                                              # off = the argument omitted, key for key
            r0, r1 = h0.results[name], h1.results[name]
            assert list(r0) == list(r1) and all(repr(r0[k]) == repr(r1[k]) for k in r0 if not k.endswith("_merge"))
        assert list(h2.results_dist) == list(SPLITS) + ["<Concat>"]
        cols = ["iters", "APDIST", "APDIST@0.5m", "APDIST@1m", "APDIST@2m", "APDIST-N", "APDIST-M", "APDIST-F", "mATE", "mASE", "mAOE"]
        for name, row in h2.results_dist.items():
            assert list(row) == cols and row["iters"] == "3"
            assert 0.0 < row["APDIST"] <= 100.0 and 0.0 < row["mATE"] < 2.0 and 0.0 < row["mASE"] < 1.0 and 0.0 < row["mAOE"] < math.pi, row
        assert set(h2.results[SPLITS[0]]) - set(h0.results[SPLITS[0]]) == {"bbox_DIST", "log_str_DIST", "bbox_DIST_merge"}
        rd = h2.results[SPLITS[0]]["bbox_DIST"]
        assert {"AP", "AP@0.5m", "AP@1m", "AP@2m", "APn", "APm", "APf", "mATE", "mASE", "mAOE"} <= set(rd)
        assert any(k.startswith("AP-") for k in rd) and all(("ATE-" + k[3:]) in rd and ("ASE-" + k[3:]) in rd and ("AOE-" + k[3:]) in rd
                                                            for k in rd if k.startswith("AP-"))
        assert "mode=DIST" in h2.results[SPLITS[0]]["log_str_DIST"]
        only2d = Omni3DEvaluationHelper(list(SPLITS), fs_test, os.path.join(root, "inference_2d"), only_2d=True, eval_dist=True)
        assert only2d.eval_dist is False
    finally:
        for n in SPLITS:
            if n in DatasetCatalog:
                DatasetCatalog.remove(n)
            MetadataCatalog.pop(n, None)
        MetadataCatalog.pop("omni3d_model", None)
        if saved_model is not None:
            MetadataCatalog["omni3d_model"] = saved_model


def test_helper_fills_results_dist_emulated(emu_lib, tmp_path, monkeypatch):
    _run_helper(tmp_path, monkeypatch)


@pytest.mark.gpu
def test_helper_fills_results_dist_gpu(hip_lib, tmp_path, monkeypatch):
    _run_helper(tmp_path, monkeypatch)


def test_config_node_and_helper():
    from omni3d_amd.cubercnn.config import add_dist_eval_config, dist_eval_args, get_cfg_defaults
    from omni3d_amd.d2.config import get_cfg
    cfg = get_cfg_defaults(get_cfg())
    assert "EVAL_DIST" not in cfg.TEST
    defaults = {"eval_dist": False, "dist_up": None, "dist_params": {"distThrs": [0.5, 1.0, 2.0, 4.0], "tpDist": 2.0, "minRecall": 0.1}}
    assert dist_eval_args(cfg) == defaults
    assert add_dist_eval_config(cfg) is cfg
    assert dict(cfg.TEST.EVAL_DIST) == {"ENABLED": False, "UP": [], "DIST_THRS": [0.5, 1.0, 2.0, 4.0], "TP_DIST": 2.0, "MIN_RECALL": 0.1}
    assert dist_eval_args(cfg) == defaults
    cfg.merge_from_list(["TEST.EVAL_DIST.ENABLED", True, "TEST.EVAL_DIST.UP", [0.0, -0.8, 0.6], "TEST.EVAL_DIST.DIST_THRS", [1.0, 3.0],
                         "TEST.EVAL_DIST.TP_DIST", 3.0, "TEST.EVAL_DIST.MIN_RECALL", 0.2])
    add_dist_eval_config(cfg)                                                # idempotent: the values that were set stay
    assert dict(cfg.TEST.EVAL_DIST) == {"ENABLED": True, "UP": [0.0, -0.8, 0.6], "DIST_THRS": [1.0, 3.0], "TP_DIST": 3.0, "MIN_RECALL": 0.2}
    assert dist_eval_args(cfg) == {"eval_dist": True, "dist_up": (0.0, -0.8, 0.6), "dist_params": {"distThrs": [1.0, 3.0], "tpDist": 3.0, "minRecall": 0.2}}
    assert "EVAL_DIST" not in get_cfg_defaults(get_cfg()).TEST                                           # the defaults stay the reference's
    other = add_dist_eval_config(get_cfg_defaults(get_cfg()))
    other.TEST.EVAL_DIST.UP.append(1.0)
    assert add_dist_eval_config(get_cfg_defaults(get_cfg())).TEST.EVAL_DIST.UP == []                     # the default list is not shared
    with pytest.raises(ValueError):
        dist_eval_args(other)                                                                            # one number: neither none nor three
    other = add_dist_eval_config(get_cfg_defaults(get_cfg()))
    other.TEST.EVAL_DIST.TP_DIST = 3.0
    with pytest.raises(ValueError):
        dist_eval_args(other)                                                                            # not one of DIST_THRS
