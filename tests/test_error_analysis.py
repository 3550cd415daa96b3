"""`Omni3Deval.errors` / `summarize_errors`, the `errors` switch of `Omni3DEvaluator` / `Omni3DEvaluationHelper`,
`config.add_error_analysis_config` and tools/error_report.py: the error decomposition after TIDE in modes 2D, 3D, BEV and LET.

The reference has nothing of the kind, so the yardstick is tests/exact_errors.py: the whole analysis (similarity by Qhull / footprint
clipping / the LET alignment, greedy matching, classification, contests, oracles, accumulation) written from the definitions in float64
with Python loops.  Everything integer -- type, attributed ground truth, missed ground truths, counts, dropped -- must be EQUAL to it,
`ap`, `ap_fixed` and `dap` within 1e-12, `loc_errors` within PAIR_TOL = 1e-9 (the bound of tests/test_tp_errors.py for `pair_errors`).
Equality can only be asked where the 1e-5 of a float32 similarity decides nothing, so, in float64 and in all four modes: no similarity
lies within 1e-4 of t_fg or t_bg, no similarity of a same-category pair within 1e-4 of any matching threshold of the mode, for no false
positive do the top two of a candidate set with a maximum >= t_bg differ by less than 1e-4, no two scores tie; and in mode 3D every
type occurs at least twice, a ground truth is contested by two Loc detections, and both Cls outcomes (ground truth free / matched) occur.
The split is generated from the first seed from 1 on that meets this, which `test_reference_alone_meets_the_conditions` asserts on the
CPU with no kernel involved.  No detection is left out of the comparison.

Largest |evaluator - float64| (ap_fixed | loc_errors), printed by every run under `-s`:
    host emulator   1.0e-15 | 2.8e-17
    MI355X          1.0e-15 | 2.8e-17
"""
import copy
import functools
import importlib.util
import json
import math
import os

import numpy as np
import pytest

import exact_errors as X
from omni3d_amd import boxgen
from test_let_eval import _nearest_rotation, _rec

N_IMG, N_CAT = 6, 3
MARGIN = 1e-4
SEED = 3                            # the first seed from 1 on that meets the conditions (asserted below)
PAIR_TOL = 1e-9
IMGS, CATS = list(range(1, N_IMG + 1)), list(range(1, N_CAT + 1))
MODES = ("3D", "2D", "BEV", "LET")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _split(seed):
    """(ground truths, detections): 6 images x 3 categories with up to 4 ground truths and 11 detections per group, groups without
    ground truth and with `ignore3D`.  Per ground truth, at random: a good copy (lateral jitter N(0, 0.08) x dimensions, dimensions x
    U[0.9, 1.1], rotation blended 10 % towards a random one), a second good copy with a lower score (a duplicate), one or two copies moved
    along the line of sight by U[0.45, 0.8] x the smallest dimension (a poor box), a good copy filed under another category; and per
    group up to three boxes far away."""
    rng = np.random.default_rng(seed)
    gts, dts = [], []

    def box(c, d, R):
        return boxgen.corners(np.asarray(c)[None], np.asarray(d)[None], R[None])[0]

    def copy_of(img, cat, c, d, R, score, slide=0.0):
        c2 = c + R @ (rng.normal(0, 0.08, 3) * d) + slide * c / np.linalg.norm(c)
        R2 = _nearest_rotation(0.9 * R + 0.1 * boxgen.rand_rot(rng, 1)[0])
        dts.append(_rec(img, cat, box(c2, d * rng.uniform(0.9, 1.1, 3), R2), score=score))

    for img in IMGS:
        for cat in CATS:
            n_gt = int(rng.integers(1, 5)) if (img + cat) % 5 else 0
            for _ in range(n_gt):
                c = np.array([rng.uniform(-5, 5), rng.uniform(-2, 2), rng.uniform(3, 60)])
                d, R = rng.uniform(0.6, 4.0, 3), boxgen.rand_rot(rng, 1)[0]
                gts.append(_rec(img, cat, box(c, d, R), ignore=int(rng.uniform() < 0.12)))
                good = rng.uniform() < 0.55
                if good:
                    copy_of(img, cat, c, d, R, rng.uniform(0.5, 0.99))
                    if rng.uniform() < 0.35:
                        copy_of(img, cat, c, d, R, rng.uniform(0.05, 0.5))
                for _ in range(int(rng.integers(0, 3)) if rng.uniform() < 0.6 else 0):
                    copy_of(img, cat, c, d, R, rng.uniform(0.05, 0.9), slide=rng.choice([-1, 1]) * rng.uniform(0.45, 0.8) * d.min())
                if rng.uniform() < 0.3:
                    copy_of(img, CATS[(cat + int(rng.integers(0, 2))) % N_CAT], c, d, R, rng.uniform(0.05, 0.9))
            for _ in range(int(rng.integers(0, 3))):
                c = np.array([rng.uniform(-5, 5), rng.uniform(-2, 2), rng.uniform(3, 60)])
                dts.append(_rec(img, cat, box(c, rng.uniform(0.6, 4.0, 3), boxgen.rand_rot(rng, 1)[0]), score=rng.uniform(0.05, 0.6)))
    for k, r in enumerate(gts + dts):
        r["id"] = k + 1
    return gts, dts


@functools.lru_cache(maxsize=None)
def _reference(seed, mode):
    gts, dts = _split(seed)
    return X.analyse(gts, dts, IMGS, CATS, mode)


def _margins(ref):
    """float64 alone -> (smallest distance of a similarity to t_fg / t_bg (same-category pairs: to any matching threshold), smallest
    gap between the top two of a candidate set with a maximum >= t_bg of a false positive)"""
    to_thr, gap = math.inf, math.inf
    for im in ref["images"]:
        sim = im["sim"]
        for d in range(sim.shape[0]):
            for g in range(sim.shape[1]):
                thrs = [ref["t_fg"], ref["t_bg"]] + (list(ref["thrs"]) if im["dt_cat"][d] == im["gt_cat"][g] else [])
                to_thr = min([to_thr] + [abs(sim[d, g] - t) for t in thrs if sim[d, g] > 0])
            if im["type"][d] in (X.TP, X.IGN):
                continue
            cand = ~np.asarray(im["gt_ignore"], bool)
            same, used = np.asarray(im["gt_cat"]) == im["dt_cat"][d], np.asarray(im["gt_matched"], bool)
            for members in (cand & same & ~used, cand & same & used, cand & ~same):
                v = np.sort(sim[d, members])[::-1]
                if len(v) >= 2 and v[0] >= ref["t_bg"]:
                    gap = min(gap, v[0] - v[1])
    return to_thr, gap


@functools.lru_cache(maxsize=None)
def _good(seed):
    gts, dts = _split(seed)
    scores = [x["score"] for x in dts]
    sizes = {}
    for x in dts:
        sizes[x["image_id"], x["category_id"]] = sizes.get((x["image_id"], x["category_id"]), 0) + 1
    if len(set(scores)) != len(scores) or max(sizes.values()) > 11:
        return False
    for mode in MODES:                                      # 3D first: it asks the most
        ref = _reference(seed, mode)
        to_thr, gap = _margins(ref)
        if to_thr < MARGIN or gap < MARGIN:
            return False
        if mode == "3D":
            typ = ref["type"]
            loc_on = ref["attr_row"][typ == X.LOC]
            cls_gt = ref["gt_matched"][ref["attr_row"][typ == X.CLS]]
            if min((typ == c).sum() for c in range(7)) < 2 or len(ref["missed_gt_ids"]) < 2 or len(loc_on) == len(set(loc_on.tolist())) \
                    or not (cls_gt.any() and (~cls_gt).any() and ref["win_cls"].any()):
                return False
    return True


def test_reference_alone_meets_the_conditions():
    assert next(s for s in range(1, 40) if _good(s)) == SEED
    ref = _reference(SEED, "3D")
    assert (ref["dap"][np.isfinite(ref["dap"])] >= -1e-15).all() and ref["counts"].sum() > 30
    assert np.isfinite(ref["loc_errors"]).any() and all(math.isfinite(e[0]) for _, _, e in ref["loc_pairs"])


def _evaluate(gts, dts, imgs=IMGS, cats=CATS, mode="3D", **kw):
    from omni3d_amd.cubercnn.evaluation import omni3d_evaluation as E
    ev = E.Omni3Deval(E.AnnotationIndex(copy.deepcopy(list(gts)), imgs, cats), E.AnnotationIndex(copy.deepcopy(list(dts)), imgs, cats), mode=mode, **kw)
    ev.evaluate()
    return ev


def _run_generated():
    gts, dts = _split(SEED)
    worst = [0.0, 0.0]
    for mode in MODES:
        ev = _evaluate(gts, dts, mode=mode)
        res, ref = ev.errors(), _reference(SEED, mode)
        assert res["t_fg"] == ref["t_fg"] and res["t_bg"] == ref["t_bg"] and res["area"] == "all"
        assert np.array_equal(res["dt_ids"], ref["dt_ids"])                                              # every detection, in order
        assert res["type"].dtype == np.int8 and np.array_equal(res["type"], ref["type"]), mode
        assert np.array_equal(res["attributed_gt"], ref["attributed_gt"]), mode
        assert sorted(res["missed_gt_ids"].tolist()) == sorted(ref["missed_gt_ids"].tolist()), mode
        assert np.array_equal(res["counts"], ref["counts"]) and np.array_equal(res["dropped"], ref["dropped"]), mode
        assert np.array_equal(res["counts_total"], ref["counts"].sum(axis=0))
        assert np.abs(res["ap"] - ref["ap"]).max() <= 1e-12 and np.abs(res["ap_fixed"] - ref["ap_fixed"]).max() <= 1e-12, mode
        assert np.array_equal(np.isnan(res["dap"]), np.isnan(ref["dap"])) and np.nanmax(np.abs(res["dap"] - ref["dap"])) <= 1e-12, mode
        assert np.allclose(res["dap_mean"], ref["dap_mean"], rtol=0, atol=1e-12, equal_nan=True)
        worst[0] = max(worst[0], float(np.abs(res["ap_fixed"] - ref["ap_fixed"]).max()))
        for key in ("s_free", "s_used", "s_other"):
            assert res[key].dtype == np.float32 and res[key].shape == res["type"].shape
        if mode == "2D":
            assert res["loc_errors"] is None and ref["loc_errors"] is None
        else:
            assert np.array_equal(np.isnan(res["loc_errors"]), np.isnan(ref["loc_errors"])) and res["loc_skipped"] == 0
            diff = np.abs(res["loc_errors"] - ref["loc_errors"])                                         # NaN where a category has no Loc pair
            err = float(diff[np.isfinite(diff)].max(initial=0.0))
            worst[1] = max(worst[1], err)
            assert err <= PAIR_TOL, (mode, err)
        # ---- invariants ----
        sumD = len(res["type"])
        assert sumD == len(ref["type"]) and set(res["type"].tolist()) <= set(range(7))                   # exactly one code each
        n_tp, n_ign = int((res["type"] == X.TP).sum()), int((res["type"] == X.IGN).sum())
        assert n_tp + n_ign + int(res["counts"][:, :5].sum()) == sumD
        assert (res["dap"][np.isfinite(res["dap"])] >= -1e-15).all()                                    # an oracle never costs AP
        R = len(ev.params.recThrs)
        for k in range(N_CAT):
            if res["ap"][k] > -1:
                # FP: precision 1 at every recall threshold <= TP / npig.  Exactly, but for one case: a category with a single true
                # positive has precision 1 / (1 + spacing(1)), one step below 1 (with two or more, 2 + spacing(1) rounds to 2)
                n_thr = int((np.asarray(ev.params.recThrs) <= ref["tp"][k] / ref["npig"][k]).sum()) if ref["tp"][k] else 0
                assert res["ap_fixed"][6, k] == n_thr / R or (ref["tp"][k] == 1 and abs(res["ap_fixed"][6, k] - n_thr / R) <= 3e-16)
                if res["ap_fixed"][7, k] > -1:                                                         # FN: recall 1, so every threshold has a value
                    assert res["ap_fixed"][7, k] >= res["ap"][k] and res["ap_fixed"][7, k] > 0
        ev.accumulate()
        t = int(np.flatnonzero(np.isclose(res["t_fg"], ev.params.iouThrs))[0])
        base = np.ascontiguousarray(ev.eval["precision"][t, :, :, 0, -1])                                # (R, K): numpy adds the rows in order
        assert np.array_equal(res["ap"], np.where((base > -1).all(axis=0), base.mean(axis=0), -1.0))
        text = ev.summarize_errors().split("\n")
        assert len(text) == (8 if mode == "2D" else 9) and all(ln.startswith("mode=%s " % mode) for ln in text)
        assert [ln.split()[2] for ln in text[:8]] == list(res["names"]) == ["Cls", "Loc", "Both", "Dupe", "Bkg", "Miss", "FP", "FN"]
        assert text[1].endswith("= %0.3f" % (100 * res["dap_mean"][1])) and ("n=%6d" % res["counts_total"][1]) in text[1]
    print("|evaluator - fp64| ap_fixed %.2e loc_errors %.2e" % tuple(worst))
    # other thresholds and another range, through the arguments
    ev = _evaluate(gts, dts, mode="3D")
    res = ev.errors(t_fg=0.5, t_bg=0.1, area="near")
    assert res["t_fg"] == 0.5 and res["area"] == "near" and not np.array_equal(res["type"], _reference(SEED, "3D")["type"])


def test_generated_split_emulated(emu_lib):
    _run_generated()


@pytest.mark.gpu
def test_generated_split_gpu(hip_lib):
    _run_generated()


def _hand_split():
    """one image, categories 1 and 2, unit cubes 30 m away.  Category 1: ground truths A, B, E; category 2: ground truth C.  Detections of
    category 1 by score: a box far from everything (0.95), A itself (0.90), B moved by (0.05, 0.05, 0.6) (0.80), C itself (0.70), A moved
    by (0.1, 0.1, 0.1) (0.60)."""
    cube = lambda c: boxgen.corners(np.array([c], np.float64), np.ones((1, 3)), np.eye(3)[None])[0]      # noqa: E731
    A, B, E, C = (-6.0, 0.0, 30.0), (-2.0, 0.0, 30.0), (2.0, 0.0, 30.0), (6.0, 0.0, 30.0)
    gts = [_rec(1, 1, cube(A)), _rec(1, 1, cube(B)), _rec(1, 1, cube(E)), _rec(1, 2, cube(C))]
    dts = [_rec(1, 1, cube((0.0, 1.5, 20.0)), score=0.95), _rec(1, 1, cube(A), score=0.90), _rec(1, 1, cube((-1.95, 0.05, 30.6)), score=0.80),
           _rec(1, 1, cube(C), score=0.70), _rec(1, 1, cube((-5.9, 0.1, 30.1)), score=0.60)]
    for k, r in enumerate(gts + dts):
        r["id"] = k + 1
    return gts, dts


def _run_hand_split():
    """IoU3D of a unit cube with itself moved by (a, b, c) is v / (2 - v), v = (1-a)(1-b)(1-c): 0.22 for B's detection (>= t_bg 0.05, <
    t_fg 0.25: Loc on B), 0.57 for A's second detection (>= t_fg on the matched A: Dupe); C's copy overlaps no ground truth of its own
    category and C by 1 (Cls, C is free); the far box overlaps nothing (Bkg); E is touched by nobody (Miss).
    Category 1 (npig 3), by score F T F F F: one true positive at precision 1/2, recall 1/3, which serves the 34 recall thresholds 0 ..
    0.33 of the 101: ap = 17/101.  Category 2 (npig 1, no detection): ap = 0.
      Cls: C's copy moves to category 2 as its true positive: ap_2 = 1, category 1 keeps 17/101 (the removed box was below the true
           positive): dap = (0, 1).
      Loc: F T T F F: precision 1/2, 2/3, envelope 2/3, recall 2/3 serves 67 thresholds: ap_1 = (67 x 2/3)/101: dap_1 = (134/3 - 17)/101.
      Both: none.  Dupe: removing a box below the last true positive changes nothing: 0.
      Bkg: T first: precision 1: ap_1 = 34/101: dap_1 = 17/101.       FP: the same.
      Miss: npig 2: recall 1/2 serves 51 thresholds at 1/2: dap_1 = (25.5 - 17)/101.
      FN: npig_1 = 1: recall 1 at precision 1/2: ap_1 = 1/2; category 2 has no matched candidate and drops out."""
    gts, dts = _hand_split()
    ev = _evaluate(gts, dts, imgs=[1], cats=[1, 2], mode="3D")
    res = ev.errors()
    assert res["type"].tolist() == [X.BKG, X.TP, X.LOC, X.CLS, X.DUPE]
    assert res["attributed_gt"].tolist() == [-1, -1, gts[1]["id"], gts[3]["id"], gts[0]["id"]] and res["missed_gt_ids"].tolist() == [gts[2]["id"]]
    assert abs(res["s_free"][2] - 0.361 / 1.639) <= 2e-5 and abs(res["s_used"][4] - 0.729 / 1.271) <= 2e-5 and res["s_other"][3] >= 1 - 2e-5
    assert res["counts"].tolist() == [[1, 1, 0, 1, 1, 1], [0, 0, 0, 0, 0, 0]] and res["dropped"].tolist() == [0, 0, 0, 0, 0, 0, 0, 1]
    assert np.abs(res["ap"] - [17 / 101, 0.0]).max() <= 1e-12
    want = np.array([[0.0, 1.0], [(134 / 3 - 17) / 101, 0.0], [0.0, 0.0], [0.0, 0.0], [17 / 101, 0.0], [8.5 / 101, 0.0], [17 / 101, 0.0],
                     [0.5 - 17 / 101, np.nan]])
    assert np.array_equal(np.isnan(res["dap"]), np.isnan(want)) and np.nanmax(np.abs(res["dap"] - want)) <= 1e-12
    assert np.abs(res["dap_mean"] - np.array([0.5, (134 / 3 - 17) / 202, 0, 0, 17 / 202, 8.5 / 202, 17 / 202, 0.5 - 17 / 101])).max() <= 1e-12
    # the one Loc pair: moved by (0.05, 0.05, 0.6) -> translation sqrt(0.365), same size, same orientation
    assert np.abs(res["loc_errors"][0] - [math.sqrt(0.365), 0.0, 0.0]).max() <= 2e-5 and np.isnan(res["loc_errors"][1]).all()
    assert np.abs(res["loc_errors_mean"] - res["loc_errors"][0]).max() == 0


def test_hand_computable_split_emulated(emu_lib):
    _run_hand_split()


@pytest.mark.gpu
def test_hand_computable_split_gpu(hip_lib):
    _run_hand_split()


def _run_errors_raised():
    from omni3d_amd.cubercnn.evaluation import omni3d_evaluation as E
    gts, dts = _hand_split()
    ev = E.Omni3Deval(E.AnnotationIndex(copy.deepcopy(gts), [1], [1, 2]), E.AnnotationIndex(copy.deepcopy(dts), [1], [1, 2]), mode="3D")
    with pytest.raises(Exception, match="evaluate"):
        ev.errors()
    with pytest.raises(Exception, match="errors"):
        ev.summarize_errors()
    ev.evaluate()
    for bad in ({"t_fg": 0.26}, {"t_bg": 0.25}, {"t_bg": 0.3}, {"t_bg": 0.0}, {"area": "huge"}):
        with pytest.raises(ValueError):
            ev.errors(**bad)
    assert ev.errors(t_fg=0.3)["t_fg"] == 0.3                # np.isclose finds the linspace value
    with pytest.raises(ValueError, match="distance"):
        _evaluate(gts, dts, imgs=[1], cats=[1, 2], mode="DIST").errors()
    empty = _evaluate([], [], imgs=[1], cats=[1, 2], mode="3D").errors()                                # an empty data set is legal
    assert len(empty["type"]) == 0 and (empty["ap"] == -1).all() and np.isnan(empty["dap_mean"]).all()


def test_errors_raised_emulated(emu_lib):
    _run_errors_raised()


@pytest.mark.gpu
def test_errors_raised_gpu(hip_lib):
    _run_errors_raised()


def _run_short_form():
    from omni3d_amd.cubercnn.evaluation import Omni3DEvaluator
    gts, dts = _split(SEED)
    by_img = {i: [d for d in dts if d["image_id"] == i] for i in IMGS}
    out = []
    for kw in ({}, {"errors": None}, {"errors": {}, "eval_dist": True}, {"errors": {"t_fg": 0.5, "t_bg": 0.1}}):
        ev = Omni3DEvaluator(copy.deepcopy(list(gts)), IMGS, CATS, False, **kw)
        ev.process([{"image_id": i} for i in IMGS], [{"instances": copy.deepcopy(by_img[i])} for i in IMGS])
        out.append(ev.evaluate()["bbox"])
    none, off, on, other = out
    assert set(none) == set(off) == {"AP2D", "AP3D", "omni_eval_2D", "omni_eval_3D"}                      # today's keys, exactly
    assert set(on) == set(off) | {"APDIST", "omni_eval_DIST", "errors_2D", "errors_3D"}                   # no analysis in mode DIST
    assert none["AP3D"] == on["AP3D"] and np.array_equal(none["omni_eval_3D"].eval["precision"], on["omni_eval_3D"].eval["precision"])
    ref = _reference(SEED, "3D")
    e3 = on["errors_3D"]
    assert e3["counts"] == dict(zip(("Cls", "Loc", "Both", "Dupe", "Bkg", "Miss"), ref["counts"].sum(axis=0).tolist()))
    assert list(e3["dAP"]) == list(X.ORACLES) and abs(e3["dAP"]["Loc"] - 100 * ref["dap_mean"][1]) <= 1e-9
    assert set(e3["loc_errors"]) == {"trans", "scale", "orient"} and on["errors_2D"]["loc_errors"] is None
    assert (other["errors_3D"]["t_fg"], other["errors_3D"]["t_bg"]) == (0.5, 0.1) and (other["errors_2D"]["t_fg"], other["errors_2D"]["t_bg"]) == (0.5, 0.1)
    assert other["errors_3D"]["counts"] != e3["counts"] and other["errors_2D"] == on["errors_2D"]         # 2D keeps its own thresholds
    for bad in ({"t_fg": 0.0}, {"t_fg": 0.2, "t_bg": 0.3}, {"threshold": 1.0}, [0.25, 0.05]):
        with pytest.raises(ValueError):
            Omni3DEvaluator(copy.deepcopy(list(gts)), IMGS, CATS, False, errors=bad)


def test_evaluator_short_form_emulated(emu_lib):
    _run_short_form()


@pytest.mark.gpu
def test_evaluator_short_form_gpu(hip_lib):
    _run_short_form()


KITTI, IDS = ["pedestrian", "car", "cyclist", "van", "truck"], [31, 3, 20, 12, 7]
SPLITS = ("KITTI_val", "KITTI_test")


def _run_helper(tmp_path, monkeypatch):
    """two tiny registered splits, the ground truth (moved, scaled and turned a little) fed back as predictions"""
    from omni3d_amd import synthetic
    from omni3d_amd.cubercnn import data
    from omni3d_amd.cubercnn.config import add_error_analysis_config, error_eval_args, get_cfg_defaults
    from omni3d_amd.cubercnn.evaluation import Omni3DEvaluationHelper
    from omni3d_amd.d2.config import get_cfg
    from omni3d_amd.d2.data import DatasetCatalog, MetadataCatalog
    from test_let_eval import _ry
    monkeypatch.chdir(tmp_path)
    saved_model = MetadataCatalog.pop("omni3d_model", None)
    root = str(tmp_path)
    try:
        synthetic.write_omni3d_stats(root, KITTI, IDS)
        files = [synthetic.write_omni3d_dataset(root, n, KITTI, IDS, num_images=3, height=96, width=128, num_gt=4, seed=7 + k, dataset_id=k,
                                                image_id_base=1000 * (k + 1)) for k, n in enumerate(SPLITS)]
        cfg = get_cfg()
        get_cfg_defaults(cfg)
        cfg.merge_from_file(os.path.join(ROOT, "configs", "cubercnn_DLA34_FPN.yaml"))
        cfg.merge_from_list(["DATASETS.CATEGORY_NAMES", tuple(KITTI), "MODEL.ROI_HEADS.NUM_CLASSES", len(KITTI)])
        fs = data.get_filter_settings_from_cfg(cfg)
        data.register_and_store_model_metadata(data.Omni3D(files, filter_settings=fs), root, fs)
        fs_test = data.get_filter_settings_from_cfg(cfg)
        fs_test.update(visibility_thres=cfg.TEST.VISIBILITY_THRES, truncation_thres=cfg.TEST.TRUNCATION_THRES, min_height_thres=0.0625, max_depth=1e8)
        id_map = MetadataCatalog.get("omni3d_model").thing_dataset_id_to_contiguous_id
        add_error_analysis_config(cfg)
        cfg.merge_from_list(["TEST.ERRORS.ENABLED", True])
        got = {}
        for tag, kw in (("none", {}), ("off", {"errors": None}), ("on", {**error_eval_args(cfg), "eval_dist": True})):
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
                        b3 = (b3 - c) * (1.0 + 0.05 * (k % 3)) @ _ry(0.05 * k).T + c * (1.0 + 0.02 * (k % 4 - 1))
                        recs.append({"image_id": img_id, "category_id": id_map[a["category_id"]], "bbox": list(a["bbox"]), "score": 0.9 - 0.01 * k,
                                     "depth": a["depth"], "bbox3D": b3.tolist()})
                    preds.append({"image_id": img_id, "K": im["K"], "width": im["width"], "height": im["height"], "instances": recs})
                helper.add_predictions(name, preds)
            ret = helper.summarize_all()
            got[tag] = (copy.deepcopy(ret), helper)
        (ana0, omni0), h0 = got["none"]
        (ana1, omni1), h1 = got["off"]
        (ana2, omni2), h2 = got["on"]
        assert h0.results_errors == {} and h1.results_errors == {} and h1.errors is None and h2.errors == {}
        assert repr(ana0) == repr(ana1) == repr(ana2) and repr(omni0) == repr(omni1) == repr(omni2)
        for name in SPLITS:
            r0, r1, r2 = h0.results[name], h1.results[name], h2.results[name]
            assert list(r0) == list(r1) and all(repr(r0[k]) == repr(r1[k]) for k in r0 if not k.endswith("_merge"))      # off = omitted
            assert all(repr(r0[k]) == repr(r2[k]) for k in r0 if not k.endswith("_merge"))
            assert set(r2) - set(r0) == {"bbox_2D_errors", "bbox_3D_errors", "bbox_DIST", "log_str_DIST", "bbox_DIST_merge"}
            e = r2["bbox_3D_errors"]
            assert set(e) == {"t_fg", "t_bg", "counts", "dAP", "loc_errors"} and list(e["dAP"]) == list(X.ORACLES) and sum(e["counts"].values()) > 0
            assert all(v >= -1e-13 for v in e["dAP"].values() if not math.isnan(v))
        assert list(h2.results_errors) == list(SPLITS)
        for name, row in h2.results_errors.items():
            assert list(row) == ["iters", "2D", "3D"] and row["iters"] == "3" and list(row["3D"]) == list(X.ORACLES)
            assert row["3D"] == h2.results[name]["bbox_3D_errors"]["dAP"]
    finally:
        for n in SPLITS:
            if n in DatasetCatalog:
                DatasetCatalog.remove(n)
            MetadataCatalog.pop(n, None)
        MetadataCatalog.pop("omni3d_model", None)
        if saved_model is not None:
            MetadataCatalog["omni3d_model"] = saved_model


def test_helper_fills_results_errors_emulated(emu_lib, tmp_path, monkeypatch):
    _run_helper(tmp_path, monkeypatch)


@pytest.mark.gpu
def test_helper_fills_results_errors_gpu(hip_lib, tmp_path, monkeypatch):
    _run_helper(tmp_path, monkeypatch)


def test_config_node_and_helper():
    from omni3d_amd.cubercnn.config import add_error_analysis_config, error_eval_args, get_cfg_defaults
    from omni3d_amd.d2.config import get_cfg
    cfg = get_cfg_defaults(get_cfg())
    assert "ERRORS" not in cfg.TEST and error_eval_args(cfg) == {"errors": None}                          # a cfg without the node: off
    assert add_error_analysis_config(cfg) is cfg
    assert dict(cfg.TEST.ERRORS) == {"ENABLED": False, "T_FG": [], "T_BG": []} and error_eval_args(cfg) == {"errors": None}
    cfg.merge_from_list(["TEST.ERRORS.ENABLED", True])
    assert error_eval_args(cfg) == {"errors": {}}                                                        # the mode defaults
    cfg.merge_from_list(["TEST.ERRORS.T_FG", [0.5], "TEST.ERRORS.T_BG", [0.1]])
    add_error_analysis_config(cfg)                                           # idempotent: the values that were set stay
    assert dict(cfg.TEST.ERRORS) == {"ENABLED": True, "T_FG": [0.5], "T_BG": [0.1]}
    assert error_eval_args(cfg) == {"errors": {"t_fg": 0.5, "t_bg": 0.1}}
    assert "ERRORS" not in get_cfg_defaults(get_cfg()).TEST                                              # the defaults stay the reference's
    for key, value in (("T_FG", [0.5, 0.25]), ("T_FG", [0.0]), ("T_BG", [1.0]), ("T_BG", [float("nan")])):
        other = add_error_analysis_config(get_cfg_defaults(get_cfg()))
        setattr(other.TEST.ERRORS, key, value)
        with pytest.raises(ValueError):
            error_eval_args(other)
    both = add_error_analysis_config(get_cfg_defaults(get_cfg()))
    both.TEST.ERRORS.T_FG, both.TEST.ERRORS.T_BG = [0.2], [0.3]
    with pytest.raises(ValueError):
        error_eval_args(both)


def _run_tool(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("error_report", os.path.join(ROOT, "tools", "error_report.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    gts, dts = _hand_split()
    gt_path, dt_path, out_path = tmp_path / "gt.json", tmp_path / "dt.json", tmp_path / "report.json"
    gt_path.write_text(json.dumps({"images": [{"id": 1}], "categories": [{"id": 1, "name": "a"}, {"id": 2, "name": "b"}], "annotations": gts}))
    dt_path.write_text(json.dumps(dts))
    assert tool.main([str(gt_path), str(dt_path), "--mode", "3D", "--json", str(out_path)]) == 0
    text = capsys.readouterr().out
    assert all(("Error %-5s" % n) in text for n in ("Cls", "Loc", "Both", "Dupe", "Bkg", "Miss")) and "Loc pairs" in text
    rep = json.loads(out_path.read_text())
    assert rep["counts_total"] == [1, 1, 0, 1, 1, 1] and rep["type"] == [X.BKG, X.TP, X.LOC, X.CLS, X.DUPE] and rep["mode"] == "3D"
    assert abs(rep["dap_mean"][0] - 0.5) <= 1e-12 and rep["dap"][7][1] is None                          # NaN is written as null
    assert tool.main([str(gt_path), str(dt_path), "--mode", "2D", "--t-fg", "0.75", "--t-bg", "0.2", "--area", "all"]) == 0
    assert "IoU=0.75/0.20" in capsys.readouterr().out


def test_error_report_tool_emulated(emu_lib, tmp_path, capsys):
    _run_tool(tmp_path, capsys)


@pytest.mark.gpu
def test_error_report_tool_gpu(hip_lib, tmp_path, capsys):
    _run_tool(tmp_path, capsys)
