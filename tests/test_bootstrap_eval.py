"""`Omni3Deval.bootstrap`, `bootstrap_compare`, the `bootstrap` switch of `Omni3DEvaluator` / `Omni3DEvaluationHelper` and
`config.add_bootstrap_config`: image-level bootstrap intervals of every AP / AR and the paired comparison of two prediction sets.
The kernel itself is held to its definition in tests/test_bootstrap_kernel.py; here the all-ones replicate must reproduce summarize()
(1e-12: `stats` averages the means over recall of the same doubles in another order), a split small enough to score by hand, the drawn
weights, the paired deltas and the plumbing."""
import copy
import os

import numpy as np
import pytest

import bootstrap_scene as S
from omni3d_amd import boxgen

MODES = ("2D", "3D", "BEV", "DIST", "LET")


def _run_all_ones():
    for mode in MODES:
        ev = S.evaluated(mode)
        bs = ev.bootstrap(weights=np.ones((1, S.N_IMG), np.int64))
        assert bs["stats"].shape == (1, 13) and bs["point"].shape == (13,) and np.array_equal(bs["point"], bs["stats"][0])
        err = float(np.abs(bs["stats"][0] - ev.stats).max())
        print("mode %s: |bootstrap(ones) - summarize()| %.2e" % (mode, err))
        assert err <= 1e-12, (mode, err)
        assert np.array_equal(bs["stats"][0] == -1, ev.stats == -1) and (ev.stats[:4] > 0).all()
        assert mode == "2D" or (ev.stats > 0).all()                                                    # no "large" 2D box in the scene
        assert np.array_equal(bs["ar"][0], ev.eval["recall"][:, :, :, :]) and np.abs(bs["ap"][0] - ev.eval["precision"].mean(axis=1)).max() <= 1e-12
        k = bs["per_category"]
        want = ev.eval["precision"][:, :, :, 0, -1].mean(axis=(0, 1))
        assert k["values"].shape == (1, 3) and k["ci"].shape == (3, 2) and np.abs(k["point"] - want).max() <= 1e-12


def test_all_ones_replicate_reproduces_the_evaluator_emulated(emu_lib):
    _run_all_ones()


@pytest.mark.gpu
def test_all_ones_replicate_reproduces_the_evaluator_gpu(hip_lib):
    _run_all_ones()


def _hand_split():
    """one category, two images: image A (id 1) holds a ground truth and its copy at score 0.9, image B (id 2) a ground truth and a
    detection 20 m beside it at 0.8"""
    dims, eye = np.array([[1.0, 1.0, 1.0]]), np.eye(3)[None]
    box = lambda x: boxgen.corners(np.array([[x, 0.0, 6.0]]), dims, eye)[0]          # noqa: E731
    gts = [S.rec(1, 1, box(0.0)), S.rec(2, 1, box(2.0))]
    dts = [S.rec(1, 1, box(0.0), score=0.9), S.rec(2, 1, box(22.0), score=0.8)]
    for k, r in enumerate(gts + dts):
        r["id"] = k + 1
    return gts, dts


def _run_hand_split():
    from omni3d_amd.cubercnn.evaluation import Omni3Deval
    gts, dts = _hand_split()
    ev = S.evaluate(gts, dts, imgs=[1, 2], cats=[1], accumulate=False)
    bs = ev.bootstrap(weights=[[2, 0], [0, 2], [1, 1], [1, 3]])
    # (2, 0): the true positive twice, recall 1 at precision 1.  (0, 2): a false positive twice.  (1, 1): precision 1 up to recall 1/2 =
    # the 51 thresholds 0 .. 0.50, nothing beyond.  (1, 3): four ground truths, recall tops out at 1/4 = the 26 thresholds 0 .. 0.25
    want = np.array([1.0, 0.0, 51 / 101, 26 / 101])
    # 1 / (1 + eps) = 1 - 2.2e-16 per threshold: 1e-12 is the bound of the kernel tests
    assert np.abs(bs["ap"][:, :, 0, 0, -1] - want[:, None]).max() <= 1e-12
    assert np.array_equal(bs["ar"][:, :, 0, 0, -1], np.repeat([[1.0], [0.0], [0.5], [0.25]], 10, axis=1))
    assert np.abs(bs["stats"][:, 0] - want).max() <= 1e-12 and np.abs(bs["per_category"]["values"][:, 0] - want).max() <= 1e-12
    assert abs(bs["point"][0] - 51 / 101) <= 1e-12
    assert (bs["stats"][:, 5] == -1).all() and (bs["stats"][:, 6] == -1).all()                        # no ground truth beyond 10 m
    assert bs["n_valid"].tolist()[:5] == [4, 4, 4, 4, 4] and bs["n_valid"][5] == 0 and np.isnan(bs["ci"][5]).all()
    with pytest.raises(Exception, match="evaluate"):
        Omni3Deval(mode="3D").bootstrap()
    for bad in ([[1, -1]], [[0.5, 1]], [[1, 1, 1]], [1, 1], [[1, float("nan")]]):
        with pytest.raises(ValueError):
            ev.bootstrap(weights=bad)
    assert np.array_equal(ev.bootstrap(weights=[[2.0, 0.0]])["ap"], bs["ap"][:1])                     # integers written as floats
    with pytest.raises(ValueError, match="2\\^31"):
        ev.bootstrap(weights=[[2 ** 31 - 1, 1]])
    for bad in (0.0, 1.0, "x"):
        with pytest.raises(ValueError):
            ev.bootstrap(n=2, confidence=bad)


def test_hand_computable_split_emulated(emu_lib):
    _run_hand_split()


@pytest.mark.gpu
def test_hand_computable_split_gpu(hip_lib):
    _run_hand_split()


def _run_drawn():
    ev = S.evaluated("3D")
    n = 8
    a, b, c = ev.bootstrap(n=n, seed=0), ev.bootstrap(n=n, seed=0), ev.bootstrap(n=n, seed=1)
    assert a["weights"].shape == (n, S.N_IMG) and a["weights"].dtype == np.int32
    assert np.array_equal(a["weights"], b["weights"]) and not np.array_equal(a["weights"], c["weights"])
    assert (a["weights"].sum(axis=1) == S.N_IMG).all() and (c["weights"].sum(axis=1) == S.N_IMG).all()
    g = np.random.default_rng(0)
    assert np.array_equal(a["weights"], g.multinomial(S.N_IMG, np.full(S.N_IMG, 1 / S.N_IMG), size=n))
    for key in ("ap", "ar", "stats", "mean", "se", "ci"):
        assert np.array_equal(a[key], b[key], equal_nan=True)
    strata = {img: ("x" if i < 2 else "y") for i, img in enumerate(S.IMGS)}
    s = ev.bootstrap(n=n, seed=0, strata=strata)
    assert (s["weights"][:, :2].sum(axis=1) == 2).all() and (s["weights"][:, 2:].sum(axis=1) == 4).all()
    g = np.random.default_rng(0)                                                                       # sorted labels: "x" first
    assert np.array_equal(s["weights"][:, :2], g.multinomial(2, np.full(2, 0.5), size=n))
    assert np.array_equal(s["weights"][:, 2:], g.multinomial(4, np.full(4, 0.25), size=n))
    with pytest.raises(ValueError):
        ev.bootstrap(n=n, strata={S.IMGS[0]: "x"})
    q = [(1 - 0.95) / 2, (1 + 0.95) / 2]
    for r in (a, s):
        assert r["stats"].shape == (n, 13) and r["ci"].shape == (13, 2) and r["n_valid"].shape == (13,)
        for j in range(13):
            v = r["stats"][:, j][r["stats"][:, j] > -1]
            assert r["n_valid"][j] == v.size and v.size >= 2
            assert np.array_equal(r["ci"][j], np.quantile(v, q)) and r["mean"][j] == v.mean() and r["se"][j] == v.std(ddof=1)
        k = r["per_category"]
        for j in range(3):
            v = k["values"][:, j][k["values"][:, j] > -1]
            assert k["n_valid"][j] == v.size and (v.size == 0 or np.array_equal(k["ci"][j], np.quantile(v, q)))
    assert np.array_equal(ev.bootstrap(n=n, seed=0, confidence=0.5)["ci"][0], np.quantile(a["stats"][:, 0], [(1 - 0.5) / 2, (1 + 0.5) / 2]))
    assert a["stats"][:, 0].std() > 0                                                                  # the replicates do differ
    one, whole = ev.bootstrap(n=n, seed=0, chunk=1), ev.bootstrap(n=n, seed=0, chunk=n)
    for key in ("ap", "ar", "stats", "point"):
        assert np.array_equal(one[key], whole[key]) and np.array_equal(one[key], a[key])               # bit for bit
    with pytest.raises(ValueError):
        ev.bootstrap(n=n, chunk=0)


def test_drawn_weights_emulated(emu_lib):
    _run_drawn()


@pytest.mark.gpu
def test_drawn_weights_gpu(hip_lib):
    _run_drawn()


def _run_compare():
    from omni3d_amd.cubercnn.evaluation import bootstrap_compare
    gts, dts = S.scene()
    ev = S.evaluated("3D")
    n = 8
    same = bootstrap_compare(ev, ev, n=n, seed=2)
    both = ~np.isnan(same["delta"])
    assert same["delta"].shape == (n, 13) and both[:, 0].all() and (same["delta"][both] == 0).all()
    assert np.array_equal(same["n_valid"], both.sum(axis=0)) and (same["p_le0"][same["n_valid"] > 0] == 1).all() and (same["n_valid"] > 0).all()
    assert (same["delta_point"] == 0).all() and (same["delta_ci"] == 0).all()
    assert np.array_equal(same["a"]["weights"], same["b"]["weights"]) and np.array_equal(same["weights"], ev.bootstrap(n=n, seed=2)["weights"])
    moved = copy.deepcopy(list(dts))
    for d in moved:
        if d["category_id"] == 1:                                                                      # 50 m further away
            d["bbox3D"] = (np.array(d["bbox3D"]) + [0.0, 0.0, 50.0]).tolist()
            d["depth"] += 50.0
    worse = S.evaluate(gts, moved)
    cmp = bootstrap_compare(ev, worse, n=n, seed=2)
    assert (cmp["delta"][:, 0] >= 0).all() and cmp["delta_point"][0] > 0 and (cmp["delta"][:, 0] > 0).any()
    assert np.array_equal(cmp["delta"][:, 0], cmp["a"]["stats"][:, 0] - cmp["b"]["stats"][:, 0])
    assert cmp["delta_ci"][0, 0] <= cmp["delta_ci"][0, 1] and cmp["p_le0"][0] == float((cmp["delta"][:, 0] <= 0).mean())
    assert (cmp["per_category"]["delta"][:, 0] > 0).all() and (cmp["per_category"]["delta"][:, 1][~np.isnan(cmp["per_category"]["delta"][:, 1])] == 0).all()
    assert (bootstrap_compare(worse, ev, n=n, seed=2)["p_le0"][0] == 1)
    fewer = S.evaluate(gts, dts, imgs=S.IMGS[:5])
    with pytest.raises(ValueError):
        bootstrap_compare(ev, fewer, n=n)
    with pytest.raises(ValueError):
        bootstrap_compare(ev, S.evaluated("2D"), n=n)                                                  # other thresholds and ranges


def test_paired_comparison_emulated(emu_lib):
    _run_compare()


@pytest.mark.gpu
def test_paired_comparison_gpu(hip_lib):
    _run_compare()


KITTI, IDS = ["pedestrian", "car", "cyclist", "van", "truck"], [31, 3, 20, 12, 7]
SPLITS = ("KITTI_val", "KITTI_test")           # names of a known family: the helper looks up the family's category list


def _run_helper(tmp_path, monkeypatch, tags):
    """the synthetic two-split setup of tests/test_let_eval.py::_run_helper: the ground truth, scaled and turned a little, is fed back
    as predictions -> {tag: (summarize_all(), helper)}"""
    from omni3d_amd import synthetic
    from omni3d_amd.cubercnn import data
    from omni3d_amd.cubercnn.config import add_bootstrap_config, bootstrap_eval_args, get_cfg_defaults
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
        add_bootstrap_config(cfg)
        cfg.merge_from_list(["TEST.BOOTSTRAP.ENABLED", True, "TEST.BOOTSTRAP.NUM_REPLICATES", 50, "TEST.BOOTSTRAP.SEED", 4])
        kwargs = {"none": {}, "off": {"bootstrap": None}, "on": bootstrap_eval_args(cfg)}
        assert kwargs["on"] == {"bootstrap": {"n": 50, "seed": 4, "confidence": 0.95}}
        got = {}
        for tag in tags:
            helper = Omni3DEvaluationHelper(list(SPLITS), fs_test, os.path.join(root, "inference_" + tag), iter_label="3", **kwargs[tag])
            for name, path in zip(SPLITS, files):
                gt = data.Omni3D([path], filter_settings=copy.deepcopy(fs_test))
                preds = []
                for img_id, im in sorted(gt.imgs.items()):
                    recs = []
                    for k, a in enumerate(gt.imgToAnns[img_id]):
                        if a["ignore"] or k % 4 == 3:                  # a detector that misses some
                            continue
                        b3 = np.array(a["bbox3D"], np.float64)
                        c = b3.mean(axis=0)
                        b3 = (b3 - c) * (1.0 + 0.1 * (k % 3)) + c * (1.0 + 0.02 * (k % 4 - 1))
                        recs.append({"image_id": img_id, "category_id": id_map[a["category_id"]], "bbox": list(a["bbox"]), "score": 0.9 - 0.01 * k,
                                     "depth": a["depth"], "bbox3D": b3.tolist()})
                    preds.append({"image_id": img_id, "K": im["K"], "width": im["width"], "height": im["height"], "instances": recs})
                helper.add_predictions(name, preds)
            ret = helper.summarize_all()
            got[tag] = (copy.deepcopy(ret), helper)
        return got
    finally:
        for n in SPLITS:
            if n in DatasetCatalog:
                DatasetCatalog.remove(n)
            MetadataCatalog.pop(n, None)
        MetadataCatalog.pop("omni3d_model", None)
        if saved_model is not None:
            MetadataCatalog["omni3d_model"] = saved_model


def test_helper_is_unchanged_with_the_option_off_emulated(emu_lib, tmp_path, monkeypatch):
    got = _run_helper(tmp_path, monkeypatch, ("none", "off"))
    (ana0, omni0), h0 = got["none"]
    (ana1, omni1), h1 = got["off"]
    assert h0.bootstrap is None and h1.bootstrap is None and h0.results_ci == {} and h1.results_ci == {}
    assert repr(ana0) == repr(ana1) and repr(omni0) == repr(omni1)                                     # NaNs compare by their text
    for name in SPLITS:
        r0, r1 = h0.results[name], h1.results[name]
        assert list(r0) == list(r1) and not any(k.endswith("_ci") for k in r0)
        assert all(repr(r0[k]) == repr(r1[k]) for k in r0 if not k.endswith("_merge"))


def _run_helper_on(tmp_path, monkeypatch):
    got = _run_helper(tmp_path, monkeypatch, ("none", "on"))
    (ana0, omni0), h0 = got["none"]
    (ana2, omni2), h2 = got["on"]
    assert repr(ana0) == repr(ana2) and repr(omni0) == repr(omni2)
    assert h2.bootstrap == {"n": 50, "seed": 4, "confidence": 0.95}
    for name in SPLITS:
        r0, r2 = h0.results[name], h2.results[name]
        assert set(r2) - set(r0) == {"bbox_2D_ci", "bbox_3D_ci"}
        assert all(repr(r0[k]) == repr(r2[k]) for k in r0 if not k.endswith("_merge"))
        for mode, names in (("2D", ["AP", "AP50", "AP75", "AP95", "APs", "APm", "APl"]), ("3D", ["AP", "AP15", "AP25", "AP50", "APn", "APm", "APf"])):
            ci = r2["bbox_%s_ci" % mode]
            assert list(ci)[:7] == names and {k for k in r2["bbox_" + mode] if k.startswith("AP-")} == {k for k in ci if k.startswith("AP-")}
            lo, hi = ci["AP"]
            assert 0.0 <= lo <= hi <= 100.0 and lo - 1e-9 <= r2["bbox_" + mode]["AP"] + 1e-9 and lo < hi, (mode, ci["AP"], r2["bbox_" + mode]["AP"])
            assert all(np.isnan(v[0]) or v[0] <= v[1] for v in ci.values())
    assert list(h2.results_ci) == list(SPLITS) + ["<Concat>"]
    for name, row in h2.results_ci.items():
        assert list(row) == ["iters", "AP2D", "AP3D"] and row["iters"] == "3"
        assert 0.0 <= row["AP2D"][0] <= row["AP2D"][1] <= 100.0 and 0.0 <= row["AP3D"][0] < row["AP3D"][1] <= 100.0, row
    assert h2.results_ci[SPLITS[0]]["AP3D"] == h2.results[SPLITS[0]]["bbox_3D_ci"]["AP"]


def test_helper_fills_results_ci_emulated(emu_lib, tmp_path, monkeypatch):
    _run_helper_on(tmp_path, monkeypatch)


@pytest.mark.gpu
def test_helper_fills_results_ci_gpu(hip_lib, tmp_path, monkeypatch):
    _run_helper_on(tmp_path, monkeypatch)


def _run_short_form():
    from omni3d_amd.cubercnn.evaluation import Omni3DEvaluator
    gts, dts = S.scene()
    by_img = {i: [d for d in dts if d["image_id"] == i] for i in S.IMGS}
    out = []
    for kw in ({}, {"bootstrap": None}, {"bootstrap": {"n": 6, "seed": 1}}):
        ev = Omni3DEvaluator(copy.deepcopy(list(gts)), S.IMGS, S.CATS, False, **kw)
        ev.process([{"image_id": i} for i in S.IMGS], [{"instances": copy.deepcopy(by_img[i])} for i in S.IMGS])
        out.append(ev.evaluate()["bbox"])
    none, off, on = out
    assert set(none) == set(off) == {"AP2D", "AP3D", "omni_eval_2D", "omni_eval_3D"} and set(on) == set(off) | {"AP2D_ci", "AP3D_ci"}
    assert none["AP3D"] == off["AP3D"] == on["AP3D"] and none["AP2D"] == on["AP2D"]
    want = on["omni_eval_3D"].bootstrap(n=6, seed=1)["ci"][0] * 100
    assert on["AP3D_ci"] == (float(want[0]), float(want[1])) and want[0] < want[1]
    for bad in ({"n": 0}, {"n": 2.5}, {"seed": -1}, {"confidence": 1.0}, {"replicates": 5}, [50]):
        with pytest.raises(ValueError):
            Omni3DEvaluator(copy.deepcopy(list(gts)), S.IMGS, S.CATS, False, bootstrap=bad)


def test_evaluator_short_form_emulated(emu_lib):
    _run_short_form()


@pytest.mark.gpu
def test_evaluator_short_form_gpu(hip_lib):
    _run_short_form()


def test_config_node_and_helper():
    from omni3d_amd.cubercnn.config import add_bootstrap_config, bootstrap_eval_args, get_cfg_defaults
    from omni3d_amd.d2.config import get_cfg
    cfg = get_cfg_defaults(get_cfg())
    assert "BOOTSTRAP" not in cfg.TEST
    assert bootstrap_eval_args(cfg) == {"bootstrap": None}                                             # a cfg without the node
    assert add_bootstrap_config(cfg) is cfg
    assert dict(cfg.TEST.BOOTSTRAP) == {"ENABLED": False, "NUM_REPLICATES": 1000, "SEED": 0, "CONFIDENCE": 0.95}
    assert bootstrap_eval_args(cfg) == {"bootstrap": None}                                             # off by default
    cfg.merge_from_list(["TEST.BOOTSTRAP.ENABLED", True, "TEST.BOOTSTRAP.NUM_REPLICATES", 200, "TEST.BOOTSTRAP.CONFIDENCE", 0.9])
    add_bootstrap_config(cfg)                                                # idempotent: the values that were set stay
    assert dict(cfg.TEST.BOOTSTRAP) == {"ENABLED": True, "NUM_REPLICATES": 200, "SEED": 0, "CONFIDENCE": 0.9}
    assert bootstrap_eval_args(cfg) == {"bootstrap": {"n": 200, "seed": 0, "confidence": 0.9}}
    assert "BOOTSTRAP" not in get_cfg_defaults(get_cfg()).TEST                                           # the defaults stay the reference's
    for key, value in (("NUM_REPLICATES", 0), ("NUM_REPLICATES", -5), ("SEED", -1), ("CONFIDENCE", 0.0), ("CONFIDENCE", 1.0),
                       ("CONFIDENCE", float("nan"))):
        other = add_bootstrap_config(get_cfg_defaults(get_cfg()))
        setattr(other.TEST.BOOTSTRAP, key, value)
        with pytest.raises(ValueError):
            bootstrap_eval_args(other)


def test_compare_tool(emu_lib, tmp_path, capsys):
    """tools/compare_predictions.py on result files as the evaluator writes them"""
    import json
    import runpy
    import sys
    gts, dts = S.scene()
    moved = [dict(d, depth=d["depth"] + 50.0, bbox3D=(np.array(d["bbox3D"]) + [0.0, 0.0, 50.0]).tolist()) if d["category_id"] == 1 else d for d in dts]
    gt = {"images": [{"id": i} for i in S.IMGS], "categories": [{"id": c, "name": "c%d" % c} for c in S.CATS], "annotations": list(gts)}
    for name, obj in (("gt.json", gt), ("a.json", list(dts)), ("b.json", moved)):
        with open(tmp_path / name, "w") as f:
            json.dump(obj, f)
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "compare_predictions.py")
    argv = sys.argv
    sys.argv = [tool, str(tmp_path / "gt.json"), str(tmp_path / "a.json"), str(tmp_path / "b.json"), "--n", "8", "--seed", "2"]
    try:
        runpy.run_path(tool, run_name="__main__")
    finally:
        sys.argv = argv
    text = capsys.readouterr().out
    ev = S.evaluated("3D")
    assert "mode=3D" in text and "n=8" in text and "A %.2f" % (100 * ev.stats[0]) in text and "p(delta <= 0) = 0.000" in text, text
