"""`KittiEval` with `params.aos` end to end, against tests/exact_kitti_aos.py fed float64 similarities and float64 headings.

The data are the 60 synthetic images of tests/test_kitti_eval.py (yaw-only cuboids) with the detections' headings changed: half keep
theirs (the ground truth's yaw with that generator's small noise), a quarter are turned by pi -- a relabelling of the same eight corner
values, so every similarity stays what it was --, a quarter get a random yaw (their BEV and 3D similarities are recomputed in float64).

Conditions, asserted on the CPU by the reference alone: no similarity lies within 1e-4 of a min-overlap (as in test_kitti_eval.py),
and some class and difficulty has 0 < AOS < AP2D.  Under them the counters equal the oracle's.

Bar on `aos_r40` / `aos_r11`, 1e-7.  The oracle's alpha is the float64 numpy evaluation of the `box_params` formulas on the same float32
corners (test_kitti_box_params.py shows the kernel within 1e-12 rad of it).  q = (1 + cos x) / 2 has |dq / dx| = |sin x| / 2 <= 1 / 2, so a
term moves by at most 5e-13 + 2^-40 (fixed point) < 1.5e-12; `aos` is a mean of such terms over tp + fp >= tp and AOS is 100 x a mean of
`aos`: <= 1.5e-10, inside 1e-7."""
import copy
import functools

import numpy as np
import pytest

import exact_bev
import exact_iou3d
import exact_kitti as X
import exact_kitti_aos as XA
import test_kitti_eval as E
from test_kitti_box_params import _exact as _box_exact
from test_kitti_drivers import _count_calls

SEED, N_IMG = E.SEED, E.N_IMG
FLIP = [5, 4, 7, 6, 1, 0, 3, 2]          # the corner order of the same box turned by pi about its vertical axis
N_EMU = 20


def _f32(b):
    return np.asarray(b, np.float32)


@functools.lru_cache(maxsize=None)
def _data():
    """-> (ground-truth annotations, detections, per image: dt (score order), gt, sim {metric: (D, G)}, dc)"""
    gts, _ = E._dataset(SEED)
    rng = np.random.default_rng(41)
    images, dts = [], []
    for im in E._similarities(SEED):
        sim = {m: v.copy() for m, v in im["sim"].items()}
        fg = [exact_bev.footprint(_f32(y["bbox3D"])) if y["valid3D"] else ([], 0.0) for y in im["gt"]]
        new = []
        for i, x in enumerate(im["dt"]):
            x, b, u = copy.deepcopy(x), np.asarray(x["bbox3D"], np.float64), rng.uniform()
            if u < 0.5:
                x["kind"] = "copy"
            elif u < 0.75:
                x["kind"], b = "flip", b[FLIP]
            else:
                x["kind"] = "random"
                dims = [np.linalg.norm(b[k] - b[0]) for k in (1, 3, 4)]
                b = E._cuboid(b.mean(axis=0), dims, rng.uniform(-np.pi, np.pi)).astype(np.float64)
                fp = exact_bev.footprint(_f32(b))
                for j, y in enumerate(im["gt"]):
                    sim["BEV"][i, j] = float(exact_bev.iou_footprints(fp, fg[j]))
                    sim["3D"][i, j] = exact_iou3d.iou3d(_f32(b).astype(np.float64), _f32(y["bbox3D"]).astype(np.float64))[1] if sim["BEV"][i, j] > 0 else 0.0
            x["bbox3D"] = b.tolist()
            new.append(x)
        images.append({"dt": new, "gt": im["gt"], "sim": sim, "dc": im["dc"]})
        dts += new
    return gts, dts, images


def _alpha_of(records):
    """float64 numpy on the float32 corners; NaN without a valid cuboid; a record's own finite `alpha` (-10: absent) wins"""
    if not records:
        return np.zeros(0)
    out = _box_exact(np.stack([_f32(r["bbox3D"]) for r in records]))[:, 7]
    for k, r in enumerate(records):
        if not r.get("valid3D", True):
            out[k] = np.nan
        a = r.get("alpha")
        if a is not None and np.isfinite(a) and a != -10:
            out[k] = a
    return out


def _oracle_slot(images, cname, diff, metric, mo):
    p = E._params()
    per = []
    for im in images:
        g = im["gt"]
        rel = [(2 if a["ignore"] or a["ignore2D"] or a["ignore3D"] else 0) if a["category_name"] == cname else
               1 if a["category_name"] in p.neighbours.get(cname, ()) else -1 for a in g]
        per.append({"sim": im["sim"][metric], "score": [x["score"] for x in im["dt"]], "dc": im["dc"],
                    "gt_flag": X.gt_flags(rel, [a["bbox"][3] for a in g], [X.occlusion_level(a, p.occCuts) for a in g],
                                          [max(a["truncation"], 0.0) for a in g], diff[1:]),
                    "dt_flag": X.dt_flags([E.NAMES[x["category_id"]] == cname for x in im["dt"]], [x["bbox"][3] for x in im["dt"]], diff[1]),
                    "gt_alpha": _alpha_of(g), "dt_alpha": _alpha_of(im["dt"])})
    return XA.evaluate_slot_aos(per, mo)


@functools.lru_cache(maxsize=None)
def _oracle(n_img=N_IMG):
    p = E._params()
    images = _data()[2][:n_img]
    return {(c, d, mi, 0): _oracle_slot(images, cname, diff, metric, p.minOverlaps["strict"][c])
            for c, cname in enumerate(p.classes) for d, diff in enumerate(p.difficulties) for mi, metric in enumerate(p.metrics)}


def test_reference_alone_meets_the_conditions():
    gts, dts, images = _data()
    dist = 1.0
    for im in images:
        for v in list(im["sim"].values()) + [im["dc"]]:
            if v.size:
                dist = min(dist, float(np.abs(v[..., None] - np.array(E.MIN_OVS)).min()))
    assert dist >= 1e-4, dist
    assert {x["kind"] for x in dts} == {"copy", "flip", "random"}
    ref = _oracle()
    between = [(k, r["aos_r40"], r["ap_r40"]) for k, r in ref.items() if k[2] == 0 and 0.0 < r["aos_r40"] < r["ap_r40"]]
    assert len(between) >= 3, between
    kinds = {images[i]["dt"][d]["kind"] for per_image in ref[(0, 1, 0, 0)]["pairs"] for i, ps in enumerate(per_image) for g, d in ps}
    assert kinds == {"copy", "flip", "random"}                               # every kind of heading is among the cars' true positives


def _evaluate(n_img, dts=None, gts=None, **kw):
    from omni3d_amd.cubercnn.evaluation.kitti import KittiEval
    g, d, _ = _data()
    d = d if dts is None else dts
    ev = KittiEval(E._index(g if gts is None else gts, n_img), copy.deepcopy([x for x in d if x["image_id"] <= n_img]),
                   params=E._params(minOverlaps={"strict": (0.7, 0.5, 0.5)}, **kw))
    ev.evaluate()
    return ev


def _run_end_to_end(n_img, monkeypatch):
    from omni3d_amd.cubercnn.evaluation.kitti import KittiParams
    assert KittiParams().aos is False
    calls = _count_calls(monkeypatch)
    plain = _evaluate(n_img)                                                # no AOS attribute is touched
    off = _evaluate(n_img, aos=False)
    assert [c for c in calls if c.startswith("omni_kitti")] == ["omni_kitti_match_tp", "omni_kitti_thresholds", "omni_kitti_match_counts",
                                                                 "omni_kitti_finalize"] * 2          # no new entry point with `aos` off
    assert list(off.eval.keys()) == list(plain.eval.keys()) and "aos" not in off.eval and "n_unoriented" not in off.eval
    assert repr(off.results(r11=True)) == repr(plain.results(r11=True)) and not any(k.startswith("AOS") for k in off.results(r11=True))
    assert off.summarize(r11=True, verbose=False) == plain.summarize(r11=True, verbose=False)
    del calls[:]
    ev = _evaluate(n_img, aos=True)
    assert [c for c in calls if c.startswith("omni_kitti")] == ["omni_kitti_box_params", "omni_kitti_match_tp", "omni_kitti_thresholds",
                                                                 "omni_kitti_match_counts_aos", "omni_kitti_finalize", "omni_kitti_finalize_aos"]
    e, ref = ev.eval, _oracle(n_img)
    for k in plain.eval:                                                    # what was there stays, to the bit
        assert repr(e[k]) == repr(plain.eval[k]) if not isinstance(e[k], np.ndarray) else e[k].tobytes() == plain.eval[k].tobytes(), k
    worst = 0.0
    for key, r in ref.items():
        assert e["n_gt"][key] == r["n_gt"] and e["K"][key] == r["K"] and np.array_equal(e["counts"][key], r["counts"]), key
        if key[2] != 0:
            assert np.isnan(e["aos_r40"][key]) and np.isnan(e["aos_r11"][key]) and np.isnan(e["aos"][key]).all() and not e["sim_sum"][key].any(), key
            continue
        assert (np.abs(e["sim_sum"][key] - r["sim_fixed"]) <= np.maximum(r["counts"][:, 0], 1) * 4).all(), key      # 1e-12 rad of alpha: a few units of 2^-40
        err = max(abs(e["aos_r40"][key] - r["aos_r40"]), abs(e["aos_r11"][key] - r["aos_r11"]), 100 * np.abs(e["aos"][key] - r["aos"]).max())
        worst = max(worst, float(err))
        assert err <= 1e-7, (key, err)
        assert (e["aos"][key] <= e["precision"][key]).all()
    print("AOS end to end: at most %.3g from the oracle" % worst)
    gts = [a for a in _data()[0] if a["image_id"] <= n_img]
    assert e["n_unoriented"] == sum(a["category_name"] in ("car", "pedestrian", "cyclist") and not a["valid3D"] for a in gts) > 0
    rows = ev.results(r11=True)
    assert rows["AOS|R40-car-moderate"] == e["aos_r40"][0, 1, 0, 0] and rows["AOS|R11-cyclist-hard"] == e["aos_r11"][2, 2, 0, 0]
    assert len(rows) == 54 + 18 and {k: v for k, v in rows.items() if not k.startswith("AOS")} == plain.results(r11=True)
    lines = ev.summarize(verbose=False).split("\n")
    assert len(lines) == 12 + 3 + 1 and [ln[:4] for ln in lines[1:5]] == ["bbox", "aos ", "bev ", "3d  "]
    assert lines[2] == "aos  AP:" + ", ".join("%.4f" % v for v in e["aos_r40"][0, :, 0, 0]) and "no heading" in lines[-1]
    assert [ln for ln in lines if not ln.startswith("aos") and not ln.startswith("AOS")] == plain.summarize(verbose=False).split("\n")
    assert len(ev.summarize(r11=True, verbose=False).split("\n")) == 2 * 15 + 1


def test_end_to_end_emulated(emu_lib, monkeypatch):
    _run_end_to_end(N_EMU, monkeypatch)


@pytest.mark.gpu
def test_end_to_end_gpu(hip_lib, monkeypatch):
    _run_end_to_end(N_IMG, monkeypatch)


def _run_variants(n_img):
    from omni3d_amd.cubercnn.evaluation.kitti import KittiEval
    small = dict(metrics=("2D", "3D"), aos=True)
    base = _evaluate(n_img, **small)
    gts, dts, _ = _data()
    # a record's own `alpha` wins over its corners: with one value everywhere every true positive has q = 1 and AOS is AP2D
    keyed = _evaluate(n_img, dts=[dict(x, alpha=0.7) for x in dts], gts=[dict(a, alpha=0.7) for a in gts], **small)
    assert np.abs(keyed.eval["aos_r40"][..., 0, :] - keyed.eval["ap_r40"][..., 0, :]).max() <= 1e-9 and keyed.eval["n_unoriented"] == 0
    assert keyed.eval["ap_r40"].tobytes() == base.eval["ap_r40"].tobytes()
    assert (base.eval["aos_r40"][..., 0, :] < base.eval["ap_r40"][..., 0, :] - 1.0).any()
    # KITTI's "unknown" -10, None and NaN count as absent: the corners are used
    absent = (-10, None, float("nan"))
    same = _evaluate(n_img, dts=[dict(x, alpha=absent[k % 3]) for k, x in enumerate(dts)], **small)
    assert same.eval["aos"].tobytes() == base.eval["aos"].tobytes() and same.eval["sim_sum"].tobytes() == base.eval["sim_sum"].tobytes()
    # detections = the valid ground-truth cuboids themselves: AOS is AP2D; the same detections turned by pi (the same eight corners,
    # relabelled): every AP to the bit, every AOS gone
    own = [{"image_id": a["image_id"], "category_id": a["category_id"], "score": 0.05 + 0.9 * ((37 * k) % 101) / 101.0, "bbox": list(a["bbox"]),
            "bbox3D": a["bbox3D"]} for k, a in enumerate(gts) if a["valid3D"] and a["category_name"] != "dontcare"]
    turned = [dict(x, bbox3D=np.asarray(x["bbox3D"])[FLIP].tolist()) for x in own]
    a, b = _evaluate(n_img, dts=own, **small), _evaluate(n_img, dts=turned, **small)
    assert a.eval["ap_r40"].tobytes() == b.eval["ap_r40"].tobytes() and a.eval["ap_r11"].tobytes() == b.eval["ap_r11"].tobytes()
    assert a.eval["counts"].tobytes() == b.eval["counts"].tobytes() and a.eval["ap_r40"].min() > 0
    oriented = [dict(g, ignore=True) if not g["valid3D"] else g for g in gts]              # for AOS == AP every counted ground truth needs a heading
    a2 = _evaluate(n_img, dts=own, gts=oriented, **small)
    assert np.abs(a2.eval["aos_r40"][..., 0, :] - a2.eval["ap_r40"][..., 0, :]).max() <= 1e-9
    print("all detections turned by pi: the largest AOS is %.3g" % max(b.eval["aos_r40"][..., 0, :].max(), b.eval["aos_r11"][..., 0, :].max()))
    assert b.eval["aos_r40"][..., 0, :].max() <= 1e-9 and b.eval["aos_r11"][..., 0, :].max() <= 1e-9
    # AOS belongs to the 2D matching
    with pytest.raises(ValueError, match="2D"):
        KittiEval(E._index(gts, n_img), [], params=E._params(metrics=("3D",), aos=True)).evaluate()


def test_variants_emulated(emu_lib):
    _run_variants(12)


@pytest.mark.gpu
def test_variants_gpu(hip_lib):
    _run_variants(N_EMU)


def test_config_node_and_args():
    from omni3d_amd.cubercnn.config import add_kitti_aos_config, add_kitti_eval_config, get_cfg_defaults, kitti_aos_eval_args, kitti_eval_args
    from omni3d_amd.d2.config import get_cfg
    cfg = get_cfg_defaults(get_cfg())
    off = {"eval_kitti": False, "kitti_params": {"occCuts": (0.75, 0.5, 0.25), "dcMetrics": ("2D", "BEV", "3D")}, "kitti_r11": False}
    assert kitti_aos_eval_args(cfg) == dict(off, kitti_params=dict(off["kitti_params"], aos=False)) and "EVAL_KITTI" not in cfg.TEST
    add_kitti_eval_config(cfg)
    assert "AOS" not in cfg.TEST.EVAL_KITTI and kitti_aos_eval_args(cfg)["kitti_params"]["aos"] is False
    assert add_kitti_aos_config(cfg) is cfg and cfg.TEST.EVAL_KITTI.AOS is False
    assert dict(cfg.TEST.EVAL_KITTI) == {"ENABLED": False, "OCC_CUTS": [0.75, 0.5, 0.25], "DC_METRICS": ["2D", "BEV", "3D"], "R11": False, "AOS": False}
    cfg.merge_from_list(["TEST.EVAL_KITTI.AOS", True, "TEST.EVAL_KITTI.ENABLED", True])
    add_kitti_aos_config(cfg)                                               # idempotent: the values that were set stay
    assert cfg.TEST.EVAL_KITTI.AOS is True
    assert kitti_eval_args(cfg) == dict(off, eval_kitti=True)               # unchanged: no new key
    assert kitti_aos_eval_args(cfg) == dict(off, eval_kitti=True, kitti_params=dict(off["kitti_params"], aos=True))
    fresh = add_kitti_aos_config(get_cfg_defaults(get_cfg()))               # on a cfg without the node
    assert fresh.TEST.EVAL_KITTI.AOS is False and fresh.TEST.EVAL_KITTI.R11 is False


def _run_helper(tmp_path, monkeypatch):
    """the long form of the drivers, as tests/test_kitti_drivers.py sets it up, with TEST.EVAL_KITTI.AOS on"""
    import os
    from test_kitti_drivers import IDS, KITTI, SPLITS, _predictions
    from omni3d_amd import synthetic
    from omni3d_amd.cubercnn import data
    from omni3d_amd.cubercnn.config import add_kitti_aos_config, get_cfg_defaults, kitti_aos_eval_args
    from omni3d_amd.cubercnn.evaluation import Omni3DEvaluationHelper
    from omni3d_amd.d2.config import get_cfg
    from omni3d_amd.d2.data import DatasetCatalog, MetadataCatalog
    monkeypatch.chdir(tmp_path)
    calls = _count_calls(monkeypatch)
    saved_model = MetadataCatalog.pop("omni3d_model", None)
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
        add_kitti_aos_config(cfg)
        cfg.merge_from_list(["TEST.EVAL_KITTI.ENABLED", True, "TEST.EVAL_KITTI.AOS", True, "TEST.EVAL_KITTI.R11", True])
        on = kitti_aos_eval_args(cfg)
        assert on["kitti_params"]["aos"] is True
        on["kitti_params"]["difficulties"] = [("easy", 10, 0, 0.15), ("moderate", 5, 1, 0.30), ("hard", 5, 2, 0.50)]      # 96-pixel images
        helper = Omni3DEvaluationHelper(list(SPLITS), fs_test, os.path.join(root, "inference"), iter_label="3", **on)
        for name, path in zip(SPLITS, files):
            helper.add_predictions(name, _predictions(data.Omni3D([path], filter_settings=copy.deepcopy(fs_test)), id_map))
        helper.summarize_all()
        assert [c for c in calls if c.startswith("omni_kitti_")] == ["omni_kitti_box_params", "omni_kitti_match_tp", "omni_kitti_thresholds",
                                                                      "omni_kitti_match_counts_aos", "omni_kitti_finalize", "omni_kitti_finalize_aos"] * len(SPLITS)
        for name in SPLITS:
            row, res = helper.results_kitti[name], helper.results[name]["bbox_KITTI"]
            assert len(row) == 1 + 2 * 2 * (27 + 9) and res == {k: v for k, v in row.items() if k != "iters"}
            for key in ("AOS|R40-car-moderate", "AOS|R11-pedestrian-easy", "AOS|R40-cyclist-hard@loose"):
                assert 0.0 <= row[key] <= row[key.replace("AOS", "AP2D")] + 1e-9, (key, row[key])
            # the predictions are the ground truth moved a little, headings kept: AOS is AP2D up to the rows without a heading
            assert max(row["AOS|R40-%s-hard@loose" % c] for c in ("car", "pedestrian", "cyclist")) > 0.0
            assert "aos  AP:" in helper.results[name]["log_str_KITTI"]
    finally:
        for n in SPLITS:
            if n in DatasetCatalog:
                DatasetCatalog.remove(n)
            MetadataCatalog.pop(n, None)
        MetadataCatalog.pop("omni3d_model", None)
        if saved_model is not None:
            MetadataCatalog["omni3d_model"] = saved_model


def test_helper_emulated(emu_lib, tmp_path, monkeypatch):
    _run_helper(tmp_path, monkeypatch)


@pytest.mark.gpu
def test_helper_gpu(hip_lib, tmp_path, monkeypatch):
    _run_helper(tmp_path, monkeypatch)
