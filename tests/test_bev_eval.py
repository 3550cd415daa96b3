"""`Omni3Deval(mode="BEV")`, `bev_overlap_groups`, the `eval_bev` switch of `Omni3DEvaluator` / `Omni3DEvaluationHelper` and
`config.add_bev_eval_config`.

The matching (`evaluate_groups`, csrc/eval_match.hip) and the accumulation are pinned to the reference's own Omni3Deval elsewhere
(tests/test_eval_match.py, tests/test_evaluator.py); what is new is the IoU pass.  So the yardstick is the SAME evaluation with its
IoU pass replaced by the float64 reference of tests/exact_bev.py: match tables, precision, recall and stats must be equal exactly.
That can only be asked of inputs on which 1e-5 of IoU (the kernel's bound, tests/test_bev_iou.py) decides nothing: in float64 no
pair's IoU lies within 1e-4 of a threshold and no two scores of a category tie; the split is generated from the first seed from 1
on that meets this, which `test_reference_alone_meets_the_conditions` asserts on the CPU.

Cross-check against the pinned 3D mode: in a split of yaw-only boxes that all share one y-centre and one height, footprint IoU and
IoU3D are the same number in exact geometry, so mode BEV and mode 3D must report identical stats; the margin to the thresholds is
1e-3 there (10 x the 1e-4 between the float32 IoU3D algorithm and exact geometry, tests/test_iou3d_oracle.py), and overlapping boxes
are turned 6 degrees or more against each other (tests/test_nms3d.py on near-parallel faces)."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

import exact_bev
from omni3d_amd import boxgen
from test_bev_iou import _ry, _upright

N_IMG, N_CAT = 6, 3
IOU_THRS = np.linspace(0.05, 0.5, 10)
SEED, SEED_FLAT = 5, 31            # first seeds from 1 on that meet the conditions (asserted below)


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
def _split(seed, flat=False):
    """(ground truths, detections) of 6 images x 3 categories: up to 6 ground truths and 12 detections per group, groups without
    detections, without ground truth and with `ignore3D`, depths over all three ranges.  flat=False: generic rotations, one
    detection with a NaN vertex, one ground truth whose footprint is a segment.  flat=True: yaw-only boxes with one y-centre and one
    height (footprint IoU = IoU3D), none invalid."""
    rng = np.random.default_rng(seed)
    gts, dts = [], []

    def box(c, d, yaw, R=None):
        if flat:
            return _upright((c[0], c[2]), 1.0, (d[0], 1.6, d[2]), yaw)
        return boxgen.corners(np.asarray(c)[None], np.asarray(d)[None], (R if R is not None else _ry(yaw))[None])[0]

    for img in range(1, N_IMG + 1):
        for cat in range(1, N_CAT + 1):
            n_gt = int(rng.integers(0, 7)) if (img + cat) % 5 else 0
            n_fp = int(rng.integers(0, 4))
            have_dt = (img + 2 * cat) % 6 != 0
            for _ in range(n_gt):
                c = np.array([rng.uniform(-8, 8), rng.uniform(-1, 1), rng.uniform(3, 60)])
                d = rng.uniform(0.6, 4.0, 3)
                yaw, R = rng.uniform(-np.pi, np.pi), boxgen.rand_rot(rng, 1)[0]
                gts.append(_rec(img, cat, box(c, d, yaw, R), ignore=int(rng.uniform() < 0.15)))
                for _ in range(int(rng.integers(0, 3)) if have_dt else 0):               # candidates: jittered copies
                    amount = rng.uniform(0.05, 0.5)
                    c2 = c + rng.normal(scale=amount, size=3) * d * np.array([1.0, 0.3, 1.0])
                    d2 = d * rng.uniform(1 - amount, 1 + amount, 3)
                    turn = rng.choice([-1, 1]) * np.radians(rng.uniform(6, 40))
                    dts.append(_rec(img, cat, box(c2, d2, yaw + turn, R @ _ry(turn)), score=rng.uniform(0.05, 0.99)))
            for _ in range(n_fp if have_dt else 0):
                c = np.array([rng.uniform(-8, 8), rng.uniform(-1, 1), rng.uniform(3, 60)])
                dts.append(_rec(img, cat, box(c, rng.uniform(0.6, 4.0, 3), rng.uniform(-np.pi, np.pi), boxgen.rand_rot(rng, 1)[0]),
                                score=rng.uniform(0.05, 0.6)))
    if not flat:
        bad = np.array(dts[3]["bbox3D"], np.float32)
        bad[2, 0] = np.nan
        dts[3]["bbox3D"] = bad.tolist()
        g = gts[2]
        c = np.mean(np.array(g["bbox3D"]), 0)
        gts[2] = _rec(g["image_id"], g["category_id"], _upright((c[0], c[2]), c[1], (0.0, 1.5, 2.0), 0.3))
    for k, r in enumerate(gts + dts):
        r["id"] = k + 1
    return gts, dts


def _by_group(recs):
    out = {}
    for r in recs:
        out.setdefault((r["image_id"], r["category_id"]), []).append(r)
    return out


@functools.lru_cache(maxsize=None)
def _conditions(seed, flat):
    """float64 alone -> (smallest distance of a pair's IoU to a threshold, number of score ties, number of overlapping pairs turned
    less than 5 degrees against each other (mod 90), facts about the split)"""
    gts, dts = _split(seed, flat)
    G, D = _by_group(gts), _by_group(dts)
    dist, ties, parallel, ious = 1.0, 0, 0, []
    for key in sorted(set(G) | set(D)):
        g, d = G.get(key, []), D.get(key, [])
        fg = exact_bev.footprints([np.array(x["bbox3D"], np.float32) for x in g])
        fd = exact_bev.footprints([np.array(x["bbox3D"], np.float32) for x in d])
        for a in fd:
            for b in fg:
                v = float(exact_bev.iou_footprints(a, b))
                ious.append(v)
                dist = min(dist, float(np.abs(IOU_THRS - v).min()))
                if flat and v > 0:
                    ea, eb = np.subtract(a[0][1], a[0][0]), np.subtract(b[0][1], b[0][0])
                    ang = np.degrees(np.arctan2(ea[0] * eb[1] - ea[1] * eb[0], ea[0] * eb[0] + ea[1] * eb[1])) % 90.0
                    parallel += int(min(ang, 90.0 - ang) < 5.0)
    for cat in range(1, N_CAT + 1):
        s = [x["score"] for x in dts if x["category_id"] == cat]
        ties += len(s) - len(set(s))
    sizes = [(len(G.get(k, [])), len(D.get(k, []))) for k in sorted(set(G) | set(D))]
    depth = np.array([x["depth"] for x in gts])
    facts = dict(ious=np.array(ious), sizes=sizes, ignore=sum(x["ignore3D"] for x in gts),
                 ranges=[int((depth < 10).sum()), int(((depth >= 10) & (depth < 35)).sum()), int((depth >= 35).sum())])
    return dist, ties, parallel, facts


def _good(seed, flat):
    """the conditions on the inputs, float64 alone: margins, no ties, and a split that has what the tests are about"""
    dist, ties, parallel, f = _conditions(seed, flat)
    fits = max(g for g, _ in f["sizes"]) <= 6 and max(d for _, d in f["sizes"]) <= 12
    kinds = any(g and not d for g, d in f["sizes"]) and any(d and not g for g, d in f["sizes"])         # no detections / no ground truth
    spread = f["ignore"] >= 2 and min(f["ranges"]) >= 3
    ious = (f["ious"] > 0.5).sum() >= 5 and ((f["ious"] > 0.05) & (f["ious"] < 0.5)).sum() >= 15 and (f["ious"] == 0).sum() >= 20
    return dist >= (1e-3 if flat else 1e-4) and ties == 0 and parallel == 0 and fits and kinds and spread and bool(ious)


@pytest.mark.parametrize("flat,seed", [(False, SEED), (True, SEED_FLAT)])
def test_reference_alone_meets_the_conditions(flat, seed):
    assert next(s for s in range(1, 50) if _good(s, flat)) == seed
    if not flat:                                                                                      # the two invalid boxes
        gts, dts = _split(seed)
        assert exact_bev.footprint(np.array(dts[3]["bbox3D"], np.float32))[0] == []
        assert exact_bev.footprint(np.array(gts[2]["bbox3D"], np.float32))[0] == []


_EXACT = {}


def _exact_groups(boxes_dt, boxes_gt, dt_sizes, gt_sizes, up=exact_bev.UP, **_):
    """stands in for `bev_overlap_groups`: the float64 reference on the same float32 boxes, in the same layout"""
    d, g = boxes_dt.cpu().numpy(), boxes_gt.cpu().numpy()
    key = (d.tobytes(), g.tobytes(), tuple(dt_sizes), tuple(gt_sizes), tuple(up))
    if key not in _EXACT:
        fd, fg = exact_bev.footprints(d, up), exact_bev.footprints(g, up)
        mats, od, og = [], 0, 0
        for nd, ng in zip(dt_sizes, gt_sizes):
            mats.append(np.array([[float(exact_bev.iou_footprints(fd[od + i], fg[og + j])) for j in range(ng)] for i in range(nd)],
                                 np.float64).reshape(nd, ng))
            od, og = od + nd, og + ng
        _EXACT[key] = mats
    return [torch.from_numpy(m).float().to(boxes_dt.device) for m in _EXACT[key]]


def _evaluate(gts, dts, mode, eval_prox=False, exact=False, monkeypatch=None):
    from omni3d_amd.cubercnn.evaluation import omni3d_evaluation as E
    imgs, cats = list(range(1, N_IMG + 1)), list(range(1, N_CAT + 1))
    calls = []
    if exact:
        monkeypatch.setattr(E, "bev_overlap_groups", _exact_groups)
    else:
        real = E.bev_overlap_groups
        monkeypatch.setattr(E, "bev_overlap_groups", lambda *a, **k: calls.append(1) or real(*a, **k))
    ev = E.Omni3Deval(E.AnnotationIndex(copy.deepcopy(list(gts)), imgs, cats), E.AnnotationIndex(copy.deepcopy(list(dts)), imgs, cats), mode=mode,
                      eval_prox=eval_prox)
    ev.evaluate()
    ev.accumulate()
    text = ev.summarize()
    assert exact or len(calls) == (1 if mode == "BEV" else 0)
    return ev, text


def _same(a, b):
    assert set(a._dev["match"]) == set(b._dev["match"])
    for k in a._dev["match"]:
        assert torch.equal(a._dev["match"][k].cpu(), b._dev["match"][k].cpu()), k
    assert np.array_equal(a.eval["precision"], b.eval["precision"]) and np.array_equal(a.eval["recall"], b.eval["recall"])
    assert np.array_equal(a.stats, b.stats)


def _run_bev_mode(monkeypatch):
    gts, dts = _split(SEED)
    for prox in (False, True):
        ev, text = _evaluate(gts, dts, "BEV", prox, monkeypatch=monkeypatch)
        ref, _ = _evaluate(gts, dts, "BEV", prox, exact=True, monkeypatch=monkeypatch)
        _same(ev, ref)
        assert (ev._dev["match"]["dt_match"] >= 0).sum() > 30 and 0.02 < ev.stats[0] < 0.98          # something is matched, not everything
        lines = text.split("\n")
        assert len(lines) == 13 and all(ln.startswith("mode=BEV ") for ln in lines)
        assert "IoU=0.05:0.50 | depth=   all" in lines[0] and "IoU=0.15 " in lines[1] and "IoU=0.25 " in lines[2] and "IoU=0.50 " in lines[3]
        assert "depth=  near" in lines[4] and "depth=   far" in lines[6]
    # the thresholds stay the user's: KITTI's 0.5 / 0.7
    from omni3d_amd.cubercnn.evaluation import omni3d_evaluation as E
    assert np.array_equal(E.Omni3DParams("BEV").iouThrs, E.Omni3DParams("3D").iouThrs) and E.Omni3DParams("BEV").areaRngLbl[1] == "near"
    assert E._METRICS["BEV"] == E._METRICS["3D"]
    with pytest.raises(Exception, match="not supported"):
        E.Omni3Deval(mode="BEV2")


def test_bev_mode_emulated(emu_lib, monkeypatch):
    _run_bev_mode(monkeypatch)


@pytest.mark.gpu
def test_bev_mode_gpu(hip_lib, monkeypatch):
    _run_bev_mode(monkeypatch)


def _run_flat_split(monkeypatch):
    gts, dts = _split(SEED_FLAT, True)
    bev, _ = _evaluate(gts, dts, "BEV", monkeypatch=monkeypatch)
    d3, _ = _evaluate(gts, dts, "3D", monkeypatch=monkeypatch)
    assert np.array_equal(bev.stats, d3.stats) and np.array_equal(bev.eval["precision"], d3.eval["precision"])
    assert 0.02 < bev.stats[0] < 0.98


def test_bev_equals_3d_on_boxes_of_one_height_emulated(emu_lib, monkeypatch):
    _run_flat_split(monkeypatch)


@pytest.mark.gpu
def test_bev_equals_3d_on_boxes_of_one_height_gpu(hip_lib, monkeypatch):
    _run_flat_split(monkeypatch)


def _run_groups(dev):
    """bev_overlap_groups: the layout of box3d_overlap_groups, empty groups, a generic up vector, errors"""
    from omni3d_amd.cubercnn.evaluation import omni3d_evaluation as E
    rng = np.random.default_rng(3)
    dt, gt, _ = boxgen.omni3d_like_pairs(rng, 12, degenerate_frac=0.0)
    dts, gts = [3, 0, 5, 4, 0], [2, 4, 0, 6, 0]
    tdt, tgt = torch.from_numpy(dt).to(dev), torch.from_numpy(gt).to(dev)
    up = (0.2, -0.9, 0.1)
    mats = E.bev_overlap_groups(tdt, tgt, dts, gts, up=up)
    want = _exact_groups(tdt, tgt, dts, gts, up=up)
    assert [tuple(m.shape) for m in mats] == [(3, 2), (0, 4), (5, 0), (4, 6), (0, 0)]
    for m, w in zip(mats, want):
        assert m.dtype == torch.float32 and (m.numel() == 0 or float((m.cpu() - w.cpu()).abs().max()) <= 1e-5)
    assert mats[0].untyped_storage().data_ptr() == mats[3].untyped_storage().data_ptr()                  # views of one flat tensor
    assert E.bev_overlap_groups(tdt[:0], tgt[:0], [], []) == []
    assert [tuple(m.shape) for m in E.bev_overlap_groups(tdt[:2], tgt[:0], [2], [0])] == [(2, 0)]
    with pytest.raises(ValueError):
        E.bev_overlap_groups(tdt, tgt, [3, 9], [2, 10, 0])
    with pytest.raises(ValueError):
        E.bev_overlap_groups(tdt, tgt, [3, 8], [2, 10])


def test_overlap_groups_emulated(emu_lib):
    _run_groups("cpu")


@pytest.mark.gpu
def test_overlap_groups_gpu(hip_lib):
    _run_groups("cuda")


def _run_short_form(monkeypatch):
    from omni3d_amd.cubercnn.evaluation import Omni3DEvaluator
    gts, dts = _split(SEED)
    imgs, cats = list(range(1, N_IMG + 1)), list(range(1, N_CAT + 1))
    by_img = {i: [d for d in dts if d["image_id"] == i] for i in imgs}
    out = {}
    for on in (False, True):
        ev = Omni3DEvaluator(copy.deepcopy(list(gts)), imgs, cats, False, **({"eval_bev": True} if on else {}))
        ev.process([{"image_id": i} for i in imgs], [{"instances": copy.deepcopy(by_img[i])} for i in imgs])
        out[on] = ev.evaluate()["bbox"]
    assert set(out[False]) == {"AP2D", "AP3D", "omni_eval_2D", "omni_eval_3D"}                           # today's keys, exactly
    assert set(out[True]) == set(out[False]) | {"APBEV", "omni_eval_BEV"}
    assert out[True]["AP2D"] == out[False]["AP2D"] and out[True]["AP3D"] == out[False]["AP3D"]
    direct, _ = _evaluate(gts, dts, "BEV", monkeypatch=monkeypatch)
    assert out[True]["APBEV"] == float(direct.stats[0] * 100) and np.array_equal(out[True]["omni_eval_BEV"].stats, direct.stats)
    ev = Omni3DEvaluator(copy.deepcopy(list(gts)), imgs, cats, True, eval_bev=True)                      # only_2d wins
    ev.process([{"image_id": i} for i in imgs], [{"instances": copy.deepcopy(by_img[i])} for i in imgs])
    assert set(ev.evaluate()["bbox"]) == {"AP2D", "omni_eval_2D"}


def test_evaluator_short_form_emulated(emu_lib, monkeypatch):
    _run_short_form(monkeypatch)


@pytest.mark.gpu
def test_evaluator_short_form_gpu(hip_lib, monkeypatch):
    _run_short_form(monkeypatch)


KITTI, IDS = ["pedestrian", "car", "cyclist", "van", "truck"], [31, 3, 20, 12, 7]
SPLITS = ("KITTI_val", "KITTI_test")           # names of a known family: the helper looks up the family's category list


def _run_helper(tmp_path, monkeypatch):
    """two tiny registered splits, the ground truth (moved a little) fed back as predictions"""
    from omni3d_amd import synthetic
    from omni3d_amd.cubercnn import data
    from omni3d_amd.cubercnn.config import get_cfg_defaults
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
        got = {}
        for on in (False, True):
            helper = Omni3DEvaluationHelper(list(SPLITS), fs_test, os.path.join(root, "inference%d" % on), iter_label="3",
                                            **({"eval_bev": True, "bev_up": (0.0, -1.0, 0.0)} if on else {}))
            for name, path in zip(SPLITS, files):
                gt = data.Omni3D([path], filter_settings=copy.deepcopy(fs_test))
                preds = []
                for img_id, im in sorted(gt.imgs.items()):
                    recs = []
                    for k, a in enumerate(gt.imgToAnns[img_id]):
                        if a["ignore"]:
                            continue
                        b3 = np.array(a["bbox3D"], np.float64)
                        b3 = b3 + np.array([0.25 * (k % 3), 0.0, 0.1 * k]) * (b3[:, 0].max() - b3[:, 0].min())       # some moved sideways
                        recs.append({"image_id": img_id, "category_id": id_map[a["category_id"]], "bbox": list(a["bbox"]), "score": 0.9 - 0.01 * k,
                                     "depth": a["depth"], "bbox3D": b3.tolist()})
                    preds.append({"image_id": img_id, "K": im["K"], "width": im["width"], "height": im["height"], "instances": recs})
                helper.add_predictions(name, preds)
            ret = helper.summarize_all()
            got[on] = (copy.deepcopy(ret), helper)
        (ana0, omni0), h0 = got[False]
        (ana1, omni1), h1 = got[True]
        assert h0.results_bev == {} and h0.eval_bev is False
        assert repr(ana0) == repr(ana1) and repr(omni0) == repr(omni1)                                   # NaNs compare by their text
        assert list(h1.results_bev) == list(SPLITS) + ["<Concat>"]
        cols = ["iters", "APBEV", "APBEV@15", "APBEV@25", "APBEV@50", "APBEV-N", "APBEV-M", "APBEV-F"]
        for name, row in h1.results_bev.items():
            assert list(row) == cols and row["iters"] == "3"
            assert 0.0 < row["APBEV"] <= 100.0 and row["APBEV"] >= ana1[name]["AP3D"] - 1e-9, (row, ana1[name])
        assert "bbox_BEV" in h1.results[SPLITS[0]] and "bbox_BEV" not in h0.results[SPLITS[0]]
        assert set(h1.results[SPLITS[0]]) - set(h0.results[SPLITS[0]]) == {"bbox_BEV", "log_str_BEV", "bbox_BEV_merge"}
    finally:
        for n in SPLITS:
            if n in DatasetCatalog:
                DatasetCatalog.remove(n)
            MetadataCatalog.pop(n, None)
        MetadataCatalog.pop("omni3d_model", None)
        if saved_model is not None:
            MetadataCatalog["omni3d_model"] = saved_model


def test_helper_fills_results_bev_emulated(emu_lib, tmp_path, monkeypatch):
    _run_helper(tmp_path, monkeypatch)


@pytest.mark.gpu
def test_helper_fills_results_bev_gpu(hip_lib, tmp_path, monkeypatch):
    _run_helper(tmp_path, monkeypatch)


def test_config_node_and_helper():
    from omni3d_amd.cubercnn.config import add_bev_eval_config, bev_eval_args, get_cfg_defaults
    from omni3d_amd.d2.config import get_cfg
    cfg = get_cfg_defaults(get_cfg())
    assert "EVAL_BEV" not in cfg.TEST
    assert bev_eval_args(cfg) == {"eval_bev": False, "bev_up": (0.0, -1.0, 0.0)}
    assert add_bev_eval_config(cfg) is cfg
    assert dict(cfg.TEST.EVAL_BEV) == {"ENABLED": False, "UP": [0.0, -1.0, 0.0]}
    assert bev_eval_args(cfg) == {"eval_bev": False, "bev_up": (0.0, -1.0, 0.0)}
    cfg.merge_from_list(["TEST.EVAL_BEV.ENABLED", True, "TEST.EVAL_BEV.UP", [0.0, -0.8, 0.6]])
    add_bev_eval_config(cfg)                                                 # idempotent: the values that were set stay
    assert dict(cfg.TEST.EVAL_BEV) == {"ENABLED": True, "UP": [0.0, -0.8, 0.6]}
    assert bev_eval_args(cfg) == {"eval_bev": True, "bev_up": (0.0, -0.8, 0.6)}
    other = add_bev_eval_config(get_cfg_defaults(get_cfg()))
    other.TEST.EVAL_BEV.UP.append(1.0)
    assert add_bev_eval_config(get_cfg_defaults(get_cfg())).TEST.EVAL_BEV.UP == [0.0, -1.0, 0.0]       # the default list is not shared
    with pytest.raises(ValueError):
        bev_eval_args(other)
