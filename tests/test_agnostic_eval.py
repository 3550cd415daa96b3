"""`Omni3Deval` with `params.useCats = 0` (class-agnostic evaluation: one group per image, K = 1).

1. Against tests/golden/eval_agnostic.npz, which tools/make_agnostic_golden.py records from the reference's own evaluator: `precision`,
   `recall` and `scores` EQUAL (the fixture keeps every IoU at least 1e-4 from a threshold, so every match decision is the same and the
   tables are quotients of the same integers), `stats` within 1e-12 (a mean of those), through both accumulation kernels.
2. The relabelling identity: the same records with every category replaced by one id, listed category-major, evaluated with
   useCats = 1, must give equal tables in all five modes -- the path the other reference fixtures already pin.
3. The refusals."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

GOLD = os.path.join(ROOT, "tests", "golden", "eval_agnostic.npz")
RUNS = (("p3d", "3D", False), ("prox", "3D", True), ("p2d", "2D", False))


def _index(records, imgs, cats):
    from omni3d_amd.cubercnn.evaluation import AnnotationIndex
    return AnnotationIndex(copy.deepcopy(list(records)), imgs, cats)


def _agnostic(ann, mode, prox):
    from omni3d_amd.cubercnn.evaluation import Omni3Deval
    ev = Omni3Deval(_index(ann["gts"], range(ann["images"]), ann["record_cats"]), _index(ann["dts"], range(ann["images"]), ann["record_cats"]),
                    mode=mode, eval_prox=prox)
    ev.params.catIds = list(ann["cat_ids"])
    ev.params.useCats = 0
    ev.evaluate()
    return ev


def _xywh_iou64(d, g):
    d, g = np.asarray(d, np.float64).reshape(-1, 1, 4), np.asarray(g, np.float64).reshape(1, -1, 4)
    w = np.minimum(d[..., 0] + d[..., 2], g[..., 0] + g[..., 2]) - np.maximum(d[..., 0], g[..., 0])
    h = np.minimum(d[..., 1] + d[..., 3], g[..., 1] + g[..., 3]) - np.maximum(d[..., 1], g[..., 1])
    inter = np.clip(w, 0, None) * np.clip(h, 0, None)
    union = d[..., 2] * d[..., 3] + g[..., 2] * g[..., 3] - inter
    return np.where(union > 0, inter / np.where(union > 0, union, 1), 0.0)


def _margin(values, thresholds):
    values = np.asarray(values, np.float64).reshape(-1, 1)
    return float(np.abs(values - np.asarray(thresholds, np.float64).reshape(1, -1)).min())


def _run_fixture(dev):
    from omni3d_amd.kernels import iou3d
    z = np.load(GOLD)
    ann = json.loads(bytes(z["annotations"]).decode())
    assert ann["images"] <= 40 and len(ann["record_cats"]) == 4
    for key, mode, prox in RUNS:
        ev = _agnostic(ann, mode, prox)
        for kw in (dict(parallel=False), dict(parallel=True, block=64)):
            ev.accumulate(**kw)
            assert ev.eval["counts"][2] == 1
            for name in ("precision", "recall", "scores"):
                got, want = ev.eval[name], z[key + "_" + name]
                assert got.shape == want.shape, (key, name, got.shape, want.shape)
                assert np.array_equal(got, want), (key, kw, name, float(np.abs(got - want).max()), int((got != want).sum()))
            ev.summarize()
            assert np.abs(ev.stats - z[key + "_stats"]).max() <= 1e-12, (key, kw)
        assert list(ev.params.catIds) == list(ann["cat_ids"])                       # the departure: catIds stays what the user set
        imgs = [e for e in ev.evalImgs if e is not None]
        assert len(ev.evalImgs) == 4 * ann["images"] and all(e["category_id"] == -1 for e in imgs)
    # ---- the conditions the fixture was built to
    gts, dts, cats = ann["gts"], ann["dts"], ann["cat_ids"]
    assert sorted({g["category_id"] for g in gts}) == [0, 1, 3] and 2 in cats and 3 not in cats      # 2 never has ground truth, 3 is not asked for
    assert {d["category_id"] for d in dts} == {0, 1, 2, 3}
    ev = _agnostic(ann, "3D", False)
    gcat, dcat = {g["id"]: g["category_id"] for g in gts}, {d["id"]: d["category_id"] for d in dts}
    cross = sum(1 for e in ev.evalImgs[:ann["images"]] if e is not None
                for did, gid in zip(e["dtIds"], e["dtMatches"][0]) if gid > 0 and gcat[int(gid)] != dcat[int(did)])
    assert cross >= 10, cross
    p3, p2 = ev.params, _agnostic(ann, "2D", False).params
    iou3, iou2, has = [], [], {"gt_only": 0, "dt_only": 0, "tie_inside": 0}
    firsts = {}
    for img in range(ann["images"]):
        gl = [g for c in cats for g in gts if g["image_id"] == img and g["category_id"] == c]
        dl = [d for c in cats for d in dts if d["image_id"] == img and d["category_id"] == c]
        has["gt_only"] += bool(gl) and not dl
        has["dt_only"] += bool(dl) and not gl
        scores = [d["score"] for d in dl]
        has["tie_inside"] += len(set(scores)) < len(scores)
        for s in set(scores):
            firsts.setdefault(s, set()).add(img)
        if gl and dl:
            b_d = torch.tensor(np.asarray([d["bbox3D"] for d in dl], np.float32), device=dev)
            b_g = torch.tensor(np.asarray([g["bbox3D"] for g in gl], np.float32), device=dev)
            iou3.append(iou3d.box3d_overlap(b_d, b_g, 1e-4, 1e-8).double().cpu().numpy().reshape(-1))
            iou2.append(_xywh_iou64([d["bbox"] for d in dl], [g["bbox"] for g in gl]).reshape(-1))
    assert has["gt_only"] and has["dt_only"] and has["tie_inside"] and any(len(v) > 1 for v in firsts.values()), has
    iou3, iou2 = np.concatenate(iou3), np.concatenate(iou2)
    margins = (_margin(iou3, p3.iouThrs), _margin(iou2, p2.iouThrs), _margin(iou2, [p3.proximity_thresh]))
    print("cross-category matches %d; smallest |IoU - threshold|: 3D %.2e, 2D %.2e, proximity %.2e" % ((cross,) + margins))
    assert min(margins) > 1e-4, margins


def test_reference_fixture_emulated(emu_lib):
    _run_fixture("cpu")


@pytest.mark.gpu
def test_reference_fixture_gpu(hip_lib):
    _run_fixture("cuda")


# ---- the relabelling identity ------------------------------------------------------------------------------------------------
N_IMG, CATS, ONE = 12, [4, 2, 9], 5           # catIds in an order that is not ascending: the category-major order is catIds' order


def _scene(seed=3):
    import bootstrap_scene as S
    from omni3d_amd import boxgen
    rng = np.random.default_rng(seed)
    gts, dts = [], []
    for img in range(N_IMG):
        n = int(rng.integers(2, 6))
        d_boxes, g_boxes, _ = boxgen.omni3d_like_pairs(rng, n + 2, overlap_frac=1.0, degenerate_frac=0.0)
        for j in range(n):
            cat = CATS[int(rng.integers(0, 3))]
            if img != 1:
                gts.append(S.rec(img, cat, g_boxes[j], ignore=int(rng.uniform() < 0.15)))
            if img != 2:
                for _ in range(int(rng.integers(0, 3))):
                    dcat = cat if rng.uniform() < 0.5 else CATS[int(rng.integers(0, 3))]
                    dts.append(S.rec(img, dcat, d_boxes[j] + rng.normal(scale=0.05, size=(1, 3)).astype(np.float32),
                                     score=float(np.round(rng.uniform(0.05, 1.0), 1))))
        if img != 2:
            for j in range(n, n + 2):
                dts.append(S.rec(img, CATS[int(rng.integers(0, 3))], d_boxes[j], score=float(np.round(rng.uniform(0.05, 0.6), 1))))
    for k, r in enumerate(gts + dts):
        r["id"] = k + 1
    return gts, dts


def _relabelled(records):
    return [dict(r, category_id=ONE) for c in CATS for r in records if r["category_id"] == c]


def _run_identity(mode):
    from omni3d_amd.cubercnn.evaluation import Omni3Deval
    gts, dts = _scene()
    imgs = list(range(N_IMG))
    W = np.random.default_rng(8).multinomial(N_IMG, np.full(N_IMG, 1.0 / N_IMG), size=8).astype(np.int32)
    a = Omni3Deval(_index(gts, imgs, CATS), _index(dts, imgs, CATS), mode=mode)
    a.params.catIds, a.params.useCats = list(CATS), 0
    b = Omni3Deval(_index(_relabelled(gts), imgs, [ONE]), _index(_relabelled(dts), imgs, [ONE]), mode=mode)
    tables = {"DIST": ("tp_errors", "tp_count"), "LET": ("precision_l", "tp_affinity", "tp_lon")}.get(mode, ())
    for ev in (a, b):
        ev.evaluate()
        ev.accumulate()
        ev.summarize()
    assert a.eval["counts"] == b.eval["counts"] and a.eval["counts"][2] == 1
    for name in ("precision", "recall", "scores") + tables:
        assert np.array_equal(a.eval[name], b.eval[name], equal_nan=True), (mode, name)
    assert (a.eval["precision"] > 0).any() and (a.eval["precision"][a.eval["precision"] > -1] < 1).any()
    assert np.array_equal(a.stats, b.stats)
    # the categories mattered: the ordinary evaluation of the same records differs
    c = Omni3Deval(_index(gts, imgs, CATS), _index(dts, imgs, CATS), mode=mode)
    c.evaluate()
    c.accumulate()
    assert c.eval["precision"].shape[2] == 3 and not np.array_equal(c.eval["precision"][:, :, :1], a.eval["precision"])
    ba, bb = a.bootstrap(weights=W), b.bootstrap(weights=W)
    for name in ("ap", "ar", "stats", "point"):
        assert np.array_equal(ba[name], bb[name], equal_nan=True), (mode, name)
    assert ba["ap"].shape == (8, len(a.params.iouThrs), 1, 4, 3)


@pytest.mark.parametrize("mode", ["2D", "3D", "BEV", "DIST", "LET"])
def test_relabelling_identity_emulated(emu_lib, mode):
    _run_identity(mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["2D", "3D", "BEV", "DIST", "LET"])
def test_relabelling_identity_gpu(hip_lib, mode):
    _run_identity(mode)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _run_refusals(L, monkeypatch):
    from omni3d_amd.cubercnn.evaluation import Omni3Deval
    gts, dts = _scene()
    imgs = list(range(N_IMG))
    ev = Omni3Deval(_index(gts, imgs, CATS), _index(dts, imgs, CATS), mode="3D")
    ev.params.useCats = 0
    ev.evaluate()
    with pytest.raises(ValueError, match="useCats"):
        ev.errors()
    many = [{"image_id": 7, "category_id": CATS[i % 3], "bbox": [float(i), 0.0, 1.0, 1.0], "area": 1.0, "id": i + 1} for i in range(1025)]
    one = [{"image_id": 7, "category_id": CATS[0], "bbox": [0.0, 0.0, 1.0, 1.0], "area": 1.0, "score": 0.5, "id": 1}]
    ev = Omni3Deval(_index(many, [7], CATS), _index(one, [7], CATS), mode="2D")
    ev.params.useCats = 0
    calls = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    with pytest.raises(ValueError, match="image 7 has 1025 ground truths"):
        ev.evaluate()
    assert calls == []
    # 1024 fit
    ev = Omni3Deval(_index(many[:1024], [7], CATS), _index(one, [7], CATS), mode="2D")
    ev.params.useCats = 0
    ev.evaluate()
    ev.accumulate()
    assert calls and ev.eval["recall"][0, 0, 0, -1] == 1.0 / 1024


def test_refusals_emulated(emu_lib, monkeypatch):
    _run_refusals(emu_lib, monkeypatch)


@pytest.mark.gpu
def test_refusals_gpu(hip_lib, monkeypatch):
    _run_refusals(hip_lib, monkeypatch)
