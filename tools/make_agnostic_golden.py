"""Writes tests/golden/eval_agnostic.npz: a seeded data set and what the reference's own `Omni3Deval` (imported unchanged through
oracle/ref_harness.py, CPU) returns for it with `params.useCats = 0`: `precision`, `recall`, `scores`, `stats` for mode 3D, mode 3D with
eval_prox=True and mode 2D, and the annotation JSON.  Needs the reference checkout.
    python tools/make_agnostic_golden.py

The data set: 36 images, categories 0..3 in the records, catIds = [0, 1, 2]: category 2 never has ground truth, category 3 is in the
records and absent from catIds.  Cuboids from `boxgen`, their 2D boxes projected with one pinhole camera (XYWH, unclipped), so that
eval_prox means something.  A detection is a jittered copy of a ground truth, relabelled with probability 0.45, or clutter.
Conditions, checked here (AssertionError otherwise) and asserted again by tests/test_agnostic_eval.py:
  - at least 10 detections are matched under useCats = 0 to a ground truth of another category (range "all", lowest threshold);
  - no IoU the evaluation compares (the IoU3D of every (detection, ground truth) pair of an image in mode 3D, the 2D IoU in mode 2D and
    against proximity_thresh), as a float64 number, lies within 1e-4 of a threshold;
  - score ties inside an image and across images; an image with ground truth and no detection; one with detections and no ground truth."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PATH = os.path.join(ROOT, "tests", "golden", "eval_agnostic.npz")
IMAGES, RECORD_CATS, CAT_IDS = 36, (0, 1, 2, 3), [0, 1, 2]
FX, FY, CX, CY = 500.0, 500.0, 320.0, 240.0
MARGIN = 1e-4
RUNS = (("p3d", "3D", False), ("prox", "3D", True), ("p2d", "2D", False))


def project(box):
    """(8, 3) corners -> the XYWH box of their projection (vertices at z < 0.1 taken at 0.1), unclipped"""
    z = np.maximum(box[:, 2].astype(np.float64), 0.1)
    u, v = FX * box[:, 0] / z + CX, FY * box[:, 1] / z + CY
    return [float(u.min()), float(v.min()), float(u.max() - u.min()), float(v.max() - v.min())]


def dataset(seed):
    from omni3d_amd import boxgen
    rs = np.random.default_rng(seed)
    gts, dts = [], []

    def rec(img, cat, box, **extra):
        bb = project(box)
        return {"image_id": img, "category_id": int(cat), "bbox3D": np.asarray(box, np.float32).tolist(), "depth": float(box[:, 2].mean()),
                "bbox": bb, "area": bb[2] * bb[3], **extra}

    for img in range(IMAGES):
        ng = int(rs.integers(1, 6))
        nclutter = int(rs.integers(0, 4))
        if img == 3:
            nclutter = 2                                                   # detections, no ground truth
        d_boxes, g_boxes, _ = boxgen.omni3d_like_pairs(rs, ng + nclutter, overlap_frac=1.0, degenerate_frac=0.0)
        for j in range(ng):
            if img == 3:
                break
            cat = int(rs.choice((0, 1, 3), p=(0.45, 0.4, 0.15)))           # category 2 never has ground truth
            gts.append(rec(img, cat, g_boxes[j], ignore3D=int(rs.uniform() < 0.15), ignore2D=int(rs.uniform() < 0.15)))
            if img == 5:
                continue                                                   # ground truth, no detection
            for _ in range(int(rs.integers(0, 3))):                        # zero, one or two detections on it
                dcat = cat if rs.uniform() > 0.45 else int(rs.choice(RECORD_CATS))
                box = d_boxes[j] + rs.normal(scale=0.05, size=(1, 3)).astype(np.float32)
                score = float(np.round(rs.uniform(0.05, 1.0), 1 if rs.uniform() < 0.6 else 6))       # coarse rounding => score ties
                dts.append(rec(img, dcat, box, score=score))
        for j in range(ng, ng + nclutter):
            if img == 5:
                break
            dts.append(rec(img, int(rs.choice(RECORD_CATS)), d_boxes[j], score=float(np.round(rs.uniform(0.05, 0.7), 1))))
    for i, r in enumerate(gts):
        r["id"] = i + 1
    for i, r in enumerate(dts):
        r["id"] = i + 1
    return gts, dts


def xywh_iou(d, g):
    d, g = np.asarray(d, np.float64).reshape(-1, 1, 4), np.asarray(g, np.float64).reshape(1, -1, 4)
    w = np.minimum(d[..., 0] + d[..., 2], g[..., 0] + g[..., 2]) - np.maximum(d[..., 0], g[..., 0])
    h = np.minimum(d[..., 1] + d[..., 3], g[..., 1] + g[..., 3]) - np.maximum(d[..., 1], g[..., 1])
    inter = np.clip(w, 0, None) * np.clip(h, 0, None)
    union = d[..., 2] * d[..., 3] + g[..., 2] * g[..., 3] - inter
    return np.where(union > 0, inter / np.where(union > 0, union, 1), 0.0)


def margin(values, thresholds):
    """the smallest distance of a value to a threshold (inf without values)"""
    values = np.asarray(values, np.float64).reshape(-1, 1)
    return float(np.abs(values - np.asarray(thresholds, np.float64).reshape(1, -1)).min()) if values.size else float("inf")


def image_lists(gts, dts, img):
    """the records of an image that take part, category-major in CAT_IDS order"""
    return ([g for c in CAT_IDS for g in gts if g["image_id"] == img and g["category_id"] == c],
            [d for c in CAT_IDS for d in dts if d["image_id"] == img and d["category_id"] == c])


def structure_facts(gts, dts):
    """the conditions on the records alone -> dict of booleans / counts"""
    by_img = {}
    for d in dts:
        if d["category_id"] in CAT_IDS:
            by_img.setdefault(d["image_id"], []).append(d["score"])
    all_scores = [s for v in by_img.values() for s in v]
    tie_inside = any(len(set(v)) < len(v) for v in by_img.values())
    firsts = {}
    for img, v in by_img.items():
        for s in set(v):
            firsts.setdefault(s, set()).add(img)
    g_imgs = {g["image_id"] for g in gts if g["category_id"] in CAT_IDS}
    d_imgs = set(by_img)
    return {"tie_inside": tie_inside, "tie_across": any(len(v) > 1 for v in firsts.values()), "n_scores": len(all_scores),
            "gt_without_dt": sorted(g_imgs - d_imgs), "dt_without_gt": sorted(d_imgs - g_imgs),
            "cats_with_gt": sorted({g["category_id"] for g in gts}), "cats_in_records": sorted({r["category_id"] for r in gts + dts})}


def run_reference(gts, dts, mode, prox):
    from oracle import ref_harness
    ref_harness.install()
    from cubercnn.evaluation.omni3d_evaluation import Omni3Deval          # the reference's file
    from omni3d_amd.cubercnn.evaluation import AnnotationIndex              # duck-typed COCO API (4 methods), no arithmetic
    np.float = float                                                        # the reference still uses the alias numpy 2 removed
    ev = Omni3Deval(AnnotationIndex([dict(g) for g in gts], range(IMAGES), RECORD_CATS),
                    AnnotationIndex([dict(d) for d in dts], range(IMAGES), RECORD_CATS), mode=mode, eval_prox=prox)
    ev.params.catIds = list(CAT_IDS)
    ev.params.useCats = 0
    ev.evaluate()
    ious, eval_imgs = dict(ev.ious), list(ev.evalImgs)
    ev.accumulate()
    ev.summarize()
    return ev, ious, eval_imgs


def main():
    gts, dts = dataset(seed=21)
    facts = structure_facts(gts, dts)
    assert facts["tie_inside"] and facts["tie_across"] and facts["gt_without_dt"] and facts["dt_without_gt"], facts
    assert facts["cats_with_gt"] == [0, 1, 3] and facts["cats_in_records"] == [0, 1, 2, 3], facts
    out, notes = {}, {}
    for key, mode, prox in RUNS:
        ev, ious, eval_imgs = run_reference(gts, dts, mode, prox)
        assert ev.eval["precision"].shape[2] == 1
        vals = np.concatenate([np.asarray(v[0], np.float64).reshape(-1) for v in ious.values() if len(v) and len(v[0])])
        notes[key + "_margin"] = margin(vals, ev.params.iouThrs)
        assert notes[key + "_margin"] > MARGIN, (key, notes)
        if key == "p3d":                                                    # detections matched to a ground truth of another category
            gcat, dcat = {g["id"]: g["category_id"] for g in gts}, {d["id"]: d["category_id"] for d in dts}
            cross = 0
            for e in eval_imgs[:IMAGES]:                                    # range "all"
                if e is not None:
                    cross += sum(1 for did, gid in zip(e["dtIds"], e["dtMatches"][0]) if gid > 0 and gcat[int(gid)] != dcat[did])
            notes["cross_matches"] = cross
            assert cross >= 10, cross
        for name in ("precision", "recall", "scores"):
            out[key + "_" + name] = ev.eval[name]
        out[key + "_stats"] = np.asarray(ev.stats)
    prox2d = np.concatenate([xywh_iou([d["bbox"] for d in dl], [g["bbox"] for g in gl]).reshape(-1)
                             for gl, dl in (image_lists(gts, dts, i) for i in range(IMAGES)) if gl and dl])
    notes["proximity_margin"] = margin(prox2d, [0.3])
    assert notes["proximity_margin"] > MARGIN, notes
    blob = json.dumps({"gts": gts, "dts": dts, "images": IMAGES, "record_cats": list(RECORD_CATS), "cat_ids": CAT_IDS})
    np.savez_compressed(PATH, annotations=np.frombuffer(blob.encode(), dtype=np.uint8), **out)
    print("%s: %d ground truths, %d detections, %s, %s, %d bytes" % (os.path.relpath(PATH, ROOT), len(gts), len(dts), facts, notes,
                                                                      os.path.getsize(PATH)))
    for key, _, _ in RUNS:
        print(key, np.round(out[key + "_stats"], 4).tolist())


if __name__ == "__main__":
    main()
