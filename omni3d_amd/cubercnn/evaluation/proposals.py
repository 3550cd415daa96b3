"""`proposal_recall`: the class-agnostic average recall of region proposals -- the standard diagnostic of the first stage of a two-stage
detector -- as one mode-2D evaluation with `params.useCats = 0`.  How proposals are taken from a model is the caller's business."""
import copy
import json

import numpy as np

_AREAS = (("", "all"), ("s", "small"), ("m", "medium"), ("l", "large"))


def _gt_records(dataset):
    """the data-set JSON (a dict or a path) -> (annotation records with `bbox` XYWH, `area`, `ignore2D`; image ids).  An annotation
    without `bbox` takes the first valid of Omni3D's XYXY boxes `bbox2D_tight`, `bbox2D_proj`, `bbox2D_trunc`."""
    if isinstance(dataset, str):
        with open(dataset) as f:
            dataset = json.load(f)
    anns = []
    for a in dataset["annotations"]:
        a = copy.deepcopy(a)
        if "bbox" not in a:
            for key in ("bbox2D_tight", "bbox2D_proj", "bbox2D_trunc"):
                b = a.get(key)
                if b is not None and len(b) == 4 and b[2] > b[0] and b[3] > b[1]:
                    a["bbox"] = [float(b[0]), float(b[1]), float(b[2] - b[0]), float(b[3] - b[1])]
                    break
            else:
                raise ValueError("annotation %r has no valid 2D box" % (a.get("id"),))
        a.setdefault("area", float(a["bbox"][2] * a["bbox"][3]))
        a.setdefault("ignore2D", int(bool(a.get("ignore", 0))))
        anns.append(a)
    return anns, [im["id"] for im in dataset["images"]]


def proposal_recall(gt, proposals, max_dets=(10, 100, 1000), device=None):
    """Average recall of class-agnostic proposals.  gt: an `AnnotationIndex` (or any object with its four calls) or the data-set JSON
    (dict or path; see `_gt_records`); proposals: a mapping image id -> (boxes XYXY (N, 4), objectness (N,)), arrays, tensors or lists;
    max_dets: the proposal budgets k, any number of them.

    This is the COCO protocol's AR, NOT detectron2's max-overlap recall: one evaluation in mode 2D with `useCats = 0` and `maxDets =
    max_dets` -- per image the k highest-scoring proposals (stable among equal scores) are matched greedily to the ground truths at each
    IoU threshold 0.50 : 0.05 : 0.95, ignored ground truths (`ignore2D`, or outside the area range) do not count -- and AR@k is
    `eval["recall"]` averaged over the thresholds.  (detectron2's proposal evaluation takes every ground truth's best overlap with any
    proposal instead, which lets one proposal cover two ground truths.)

    -> dict of fractions in [0, 1], NaN where no ground truth counts: 'AR@k', and by area of the ground truth (COCO's ranges: below
    32^2, up to 96^2, above) 'ARs@k', 'ARm@k', 'ARl@k', for every k; 'max_dets' the sorted budgets; 'eval' the `Omni3Deval`."""
    from .omni3d_evaluation import AnnotationIndex, Omni3Deval
    max_dets = sorted(int(k) for k in max_dets)
    if not max_dets or max_dets[0] < 1:
        raise ValueError("max_dets must hold positive integers")
    if not hasattr(gt, "getAnnIds"):
        anns, img_ids = _gt_records(gt)
        gt = AnnotationIndex(anns, img_ids)
    cat_ids = sorted(gt.getCatIds())
    if not cat_ids:
        raise ValueError("the ground truth has no category")
    recs = []
    for img_id, (boxes, scores) in proposals.items():
        boxes = np.asarray(boxes.detach().cpu() if hasattr(boxes, "detach") else boxes, dtype=np.float64).reshape(-1, 4)
        scores = np.asarray(scores.detach().cpu() if hasattr(scores, "detach") else scores, dtype=np.float64).reshape(-1)
        if len(boxes) != len(scores):
            raise ValueError("image %r: %d boxes and %d scores" % (img_id, len(boxes), len(scores)))
        for b, s in zip(boxes.tolist(), scores.tolist()):
            w, h = b[2] - b[0], b[3] - b[1]
            # the category is a place holder from the evaluated list: under useCats = 0 only membership in catIds matters
            recs.append({"image_id": img_id, "category_id": cat_ids[0], "bbox": [b[0], b[1], w, h], "area": w * h, "score": s})
    ev = Omni3Deval(gt, AnnotationIndex(recs, gt.getImgIds(), cat_ids), mode="2D")
    ev.params.useCats = 0
    ev.params.maxDets = list(max_dets)
    ev.evaluate(device=device)
    ev.accumulate()
    rec = ev.eval["recall"]                                    # (T, 1, A, M)
    out = {"max_dets": max_dets, "eval": ev}
    for short, label in _AREAS:
        a = ev.params.areaRngLbl.index(label)
        for m, k in enumerate(max_dets):
            v = rec[:, 0, a, m]
            out["AR%s@%d" % (short, k)] = float(np.mean(v[v > -1])) if (v > -1).any() else float("nan")
    return out


def proposal_recall_table(result):
    """the text table of a `proposal_recall` result: one line per budget"""
    lines = ["%8s %8s %8s %8s %8s" % ("maxDets", "AR", "AR-small", "AR-med", "AR-large")]
    for k in result["max_dets"]:
        lines.append("%8d %8.4f %8.4f %8.4f %8.4f" % ((k,) + tuple(result["AR%s@%d" % (s, k)] for s, _ in _AREAS)))
    return "\n".join(lines)
