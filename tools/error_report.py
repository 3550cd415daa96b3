"""What is the AP lost to?  The error decomposition of `Omni3Deval.errors` (after TIDE, Bolya et al., ECCV 2020) for one ground-truth
file and one prediction file:

    python tools/error_report.py GT.json DT.json --mode 3D [--t-fg 0.25 --t-bg 0.05 --area all --json OUT.json]

GT.json: a COCO / Omni3D style dict with `annotations` (and optionally `images`, `categories`), or a plain list of annotation records;
DT.json: a list of prediction records (`image_id`, `category_id`, `score`, `bbox`, and in the cuboid modes `bbox3D`, `depth`), e.g. the
`omni_instances_results.json` the evaluator writes.  Prints one line per error type (count, dAP x 100) and, in the cuboid modes, the mean
translation / scale / orientation error of the poorly placed boxes; --json also writes the per-detection codes and the tables."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _jsonable(v):
    if isinstance(v, np.ndarray):
        return _jsonable(v.tolist())
    if isinstance(v, (list, tuple)):
        return [_jsonable(x) for x in v]
    if isinstance(v, (float, np.floating)):
        return float(v) if np.isfinite(v) else None
    if isinstance(v, np.integer):
        return int(v)
    return v


def main(argv=None):
    from omni3d_amd.cubercnn.evaluation.omni3d_evaluation import AnnotationIndex, Omni3Deval
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("gt")
    ap.add_argument("dt")
    ap.add_argument("--mode", default="3D", choices=["2D", "3D", "BEV", "LET"])
    ap.add_argument("--t-fg", type=float, default=None)
    ap.add_argument("--t-bg", type=float, default=None)
    ap.add_argument("--area", default="all")
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    with open(args.gt) as f:
        gt = json.load(f)
    with open(args.dt) as f:
        dts = json.load(f)
    anns = gt["annotations"] if isinstance(gt, dict) else gt
    img_ids = [im["id"] for im in gt["images"]] if isinstance(gt, dict) and "images" in gt else None
    cat_ids = [c["id"] for c in gt["categories"]] if isinstance(gt, dict) and "categories" in gt else None
    g = AnnotationIndex(anns, img_ids, cat_ids)
    ev = Omni3Deval(g, AnnotationIndex(dts, g.getImgIds(), g.getCatIds()), mode=args.mode)
    ev.evaluate()
    res = ev.errors(t_fg=args.t_fg, t_bg=args.t_bg, area=args.area)
    print(ev.summarize_errors())
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"mode": args.mode, "cat_ids": _jsonable(ev.params.catIds), **{k: _jsonable(v) for k, v in res.items()}}, f)
    return 0


if __name__ == "__main__":
    sys.exit(main())
