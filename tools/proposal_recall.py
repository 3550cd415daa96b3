"""Average recall of class-agnostic region proposals against a split's ground truth: `omni3d_amd.cubercnn.evaluation.proposal_recall`.

    python tools/proposal_recall.py GT.json PROPOSALS.json [--max-dets 10 100 1000]

GT.json: the split's annotation file ({"images": [...], "annotations": [...]}; annotations with `bbox` XYWH, or Omni3D's XYXY
`bbox2D_tight` / `bbox2D_proj` / `bbox2D_trunc`).  PROPOSALS.json: a list of {"image_id", "boxes": [[x1, y1, x2, y2], ...], "scores":
[...]}, one entry per image (several entries of one image are joined).  Printed: AR at every budget, overall and by the area of the
ground truth.  This is the COCO protocol's AR (greedy one-to-one matching, IoU 0.50 : 0.95), not detectron2's max-overlap recall."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_proposals(path):
    with open(path) as f:
        entries = json.load(f)
    out = {}
    for e in entries:
        boxes, scores = out.setdefault(e["image_id"], ([], []))
        boxes.extend(e["boxes"])
        scores.extend(e["scores"])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("gt")
    ap.add_argument("proposals")
    ap.add_argument("--max-dets", type=int, nargs="+", default=[10, 100, 1000])
    args = ap.parse_args(argv)
    from omni3d_amd.cubercnn.evaluation import proposal_recall, proposal_recall_table
    result = proposal_recall(args.gt, load_proposals(args.proposals), max_dets=args.max_dets)
    print(proposal_recall_table(result))
    return result


if __name__ == "__main__":
    main()
