"""`evaluation.proposal_recall` and tools/proposal_recall.py on three images scored by hand.

Ground truths (XYWH; COCO's area ranges: small < 32^2, medium up to 96^2, large above) and proposals (XYXY, objectness):
  image 1: G1 20 x 20 (small), G2 50 x 50 at (100, 100) (medium); P1 = G1 at 0.9 (IoU 1), P2 = the upper 50 x 36 of G2 at 0.8
           (IoU 1800 / 2500 = 0.72: a match at the thresholds 0.50 .. 0.70, five of the ten, none at 0.75 .. 0.95);
  image 2: G3 200 x 100 (large); P3 far away at 0.95 (IoU 0), P4 = G3 at 0.5 (IoU 1);
  image 3: G4 40 x 40 with ignore2D (does not count), G5 100 x 100 (large) without any proposal; P5 = G4 at 0.7.
Counted ground truths: 4 (small 1, medium 1, large 2).
  k = 1 (P1, P3, P5): G1 found at every threshold                       -> AR 1/4, small 1, medium 0, large 0
  k = 2: G1 and G3 at every threshold, G2 at five of ten                -> AR (5 x 3/4 + 5 x 2/4) / 10 = 0.625, small 1, medium 0.5, large 0.5"""
import importlib.util
import json
import os

import pytest

from conftest import ROOT

GTS = [{"id": 1, "image_id": 1, "category_id": 3, "bbox": [0, 0, 20, 20], "area": 400.0, "ignore2D": 0},
       {"id": 2, "image_id": 1, "category_id": 8, "bbox": [100, 100, 50, 50], "area": 2500.0, "ignore2D": 0},
       {"id": 3, "image_id": 2, "category_id": 8, "bbox": [0, 0, 200, 100], "area": 20000.0, "ignore2D": 0},
       {"id": 4, "image_id": 3, "category_id": 5, "bbox": [10, 10, 40, 40], "area": 1600.0, "ignore2D": 1},
       {"id": 5, "image_id": 3, "category_id": 3, "bbox": [300, 300, 100, 100], "area": 10000.0, "ignore2D": 0}]
PROPOSALS = {1: ([[0, 0, 20, 20], [100, 100, 150, 136]], [0.9, 0.8]),
             2: ([[500, 500, 510, 510], [0, 0, 200, 100]], [0.95, 0.5]),
             3: ([[10, 10, 50, 50]], [0.7])}
WANT = {"AR@1": 0.25, "ARs@1": 1.0, "ARm@1": 0.0, "ARl@1": 0.0, "AR@2": 0.625, "ARs@2": 1.0, "ARm@2": 0.5, "ARl@2": 0.5}


def _check(result):
    assert result["max_dets"] == [1, 2]
    for key, want in WANT.items():
        assert abs(result[key] - want) <= 1e-15, (key, result[key], want)
    assert result["eval"].eval["recall"].shape == (10, 1, 4, 2)


def _run(tmp_path, capsys):
    import copy
    from omni3d_amd.cubercnn.evaluation import AnnotationIndex, proposal_recall
    dataset = {"images": [{"id": i} for i in (1, 2, 3)], "annotations": GTS}
    _check(proposal_recall(copy.deepcopy(dataset), PROPOSALS, max_dets=(2, 1)))
    _check(proposal_recall(AnnotationIndex(copy.deepcopy(GTS), [1, 2, 3]), PROPOSALS, max_dets=(1, 2)))
    # Omni3D's XYXY boxes stand in for a missing `bbox`
    omni = copy.deepcopy(dataset)
    for a in omni["annotations"]:
        x, y, w, h = a.pop("bbox")
        a.pop("area")
        a["ignore"] = bool(a.pop("ignore2D"))
        a["bbox2D_tight"], a["bbox2D_proj"] = [-1, -1, -1, -1], [x, y, x + w, y + h]
    _check(proposal_recall(omni, PROPOSALS, max_dets=(1, 2)))
    with pytest.raises(ValueError, match="max_dets"):
        proposal_recall(copy.deepcopy(dataset), PROPOSALS, max_dets=(0, 1))
    # the tool prints the same numbers
    gt_path, prop_path = str(tmp_path / "gt.json"), str(tmp_path / "proposals.json")
    with open(gt_path, "w") as f:
        json.dump(dataset, f)
    with open(prop_path, "w") as f:                                       # image 1 in two entries: they are joined
        json.dump([{"image_id": 1, "boxes": PROPOSALS[1][0][:1], "scores": PROPOSALS[1][1][:1]},
                   {"image_id": 2, "boxes": PROPOSALS[2][0], "scores": PROPOSALS[2][1]},
                   {"image_id": 1, "boxes": PROPOSALS[1][0][1:], "scores": PROPOSALS[1][1][1:]},
                   {"image_id": 3, "boxes": PROPOSALS[3][0], "scores": PROPOSALS[3][1]}], f)
    spec = importlib.util.spec_from_file_location("proposal_recall_tool", os.path.join(ROOT, "tools", "proposal_recall.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    capsys.readouterr()
    _check(tool.main([gt_path, prop_path, "--max-dets", "1", "2"]))
    rows = [line.split() for line in capsys.readouterr().out.strip().splitlines()]
    assert rows[0] == ["maxDets", "AR", "AR-small", "AR-med", "AR-large"]
    assert [[float(v) for v in r] for r in rows[1:]] == [[1, 0.25, 1.0, 0.0, 0.0], [2, 0.625, 1.0, 0.5, 0.5]]


def test_three_images_by_hand_emulated(emu_lib, tmp_path, capsys):
    _run(tmp_path, capsys)


@pytest.mark.gpu
def test_three_images_by_hand_gpu(hip_lib, tmp_path, capsys):
    _run(tmp_path, capsys)
