"""tools/show_augment.py on the emulated library: the training mapper with crop + jitter over a synthetic on-disk dataset, the kept
cuboids drawn through the returned camera, --n images written."""
import importlib.util
import os

import numpy as np

from conftest import ROOT

NAMES = ["pedestrian", "car", "cyclist"]


def _tool():
    spec = importlib.util.spec_from_file_location("show_augment_tool", os.path.join(ROOT, "tools", "show_augment.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cuboids_are_drawn_on_their_objects_flipped_or_not(emu_lib):
    """One off-centre cuboid on a black image under crop + random flip: the drawn pixels lie inside the instance's transformed 2D box
    (the hull of the projected corners) and around its projected centre `gt_boxes3D[:, :2]`, on flipped and on unflipped outputs.  The
    cuboid's mirror position is 80 pixels away, so drawing from the unmirrored `center_cam` fails this on every flipped output."""
    import copy
    import torch
    import ref_augment as ref
    from test_mapper_augment import H, W, K0, _anno, _at, _cfg, _crop, _mapper
    tool = _tool()
    anno = _anno(_at(40, 50, 8.0), (1.0, 1.2, 0.8), 1)
    rec = {"image_array": np.zeros((H, W, 3), np.uint8), "height": H, "width": W, "K": copy.deepcopy(K0), "image_id": 1, "dataset_id": 0,
           "file_name": "memory://1", "annotations": [anno]}
    cfg = _cfg(*_crop("relative", (0.9, 0.9)), "INPUT.MIN_SIZE_TRAIN", (0, 162), "INPUT.RANDOM_FLIP", "horizontal")
    mapper = _mapper(cfg, torch.device("cpu"), 0)
    seen = set()
    for _ in range(12):
        out = mapper(rec)
        inst = out["instances"]
        assert len(inst) == 1
        flipped = float(inst.gt_poses[0, 0, 0]) < 0                   # the mapper mirrors the pose under a flip (identity -> diag(-1, 1, -1))
        seen.add((flipped, out["image"].shape[1] != out["height"]))
        K, boxes = tool.camera_and_cuboids(out)
        u, v = inst.gt_boxes3D[0, :2].tolist()
        assert np.allclose(ref.project(K, [boxes[0][:3]])[0], [u, v], atol=1e-4), "the cuboid's centre projects onto the target's (u, v)"
        im, n = tool.draw_record(out, "BGR")
        assert n == 1 and im.shape[:2] == tuple(out["image"].shape[1:])
        ys, xs = np.nonzero(im.any(axis=2))                           # the source is black: every lit pixel was drawn
        assert len(xs) > 20
        x1, y1, x2, y2 = inst.gt_boxes.tensor[0].tolist()
        assert x1 - 3 <= xs.min() and xs.max() <= x2 + 3 and y1 - 3 <= ys.min() and ys.max() <= y2 + 3, (flipped, (x1, y1, x2, y2), xs.min(), xs.max())
        assert xs.min() < u < xs.max() and ys.min() < v < ys.max()
        assert (u > im.shape[1] / 2) == flipped                       # the object is left of the centre; its mirror image is right of it
    assert {f for f, _ in seen} == {True, False} and {r for _, r in seen} == {True, False}


def test_show_augment_writes_the_augmented_images(emu_lib, tmp_path, capsys):
    from PIL import Image
    from omni3d_amd import synthetic
    from omni3d_amd.d2.data import MetadataCatalog
    path = synthetic.write_omni3d_dataset(str(tmp_path), "Synth_train", NAMES, [5, 2, 9], num_images=4, height=96, width=128, num_gt=3, seed=6)
    out_dir = str(tmp_path / "shown")
    saved = {k: MetadataCatalog.get(k) for k in ("omni3d_model", "Synth_train") if k in MetadataCatalog}
    try:
        tool = _tool()
        written = tool.main([path, out_dir, "--n", "3", "--seed", "4", "INPUT.CROP.ENABLED", "True", "INPUT.CROP.TYPE", "relative", "INPUT.CROP.SIZE",
                             "[0.75,0.5]", "INPUT.COLOR_JITTER.ENABLED", "True", "INPUT.MIN_SIZE_TRAIN", "(80,)", "INPUT.MAX_SIZE_TRAIN", "400"])
        plain = tool.main([path, str(tmp_path / "plain"), "--n", "1", "INPUT.MIN_SIZE_TRAIN", "(0,)", "INPUT.RANDOM_FLIP", "none"])
    finally:
        for k in ("omni3d_model", "Synth_train"):
            MetadataCatalog.pop(k, None)
        MetadataCatalog.update(saved)
    assert len(written) == 3 and sorted(os.listdir(out_dir)) == sorted(os.path.basename(p) for p in written)
    for p in written:
        with Image.open(p) as im:
            assert im.mode == "RGB" and im.size == (80, 90)           # 96 x 128 -> crop 72 x 64 -> short edge 80: 90 x 80
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "cuboids kept" in ln]
    assert len(lines) == 4 and all("crop (" in ln for ln in lines[:3]) and "crop None" in lines[3]
    # without augmentation the picture is the file's image plus the drawn cuboids: same size, some pixels painted
    with Image.open(plain[0]) as im, Image.open(os.path.join(str(tmp_path), "datasets", "Synth_train", "images", "000000.png")) as src:
        a, b = np.asarray(im), np.asarray(src.convert("RGB"))
    assert a.shape == b.shape == (96, 128, 3) and 0 < int((a != b).any(axis=2).sum()) < 96 * 128 // 2
