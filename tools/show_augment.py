"""Shows what the training mapper's augmentation does to an Omni3D annotation file: runs `DatasetMapper3D(cfg, is_train=True)` with the
configured INPUT.CAMERA_ROTATION / INPUT.CROP / INPUT.COLOR_JITTER / resize / flip over the first --n images and draws every kept ground-truth cuboid on the
augmented image through the camera the mapper returns (`K` scaled by image height / `height`).  The boxes sit on their objects when
pixels, camera and 3D targets still belong together; under a crop or a camera rotation that is the point of looking.
    python tools/show_augment.py DATASET.json OUT_DIR [--n 8] [--seed 0] [--image-root DIR] [--config-file YAML] [KEY VALUE ...]
e.g. ... INPUT.CAMERA_ROTATION.ENABLED True INPUT.CROP.ENABLED True INPUT.COLOR_JITTER.ENABLED True.  Images are read from --image-root (default: the directory above the
JSON file's, the Omni3D layout datasets/Omni3D/<name>.json + datasets/<file_path>)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COLORS = [(0, 200, 200), (250, 100, 100), (100, 250, 100), (100, 100, 250), (250, 200, 50), (200, 50, 250)]


def camera_and_cuboids(out):
    """one mapper output -> (K of the output image: the returned `K` scaled by image height / `height`, [[X, Y, Z, w, h, l], ...] of the
    kept instances).  The centre is back-projected from the target's (u, v, z) through that K, as the training drawings do (rcnn3d.py):
    the mapper mirrors (u, v) and the pose under a flip but leaves `center_cam` as annotated, so the stored X would draw a flipped
    image's boxes at their mirror positions."""
    s = out["image"].shape[1] / out["height"]
    K = np.diag([s, s, 1.0]) @ np.asarray(out["K"], dtype=np.float64)
    inst = out.get("instances")
    boxes = []
    for g in ([] if inst is None else inst.gt_boxes3D.tolist()):          # [u, v, z, w, h, l, X, Y, Z]
        u, v, z = g[:3]
        boxes.append([z * (u - K[0, 2]) / K[0, 0], z * (v - K[1, 2]) / K[1, 1], z] + g[3:6])
    return K, boxes


def draw_record(out, image_format="BGR"):
    """one mapper output -> (HWC uint8 RGB image with its kept cuboids drawn, number drawn)"""
    from omni3d_amd.cubercnn.vis import vis
    from omni3d_amd.kernels import render
    im = out["image"].to(render.default_device()).contiguous()
    if image_format == "BGR":
        im = im.flip(0).contiguous()
    K, boxes = camera_and_cuboids(out)
    for i, box in enumerate(boxes):
        inst = out["instances"]
        im = vis.draw_3d_box(im, K, box, inst.gt_poses[i].numpy(), color=COLORS[int(inst.gt_classes[i]) % len(COLORS)], thickness=2)
    return np.ascontiguousarray(im.cpu().numpy().transpose(1, 2, 0)), len(boxes)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("dataset")
    ap.add_argument("out_dir")
    ap.add_argument("--n", type=int, default=8, help="number of images")
    ap.add_argument("--seed", type=int, default=0, help="seed of the augmentation's draws")
    ap.add_argument("--image-root", default=None)
    ap.add_argument("--config-file", default=None)
    args, opts = ap.parse_known_args(argv)                    # what is left: KEY VALUE pairs merged into the config last
    if len(opts) % 2 or any(o.startswith("--") for o in opts[0::2]):
        ap.error("unrecognized arguments: " + " ".join(opts))

    import torch
    from PIL import Image
    from omni3d_amd import lib
    from omni3d_amd.cubercnn import data
    from omni3d_amd.cubercnn.config import add_camera_rotation_config, add_color_jitter_config, get_cfg_defaults
    from omni3d_amd.d2.config import get_cfg
    from omni3d_amd.d2.data import MetadataCatalog

    cfg = get_cfg()
    get_cfg_defaults(cfg)
    add_color_jitter_config(cfg)
    add_camera_rotation_config(cfg)
    if args.config_file:
        cfg.merge_from_file(args.config_file)
    cfg.merge_from_list(opts)

    with open(args.dataset) as f:
        cats = sorted(json.load(f)["categories"], key=lambda c: c["id"])
    fs = data.get_filter_settings_from_cfg(cfg)
    fs["category_names"] = [c["name"] for c in cats]          # every category of the file, in the model's order (by id)
    MetadataCatalog.get("omni3d_model").set(thing_classes=fs["category_names"],
                                            thing_dataset_id_to_contiguous_id={c["id"]: k for k, c in enumerate(cats)})
    image_root = args.image_root or os.path.dirname(os.path.dirname(os.path.abspath(args.dataset)))
    name = os.path.splitext(os.path.basename(args.dataset))[0]
    records = data.load_omni3d_json(args.dataset, image_root, name, fs, filter_empty=True)[: max(args.n, 0)]

    device = torch.device("cpu" if lib.get().emulated else "cuda")
    mapper = data.DatasetMapper3D(cfg, is_train=True, device=device, rng=np.random.RandomState(args.seed))
    mapper.dataset_id_to_unknown_cats = {r["dataset_id"]: set() for r in records}
    os.makedirs(args.out_dir, exist_ok=True)
    written = []
    for k, rec in enumerate(records):
        out = mapper(rec)
        im, n = draw_record(out, cfg.INPUT.FORMAT)
        path = os.path.join(args.out_dir, "%04d_%s.png" % (k, out["image_id"]))
        Image.fromarray(im).save(path)
        written.append(path)
        print("%s: %d x %d, crop %s, %d of %d cuboids kept" % (path, im.shape[1], im.shape[0], out.get("crop"), n, len(rec["annotations"])))
    return written


if __name__ == "__main__":
    main()
