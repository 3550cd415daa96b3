"""Run a Cube R-CNN model on a folder of images and draw the predicted 3D boxes (reference demo/demo.py): for every image
`<name>_boxes.jpg` (the boxes over the image), `<name>_novel.jpg` (the scene from a second viewpoint, on the reference's ground
grid with --ground-grid) and `<name>.json` (the kept
detections: class name, score, center_cam, dimensions, pose, bbox3D) are written to cfg.OUTPUT_DIR.  Without a detection above the
threshold the untouched image is written as `<name>_boxes.jpg` only.

    python demo/demo.py --config-file configs/cubercnn_DLA34_FPN.yaml --input-folder images/ --threshold 0.25 \\
        MODEL.WEIGHTS model_final.pth OUTPUT_DIR output/demo

The category names are read from `category_meta.json` next to the config file (training writes it to its output directory).
Resize, model and drawing all run on the device; only image decoding / encoding and the text labels are host work."""
import argparse
import logging
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from omni3d_amd.cubercnn import util, vis  # noqa: E402
from omni3d_amd.cubercnn.config import add_nms3d_exact_config, add_tta_config, build_tta_model, get_cfg_defaults  # noqa: E402
from omni3d_amd.cubercnn.data.dataset_mapper import DatasetMapper3D  # noqa: E402
from omni3d_amd.d2.checkpoint import DetectionCheckpointer  # noqa: E402
from omni3d_amd.d2.config import get_cfg  # noqa: E402
from omni3d_amd.d2.engine import default_setup  # noqa: E402

logger = logging.getLogger("detectron2")


def do_test(args, cfg, model):
    list_of_ims = util.list_files(os.path.join(args.input_folder, ""), "*")
    model.eval()
    focal_length, principal_point, thres = args.focal_length, args.principal_point, args.threshold
    output_dir = cfg.OUTPUT_DIR
    device = next(model.parameters()).device
    mapper = DatasetMapper3D(cfg, is_train=False, device=device)         # the test-time ResizeShortestEdge, on csrc/resize.hip
    util.mkdir_if_missing(output_dir)
    category_path = os.path.join(util.file_parts(args.config_file)[0], "category_meta.json")
    if category_path.startswith(util.CubeRCNNHandler.PREFIX):
        category_path = util.CubeRCNNHandler._get_local_path(util.CubeRCNNHandler, category_path)
    cats = util.load_json(category_path)["thing_classes"]
    if getattr(args, "display", False):
        logger.info("--display is ignored: there is no window to show images in; see the files in {}".format(output_dir))

    for path in list_of_ims:
        im_name = util.file_parts(path)[1]
        im = util.imread(path)
        if im is None:
            continue
        h, w = im.shape[:2]
        # demo.py:66-79: focal length 4.0 in NDC units, principal point at the image centre.  Per image: the reference keeps the
        # first image's focal length for the rest of the folder, which is only right when all images have one height.
        f = 4.0 * h / 2 if focal_length == 0 else focal_length
        px, py = (w / 2, h / 2) if len(principal_point) == 0 else principal_point
        K = np.array([[f, 0.0, px], [0.0, f, py], [0.0, 0.0, 1.0]])

        _, out_hw, _ = mapper.sample_transforms(h, w)
        image = mapper.apply_image(im, out_hw, False)
        dets = model([{"image": image, "height": h, "width": w, "K": K}])[0]["instances"]

        meshes, meshes_text, rows = [], [], []
        for idx in range(len(dets)):
            score = float(dets.scores[idx])
            if score < thres:
                continue
            cat = cats[int(dets.pred_classes[idx])]
            center_cam, dimensions, pose = dets.pred_center_cam[idx].tolist(), dets.pred_dimensions[idx].tolist(), dets.pred_pose[idx].tolist()
            meshes_text.append("{} {:.2f}".format(cat, score))
            color = [c / 255.0 for c in util.get_color(idx)]
            meshes.append(util.mesh_cuboid(center_cam + dimensions, pose, color=color))
            rows.append({"category": cat, "score": score, "center_cam": center_cam, "dimensions": dimensions, "pose": pose,
                         "bbox3D": dets.pred_bbox3D[idx].tolist()})
        print("File: {} with {} dets".format(im_name, len(meshes)))
        util.save_json(os.path.join(output_dir, im_name + ".json"), rows)

        if len(meshes) > 0:
            im_drawn_rgb, im_topdown, _ = vis.draw_scene_view(im, K, meshes, text=meshes_text, scale=im.shape[0], blend_weight=0.5,
                                                              blend_weight_overlay=0.85, ground_grid=getattr(args, "ground_grid", False))
            util.imwrite(im_drawn_rgb, os.path.join(output_dir, im_name + "_boxes.jpg"))
            util.imwrite(im_topdown, os.path.join(output_dir, im_name + "_novel.jpg"))
        else:
            util.imwrite(im, os.path.join(output_dir, im_name + "_boxes.jpg"))


def setup(args):
    cfg = get_cfg()
    get_cfg_defaults(cfg)
    add_nms3d_exact_config(cfg)                   # TEST.NMS_3D.* with IOU_TYPE: settable from the YAML file and from `opts`
    add_tta_config(cfg)                           # TEST.AUG.*: test-time augmentation, likewise
    config_file = args.config_file
    if config_file.startswith(util.CubeRCNNHandler.PREFIX):
        config_file = util.CubeRCNNHandler._get_local_path(util.CubeRCNNHandler, config_file)
    cfg.merge_from_file(config_file)
    cfg.merge_from_list(args.opts)
    if getattr(args, "nms3d", None) is not None:
        cfg.merge_from_list(["TEST.NMS_3D.ENABLED", True, "TEST.NMS_3D.IOU_THRESH", float(args.nms3d)])
    if getattr(args, "nms3d_iou", None) is not None:
        cfg.merge_from_list(["TEST.NMS_3D.IOU_TYPE", args.nms3d_iou])
    if getattr(args, "tta", False):
        cfg.merge_from_list(["TEST.AUG.ENABLED", True])
    cfg.freeze()
    default_setup(cfg, args)
    return cfg


def main(args):
    import omni3d_amd.cubercnn.modeling.backbone  # noqa: F401  (registries)
    import omni3d_amd.cubercnn.modeling.proposal_generator  # noqa: F401
    import omni3d_amd.cubercnn.modeling.roi_heads  # noqa: F401
    from omni3d_amd.cubercnn.modeling.meta_arch import build_model
    cfg = setup(args)
    model = build_model(cfg)
    DetectionCheckpointer(model, save_dir=cfg.OUTPUT_DIR).resume_or_load(cfg.MODEL.WEIGHTS, resume=True)
    with torch.no_grad():
        do_test(args, cfg, build_tta_model(cfg, model))        # (the model itself unless TEST.AUG.ENABLED)


def argument_parser():
    parser = argparse.ArgumentParser(formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--config-file", default="", metavar="FILE", help="path to config file")
    parser.add_argument("--input-folder", type=str, help="folder of images to process", required=True)
    parser.add_argument("--focal-length", type=float, default=0, help="focal length for image inputs (in px)")
    parser.add_argument("--principal-point", type=float, default=[], nargs=2, help="principal point for image inputs (in px)")
    parser.add_argument("--threshold", type=float, default=0.25, help="threshold on score for visualizing")
    parser.add_argument("--ground-grid", default=False, action="store_true", help="draw the ground plane and its grid in the novel view")
    parser.add_argument("--nms3d", type=float, default=None, metavar="THRESH",
                        help="drop duplicate cuboids across categories by IoU3D above THRESH (TEST.NMS_3D.ENABLED True + IOU_THRESH)")
    parser.add_argument("--nms3d-iou", choices=("evaluator", "exact"), default=None,
                        help="IoU3D --nms3d decides with: the evaluator's pair algorithm, or exact geometry (TEST.NMS_3D.IOU_TYPE)")
    parser.add_argument("--tta", default=False, action="store_true",
                        help="test-time augmentation with the defaults of TEST.AUG: the image and its mirror image, cuboids fused (TEST.AUG.ENABLED True)")
    parser.add_argument("--display", default=False, action="store_true", help="accepted and ignored (logged)")
    parser.add_argument("opts", default=None, nargs=argparse.REMAINDER, help="'KEY VALUE' pairs that override the config")
    return parser


if __name__ == "__main__":
    args = argument_parser().parse_args()
    print("Command Line Args:", args)
    main(args)
