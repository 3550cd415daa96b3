"""Cube R-CNN config keys added on top of the detectron2 defaults.  Same keys and default values
as /root/reference/cubercnn/config/config.py:4-158 (the YAML files under configs/ rely on them)."""
from ...d2.config import CfgNode as CN

_ADDED = {
    "DATASETS.CATEGORY_NAMES": [], "DATASETS.IGNORE_NAMES": [], "DATALOADER.BALANCE_DATASETS": False,
    "DATASETS.TRUNCATION_THRES": 0.99, "DATASETS.VISIBILITY_THRES": 0.01, "DATASETS.MIN_HEIGHT_THRES": 0.00,
    "DATASETS.MAX_DEPTH": 1e8, "DATASETS.MODAL_2D_BOXES": False, "DATASETS.TRUNC_2D_BOXES": True,
    "MODEL.RPN.IGNORE_THRESHOLD": 0.5,
    "MODEL.ROI_CUBE_HEAD": CN, "MODEL.ROI_CUBE_HEAD.NAME": "CubeHead", "MODEL.ROI_CUBE_HEAD.POOLER_RESOLUTION": 7,
    "MODEL.ROI_CUBE_HEAD.POOLER_SAMPLING_RATIO": 0, "MODEL.ROI_CUBE_HEAD.POOLER_TYPE": "ROIAlignV2",
    "MODEL.ROI_CUBE_HEAD.NUM_CONV": 0, "MODEL.ROI_CUBE_HEAD.CONV_DIM": 256, "MODEL.ROI_CUBE_HEAD.NUM_FC": 2,
    "MODEL.ROI_CUBE_HEAD.FC_DIM": 1024, "MODEL.ROI_CUBE_HEAD.Z_TYPE": "direct", "MODEL.ROI_CUBE_HEAD.POSE_TYPE": "6d",
    "MODEL.ROI_CUBE_HEAD.INVERSE_Z_WEIGHT": False, "MODEL.ROI_CUBE_HEAD.VIRTUAL_DEPTH": True,
    "MODEL.ROI_CUBE_HEAD.VIRTUAL_FOCAL": 512.0, "MODEL.ROI_CUBE_HEAD.DISENTANGLED_LOSS": True,
    "MODEL.ROI_CUBE_HEAD.CLUSTER_BINS": 1, "MODEL.USE_BN": True, "MODEL.ROI_CUBE_HEAD.ALLOCENTRIC_POSE": True,
    "MODEL.ROI_CUBE_HEAD.CHAMFER_POSE": True, "MODEL.ROI_CUBE_HEAD.SHARED_FC": True, "MODEL.STABILIZE": 0.01,
    "MODEL.ROI_CUBE_HEAD.DIMS_PRIORS_ENABLED": True, "MODEL.ROI_CUBE_HEAD.DIMS_PRIORS_FUNC": "exp",
    "MODEL.ROI_CUBE_HEAD.USE_CONFIDENCE": 1.0, "MODEL.ROI_CUBE_HEAD.LOSS_W_3D": 1.0, "MODEL.ROI_CUBE_HEAD.LOSS_W_XY": 1.0,
    "MODEL.ROI_CUBE_HEAD.LOSS_W_Z": 1.0, "MODEL.ROI_CUBE_HEAD.LOSS_W_DIMS": 1.0, "MODEL.ROI_CUBE_HEAD.LOSS_W_POSE": 1.0,
    "MODEL.DLA": CN, "MODEL.DLA.TYPE": "dla34", "MODEL.DLA.TRICKS": False, "MODEL.ROI_CUBE_HEAD.LOSS_W_JOINT": 1.0,
    "SOLVER.TYPE": "sgd", "MODEL.RESNETS.TORCHVISION": True, "TEST.DETECTIONS_PER_IMAGE": 100,
    "TEST.VISIBILITY_THRES": 1 / 2.0, "TEST.TRUNCATION_THRES": 1 / 2.0, "INPUT.RANDOM_FLIP": "horizontal",
    "MODEL.RPN.OBJECTNESS_UNCERTAINTY": "IoUness", "MODEL.ROI_CUBE_HEAD.SCALE_ROI_BOXES": 0.0,
    "MODEL.WEIGHTS_PRETRAIN": "",
}


def get_cfg_defaults(cfg):
    for key, value in _ADDED.items():
        node = cfg
        parts = key.split(".")
        for p in parts[:-1]:
            node = node[p]
        node[parts[-1]] = CN() if value is CN else (list(value) if isinstance(value, list) else value)
    return cfg


_NMS_3D = {"ENABLED": False, "IOU_THRESH": 0.25, "CLASS_AGNOSTIC": True}


def add_nms3d_config(cfg):
    """TEST.NMS_3D.*: suppression of duplicate cuboids by IoU3D at inference (csrc/iou_box3d.hip, omni_nms3d).  The reference has no
    such step and `get_cfg_defaults` stays key for key what the reference defines, so -- detectron2's convention for project keys --
    the node is added by this call; a cfg without it builds a model with the feature off.  Idempotent: values already set are kept.
    IOU_THRESH 0.25 is a convention, the middle of the evaluator's 0.05 .. 0.5 IoU3D range, not a measured optimum."""
    if "NMS_3D" not in cfg.TEST:
        cfg.TEST.NMS_3D = CN()
    for key, value in _NMS_3D.items():
        cfg.TEST.NMS_3D.setdefault(key, value)
    return cfg
