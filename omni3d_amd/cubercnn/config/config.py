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
    """TEST.NMS_3D.*: suppression of duplicate cuboids by IoU3D at inference (csrc/nms3d.hip, omni_nms3d).  The reference has no
    such step and `get_cfg_defaults` stays key for key what the reference defines, so -- detectron2's convention for project keys --
    the node is added by this call; a cfg without it builds a model with the feature off.  Idempotent: values already set are kept.
    IOU_THRESH 0.25 is a convention, the middle of the evaluator's 0.05 .. 0.5 IoU3D range, not a measured optimum."""
    if "NMS_3D" not in cfg.TEST:
        cfg.TEST.NMS_3D = CN()
    for key, value in _NMS_3D.items():
        cfg.TEST.NMS_3D.setdefault(key, value)
    return cfg


NMS_3D_IOU_TYPES = ("evaluator", "exact")


def add_nms3d_exact_config(cfg):
    """`add_nms3d_config` plus TEST.NMS_3D.IOU_TYPE: which IoU3D the suppression decides with.  "evaluator" (the default) is the
    pair algorithm AP3D is computed with (omni_nms3d); "exact" is the exact geometry of the cuboids fitted to the corners
    (omni_nms3d_exact, csrc/cuboid_exact.h), right on the near-aligned duplicates the evaluator's algorithm misjudges by up to 0.3.
    A separate call because `add_nms3d_config` keeps adding exactly its three keys; a cfg without the key builds a model that decides
    as before.  Idempotent: values already set are kept."""
    add_nms3d_config(cfg)
    cfg.TEST.NMS_3D.setdefault("IOU_TYPE", NMS_3D_IOU_TYPES[0])
    return cfg


_EVAL_BEV = {"ENABLED": False, "UP": [0.0, -1.0, 0.0]}


def add_bev_eval_config(cfg):
    """TEST.EVAL_BEV.*: AP in the bird's-eye view next to AP2D / AP3D (`Omni3Deval(mode="BEV")`, csrc/bev_iou.hip): detections are
    matched by the IoU of the cuboids' footprints on the ground plane, under the 3D protocol otherwise.  The reference has no such
    mode and `get_cfg_defaults` stays key for key what the reference defines, so, as with `add_nms3d_config`, the node is absent
    until this call; without it nothing is evaluated in BEV.  Idempotent: values already set are kept.
    UP is the up vector of the ground plane IN THE CAMERA FRAME, one for the whole evaluation.  [0, -1, 0] (camera y points down)
    is the right ground plane for the outdoor splits (KITTI, nuScenes), whose cameras are level with the road.  For indoor splits
    with a pitched camera a single camera-frame vector is an approximation the user chooses knowingly."""
    if "EVAL_BEV" not in cfg.TEST:
        cfg.TEST.EVAL_BEV = CN()
    for key, value in _EVAL_BEV.items():
        cfg.TEST.EVAL_BEV.setdefault(key, list(value) if isinstance(value, list) else value)
    return cfg


def bev_eval_args(cfg):
    """TEST.EVAL_BEV -> the keyword arguments of `Omni3DEvaluationHelper` / `Omni3DEvaluator`:
    `Omni3DEvaluationHelper(names, filter_settings, folder, **bev_eval_args(cfg))`.  A cfg without the node: the feature off."""
    node = cfg.TEST.get("EVAL_BEV")
    if node is None:
        return {"eval_bev": False, "bev_up": tuple(_EVAL_BEV["UP"])}
    up = tuple(float(v) for v in node.UP)
    if len(up) != 3:
        raise ValueError("TEST.EVAL_BEV.UP must hold three numbers")
    return {"eval_bev": bool(node.ENABLED), "bev_up": up}


_EVAL_KITTI = {"ENABLED": False, "OCC_CUTS": [0.75, 0.5, 0.25], "DC_METRICS": ["2D", "BEV", "3D"], "R11": False}


def add_kitti_eval_config(cfg):
    """TEST.EVAL_KITTI.*: the KITTI object benchmark's own protocol next to AP2D / AP3D (`cubercnn.evaluation.kitti.KittiEval`,
    csrc/eval_kitti.hip): AP|R40 of the 2D box, the bird's-eye view and the 3D box at Easy / Moderate / Hard for car, pedestrian and
    cyclist.  The reference has no such pass and `get_cfg_defaults` stays key for key what the reference defines, so, as with
    `add_bev_eval_config`, the node is absent until this call; without it nothing is evaluated this way.  Idempotent: values already
    set are kept.
    OCC_CUTS: the visibility cuts that make the occlusion level (a convention of this project, see `KittiParams`); DC_METRICS: the
    metrics in which DontCare regions absorb false positives; R11: also report the 11-point AP."""
    if "EVAL_KITTI" not in cfg.TEST:
        cfg.TEST.EVAL_KITTI = CN()
    for key, value in _EVAL_KITTI.items():
        cfg.TEST.EVAL_KITTI.setdefault(key, list(value) if isinstance(value, list) else value)
    return cfg


def kitti_eval_args(cfg):
    """TEST.EVAL_KITTI -> the keyword arguments of `Omni3DEvaluationHelper` / `Omni3DEvaluator`:
    `Omni3DEvaluationHelper(names, filter_settings, folder, **kitti_eval_args(cfg))`.  A cfg without the node: the feature off."""
    node = cfg.TEST.get("EVAL_KITTI")
    if node is None:
        node = _EVAL_KITTI
        get = node.__getitem__
    else:
        get = lambda k: getattr(node, k)      # noqa: E731
    cuts, dc = tuple(float(v) for v in get("OCC_CUTS")), tuple(str(v) for v in get("DC_METRICS"))
    if any(m not in ("2D", "BEV", "3D") for m in dc):
        raise ValueError("TEST.EVAL_KITTI.DC_METRICS must be taken from 2D, BEV, 3D")
    if list(cuts) != sorted(cuts, reverse=True):
        raise ValueError("TEST.EVAL_KITTI.OCC_CUTS must descend")
    return {"eval_kitti": bool(get("ENABLED")), "kitti_params": {"occCuts": cuts, "dcMetrics": dc}, "kitti_r11": bool(get("R11"))}


def add_kitti_aos_config(cfg):
    """`add_kitti_eval_config` plus TEST.EVAL_KITTI.AOS (default False): also report the benchmark's average orientation similarity
    (`KittiParams.aos`; 'AOS|R40-car-moderate', ... in `bbox_KITTI` and the `aos` line of the table).  A separate call, as with
    `add_nms3d_exact_config`, because `add_kitti_eval_config` keeps adding exactly its four keys.  Idempotent: values already set are kept."""
    add_kitti_eval_config(cfg)
    cfg.TEST.EVAL_KITTI.setdefault("AOS", False)
    return cfg


def kitti_aos_eval_args(cfg):
    """`kitti_eval_args(cfg)` with `kitti_params["aos"]` = TEST.EVAL_KITTI.AOS (False for a cfg without the key)"""
    args = kitti_eval_args(cfg)
    node = cfg.TEST.get("EVAL_KITTI")
    args["kitti_params"]["aos"] = bool(node.get("AOS", False)) if node is not None else False
    return args


_EVAL_DIST = {"ENABLED": False, "UP": [], "DIST_THRS": [0.5, 1.0, 2.0, 4.0], "TP_DIST": 2.0, "MIN_RECALL": 0.1}


def add_dist_eval_config(cfg):
    """TEST.EVAL_DIST.*: the centre-distance protocol of nuScenes next to AP2D / AP3D (`Omni3Deval(mode="DIST")`, csrc/tp_errors.hip):
    detections are matched by the distance of the fitted centres, under the 3D protocol otherwise, and the matched pairs are scored
    for translation, scale and orientation error along the recall curve (ATE / ASE / AOE).  The reference has no such mode and
    `get_cfg_defaults` stays key for key what the reference defines, so, as with `add_bev_eval_config`, the node is absent until this
    call; without it nothing is evaluated by distance.  Idempotent: values already set are kept.
    UP: empty = the full 3D distance (Omni3D has no world frame; indoor cameras are pitched), else the three components of the up
    vector IN THE CAMERA FRAME, and the distance is taken in the ground plane orthogonal to it ([0, -1, 0] for the level outdoor
    cameras, nuScenes' definition).  DIST_THRS: the matching thresholds in metres; TP_DIST: the one of them at which the three
    errors are taken; MIN_RECALL: the recall below which they are not averaged.  The defaults are nuScenes'."""
    if "EVAL_DIST" not in cfg.TEST:
        cfg.TEST.EVAL_DIST = CN()
    for key, value in _EVAL_DIST.items():
        cfg.TEST.EVAL_DIST.setdefault(key, list(value) if isinstance(value, list) else value)
    return cfg


def dist_eval_args(cfg):
    """TEST.EVAL_DIST -> the keyword arguments of `Omni3DEvaluationHelper` / `Omni3DEvaluator`:
    `Omni3DEvaluationHelper(names, filter_settings, folder, **dist_eval_args(cfg))`.  A cfg without the node: the feature off.
    ValueError when UP holds neither none nor three numbers, or TP_DIST is not one of DIST_THRS."""
    node = cfg.TEST.get("EVAL_DIST")
    if node is None:
        node = _EVAL_DIST
    get = (lambda k: node[k]) if isinstance(node, dict) else (lambda k: getattr(node, k))       # noqa: E731
    up = tuple(float(v) for v in get("UP"))
    if len(up) not in (0, 3):
        raise ValueError("TEST.EVAL_DIST.UP must be empty or hold three numbers")
    thrs = [float(v) for v in get("DIST_THRS")]
    if float(get("TP_DIST")) not in thrs:
        raise ValueError("TEST.EVAL_DIST.TP_DIST must be one of DIST_THRS")
    return {"eval_dist": bool(get("ENABLED")), "dist_up": up if up else None,
            "dist_params": {"distThrs": thrs, "tpDist": float(get("TP_DIST")), "minRecall": float(get("MIN_RECALL"))}}


_EVAL_LET = {"ENABLED": False, "LON_TOL_FRAC": 0.1, "LON_TOL_MIN": 0.5}


def add_let_eval_config(cfg):
    """TEST.EVAL_LET.*: the longitudinal-error-tolerant metrics of the Waymo camera-only benchmark next to AP2D / AP3D
    (`Omni3Deval(mode="LET")`, csrc/let_iou.hip): a detection may slide along its own line of sight onto the ground truth, the exact
    IoU3D of the slid box decides the match under the 3D protocol (LET-AP), and LET-APL scales precision by how little sliding was
    needed.  The reference has no such mode and `get_cfg_defaults` stays key for key what the reference defines, so, as with
    `add_dist_eval_config`, the node is absent until this call; without it nothing is evaluated this way.  Idempotent: values already
    set are kept.
    LON_TOL_FRAC / LON_TOL_MIN: the slide may be as long as max(LON_TOL_FRAC x the range of the ground truth, LON_TOL_MIN metres).  The
    defaults are Waymo's, taken as a convention."""
    if "EVAL_LET" not in cfg.TEST:
        cfg.TEST.EVAL_LET = CN()
    for key, value in _EVAL_LET.items():
        cfg.TEST.EVAL_LET.setdefault(key, value)
    return cfg


def let_eval_args(cfg):
    """TEST.EVAL_LET -> the keyword arguments of `Omni3DEvaluationHelper` / `Omni3DEvaluator`:
    `Omni3DEvaluationHelper(names, filter_settings, folder, **let_eval_args(cfg))`.  A cfg without the node: the feature off.
    ValueError unless LON_TOL_FRAC is finite and >= 0 and LON_TOL_MIN finite and > 0."""
    import math
    node = cfg.TEST.get("EVAL_LET")
    if node is None:
        node = _EVAL_LET
    get = (lambda k: node[k]) if isinstance(node, dict) else (lambda k: getattr(node, k))       # noqa: E731
    try:
        frac, tmin = float(get("LON_TOL_FRAC")), float(get("LON_TOL_MIN"))
    except (TypeError, ValueError):
        raise ValueError("TEST.EVAL_LET.LON_TOL_FRAC / LON_TOL_MIN must be numbers") from None
    if not (math.isfinite(frac) and frac >= 0.0):
        raise ValueError("TEST.EVAL_LET.LON_TOL_FRAC must be finite and >= 0")
    if not (math.isfinite(tmin) and tmin > 0.0):
        raise ValueError("TEST.EVAL_LET.LON_TOL_MIN must be finite and > 0")
    return {"eval_let": bool(get("ENABLED")), "let_params": {"lonTolFrac": frac, "lonTolMin": tmin}}


_BOOTSTRAP = {"ENABLED": False, "NUM_REPLICATES": 1000, "SEED": 0, "CONFIDENCE": 0.95}


def add_bootstrap_config(cfg):
    """TEST.BOOTSTRAP.*: image-level bootstrap confidence intervals next to every AP the evaluation reports (`Omni3Deval.bootstrap`,
    csrc/eval_bootstrap.hip): the test images are resampled with replacement NUM_REPLICATES times (generator seeded with SEED), AP is
    recomputed for each replicate from the one set of match tables, and the percentile interval at CONFIDENCE is reported.  The
    reference has no such option and `get_cfg_defaults` stays key for key what the reference defines, so, as with
    `add_let_eval_config`, the node is absent until this call; without it no interval is computed.  Idempotent: values already set
    are kept.  1000 replicates and 95 % are the customary choices, not tuned values."""
    if "BOOTSTRAP" not in cfg.TEST:
        cfg.TEST.BOOTSTRAP = CN()
    for key, value in _BOOTSTRAP.items():
        cfg.TEST.BOOTSTRAP.setdefault(key, value)
    return cfg


def bootstrap_eval_args(cfg):
    """TEST.BOOTSTRAP -> the keyword argument of `Omni3DEvaluationHelper` / `Omni3DEvaluator`:
    `Omni3DEvaluationHelper(names, filter_settings, folder, **bootstrap_eval_args(cfg))`.  A cfg without the node, or ENABLED False:
    {"bootstrap": None}, the feature off.  ValueError unless NUM_REPLICATES is an integer >= 1, SEED an integer >= 0 and CONFIDENCE
    lies in (0, 1)."""
    node = cfg.TEST.get("BOOTSTRAP")
    if node is None:
        node = _BOOTSTRAP
    get = (lambda k: node[k]) if isinstance(node, dict) else (lambda k: getattr(node, k))       # noqa: E731
    n, seed, conf = get("NUM_REPLICATES"), get("SEED"), get("CONFIDENCE")
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError("TEST.BOOTSTRAP.NUM_REPLICATES must be an integer >= 1")
    if isinstance(seed, bool) or not isinstance(seed, int) or seed < 0:
        raise ValueError("TEST.BOOTSTRAP.SEED must be an integer >= 0")
    if isinstance(conf, bool) or not isinstance(conf, (int, float)) or not 0.0 < float(conf) < 1.0:
        raise ValueError("TEST.BOOTSTRAP.CONFIDENCE must lie in (0, 1)")
    if not bool(get("ENABLED")):
        return {"bootstrap": None}
    return {"bootstrap": {"n": n, "seed": seed, "confidence": float(conf)}}


_ERRORS = {"ENABLED": False, "T_FG": [], "T_BG": []}


def add_error_analysis_config(cfg):
    """TEST.ERRORS.*: the error decomposition next to every AP the evaluation reports (`Omni3Deval.errors`, csrc/eval_errors.hip; after
    TIDE, Bolya et al., ECCV 2020): every false positive is typed as wrong class, poor box, both, duplicate or background, every unfound
    ground truth is a miss, and each type is priced by the AP an oracle repairing it alone would gain.  The reference has no such option
    and `get_cfg_defaults` stays key for key what the reference defines, so, as with `add_bootstrap_config`, the node is absent until
    this call; without it nothing is analysed.  Idempotent: values already set are kept.
    T_FG / T_BG: empty = the defaults of each mode (0.5 / 0.1 in 2D, 0.25 / 0.05 in the modes of the 3D protocol: conventions, not
    tuned values); otherwise one number each, applied to every mode of the 3D protocol -- mode 2D keeps its own."""
    if "ERRORS" not in cfg.TEST:
        cfg.TEST.ERRORS = CN()
    for key, value in _ERRORS.items():
        cfg.TEST.ERRORS.setdefault(key, list(value) if isinstance(value, list) else value)
    return cfg


def error_eval_args(cfg):
    """TEST.ERRORS -> the keyword argument of `Omni3DEvaluationHelper` / `Omni3DEvaluator`:
    `Omni3DEvaluationHelper(names, filter_settings, folder, **error_eval_args(cfg))`.  A cfg without the node, or ENABLED False:
    {"errors": None}, the feature off.  ValueError unless T_FG / T_BG are empty or hold one number in (0, 1) each, T_BG below T_FG."""
    import math
    node = cfg.TEST.get("ERRORS")
    if node is None:
        node = _ERRORS
    get = (lambda k: node[k]) if isinstance(node, dict) else (lambda k: getattr(node, k))       # noqa: E731
    out = {}
    for key, name in (("T_FG", "t_fg"), ("T_BG", "t_bg")):
        try:
            values = [float(v) for v in get(key)]
        except (TypeError, ValueError):
            raise ValueError("TEST.ERRORS.%s must be empty or hold one number" % key) from None
        if len(values) > 1 or any(not (math.isfinite(v) and 0.0 < v < 1.0) for v in values):
            raise ValueError("TEST.ERRORS.%s must be empty or hold one number in (0, 1)" % key)
        if values:
            out[name] = values[0]
    if "t_fg" in out and "t_bg" in out and not out["t_bg"] < out["t_fg"]:
        raise ValueError("TEST.ERRORS.T_BG must be below T_FG")
    return {"errors": out if bool(get("ENABLED")) else None}


_EVAL_AGNOSTIC = {"ENABLED": False}


def add_agnostic_eval_config(cfg):
    """TEST.EVAL_AGNOSTIC.*: class-agnostic AP and AR next to every AP the evaluation reports (`Omni3Deval` with `params.useCats = 0`,
    csrc/eval_accumulate_par.hip): every enabled mode is evaluated a second time with one group per image and the categories ignored --
    is the cuboid wrong, or only its label?  The reference's evaluator has the switch but no config key, and `get_cfg_defaults` stays key
    for key what the reference defines, so, as with `add_bev_eval_config`, the node is absent until this call; without it nothing is
    evaluated class-agnostically.  Idempotent: values already set are kept."""
    if "EVAL_AGNOSTIC" not in cfg.TEST:
        cfg.TEST.EVAL_AGNOSTIC = CN()
    for key, value in _EVAL_AGNOSTIC.items():
        cfg.TEST.EVAL_AGNOSTIC.setdefault(key, value)
    return cfg


def agnostic_eval_args(cfg):
    """TEST.EVAL_AGNOSTIC -> the keyword argument of `Omni3DEvaluationHelper` / `Omni3DEvaluator`:
    `Omni3DEvaluationHelper(names, filter_settings, folder, **agnostic_eval_args(cfg))`.  A cfg without the node: the feature off."""
    node = cfg.TEST.get("EVAL_AGNOSTIC")
    return {"eval_agnostic": False if node is None else bool(node.ENABLED)}


_TTA = {"MIN_SIZES": (), "MAX_SIZE": 4000, "FLIP": True, "FUSE_IOU_THRESH": 0.5, "CLASS_AGNOSTIC": False}


def add_tta_config(cfg):
    """TEST.AUG.*: test-time augmentation (`RCNN3DWithTTA`, meta_arch/tta.py): the image is run at several sizes and mirrored, the
    views' cuboids are brought into one camera frame and overlapping ones are fused into one (csrc/nms3d.hip, omni_fuse3d).
    detectron2 defines the node and its first three keys; `get_cfg_defaults` carries it as {"ENABLED": False}, so the keys are added to
    the existing node by this call.  Idempotent: values already set are kept.
    MIN_SIZES: the shorter sides of the views, capped by MAX_SIZE (detectron2's default 4000); () = the size the loader delivered only.
    FLIP doubles the views.  FUSE_IOU_THRESH: cuboids of exact IoU3D above it are one object; 0.5 is a convention (the loosest
    threshold at which two boxes are commonly called the same detection), not a tuned value.  CLASS_AGNOSTIC False: the views of one
    object should agree on its class.  Whether any of this raises AP3D on real data has not been measured."""
    if "AUG" not in cfg.TEST:
        cfg.TEST.AUG = CN({"ENABLED": False})
    cfg.TEST.AUG.setdefault("ENABLED", False)
    for key, value in _TTA.items():
        cfg.TEST.AUG.setdefault(key, value)
    return cfg


def tta_args(cfg):
    """TEST.AUG -> the keyword arguments of `RCNN3DWithTTA`: `RCNN3DWithTTA(cfg, model)` reads them through this.  Keys the node does
    not carry (a cfg without `add_tta_config`) take their defaults.  ValueError unless MIN_SIZES is a sequence of integers > 0,
    MAX_SIZE an integer > 0 and FUSE_IOU_THRESH a finite number >= 0."""
    import math
    node = cfg.TEST.get("AUG")
    have = dict(node) if node is not None else {}
    get = lambda k: have.get(k, _TTA.get(k, False))       # noqa: E731
    sizes = get("MIN_SIZES")
    if isinstance(sizes, (str, bytes)) or not hasattr(sizes, "__iter__"):
        raise ValueError("TEST.AUG.MIN_SIZES must be a sequence of integers")
    sizes = tuple(sizes)
    if any(isinstance(v, bool) or not isinstance(v, int) or v <= 0 for v in sizes):
        raise ValueError("TEST.AUG.MIN_SIZES must hold integers > 0")
    max_size = get("MAX_SIZE")
    if isinstance(max_size, bool) or not isinstance(max_size, int) or max_size <= 0:
        raise ValueError("TEST.AUG.MAX_SIZE must be an integer > 0")
    try:
        thr = float(get("FUSE_IOU_THRESH"))
    except (TypeError, ValueError):
        raise ValueError("TEST.AUG.FUSE_IOU_THRESH must be a number") from None
    if not (math.isfinite(thr) and thr >= 0.0):
        raise ValueError("TEST.AUG.FUSE_IOU_THRESH must be finite and >= 0")
    return {"enabled": bool(get("ENABLED")), "min_sizes": sizes, "max_size": max_size, "flip": bool(get("FLIP")), "fuse_iou_thresh": thr,
            "class_agnostic": bool(get("CLASS_AGNOSTIC"))}


_COLOR_JITTER = {"ENABLED": False, "BRIGHTNESS": [0.8, 1.2], "CONTRAST": [0.8, 1.2], "SATURATION": [0.8, 1.2]}


def add_color_jitter_config(cfg):
    """INPUT.COLOR_JITTER.*: photometric augmentation of the training images (`DatasetMapper3D`, csrc/augment.hip,
    omni_color_jitter_u8): a brightness, a contrast and a saturation weight are drawn uniformly from their [low, high] interval for
    every image and applied, in that order, by the integer definition of include/omni3d_hip.h.  Neither detectron2's defaults nor the
    reference define the node, so, as with `add_bev_eval_config`, it is absent until this call; without it nothing is jittered.
    Idempotent: values already set are kept.  An interval of [1, 1] switches its step off and draws nothing.
    The intervals [0.8, 1.2] are conventions (the mild setting detection code bases commonly ship), not tuned values; their effect
    on AP has not been measured."""
    if "COLOR_JITTER" not in cfg.INPUT:
        cfg.INPUT.COLOR_JITTER = CN()
    for key, value in _COLOR_JITTER.items():
        cfg.INPUT.COLOR_JITTER.setdefault(key, list(value) if isinstance(value, list) else value)
    return cfg


def color_jitter_args(cfg):
    """INPUT.COLOR_JITTER -> {"enabled", "brightness", "contrast", "saturation"}, the intervals as (low, high) floats;
    `DatasetMapper3D` reads them through this.  A cfg without the node: the feature off.  ValueError unless every interval is two
    finite numbers with 0 <= low <= high <= 4 (4 is the largest weight the kernel's 32-bit arithmetic is shown to hold)."""
    import math
    node = cfg.INPUT.get("COLOR_JITTER")
    have = dict(node) if node is not None else {}
    out = {"enabled": bool(have.get("ENABLED", False))}
    for key in ("BRIGHTNESS", "CONTRAST", "SATURATION"):
        iv = have.get(key, _COLOR_JITTER[key])
        if isinstance(iv, (str, bytes)) or not hasattr(iv, "__len__") or len(iv) != 2 or any(
                isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) for v in iv):
            raise ValueError(f"INPUT.COLOR_JITTER.{key} must be two numbers [low, high], got {iv!r}")
        lo, hi = float(iv[0]), float(iv[1])
        if not 0.0 <= lo <= hi <= 4.0:
            raise ValueError(f"INPUT.COLOR_JITTER.{key} must satisfy 0 <= low <= high <= 4, got {iv!r}")
        out[key.lower()] = (lo, hi)
    return out


_CAMERA_ROTATION = {"ENABLED": False, "ROLL": [-5.0, 5.0], "PITCH": [-3.0, 3.0], "YAW": [0.0, 0.0], "FILL": []}
CAMERA_ROTATION_MAX_DEG = 15.0


def add_camera_rotation_config(cfg):
    """INPUT.CAMERA_ROTATION.*: geometric augmentation of the training images (`DatasetMapper3D`, csrc/warp.hip,
    omni_warp_homography_u8): a roll, a pitch and a yaw of the camera about its optical centre are drawn uniformly, in degrees, from
    their [low, high] interval for every image; the pixels move by the homography K Q K^-1, the 3D targets by Q, and `K`, the image
    size and the virtual depth stay as they are.  FILL: the three bytes, in INPUT.FORMAT channel order, of the border the rotation
    uncovers; empty = MODEL.PIXEL_MEAN rounded to the nearest byte, about zero after normalisation.  Neither detectron2's defaults nor
    the reference define the node, so it is absent until this call; without it nothing is rotated.  Idempotent: values already set are
    kept.  An interval of [c, c] fixes its angle and draws nothing.
    The intervals (roll +-5, pitch +-3, no yaw) are conventions, not tuned values; their effect on AP has not been measured."""
    if "CAMERA_ROTATION" not in cfg.INPUT:
        cfg.INPUT.CAMERA_ROTATION = CN()
    for key, value in _CAMERA_ROTATION.items():
        cfg.INPUT.CAMERA_ROTATION.setdefault(key, list(value) if isinstance(value, list) else value)
    return cfg


def camera_rotation_args(cfg):
    """INPUT.CAMERA_ROTATION -> {"enabled", "roll", "pitch", "yaw", "fill"}: the intervals as (low, high) floats in degrees, the fill as
    three bytes; `DatasetMapper3D` reads them through this.  A cfg without the node: the feature off.  ValueError unless every interval
    is two finite numbers with -15 <= low <= high <= 15 and FILL is empty or three integers in [0, 255]."""
    import math
    node = cfg.INPUT.get("CAMERA_ROTATION")
    have = dict(node) if node is not None else {}
    out = {"enabled": bool(have.get("ENABLED", False))}
    for key in ("ROLL", "PITCH", "YAW"):
        iv = have.get(key, _CAMERA_ROTATION[key])
        if isinstance(iv, (str, bytes)) or not hasattr(iv, "__len__") or len(iv) != 2 or any(
                isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) for v in iv):
            raise ValueError(f"INPUT.CAMERA_ROTATION.{key} must be two numbers [low, high] in degrees, got {iv!r}")
        lo, hi = float(iv[0]), float(iv[1])
        if not -CAMERA_ROTATION_MAX_DEG <= lo <= hi <= CAMERA_ROTATION_MAX_DEG:
            raise ValueError(f"INPUT.CAMERA_ROTATION.{key} must satisfy -15 <= low <= high <= 15, got {iv!r}")
        out[key.lower()] = (lo, hi)
    fill = have.get("FILL", [])
    if isinstance(fill, (str, bytes)) or not hasattr(fill, "__len__") or len(fill) not in (0, 3) or any(
            isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 255 for v in fill):
        raise ValueError(f"INPUT.CAMERA_ROTATION.FILL must be empty or three integers in [0, 255], got {fill!r}")
    if len(fill) == 0:
        mean = list(cfg.MODEL.PIXEL_MEAN)
        if len(mean) != 3:
            raise ValueError(f"INPUT.CAMERA_ROTATION.FILL is empty and MODEL.PIXEL_MEAN does not hold three values: {mean!r}")
        fill = [min(max(int(math.floor(float(v) + 0.5)), 0), 255) for v in mean]
    out["fill"] = tuple(int(v) for v in fill)
    return out


def build_tta_model(cfg, model):
    """the model wrapped for test-time augmentation when TEST.AUG.ENABLED, else the model itself"""
    if not tta_args(cfg)["enabled"]:
        return model
    from ..modeling.meta_arch.tta import RCNN3DWithTTA
    return RCNN3DWithTTA(cfg, model)
