from .omni3d_evaluation import (AnnotationIndex, Omni3DEvaluationHelper, Omni3DEvaluator, Omni3DParams, Omni3Deval,  # noqa: F401
                                bev_overlap_groups, bootstrap_compare, bootstrap_weights, box3d_overlap, box3d_overlap_groups, dist_errors_groups, evaluate_groups, inference_on_dataset, instances_to_coco_json, let_overlap_groups)
from .kitti import KittiEval, KittiParams  # noqa: F401,E402
from .proposals import proposal_recall, proposal_recall_table  # noqa: F401,E402
from ...kernels.iou3d import box3d_overlap_exact  # noqa: F401,E402  (exact geometry; Omni3Deval keeps box3d_overlap, see its docstring)
