from .config import add_bev_eval_config, add_dist_eval_config, add_nms3d_config, add_nms3d_exact_config, bev_eval_args, dist_eval_args, get_cfg_defaults  # noqa: F401
