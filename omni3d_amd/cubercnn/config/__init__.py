from .config import add_nms3d_config, get_cfg_defaults  # noqa: F401
