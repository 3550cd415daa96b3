from .math_util import *  # noqa: F401,F403
from .math_util import R_from_allocentric, R_to_allocentric  # noqa: F401
from .util import (CubeRCNNHandler, compute_priors, file_parts, get_color, imread, imwrite, list_files, load_json,  # noqa: F401
                   mkdir_if_missing, save_json)
