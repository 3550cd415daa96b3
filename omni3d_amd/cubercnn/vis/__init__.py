"""`cubercnn.vis` (reference cubercnn/vis/*).  `vis.py` draws predicted 3D boxes on the device (csrc/render.hip): `draw_scene_view`,
`draw_3d_box_from_verts`, `draw_3d_box`, `draw_text`, `draw_line`, `draw_2d_box`, `draw_bev`.  `visualize_from_instances`, the last
step of every evaluation, returns the per-dataset 3D error line (one launch of csrc/vis_errors.hip) and writes a drawing of every
50th image; `match_errors_from_instances` gives the numbers behind the line.  The training-time drawings of VIS_PERIOD are
`RCNN3D.visualize_training` (meta_arch/rcnn3d.py), built from these helpers on the rows csrc/train_vis.hip picks; `logperf` prints
the evaluation tables."""
from . import logperf  # noqa: F401
from .vis import (draw_2d_box, draw_3d_box, draw_3d_box_from_verts, draw_bev, draw_line, draw_scene_view, draw_text,  # noqa: F401
                  match_errors_from_instances, visualize_from_instances)
