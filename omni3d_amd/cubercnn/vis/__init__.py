"""`cubercnn.vis` (reference cubercnn/vis/*).  `vis.py` draws predicted 3D boxes on the device (csrc/render.hip): `draw_scene_view`,
`draw_3d_box_from_verts`, `draw_3d_box`, `draw_text`, `draw_line`, `draw_2d_box`, `draw_bev`, and the filled shapes of
csrc/shapes.hip: `draw_transparent_polygon`, `get_polygon_grid`, `draw_circle`, `draw_transparent_square`; `interp_color`,
`create_colorbar`, `imhstack` and `imvstack` are host helpers.  `visualize_from_instances`, the last
step of every evaluation, returns the per-dataset 3D error line (one launch of csrc/vis_errors.hip) and writes a drawing of every
50th image; `match_errors_from_instances` gives the numbers behind the line.  The training-time drawings of VIS_PERIOD are
`RCNN3D.visualize_training` (meta_arch/rcnn3d.py), built from these helpers on the rows csrc/train_vis.hip picks; `logperf` prints
the evaluation tables."""
from . import logperf  # noqa: F401
from .vis import (create_colorbar, draw_2d_box, draw_3d_box, draw_3d_box_from_verts, draw_bev, draw_circle, draw_line,  # noqa: F401
                  draw_scene_view, draw_text, draw_transparent_polygon, draw_transparent_square, get_polygon_grid, imhstack, imvstack,
                  interp_color, match_errors_from_instances, visualize_from_instances)
