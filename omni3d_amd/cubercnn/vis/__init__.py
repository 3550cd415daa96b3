"""`cubercnn.vis` (reference cubercnn/vis/*).  `vis.py` draws predicted 3D boxes on the device (csrc/render.hip): `draw_scene_view`,
`draw_3d_box_from_verts`, `draw_3d_box`, `draw_text`.  The per-dataset figure of the evaluation loop is still not produced:
`visualize_from_instances` renders nothing and says so in the log string `tools/train_net.py:do_test` prints (:99-106); `logperf`
prints the evaluation tables."""
from . import logperf  # noqa: F401
from .vis import draw_3d_box, draw_3d_box_from_verts, draw_scene_view, draw_text  # noqa: F401


def visualize_from_instances(detections, dataset, dataset_name, min_size_test, output_folder, category_names_official, iteration=""):
    """reference vis/vis.py: draws predictions next to the ground truth for a sample of images and returns a log line with the
    mean 3D error of matched boxes.  Here: no rendering (that figure is laid out with matplotlib, which the MI355X image lacks)."""
    return "Visualisation skipped for {} ({} predictions, iteration {}): cubercnn.vis renders nothing in this package".format(
        dataset_name, len(detections), iteration)
