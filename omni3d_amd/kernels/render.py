"""Launchers of csrc/render.hip: the device side of `render_depth_map` / `estimate_visibility`
(/root/reference/cubercnn/util/math_util.py:707-743) and of `draw_scene_view` / `draw_3d_box_from_verts`
(/root/reference/cubercnn/vis/vis.py:210-383, 571-626).  pytorch3d's rasteriser and OpenCV's line drawing are replaced by a
per-pixel ray cast against the cuboids and a per-pixel capsule test; the pixel centre is (x + 0.5, y + 0.5).
"""
import torch

from .. import lib as _lib


def default_device():
    """where the drawing helpers put host data: the GPU (the host-emulated build of the test-suite keeps it on the CPU)"""
    return torch.device("cpu" if _lib.get().emulated else "cuda")


def _f32(t, shape, name):
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    return t.contiguous()


def _image(image):
    if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[0] != 3:
        raise ValueError(f"image must be a uint8 (3, H, W) tensor, got {image.dtype} {tuple(image.shape)}")
    if not image.is_contiguous():
        raise ValueError("image must be contiguous (it is written in place)")
    return image


def cuboid_depth(box3d, R, K, height, width, zplane=0.05):
    """box3d (N,6) [X,Y,Z,W,H,L], R (N,3,3) or (N,9), K (3,3) or (9,) -> depth (H,W) float32 (+inf: no hit), index (H,W) int32
    (-1: no hit), face (H,W) int32 0..5, area (N,) int32, visible (N,) int32.  Depth is the camera z of the true intersection of
    the pixel-centre ray with the box surface (pytorch3d interpolates z in screen space, perspective_correct=False)."""
    N = box3d.shape[0]
    box3d, R, K = _f32(box3d, (N, 6), "box3d"), _f32(R.reshape(N, 9), (N, 9), "R"), _f32(K.reshape(9), (9,), "K")
    if not zplane > 0:
        raise ValueError("zplane must be positive")
    L = _lib.check_device(box3d, R, K)
    dev, H, W = box3d.device, int(height), int(width)
    depth = torch.empty((H, W), dtype=torch.float32, device=dev)
    index = torch.empty((H, W), dtype=torch.int32, device=dev)
    face = torch.empty((H, W), dtype=torch.int32, device=dev)
    area = torch.empty(N, dtype=torch.int32, device=dev)
    visible = torch.empty(N, dtype=torch.int32, device=dev)
    L.call("omni_cuboid_depth", _lib.ptr(box3d), _lib.ptr(R), _lib.ptr(K), N, H, W, float(zplane), _lib.ptr(depth), _lib.ptr(index),
           _lib.ptr(face), _lib.ptr(area), _lib.ptr(visible), _lib.stream_of(box3d))
    return depth, index, face, area, visible


def scene_compose(image, index, face, R, K, color, blend_weight):
    """In place on image (3,H,W) uint8: pixels with index >= 0 become round(shaded * blend_weight + image * (1 - blend_weight)),
    shaded = 255 * color[index] * (0.5 + 0.3 * max(0, n . l)) -- ambient and diffuse terms of pytorch3d's PointLights defaults with
    the light at the camera origin; the specular term is left out.  color (N,3) in [0,1], one value per image plane."""
    image = _image(image)
    H, W = image.shape[1:]
    N = color.shape[0]
    R, K, color = _f32(R.reshape(N, 9), (N, 9), "R"), _f32(K.reshape(9), (9,), "K"), _f32(color, (N, 3), "color")
    if index.dtype != torch.int32 or face.dtype != torch.int32 or tuple(index.shape) != (H, W) or tuple(face.shape) != (H, W):
        raise ValueError("index and face must be int32 (H, W)")
    if not 0.0 <= blend_weight <= 1.0:
        raise ValueError("blend_weight must lie in [0, 1]")
    index, face = index.contiguous(), face.contiguous()
    L = _lib.check_device(image, index, face, R, K, color)
    L.call("omni_scene_compose", _lib.ptr(index), _lib.ptr(face), _lib.ptr(R), _lib.ptr(K), _lib.ptr(color), N, H, W,
           float(blend_weight), _lib.ptr(image), _lib.stream_of(image))
    return image


def draw_segments(image, segments):
    """In place on image (3,H,W) uint8: segments (S,8) float32 [x0, y0, x1, y1, thickness, c0, c1, c2] in paint order; a pixel whose
    centre lies within thickness / 2 of a segment takes the colour of the last such segment."""
    image = _image(image)
    H, W = image.shape[1:]
    S = segments.shape[0]
    segments = _f32(segments, (S, 8), "segments")
    L = _lib.check_device(image, segments)
    L.call("omni_draw_segments", _lib.ptr(segments), S, _lib.ptr(image), H, W, _lib.stream_of(image))
    return image


def fill_shapes(image, shapes):
    """In place on image (3,H,W) uint8: shapes (S,13) float32 [kind, x0, y0, x1, y1, x2, y2, x3, y3, blend, c0, c1, c2] in paint order.
    kind 0: the quadrilateral of the four vertices (even-odd rule at the pixel centre); kind 1: the ring around (x0, y0) with outer
    radius x1 and inner radius y1.  A covered pixel's value v becomes floor(v * blend + (1 - blend) * c) in float64, shape after
    shape; rows that are not finite cover nothing."""
    image = _image(image)
    H, W = image.shape[1:]
    S = shapes.shape[0]
    shapes = _f32(shapes, (S, 13), "shapes")
    L = _lib.check_device(image, shapes)
    L.call("omni_fill_shapes", _lib.ptr(shapes), S, _lib.ptr(image), H, W, _lib.stream_of(image))
    return image


def _rgb(color, name):
    c = [int(v) for v in color]
    if len(c) != 3 or min(c) < 0 or max(c) > 255:
        raise ValueError(f"{name} must be three values in 0..255")
    return (c[0] << 16) | (c[1] << 8) | c[2]


def ground_grid(image, K, A, t, y0, bounds, index=None, near=0.25, thickness=1.0, bg_color=(225, 225, 225), line_color=(175, 175, 175)):
    """In place on image (3,H,W) uint8: the plane y = y0 of the scene, seen through p' = A p + t (A a rotation, (3,3) or (9,)) and K,
    with the grid lines X = k, k = x_start .. x_end - 2, and Z = k, k = z_start .. z_end - 2, of bounds = (x_start, x_end, z_start,
    z_end), `thickness` pixels wide in `line_color` on `bg_color`.  Pixels with index (H,W) int32 >= 0 keep their bytes; all others
    are written.  Plane points nearer than `near` or outside the bounds are background."""
    image = _image(image)
    H, W = image.shape[1:]
    K, A, t = _f32(K.reshape(9), (9,), "K"), _f32(A.reshape(9), (9,), "A"), _f32(t.reshape(3), (3,), "t")
    if index is not None:
        if index.dtype != torch.int32 or tuple(index.shape) != (H, W):
            raise ValueError("index must be int32 (H, W)")
        index = index.contiguous()
    x_start, x_end, z_start, z_end = (int(b) for b in bounds)
    if not near > 0 or not thickness >= 0:
        raise ValueError("near must be positive and thickness not negative")
    L = _lib.check_device(image, index, K, A, t)
    L.call("omni_ground_grid", _lib.ptr(image), _lib.ptr(index), _lib.ptr(K), _lib.ptr(A), _lib.ptr(t), float(y0), x_start, x_end,
           z_start, z_end, float(near), float(thickness), _rgb(bg_color, "bg_color"), _rgb(line_color, "line_color"), H, W,
           _lib.stream_of(image))
    return image
