"""The five geometry helpers of the reference's util/math_util.py that sit on the hot path
(SURVEY.md 2.1 #9).  In the training / inference path they are fused into csrc/cube_head.hip; these
entry points expose them with the reference's names and argument meaning.  The cuboid renderer (`mesh_cuboid`,
`render_depth_map`, `estimate_visibility`) runs on csrc/render.hip; the annotation helpers (`get_cuboid_verts`,
`convert_3d_box_to_2d`, `estimate_truncation`) run on csrc/annotate.hip, a single box being a batch of one."""
import math

import numpy as np
import torch

from ...kernels import annotate, det, render


def get_cuboid_verts_faces(box3d=None, R=None):
    """math_util.py:116-219 -> (verts (n,8,3), faces (n,12,3))."""
    if box3d is None:
        box3d = [0, 0, 0, 1, 1, 1]
    box3d = torch.as_tensor(box3d, dtype=torch.float32)
    squeeze = box3d.dim() == 1
    if squeeze:
        box3d = box3d.unsqueeze(0)
    n = len(box3d)
    R = torch.eye(3).repeat(n, 1, 1) if R is None else torch.as_tensor(R, dtype=torch.float32).reshape(n, 3, 3)
    dev = box3d.device if box3d.is_cuda else torch.device("cuda")
    verts = det.cuboid_corners(box3d.to(dev), R.to(dev).reshape(n, 9)).to(box3d.device)
    faces = torch.tensor([[0, 1, 2], [2, 3, 0], [1, 5, 6], [6, 2, 1], [4, 0, 3], [3, 7, 4], [5, 4, 7], [7, 6, 5], [4, 5, 1],
                          [1, 0, 4], [3, 2, 6], [6, 7, 3]]).float().unsqueeze(0).repeat([n, 1, 1]).to(verts.device)
    if squeeze:
        verts, faces = verts.squeeze(), faces.squeeze()
    return verts, faces


def compute_virtual_scale_from_focal_spaces(f, H, f0, H0):
    """math_util.py:581-592"""
    return (H0 * f) / (f0 * H)


def scaled_sigmoid(vals, min=0.0, max=1.0):
    """math_util.py:969-978"""
    return min + (max - min) * torch.sigmoid(vals)


def _viewing_rotation(K, u, v):
    """M (n,3,3): the rotation that takes the optical axis e_z onto the unit viewing ray through pixel (u, v) --
    Rodrigues' formula about a = (-o_y, o_x, 0) / |.| by the angle acos(o_z); identical to the reference's
    axis_angle_to_matrix(angle * axis / |axis|) (math_util.py:609-622).  valid (n,) = angle > 0."""
    fx, fy, sx, sy = K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]
    o = torch.stack(((u - sx) / fx, (v - sy) / fy, torch.ones_like(u)), dim=1)
    o = o / torch.linalg.norm(o, dim=1, keepdim=True)
    c = o[:, 2].clamp(-1.0, 1.0)
    s = torch.sqrt((o[:, 0] ** 2 + o[:, 1] ** 2).clamp(min=0))
    valid = torch.acos(c) > 0
    safe = torch.where(s > 0, s, torch.ones_like(s))
    ax, ay = -o[:, 1] / safe, o[:, 0] / safe
    z = torch.zeros_like(ax)
    Kx = torch.stack((z, z, ay, z, z, -ax, -ay, ax, z), dim=1).view(-1, 3, 3)          # [a]_x for a = (ax, ay, 0)
    a = torch.stack((ax, ay, z), dim=1)
    eye = torch.eye(3, dtype=K.dtype, device=K.device).expand(len(K), 3, 3)
    M = c[:, None, None] * eye + s[:, None, None] * Kx + (1 - c)[:, None, None] * (a[:, :, None] * a[:, None, :])
    return M, valid


def R_to_allocentric(K, R, u=None, v=None):
    """math_util.py:595-648: egocentric -> allocentric (viewpoint-normalised) rotation(s) for objects seen at pixel (u, v).
    Batched tensor form: K (n,3,3), R (n,3,3), u, v (n,); array form: K 3x3, R 3x3 (u, v default to the principal point)."""
    if isinstance(K, torch.Tensor):
        M, valid = _viewing_rotation(K, u, v)
        return torch.where(valid[:, None, None], torch.bmm(M.transpose(2, 1), R), R)
    import numpy as np
    Kt = torch.as_tensor(np.asarray(K, dtype=np.float64)).reshape(1, 3, 3)
    ut = torch.tensor([float(Kt[0, 0, 2] if u is None else u)], dtype=torch.float64)
    vt = torch.tensor([float(Kt[0, 1, 2] if v is None else v)], dtype=torch.float64)
    M, valid = _viewing_rotation(Kt, ut, vt)
    R = np.asarray(R)
    return (M[0].numpy().T @ R) if bool(valid[0]) else R


def R_from_allocentric(K, R_view, u=None, v=None):
    """math_util.py:651-705: the inverse of R_to_allocentric (allocentric -> egocentric).  In the training / inference path
    this is fused into csrc/cube_head.hip (cube_decode / cube_loss); this is the standalone entry point."""
    if isinstance(K, torch.Tensor):
        M, valid = _viewing_rotation(K, u, v)
        return torch.where(valid[:, None, None], torch.bmm(M, R_view), R_view)
    import numpy as np
    Kt = torch.as_tensor(np.asarray(K, dtype=np.float64)).reshape(1, 3, 3)
    ut = torch.tensor([float(Kt[0, 0, 2] if u is None else u)], dtype=torch.float64)
    vt = torch.tensor([float(Kt[0, 1, 2] if v is None else v)], dtype=torch.float64)
    M, valid = _viewing_rotation(Kt, ut, vt)
    R_view = np.asarray(R_view)
    return (M[0].numpy() @ R_view) if bool(valid[0]) else R_view


def euler2mat(euler):
    """math_util.py:86-105: rotation matrix R_z R_y R_x of the euler angles (x, y, z)"""
    cx, sx, cy, sy, cz, sz = (math.cos(euler[0]), math.sin(euler[0]), math.cos(euler[1]), math.sin(euler[1]), math.cos(euler[2]),
                              math.sin(euler[2]))
    R_x = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    R_y = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    R_z = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return np.dot(R_z, np.dot(R_y, R_x))


class CuboidMesh:
    """What `mesh_cuboid` returns in place of a pytorch3d `Meshes` (which does not exist here): the cuboids themselves -- box3d (n,6)
    [X,Y,Z,W,H,L], R (n,3,3), color (n,3) in [0,1] or None -- since csrc/render.hip casts rays against boxes, not triangles."""

    def __init__(self, box3d, R, color=None):
        self.box3d, self.R, self.color = box3d, R, color

    def __len__(self):
        return len(self.box3d)

    def verts_padded(self):
        """(n,8,3) vertices in the order of get_cuboid_verts_faces (math_util.py:116-219), on the host"""
        b, dt = self.box3d, self.box3d.dtype
        sx = torch.tensor([-1, 1, 1, -1, -1, 1, 1, -1], dtype=dt) * 0.5
        sy = torch.tensor([-1, -1, 1, 1, -1, -1, 1, 1], dtype=dt) * 0.5
        sz = torch.tensor([-1, -1, -1, -1, 1, 1, 1, 1], dtype=dt) * 0.5
        local = torch.stack((b[:, 5:6] * sx, b[:, 4:5] * sy, b[:, 3:4] * sz), dim=1)
        return (self.R @ local + b[:, :3, None]).transpose(1, 2)

    def clone(self):
        return CuboidMesh(self.box3d.clone(), self.R.clone(), None if self.color is None else self.color.clone())


def mesh_cuboid(box3d=None, R=None, color=None):
    """math_util.py:761-782.  box3d [X,Y,Z,W,H,L] or (n,6); R 3x3 or (n,3,3); color: 3 values in [0,1] or (n,3)."""
    box3d = torch.as_tensor([0, 0, 0, 1, 1, 1] if box3d is None else box3d, dtype=torch.float32).reshape(-1, 6).cpu()
    n = len(box3d)
    R = torch.eye(3).repeat(n, 1, 1) if R is None else torch.as_tensor(R, dtype=torch.float32).reshape(n, 3, 3).cpu()
    if color is not None:
        color = torch.as_tensor(color, dtype=torch.float32).reshape(-1, 3).cpu().expand(n, 3).contiguous()
    return CuboidMesh(box3d, R, color)


def _cast(K, box3d, pose, width, height, device, zplane=0.05):
    dev = render.default_device() if device is None else torch.device(device)
    mesh = mesh_cuboid(box3d, pose)
    K = torch.as_tensor(np.asarray(K, dtype=np.float32) if not isinstance(K, torch.Tensor) else K, dtype=torch.float32).reshape(9)
    return mesh, dev, render.cuboid_depth(mesh.box3d.to(dev), mesh.R.to(dev), K.to(dev), height, width, zplane)


def render_depth_map(K, box3d, pose, width, height, device=None):
    """math_util.py:707-726 -> (silhouettes (N,H,W) bool, depth_map (H,W), depth_map_inds (H,W) int64).  Two departures from
    pytorch3d's rasteriser, both of csrc/render.hip: a pixel is sampled at its centre (x + 0.5, y + 0.5), and depth is the true depth
    of the ray / surface intersection (the reference sets perspective_correct=False and interpolates depth in screen space).  The
    N silhouettes come from one single-box cast each; `estimate_visibility` does not need them.  Without a hit depth_map is +inf
    and, since the reference takes `zbuf.min(dim=0)` of all-inf columns there, depth_map_inds is 0."""
    mesh, dev, (depth, index, _, _, _) = _cast(K, box3d, pose, width, height, device)
    sil = torch.zeros((len(mesh), height, width), dtype=torch.bool, device=dev)
    Kd = torch.as_tensor(np.asarray(K, dtype=np.float32) if not isinstance(K, torch.Tensor) else K, dtype=torch.float32).reshape(9).to(dev)
    for b in range(len(mesh)):
        sil[b] = render.cuboid_depth(mesh.box3d[b:b + 1].to(dev), mesh.R[b:b + 1].to(dev), Kd, height, width)[1] >= 0
    return sil, depth, index.clamp(min=0).long()


def estimate_visibility(K, box3d, pose, width, height, device=None):
    """math_util.py:728-743 -> [visible / area per box]: the share of a box's pixels where it is the nearest surface, read from the
    counters of omni_cuboid_depth (no silhouette is materialised); nan where the box covers no pixel, as the reference's division."""
    _, _, (_, _, _, area, visible) = _cast(K, box3d, pose, width, height, device)
    return (visible / area).tolist()


# ---- annotation helpers (csrc/annotate.hip) and the small host-side names of the reference's math_util -----------------------------

def upto_2Pi(val):
    """math_util.py:48-56: the angle brought into [0, 2 pi) by whole turns"""
    while val >= 2 * math.pi:
        val -= 2 * math.pi
    while val < 0:
        val += 2 * math.pi
    return val


def upto_Pi(val):
    """math_util.py:58-66: the angle brought into [0, pi) by half turns"""
    while val >= math.pi:
        val -= math.pi
    while val < 0:
        val += math.pi
    return val


def mat2euler(R):
    """math_util.py:72-82: the euler angles (x, y, z) of R = R_z R_y R_x, the inverse of `euler2mat` for |y| < pi / 2"""
    return np.array([math.atan2(R[2, 1], R[2, 2]), math.atan2(-R[2, 0], math.hypot(R[0, 0], R[1, 0])), math.atan2(R[1, 0], R[0, 0])])


def to_float_tensor(input):
    """math_util.py:107-114: anything torch.tensor accepts -> float32 tensor (a tensor keeps its device)"""
    return (input if isinstance(input, torch.Tensor) else torch.tensor(input)).float()


def _annotate_batch(K, box3d, R, width, height, min_z):
    """(n,6) boxes, (n,3,3) poses or None, K (3,3) or (n,3,3), all seen in one frame -> the outputs of `annotate.box_annotate`, on the
    device of box3d.  Every box is its own image row, so a batched K is allowed."""
    n = len(box3d)
    dev = box3d.device if box3d.is_cuda else render.default_device()
    R = torch.eye(3).repeat(n, 1, 1) if R is None else R.reshape(n, 3, 3)
    K = K.reshape(1, 3, 3).expand(n, 3, 3) if K.dim() == 2 else K.reshape(n, 3, 3)
    off = torch.arange(n + 1, dtype=torch.int32)
    size = torch.tensor([[int(width), int(height)]], dtype=torch.int32).repeat(n, 1)
    out = annotate.box_annotate(box3d.contiguous().to(dev), R.contiguous().to(dev), off.to(dev), K.contiguous().to(dev), size.to(dev), min_z)
    return [o.to(box3d.device) for o in out]


def get_cuboid_verts(K, box3d, R=None, view_R=None, view_T=None):
    """math_util.py:221-259 -> (corners_2d (n,8,3) [u, v, z], corners_3d (n,8,3)); a single box gives (8,3) each.  Without a view
    transform both come from omni_box_annotate.  With one the reference's arithmetic is kept on the host: the vertices are moved by
    -view_T, turned by view_R (one box only: the reference turns the first box and drops the others) and pushed back along z by
    1.25 * view_T.z before they are projected."""
    K, box3d = to_float_tensor(K), to_float_tensor(box3d)
    R = None if R is None else to_float_tensor(R)
    squeeze = box3d.dim() == 1
    if squeeze:
        box3d = box3d.unsqueeze(0)
    n = len(box3d)
    if view_R is None and view_T is None:
        v3, v2 = _annotate_batch(K, box3d, R, 1, 1, 0.20)[:2]
    else:
        v3 = mesh_cuboid(box3d, R).verts_padded().to(box3d.device)
        if view_T is not None:
            v3 = v3 - view_T.reshape(1, 1, 3)
        if view_R is not None:
            v3 = (view_R @ v3[0].T).T.unsqueeze(0)
        if view_T is not None:
            v3 = torch.cat((v3[:, :, :2], v3[:, :, 2:] + 1.25 * view_T.reshape(3)[2]), dim=2)
        Kn = K.unsqueeze(0).expand(len(v3), 3, 3) if K.dim() == 2 else K
        p = (Kn @ v3.transpose(1, 2)).transpose(1, 2)
        v2 = torch.cat((p[:, :, :2] / p[:, :, 2:], p[:, :, 2:]), dim=2)
    return (v2.squeeze(), v3.squeeze()) if squeeze else (v2, v3)


def convert_3d_box_to_2d(K, box3d, R=None, clipw=0, cliph=0, XYWH=True, min_z=0.20):
    """math_util.py:498-577 -> (box2d (n,4), behind_camera (n,) bool, fully_behind (n,) bool); a single box gives (4,) and two
    0-d tensors.  The 2D box of the projected vertices, a vertex at z <= min_z counting as the corner of the clipw x cliph frame its
    camera-space x and y point to; XYWH or XYXY.  One launch of omni_box_annotate for the whole batch."""
    K, box3d = to_float_tensor(K), to_float_tensor(box3d)
    R = None if R is None else to_float_tensor(R)
    squeeze = box3d.dim() == 1
    if squeeze:
        box3d = box3d.unsqueeze(0)
    _, _, proj, _, _, behind, fully = _annotate_batch(K, box3d, R, clipw, cliph, min_z)
    box2d = torch.cat((proj[:, :2], proj[:, 2:] - proj[:, :2]), dim=1) if XYWH else proj
    behind, fully = behind.bool(), fully.bool()
    return (box2d.squeeze(), behind.squeeze(), fully.squeeze()) if squeeze else (box2d, behind, fully)


def estimate_truncation(K, box3d, R, imW, imH):
    """math_util.py:745-758, one box -> float: 1.0 when every vertex is behind the camera, otherwise the share of the projected box
    that lies outside [0, imW - 1] x [0, imH - 1], in float64 from the float32 box (nan for a projection of no area, as the reference's
    division).  The `truncation` output of omni_box_annotate."""
    box3d = to_float_tensor(box3d).reshape(1, 6)
    return float(_annotate_batch(to_float_tensor(K), box3d, to_float_tensor(R), imW, imH, 0.20)[4][0])


def intersect(box_a, box_b, mode="cross"):
    """math_util.py:908-966: intersection areas of XYXY boxes, numpy arrays or tensors.  'cross': a (M,4), b (N,4) -> (N,M) (rows
    follow box_b, as in the reference); 'list': a, b (M,4) -> (M,).  The reference's numpy branch of 'list' calls `np.min(a, b)` and
    cannot run; this one computes what its torch branch does, the element-wise minimum / maximum."""
    if isinstance(box_a, torch.Tensor):
        lo, hi, clip = torch.max, torch.min, lambda d: torch.clamp(d, 0)
        lift = lambda t: t.unsqueeze(1)                                                      # noqa: E731
    elif isinstance(box_a, np.ndarray):
        lo, hi, clip = np.maximum, np.minimum, lambda d: np.clip(d, a_min=0, a_max=None)
        lift = lambda t: np.expand_dims(t, 1)                                                # noqa: E731
    else:
        raise ValueError("unknown data type {}".format(type(box_a)))
    if mode == "cross":
        side = clip(hi(box_a[:, 2:4], lift(box_b[:, 2:4])) - lo(box_a[:, 0:2], lift(box_b[:, 0:2])))
        return side[:, :, 0] * side[:, :, 1]
    if mode == "list":
        side = clip(hi(box_a[:, 2:4], box_b[:, 2:4]) - lo(box_a[:, 0:2], box_b[:, 0:2]))
        return side[:, 0] * side[:, 1]
    raise ValueError("unknown mode {}".format(mode))


def iou(box_a, box_b, mode="cross", ign_area_b=False):
    """math_util.py:850-905: intersection over union of XYXY boxes, numpy arrays or tensors.  'cross': a (M,4), b (N,4) -> (M,N);
    ign_area_b leaves the area of b out of the union, which makes it the share of a that lies inside b.  'list': a, b (M,4) -> (M,)
    (ign_area_b has no effect there, as in the reference).  No +1, and 0 / 0 where the union is 0."""
    area = lambda b: (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])                               # noqa: E731
    inter = intersect(box_a, box_b, mode=mode)
    if mode == "list":
        return inter / (area(box_a) + area(box_b) - inter)
    union = area(box_a)[None, :]
    if not ign_area_b:
        union = union + area(box_b)[:, None] - inter
    return (inter / union).T
