"""Times of csrc/render.hip at a size a user would draw: one 512 x 512 cast of 100 boxes (omni_cuboid_depth) and one
`draw_scene_view('front_and_novel')` of 20 boxes on a 512 x 512 image (scale 512).  Device events around `reps` back-to-back calls
after a warm-up for the kernel; a host clock around calls that end in a device-to-host copy for draw_scene_view (it returns
host arrays).  Information only: there is nothing to compare these with.
The leg of csrc/shapes.hip: `omni_ground_grid` on a 1000 x 1000 image and `omni_fill_shapes` with the back and top faces of 30 boxes on
it (device events), and the novel view of 30 boxes at scale 1000 with the ground grid off and on, the two arms alternating call by
call (host clock).  Grid off is what the call cost before it could draw a grid.
    python tools/bench_render.py [reps]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from omni3d_amd.cubercnn import util, vis  # noqa: E402
from omni3d_amd.kernels import render  # noqa: E402


def main(reps=200):
    assert torch.cuda.is_available(), "needs the GPU"          # a timing without the GPU says nothing: no fall-back
    rs = np.random.RandomState(0)
    H = W = 512
    N = 100
    K = np.array([[460.0, 0, 256.0], [0, 460.0, 256.0], [0, 0, 1]], np.float32)
    z = rs.uniform(2, 12, N)
    box = np.stack([rs.uniform(-0.5, 0.5, N) * z, rs.uniform(-0.5, 0.5, N) * z, z] + [rs.uniform(0.3, 2.0, N) for _ in range(3)], 1).astype(np.float32)
    R = np.stack([util.euler2mat([rs.uniform(-0.3, 0.3), rs.uniform(-3, 3), rs.uniform(-0.3, 0.3)]) for _ in range(N)]).astype(np.float32)
    b, r, k = torch.tensor(box).cuda(), torch.tensor(R).cuda(), torch.tensor(K).cuda()
    for _ in range(20):
        out = render.cuboid_depth(b, r, k, H, W)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = render.cuboid_depth(b, r, k, H, W)
    e1.record()
    torch.cuda.synchronize()
    covered = float((out[1] >= 0).float().mean())
    print("omni_cuboid_depth 512x512, 100 boxes (%.0f %% of the pixels covered): %.1f us per call (launcher + 2 fills + kernel, %d calls)"
          % (100 * covered, 1e3 * e0.elapsed_time(e1) / reps, reps))
    im = rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    meshes = [util.mesh_cuboid(box[i], R[i], color=[c / 255.0 for c in util.get_color(i)]) for i in range(20)]
    for _ in range(3):
        vis.draw_scene_view(im, K, meshes, scale=512, blend_weight=0.5, blend_weight_overlay=0.85)
    torch.cuda.synchronize()
    n = max(reps // 10, 5)
    t0 = time.perf_counter()
    for _ in range(n):
        vis.draw_scene_view(im, K, meshes, scale=512, blend_weight=0.5, blend_weight_overlay=0.85)
    torch.cuda.synchronize()
    print("draw_scene_view('front_and_novel') 512x512, 20 boxes, scale 512: %.2f ms per call, host clock, host geometry and copies "
          "included (%d calls)" % (1e3 * (time.perf_counter() - t0) / n, n))
    shapes_leg(rs, box, R, reps)


def _events(fn, reps):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def shapes_leg(rs, box, R, reps):
    scale, n_box = 1000, 30
    K = np.array([[900.0, 0, 500.0], [0, 900.0, 500.0], [0, 0, 1]], np.float32)
    image = torch.full((3, scale, scale), 255, dtype=torch.uint8, device="cuda")
    A = torch.tensor(util.euler2mat([np.pi / 3, 0, 0]), dtype=torch.float32).cuda()
    t = torch.tensor([0.0, 3.0, 9.0]).cuda()
    k = torch.tensor(K).cuda()
    us = _events(lambda: render.ground_grid(image, k, A, t, 1.5, (-400, 400, -400, 400), thickness=2), reps)
    inked = float((image[0] == 175).float().mean())
    print("omni_ground_grid 1000x1000 (%.0f %% of the pixels on a line): %.1f us per call (launcher + kernel, %d calls)" % (100 * inked, us, reps))
    shapes = []
    for i in range(n_box):
        verts = util.mesh_cuboid(box[i], R[i]).verts_padded()[0].double().numpy()
        shapes += vis.vis.face_shapes(K.astype(np.float64), verts, util.get_color(i))
    rows = torch.tensor(shapes, dtype=torch.float32).cuda()
    us = _events(lambda: render.fill_shapes(image, rows), reps)
    print("omni_fill_shapes 1000x1000, %d faces of %d boxes: %.1f us per call (launcher + kernel, %d calls)" % (len(shapes), n_box, us, reps))
    im = rs.randint(0, 256, size=(512, 512, 3)).astype(np.uint8)
    K512 = np.array([[460.0, 0, 256.0], [0, 460.0, 256.0], [0, 0, 1]])
    meshes = [util.mesh_cuboid(box[i], R[i], color=[c / 255.0 for c in util.get_color(i)]) for i in range(n_box)]
    arms = {"off": dict(ground_grid=False), "on": dict(ground_grid=True)}
    for _ in range(3):
        for kw in arms.values():
            vis.draw_scene_view(im, K512, meshes, scale=scale, mode="novel", **kw)
    torch.cuda.synchronize()
    n = max(reps // 10, 5)
    spent = {name: [] for name in arms}
    for _ in range(n):                                   # alternating, so that both arms see the same machine
        for name, kw in arms.items():
            t0 = time.perf_counter()
            vis.draw_scene_view(im, K512, meshes, scale=scale, mode="novel", **kw)
            torch.cuda.synchronize()
            spent[name].append(1e3 * (time.perf_counter() - t0))
    for name in arms:
        v = np.sort(spent[name])
        print("draw_scene_view('novel') scale 1000, %d boxes, ground grid %s: median %.2f ms per call (min %.2f, max %.2f), host clock, "
              "host geometry and copies included (%d calls)" % (n_box, name, v[len(v) // 2], v[0], v[-1], n))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200)
