"""Times of csrc/render.hip at a size a user would draw: one 512 x 512 cast of 100 boxes (omni_cuboid_depth) and one
`draw_scene_view('front_and_novel')` of 20 boxes on a 512 x 512 image (scale 512).  Device events around `reps` back-to-back calls
after a warm-up for the kernel; a host clock around calls that end in a device-to-host copy for draw_scene_view (it returns
host arrays).  Information only: there is nothing to compare these with.
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
    assert torch.cuda.is_available(), "needs the GPU"
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


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200)
