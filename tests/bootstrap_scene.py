"""The synthetic split tests/test_bootstrap_kernel.py and tests/test_bootstrap_eval.py share, and its physical duplication.

6 images x 3 categories of cuboids (`boxgen.corners`): category 1 has 130 detections in all (the 64-lane scan crosses two chunk
boundaries), image 2 holds 14 detections of category 2 (maxDets 1 / 10 / 100 cut differently), category 3 lives in images 1 and 4 only
(a replicate can lose it), some ground truths carry `ignore3D`, the ground truths cover the three depth ranges, and no two scores of a
category tie (asserted by `scene()`)."""
import copy
import functools

import numpy as np

from omni3d_amd import boxgen

N_IMG = 6
CATS = [1, 2, 3]
IMGS = [16 * i for i in range(N_IMG)]                   # copy c of image index i is image 16 i + c in the duplicated split
CAT1_DETS = (22, 22, 22, 22, 21, 21)                    # 130
CAT3_IMGS = (1, 4)


def rec(img, cat, box, score=None, ignore=0):
    box = np.asarray(box, np.float32)
    depth = float(box[:, 2].mean())
    u, v = 64.0 + 40.0 * box[:, 0] / np.maximum(box[:, 2], 0.1), 48.0 + 40.0 * box[:, 1] / np.maximum(box[:, 2], 0.1)
    bbox = [float(u.min()), float(v.min()), float(u.max() - u.min() + 1.0), float(v.max() - v.min() + 1.0)]
    r = {"image_id": img, "category_id": cat, "bbox3D": box.tolist(), "depth": depth, "bbox": bbox, "area": bbox[2] * bbox[3]}
    if score is None:
        r.update(ignore3D=ignore, ignore2D=0, iscrowd=0)
    else:
        r["score"] = float(score)
    return r


@functools.lru_cache(maxsize=None)
def scene(seed=11):
    """-> (ground truths, detections) with image ids IMGS"""
    rng = np.random.default_rng(seed)
    gts, dts = [], []
    scores = {c: list(rng.permutation(400) / 400.0 * 0.9 + 0.05) for c in CATS}      # distinct inside a category

    def cuboid(c, d, R):
        return boxgen.corners(np.asarray(c)[None], np.asarray(d)[None], R[None])[0]

    def one(z_lo, z_hi):
        return np.array([rng.uniform(-4, 4), rng.uniform(-1.5, 1.5), rng.uniform(z_lo, z_hi)]), rng.uniform(0.8, 3.0, 3), boxgen.rand_rot(rng, 1)[0]

    def group(i, cat, n_gt, n_dt):
        made = 0
        for j in range(n_gt):
            c, d, R = one(*((3, 9), (12, 30), (40, 70))[(i + j + cat) % 3])
            gts.append(rec(IMGS[i], cat, cuboid(c, d, R), ignore=int((i + 2 * j + cat) % 7 == 0)))
            if made < n_dt and (i + j) % 4 != 3:                                          # a detection near its ground truth
                c2 = c + R @ (rng.normal(0, 0.12, 3) * d)
                dts.append(rec(IMGS[i], cat, cuboid(c2, d * rng.uniform(0.85, 1.15, 3), R), score=scores[cat].pop()))
                made += 1
        while made < n_dt:                                                                # and boxes elsewhere
            c, d, R = one(3, 70)
            dts.append(rec(IMGS[i], cat, cuboid(c, d, R), score=scores[cat].pop()))
            made += 1

    for i in range(N_IMG):
        group(i, 1, 6, CAT1_DETS[i])
        group(i, 2, 3 if i != 5 else 0, 14 if i == 2 else (0 if i == 3 else 4))
        if i in CAT3_IMGS:
            group(i, 3, 4, 5)
    for k, r in enumerate(gts + dts):
        r["id"] = k + 1
    for c in CATS:
        s = [x["score"] for x in dts if x["category_id"] == c]
        assert len(s) == len(set(s))
    return gts, dts


def weight_rows():
    """the six replicates of the defining test"""
    rng = np.random.default_rng(3)
    no_cat3 = [2, 0, 1, 1, 0, 2]
    assert all(no_cat3[i] == 0 for i in CAT3_IMGS)
    rows = [[1] * N_IMG, [3, 0, 1, 0, 2, 0], [0, 0, 6, 0, 0, 0], no_cat3]
    rows += rng.multinomial(N_IMG, np.full(N_IMG, 1.0 / N_IMG), size=2).tolist()
    return np.array(rows, dtype=np.int32)


def duplicated(gts, dts, w):
    """the split in which image index i is present w[i] times: copy c has image id 16 i + c -> (gts, dts, image ids)"""
    out_g, out_d, imgs = [], [], []
    for i, n in enumerate(w):
        imgs += [IMGS[i] + c for c in range(int(n))]
    for src, dst in ((gts, out_g), (dts, out_d)):
        for r in src:
            for c in range(int(w[r["image_id"] // 16])):
                q = copy.deepcopy(r)
                q["image_id"] = r["image_id"] + c
                dst.append(q)
    for k, r in enumerate(out_g + out_d):
        r["id"] = k + 1
    return out_g, out_d, imgs


def evaluate(gts, dts, imgs=IMGS, cats=CATS, mode="3D", accumulate=True):
    from omni3d_amd.cubercnn.evaluation import omni3d_evaluation as E
    ev = E.Omni3Deval(E.AnnotationIndex(copy.deepcopy(list(gts)), imgs, cats), E.AnnotationIndex(copy.deepcopy(list(dts)), imgs, cats), mode=mode)
    ev.evaluate()
    if accumulate:
        ev.accumulate()
        ev.summarize()
    return ev


@functools.lru_cache(maxsize=None)
def _evaluated(mode, emulated):
    return evaluate(*scene(), mode=mode)


def evaluated(mode):
    """the scene evaluated, accumulated and summarised in `mode` by the library in use, once per session"""
    from omni3d_amd import lib
    return _evaluated(mode, bool(lib.get().emulated))
