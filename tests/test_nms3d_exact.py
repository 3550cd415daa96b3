"""omni_nms3d_exact (`kernels.det.nms3d(method="exact")`, csrc/nms3d.hip + csrc/cuboid_exact.h) on the case tests/test_nms3d.py had
to exclude: near-aligned duplicates.  B = 2, S = 64.  Image 0 holds four clusters of 12 copies of an upright box, jittered by 0.15:
half of each cluster is yaw-only (relative yaw from {0, 1e-6, 1e-4, 1e-3, 0.01, 0.03, 0.1} rad) with the height and y centre of its
original, the other half is turned 0 to 2 degrees about random axes; the other 16 slots are sparse.  Image 1 is sparse with count
37 < S, and the slots behind the count hold the image's best scores on real boxes.

Reference, float64 from the same float32 vertices: IoU3D = footprint intersection (tests/exact_bev.py) x overlap of the y extents for
two yaw-only boxes (they share face planes; tests/test_iou3d_exact.py::_yaw_reference), tests/exact_iou3d.py for every other pair
whose bounding spheres intersect, exactly 0 for the rest; a slot takes part if it passes the evaluator's validity test and the fit;
greedy suppression as defined in tests/test_nms3d.py.  `keep`, `order` and `new_count` must be exact; the matrix is within 1e-5 on
the compared pairs, exactly 0 elsewhere, symmetric with a zero diagonal and written everywhere; `invalid` is 0; two launches give
the same bits.  One class-specific variant runs on the same scene (the second launch's own cases are those of tests/test_nms3d.py).

The committed seed is the first from 1 on for which, on the CPU and in float64 alone, no compared IoU lies within 1e-3 of the
threshold, no two scores are closer than 1e-6 relative, at least 10 rows are removed, and the greedy result computed from the IoUs
of the evaluator's float32 pair algorithm (oracle/iou_box3d_oracle.c) differs from the float64 one in at least one row:
`test_reference_alone_meets_the_conditions` asserts all four.

Largest |iou - float64| over the compared pairs, kernel | float32 pair algorithm, printed by every run under `-s`:
    host emulator   3.71e-07 | 2.10e-01   (class-specific run: 3.26e-07 | 2.10e-01)
    MI355X          3.71e-07 | 2.10e-01   (class-specific run: 3.26e-07 | 2.10e-01)
Seed 30: 39 rows removed, the float32 pair algorithm's IoUs decide one row differently (seeds 1 .. 29 fail the first or the last condition).
"""
import functools

import numpy as np
import pytest
import torch

import exact_iou3d
from omni3d_amd import boxgen
from test_iou3d_exact import YAWS, _axis_turn, _ry, _yaw_reference, fit64
from test_nms3d import EPS_COPLANAR, EPS_NONZERO, MARGIN, POISON, SCORE_TOL, THR, _oracle32, _valid64

SEED, B, S, K = 30, 2, 64, 3
COUNTS = (64, 37)
IOU_TOL = 1e-5
CLUSTERS, COPIES = 4, 12


@functools.lru_cache(maxsize=None)
def _scene(seed=SEED):
    rng = np.random.default_rng(seed)
    verts = np.zeros((B, S, 8, 3), np.float32)
    upright = np.zeros((B, S), bool)                                # yaw-only boxes: their pairs have the closed form
    score = rng.uniform(0.05, 0.98, size=(B, S)).astype(np.float32)
    cls = rng.integers(K, size=(B, S)).astype(np.int32)
    for b in range(B):
        c = rng.uniform(-12, 12, size=(S, 3)) + np.array([0.0, 0.0, 30.0])
        verts[b] = boxgen.corners(c, rng.uniform(0.5, 2.0, size=(S, 3)), boxgen.rand_rot(rng, S))
    for g in range(CLUSTERS):
        c0 = np.array([rng.uniform(-12, 12), rng.uniform(-2, 2), rng.uniform(8, 50)])
        d0, yaw0 = rng.uniform(1.0, 4.0, size=3), rng.uniform(-np.pi, np.pi)
        for k in range(COPIES):
            s = g + CLUSTERS * k                                   # the clusters interleave over the slots 0 .. 47
            c = c0 + rng.normal(scale=0.15, size=3) * d0
            d = d0 * rng.uniform(0.85, 1.15, size=3)
            if k % 2 == 0:
                c[1], d[1] = c0[1], d0[1]
                R = _ry(yaw0 + rng.choice(YAWS) * rng.choice([-1.0, 1.0]))
                upright[0, s] = True
            else:
                R = _axis_turn(rng.normal(size=3), np.radians(rng.uniform(0.0, 2.0))) @ _ry(yaw0)
            verts[0, s] = boxgen.corners(c[None], d[None], R[None])[0]
    n = COUNTS[1]
    for s in range(n, S):                                           # behind the count: neither read nor kept
        verts[1, s], cls[1, s], score[1, s] = verts[1, (s - n) % n], cls[1, (s - n) % n], 2.0
    out = dict(verts=verts.reshape(B * S, 8, 3), score=score.reshape(-1), cls=cls, count=np.asarray(COUNTS, np.int32), upright=upright)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _geometry(seed=SEED):
    """per image, float64: validity of the slots < count, IoU3D of every pair of valid boxes, the pairs with disjoint spheres"""
    a = _scene(seed)
    verts = a["verts"].reshape(B, S, 8, 3).astype(np.float64)
    out = []
    for b in range(B):
        n = COUNTS[b]
        valid = np.array([_valid64(verts[b, s]) and fit64(verts[b, s])[3] for s in range(n)], bool)
        iou, apart = np.zeros((n, n)), np.zeros((n, n), bool)
        ctr = verts[b, :n].mean(1)
        rad = np.linalg.norm(verts[b, :n] - ctr[:, None], axis=2).max(1)
        for i in range(n):
            for j in range(i + 1, n):
                if not (valid[i] and valid[j]):
                    continue
                if np.linalg.norm(ctr[i] - ctr[j]) > rad[i] + rad[j]:
                    apart[i, j] = apart[j, i] = True
                elif a["upright"][b, i] and a["upright"][b, j]:
                    iou[i, j] = iou[j, i] = _yaw_reference(verts[b, i], verts[b, j])
                else:
                    iou[i, j] = iou[j, i] = exact_iou3d.iou3d(verts[b, i], verts[b, j])[1]
        out.append((valid, iou, apart))
    return out


def _greedy(score, valid, cmp_, iou, n):
    ranked = [s for s in range(n) if valid[s] and np.isfinite(score[s])]
    ranking = sorted(ranked, key=lambda s: (-score[s], s))
    dead = set()
    for p, i in enumerate(ranking):
        if i not in dead:
            dead.update(j for j in ranking[p + 1:] if cmp_[i, j] and iou[i, j] > THR)
    return [s for s in range(n) if s not in dead], ranked


@functools.lru_cache(maxsize=None)
def _case(agnostic, seed=SEED):
    """the arrays and their reference, computed once and shared by the emulator and GPU variants (never written to)"""
    a = _scene(seed)
    score = a["score"].reshape(B, S).astype(np.float64)
    keep, order, new_count = np.zeros((B, S), np.int32), np.full((B, S), -1, np.int32), np.zeros(B, np.int32)
    near, close, compared, ious, aparts = 0, 0, [], [], []
    for b, (valid, iou, apart) in enumerate(_geometry(seed)):
        n = len(valid)
        cmp_ = valid[:, None] & valid[None, :] & ~np.eye(n, dtype=bool)
        if not agnostic:
            cmp_ &= a["cls"][b, :n, None] == a["cls"][b, None, :n]
        kept, ranked = _greedy(score[b], valid, cmp_, iou, n)
        keep[b, kept], order[b, :len(kept)], new_count[b] = 1, kept, len(kept)
        near += int((np.triu(cmp_, 1) & (np.abs(iou - THR) < MARGIN)).sum())
        sc = np.sort(score[b, ranked])
        gap = np.diff(sc)
        close += int(((gap > 0) & (gap < SCORE_TOL * np.abs(sc[1:]))).sum())
        compared.append(cmp_), ious.append(iou), aparts.append(apart)
    out = dict(a, keep=keep, order=order, new_count=new_count, near=near, close=close, compared=compared, ious=ious, aparts=aparts)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def conditions(oracle_lib, seed=SEED):
    """the four conditions on a seed (module docstring), float64 and the CPU oracle alone -> (near, close, removed, rows in which the
    greedy result from the float32 pair algorithm's IoUs differs)"""
    c = _case(True, seed)
    verts = c["verts"].reshape(B, S, 8, 3)
    differ = 0
    for b in range(B):
        n, cmp_ = COUNTS[b], c["compared"][b]
        valid = _geometry(seed)[b][0]
        o32 = _oracle32(oracle_lib, verts[b, :n]).astype(np.float64)
        kept32, _ = _greedy(c["score"].reshape(B, S)[b].astype(np.float64), valid, cmp_, o32, n)
        differ += len(set(kept32) ^ set(np.flatnonzero(c["keep"][b, :n]).tolist()))
    return c["near"], c["close"], int(sum(COUNTS) - c["new_count"].sum()), differ


def test_reference_alone_meets_the_conditions(oracle_lib):
    near, close, removed, differ = conditions(oracle_lib)
    print("seed %d: %d rows removed, the float32 pair algorithm's IoUs decide %d rows differently" % (SEED, removed, differ))
    assert near == 0 and close == 0 and removed >= 10 and differ >= 1
    c = _case(False)
    assert c["near"] == 0 and c["close"] == 0 and c["new_count"].sum() > _case(True)["new_count"].sum()
    for b in range(B):
        assert all(v.all() for v in _geometry()[b][:1])                       # every slot in use is a valid cuboid
        assert _case(True)["keep"][b, COUNTS[b]:].sum() == 0
    crowd = _case(True)["ious"][0][:48, :48]
    assert (crowd > THR).sum() > 200 and _case(True)["new_count"][1] >= 33    # a crowd in image 0, the sparse image loses next to nothing


def _bits(t):
    return t.cpu().contiguous().view(torch.int32)


def _launch(dev, c, agnostic, monkeypatch):
    from omni3d_amd.kernels import det
    monkeypatch.setattr(det, "_empty", lambda shape, dtype, like: torch.full(shape, POISON, dtype=dtype, device=like.device))   # poison
    t = {k: torch.from_numpy(np.array(c[k])).to(dev) for k in ("verts", "score", "cls", "count")}
    return det.nms3d(t["verts"], t["score"], t["cls"], t["count"], THR, class_agnostic=agnostic, eps_coplanar=EPS_COPLANAR,
                     eps_nonzero=EPS_NONZERO, method="exact")


def _run_case(dev, agnostic, monkeypatch, oracle_lib):
    c = _case(agnostic)
    assert c["near"] == 0 and c["close"] == 0
    outs = [_launch(dev, c, agnostic, monkeypatch) for _ in range(2)]
    for x, y in zip(*outs):
        assert torch.equal(_bits(x), _bits(y))                                                # two launches are bit-identical
    keep, order, new_count, iou, invalid = [o.cpu().numpy() for o in outs[0]]
    assert keep.shape == (B, S) and order.shape == (B, S) and new_count.shape == (B,) and iou.shape == (B, S, S) and invalid.shape == (1,)
    assert np.array_equal(new_count, c["new_count"]), (new_count, c["new_count"])
    assert np.array_equal(keep, c["keep"]), np.argwhere(keep != c["keep"])
    assert np.array_equal(order, c["order"]), (order, c["order"])
    assert invalid[0] == 0
    e_hip = e_ref = 0.0
    verts = c["verts"].reshape(B, S, 8, 3)
    for b in range(B):
        M, cmp_, want, apart = iou[b], c["compared"][b], c["ious"][b], c["aparts"][b]
        n = len(cmp_)
        assert np.array_equal(M.view(np.int32), M.T.copy().view(np.int32)) and (np.diag(M) == 0).all()       # symmetric, zero diagonal
        full = np.zeros((S, S), bool)
        full[:n, :n] = cmp_
        assert (M[~full] == 0).all()                                                          # written everywhere, 0 where nothing is compared
        assert (M[:n, :n][cmp_ & apart] == 0).all()
        e_hip = max(e_hip, float(np.abs(M[:n, :n][cmp_] - want[cmp_]).max()))
        e_ref = max(e_ref, float(np.abs(_oracle32(oracle_lib, verts[b, :n])[cmp_] - want[cmp_]).max()))
    print("agnostic=%d: |hip-fp64| %.2e  |float32 pair algorithm-fp64| %.2e over the compared pairs" % (agnostic, e_hip, e_ref))
    assert e_hip <= IOU_TOL, e_hip


@pytest.mark.parametrize("agnostic", (True, False))
def test_nms3d_exact_emulated(emu_lib, oracle_lib, monkeypatch, agnostic):
    _run_case("cpu", agnostic, monkeypatch, oracle_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("agnostic", (True, False))
def test_nms3d_exact_gpu(hip_lib, oracle_lib, monkeypatch, agnostic):
    _run_case("cuda", agnostic, monkeypatch, oracle_lib)


def _invalid_slots(dev):
    """a slot whose corners are no cuboid (one face pushed out and a corner moved by 0.3: whatever the evaluator's validity test says
    of it, the fit refuses it) is counted, kept, and takes no part although the best score in use sits on it, on top of another box"""
    from omni3d_amd.kernels import det
    base = boxgen.corners(np.array([[0.0, 0.0, 10.0]]), np.array([[2.0, 1.0, 1.5]]), np.eye(3)[None])[0]
    bent = base.copy()
    bent[[0, 1, 2, 3], 2] -= np.float32(0.2)
    bent[0, 0] -= np.float32(0.3)
    verts = torch.from_numpy(np.stack([bent, base, base, base]).astype(np.float32)).to(dev)
    score = torch.tensor([0.9, 0.8, 0.7, 2.0], device=dev)
    cls, count = torch.zeros(4, dtype=torch.int32, device=dev), torch.tensor([3], dtype=torch.int32, device=dev)
    assert not fit64(bent)[3]
    keep, order, new_count, iou, invalid = det.nms3d(verts, score, cls, count, THR, method="exact")
    assert int(invalid) == 1 and keep.tolist() == [[1, 1, 0, 0]] and order.tolist() == [[0, 1, -1, -1]] and int(new_count) == 2
    assert (iou[0, 0] == 0).all() and (iou[0, :, 0] == 0).all() and abs(float(iou[0, 1, 2]) - 1.0) <= IOU_TOL
    with pytest.raises(ValueError):
        det.nms3d(verts, score, cls, count, THR, method="bev")
    # the sizes omni_nms3d refuses or skips: the same here
    from omni3d_amd import lib
    big = torch.from_numpy(boxgen.random_boxes(np.random.default_rng(0), 1025)).to(dev)
    with pytest.raises(lib.OmniHipError):
        det.nms3d(big, torch.ones(1025, device=dev), torch.zeros(1025, dtype=torch.int32, device=dev),
                  torch.full((1,), 1025, dtype=torch.int32, device=dev), THR, method="exact")
    for B_ in (0, 2):
        k, o, nc, m, bad = det.nms3d(verts[:0], score[:0], cls[:0], count.new_zeros(B_), THR, method="exact")
        assert k.shape == (B_, 0) and m.shape == (B_, 0, 0) and int(bad) == 0


def test_invalid_slots_and_sizes_emulated(emu_lib):
    _invalid_slots("cpu")


@pytest.mark.gpu
def test_invalid_slots_and_sizes_gpu(hip_lib):
    _invalid_slots("cuda")
