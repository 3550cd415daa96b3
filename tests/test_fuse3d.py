"""omni_fuse3d (`kernels.det.fuse3d`, csrc/nms3d.hip) against a float64 reference written here from the definition in
include/omni3d_hip.h: the exact IoU3D matrix, the ranking and greedy walk of tests/test_nms3d_exact.py, then per cluster the
alignment of every member to its head's axis naming, score-weighted means of centre, dimensions and aux columns, and the orthogonal
polar factor (numpy SVD here, Newton steps in the kernel) of the weighted mean of the aligned axes.

Scene, B = 2, S = 64, counts (64, 37), every coordinate within 64 m.  Image 0: four clusters of 12 jittered copies interleaved over
the slots 0 .. 47 as in tests/test_nms3d_exact.py; in cluster 0 every second member is the same body with its axes cyclically renamed
(dimensions permuted alike), in cluster 1 with two axes negated (a half turn), which a naive mean of poses or dimensions gets wrong;
slots 48 .. 52 are one cluster whose scores are all 0; slot 53 is a box of zero thickness under the best score in use; slot 54
carries a NaN score on a valid box; the rest is sparse.  Image 1 is sparse and the slots behind its count hold the best scores on
real boxes, on poisoned output buffers.

Runs: class-agnostic and class-specific x views 1 and 3 x A = 0 and A = 5.  `cluster`, `head`, `size`, `cls`, `count`, the row
order and the zeros / -1 behind the count are exact.  Tolerances: iou 1e-5 on the compared pairs and 0 elsewhere (the bound of
tests/test_nms3d_exact.py); verts and centre 2e-5 absolute (float32 rounding at |x| < 64 is 3.8e-6; the double arithmetic adds
nothing visible); dims, axes, score and aux 1e-5 relative to their scale (the element itself for dims and score, 1 for the unit
axes, AUX_SCALE = 50, the range the aux columns are drawn from).  Properties: two calls give the same bits; `out_axes` is
orthonormal to 1e-6; `fit64(out_verts)` returns the fused parameters to what the rounding of the corners allows: with
e = 2^-24 x 64 = 3.8e-6 per coordinate, the centre (a mean of 8) within 1e-5, a mean edge within 2 e per component so a dimension
within 2 sqrt(3) e = 1.4e-5, a unit axis within that over the smallest dimension, doubled for the Gram-Schmidt step that carries the
error of x into y and z.

The committed seed is the first from 1 on for which, in float64 alone and for every (class mode, views) pair that is run: no
compared IoU lies within 1e-3 of the threshold, no two distinct scores, raw or fused, are closer than 1e-6 relative, every member's
best alignment beats the runner-up by 1e-3 or more, at least 10 slots are merged away, some fused cuboid has a vertex more than
1e-2 m from its head's, and some member's best permutation is not the identity: `test_reference_alone_meets_the_conditions`.

Largest deviations from the float64 reference over all runs, printed by every run under `-s` (iou | verts | centre | dims rel | axes |
score rel | aux / 50):
    host emulator   1.73e-07 | 1.72e-06 | 1.91e-06 | 5.21e-08 | 2.97e-08 | 4.47e-08 | 3.25e-08
    MI355X          1.73e-07 | 1.72e-06 | 1.91e-06 | 5.21e-08 | 2.97e-08 | 4.47e-08 | 3.25e-08
`fit64(out_verts)` against the fused parameters: centre 1.91e-06, dimensions 1.18e-06, axes x smallest dimension 4.85e-07;
`out_axes` orthonormal to 7.55e-08 (both).
Seed 1: 44 slots merged away class-agnostic and 32 class-specific, the smallest alignment lead is 1.78, a fused vertex lies up to
0.70 m from its head's, and the cyclic renamings (1,2,0) and (2,0,1) are among the permutations used.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

import exact_iou3d
from omni3d_amd import boxgen
from test_iou3d_exact import YAWS, _axis_turn, _ry, _yaw_reference, fit64
from test_nms3d import EPS_COPLANAR, EPS_NONZERO, MARGIN, POISON, SCORE_TOL, THR, _valid64

SEED, B, S, K, A = 1, 2, 64, 3, 5
COUNTS = (64, 37)
IOU_TOL, POS_TOL, REL_TOL, ORTHO_TOL, AUX_SCALE = 1e-5, 2e-5, 1e-5, 1e-6, 50.0
ALIGN_MARGIN, MOVED = 1e-3, 1e-2
CLUSTERS, COPIES = 4, 12
ZERO_SLOTS, FLAT_SLOT, NAN_SLOT = range(48, 53), 53, 54
PERMS = list(itertools.permutations(range(3)))                      # lexicographic
RUNS = [(ag, v, a) for ag in (True, False) for v in (1, 3) for a in (0, A)]
E32 = 2.0 ** -24 * 64.0                                             # float32 rounding of a coordinate below 64


@functools.lru_cache(maxsize=None)
def _scene(seed=SEED):
    rng = np.random.default_rng(seed)
    verts = np.zeros((B, S, 8, 3), np.float32)
    upright = np.zeros((B, S), bool)                                # yaw-only bodies: their pairs have the closed form
    score = rng.uniform(0.05, 0.98, size=(B, S)).astype(np.float32)
    cls = rng.integers(K, size=(B, S)).astype(np.int32)
    aux = rng.uniform(-AUX_SCALE, AUX_SCALE, size=(B * S, A)).astype(np.float32)
    for b in range(B):
        c = rng.uniform(-12, 12, size=(S, 3)) + np.array([0.0, 0.0, 30.0])
        verts[b] = boxgen.corners(c, rng.uniform(0.5, 2.0, size=(S, 3)), boxgen.rand_rot(rng, S))

    def copy_of(c0, d0, yaw0, yaw_only):
        c = c0 + rng.normal(scale=0.15, size=3) * d0
        d = d0 * rng.uniform(0.85, 1.15, size=3)
        if yaw_only:
            c[1], d[1] = c0[1], d0[1]
            return c, d, _ry(yaw0 + rng.choice(YAWS) * rng.choice([-1.0, 1.0]))
        return c, d, _axis_turn(rng.normal(size=3), np.radians(rng.uniform(0.0, 2.0))) @ _ry(yaw0)

    for g in range(CLUSTERS + 1):
        c0 = np.array([rng.uniform(-12, 12), rng.uniform(-2, 2), rng.uniform(8, 50)])
        d0, yaw0 = rng.uniform(1.0, 4.0, size=3), rng.uniform(-np.pi, np.pi)
        slots = [g + CLUSTERS * k for k in range(COPIES)] if g < CLUSTERS else list(ZERO_SLOTS)
        for k, s in enumerate(slots):
            c, d, R = copy_of(c0, d0, yaw0, k % 2 == 0)
            upright[0, s] = k % 2 == 0
            if g == 0 and k % 4 >= 2:                               # the same body, axes renamed x -> y -> z -> x
                R, d = R[:, [1, 2, 0]], d[[1, 2, 0]]
            if g == 1 and k % 4 >= 2:                               # the same body, turned by half a turn about its own y
                R = R * np.array([-1.0, 1.0, -1.0])
            verts[0, s] = boxgen.corners(c[None], d[None], R[None])[0]
    score[0, list(ZERO_SLOTS)] = 0.0
    flat = fit64(verts[0, 1])
    verts[0, FLAT_SLOT] = boxgen.corners(flat[0][None], (flat[2] * np.array([1.0, 0.0, 1.0]))[None], flat[1].T[None])[0]   # on slot 1
    score[0, FLAT_SLOT] = 0.99
    verts[0, NAN_SLOT], score[0, NAN_SLOT] = verts[0, 2], np.nan    # on slot 2
    n = COUNTS[1]
    for s in range(n, S):                                           # behind the count: neither read nor kept
        verts[1, s], cls[1, s], score[1, s] = verts[1, (s - n) % n], cls[1, (s - n) % n], 2.0
    out = dict(verts=verts.reshape(B * S, 8, 3), score=score.reshape(-1), cls=cls, count=np.asarray(COUNTS, np.int32), upright=upright, aux=aux)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _geometry(seed=SEED):
    """per image, float64: which slots < count are valid cuboids, the IoU3D of every pair of them, the pairs with disjoint spheres"""
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


def align64(head, member):
    """(aligned axes (3, 3) rows, aligned dims, index of the permutation, its lead over the runner-up) of a fitted member"""
    dot = head[1] @ member[1].T
    sums = np.array([sum(abs(dot[k, p[k]]) for k in range(3)) for p in PERMS])
    pick = int(np.argmax(sums))                                     # the first maximum
    p = PERMS[pick]
    sg = np.array([1.0 if dot[k, p[k]] >= 0 else -1.0 for k in range(3)])
    return sg[:, None] * member[1][list(p)], member[2][list(p)], pick, float(sums[pick] - np.sort(sums)[-2])


def fuse64(fits, w, aux):
    """members in rank order, the head first -> (centre, axes, dims, aux, smallest alignment lead, permutations used)"""
    head = fits[0]
    sw, sc, sd, M, sa = 0.0, np.zeros(3), np.zeros(3), np.zeros((3, 3)), np.zeros(aux.shape[1])
    lead, picks = np.inf, []
    for i, f in enumerate(fits):
        if i == 0:
            ax, dd = f[1], f[2]
        else:
            ax, dd, pick, gap = align64(head, f)
            lead, picks = min(lead, gap), picks + [pick]
        sw, sc, sd, M, sa = sw + w[i], sc + w[i] * f[0], sd + w[i] * dd, M + w[i] * ax, sa + w[i] * aux[i]
    u, _, vt = np.linalg.svd(M / sw)
    return sc / sw, u @ vt, sd / sw, sa / sw, lead, picks


@functools.lru_cache(maxsize=None)
def _case(agnostic, views, seed=SEED):
    """the float64 reference of one (class mode, views) pair with A = 5 aux columns (a run with A = 0 ignores them), never written to"""
    a = _scene(seed)
    score = a["score"].reshape(B, S).astype(np.float64)
    verts = a["verts"].reshape(B, S, 8, 3)
    aux = a["aux"].reshape(B, S, A).astype(np.float64)
    o = dict(cluster=np.full((B, S), -1, np.int32), head=np.full((B, S), -1, np.int32), size=np.zeros((B, S), np.int32),
             out_cls=np.zeros((B, S), np.int32), out_count=np.zeros(B, np.int32), out_score=np.zeros((B, S)), out_verts=np.zeros((B, S, 8, 3)),
             centre=np.zeros((B, S, 3)), axes=np.zeros((B, S, 3, 3)), dims=np.zeros((B, S, 3)), out_aux=np.zeros((B, S, A)))
    near = close = 0
    lead, moved, picks, compared, ious, aparts = np.inf, 0.0, [], [], [], []
    for b, (valid, iou, apart) in enumerate(_geometry(seed)):
        n = len(valid)
        cmp_ = valid[:, None] & valid[None, :] & ~np.eye(n, dtype=bool)
        if not agnostic:
            cmp_ &= a["cls"][b, :n, None] == a["cls"][b, None, :n]
        ranked = [s for s in range(n) if valid[s] and np.isfinite(score[b, s])]
        ranking = sorted(ranked, key=lambda s: (-score[b, s], s))
        dead, clusters = set(), []
        for p, i in enumerate(ranking):
            if i not in dead:
                members = [i] + [j for j in ranking[p + 1:] if j not in dead and cmp_[i, j] and iou[i, j] > THR]
                dead.update(members[1:])
                clusters.append(members)
        clusters += [[s] for s in range(n) if s not in ranked]
        fused = [sum(score[b, m] for m in members) / max(len(members), views) for members in clusters]
        order = sorted(range(len(clusters)), key=lambda q: (not np.isfinite(fused[q]), -fused[q] if np.isfinite(fused[q]) else 0.0, clusters[q][0]))
        o["out_count"][b] = len(clusters)
        for r, q in enumerate(order):
            members = clusters[q]
            h = members[0]
            o["cluster"][b, members] = h
            o["head"][b, r], o["size"][b, r], o["out_cls"][b, r], o["out_score"][b, r] = h, len(members), a["cls"][b, h], fused[q]
            w = np.maximum(score[b, members], 0.0)
            hf = fit64(verts[b, h])
            if len(members) == 1 or not w.sum() > 0:
                o["out_verts"][b, r], o["centre"][b, r], o["axes"][b, r], o["dims"][b, r], o["out_aux"][b, r] = verts[b, h], hf[0], hf[1], hf[2], aux[b, h]
                continue
            c, X, d, av, gap, pk = fuse64([fit64(verts[b, m]) for m in members], w, aux[b, members])
            o["out_verts"][b, r], o["centre"][b, r], o["axes"][b, r], o["dims"][b, r], o["out_aux"][b, r] = c + (boxgen.UNIT * d) @ X, c, X, d, av
            lead, picks = min(lead, gap), picks + pk
            moved = max(moved, float(np.abs(o["out_verts"][b, r] - verts[b, h]).max()))
        near += int((np.triu(cmp_, 1) & (np.abs(iou - THR) < MARGIN)).sum())
        for sc in (np.sort(score[b, ranked]), np.sort([f for f in fused if np.isfinite(f)])):
            gap = np.diff(sc)
            close += int(((gap > 0) & (gap < SCORE_TOL * np.abs(sc[1:]))).sum())
        compared.append(cmp_), ious.append(iou), aparts.append(apart)
    o.update(a, near=near, close=close, lead=lead, moved=moved, picks=picks, compared=compared, ious=ious, aparts=aparts,
             merged=int(sum(COUNTS) - o["out_count"].sum()))
    for v in o.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return o


def conditions(seed=SEED):
    """the six conditions on a seed (module docstring) for every (class mode, views) pair of RUNS, in float64 alone"""
    ok = True
    for agnostic, views in sorted({(r[0], r[1]) for r in RUNS}):
        c = _case(agnostic, views, seed)
        ok = ok and (c["near"] == 0 and c["close"] == 0 and c["lead"] >= ALIGN_MARGIN and c["merged"] >= 10 and c["moved"] > MOVED
                     and any(p != 0 for p in c["picks"]))
    return ok


def test_reference_alone_meets_the_conditions():
    for agnostic, views in sorted({(r[0], r[1]) for r in RUNS}):
        c = _case(agnostic, views)
        print("seed %d agnostic=%d views=%d: %d slots merged away, smallest alignment lead %.3f, a fused vertex %.3f m from its head's, "
              "permutations used %s" % (SEED, agnostic, views, c["merged"], c["lead"], c["moved"], sorted(set(c["picks"]))))
        assert c["near"] == 0 and c["close"] == 0
        assert c["lead"] >= ALIGN_MARGIN
        assert c["merged"] >= 10
        assert c["moved"] > MOVED
        assert any(p != 0 for p in c["picks"])
    assert conditions()
    valid = _geometry()[0][0]
    assert not valid[FLAT_SLOT] and valid[NAN_SLOT] and valid[list(ZERO_SLOTS)].all()
    c = _case(True, 1)
    assert (c["cluster"][0, list(ZERO_SLOTS)] == ZERO_SLOTS[0]).all()                       # all scores 0: one cluster, headed by the lowest slot
    assert c["cluster"][0, FLAT_SLOT] == FLAT_SLOT and c["cluster"][0, NAN_SLOT] == NAN_SLOT
    assert c["head"][0, c["out_count"][0] - 1] == NAN_SLOT                                  # the score that is not finite sorts last
    assert c["head"][0, 0] == FLAT_SLOT                                                      # 0.99 on a box that is none leads, alone
    assert (c["cluster"][1, COUNTS[1]:] == -1).all() and c["out_count"][1] >= 33
    for s in range(1, SEED):
        assert not conditions(s), s                                                          # the first seed from 1 on


def _bits(t):
    return t.cpu().contiguous().view(torch.int32)


def _launch(dev, c, agnostic, views, ncols, monkeypatch):
    from omni3d_amd.kernels import det
    monkeypatch.setattr(det, "_empty", lambda shape, dtype, like: torch.full(shape, POISON, dtype=dtype, device=like.device))   # poison
    t = {k: torch.from_numpy(np.array(c[k])).to(dev) for k in ("verts", "score", "cls", "count", "aux")}
    return det.fuse3d(t["verts"], t["score"], t["cls"], t["count"], THR, views=views, aux=t["aux"] if ncols else None, class_agnostic=agnostic,
                      eps_coplanar=EPS_COPLANAR, eps_nonzero=EPS_NONZERO)


def _run_case(dev, agnostic, views, ncols, monkeypatch):
    c = _case(agnostic, views)
    outs = [_launch(dev, c, agnostic, views, ncols, monkeypatch) for _ in range(2)]
    for x, y in zip(*outs):
        assert torch.equal(_bits(x), _bits(y))                                                # two launches are bit-identical
    g = {k: v.cpu().numpy() for k, v in outs[0]._asdict().items()}
    assert g["verts"].shape == (B * S, 8, 3) and g["axes"].shape == (B * S, 3, 3) and g["aux"].shape == (B * S, ncols) and g["iou"].shape == (B, S, S)
    assert np.array_equal(g["count"], c["out_count"]), (g["count"], c["out_count"])
    assert np.array_equal(g["cluster"], c["cluster"]), np.argwhere(g["cluster"] != c["cluster"])
    assert np.array_equal(g["head"].reshape(B, S), c["head"]), (g["head"].reshape(B, S), c["head"])
    assert np.array_equal(g["size"].reshape(B, S), c["size"]) and np.array_equal(g["cls"].reshape(B, S), c["out_cls"])
    assert g["invalid"][0] == 1                                                               # the box of zero thickness
    e = dict.fromkeys(("iou", "verts", "centre", "dims", "axes", "score", "aux", "refit_c", "refit_d", "refit_x", "ortho"), 0.0)
    for b in range(B):
        M, cmp_, want, apart = g["iou"][b], c["compared"][b], c["ious"][b], c["aparts"][b]
        n = len(cmp_)
        assert np.array_equal(M.view(np.int32), M.T.copy().view(np.int32)) and (np.diag(M) == 0).all()
        full = np.zeros((S, S), bool)
        full[:n, :n] = cmp_
        assert (M[~full] == 0).all() and (M[:n, :n][cmp_ & apart] == 0).all()
        e["iou"] = max(e["iou"], float(np.abs(M[:n, :n][cmp_] - want[cmp_]).max()))
        rows = slice(b * S, b * S + c["out_count"][b])
        behind = slice(b * S + c["out_count"][b], (b + 1) * S)
        for k in ("verts", "centre", "axes", "dims", "score", "cls", "aux", "size"):
            assert (g[k][behind] == 0).all(), k                                               # zeros behind the count
        k_ = c["out_count"][b]
        finite = np.isfinite(c["out_score"][b, :k_])
        assert np.array_equal(np.isnan(g["score"][rows]), np.isnan(c["out_score"][b, :k_]))
        e["verts"] = max(e["verts"], float(np.abs(g["verts"][rows] - c["out_verts"][b, :k_]).max()))
        e["centre"] = max(e["centre"], float(np.abs(g["centre"][rows] - c["centre"][b, :k_]).max()))
        e["axes"] = max(e["axes"], float(np.abs(g["axes"][rows] - c["axes"][b, :k_]).max()))
        with np.errstate(invalid="ignore", divide="ignore"):
            rel_d = np.abs(g["dims"][rows] - c["dims"][b, :k_]) / np.abs(c["dims"][b, :k_])
            rel_s = np.abs(g["score"][rows][finite] - c["out_score"][b, :k_][finite]) / np.abs(c["out_score"][b, :k_][finite])
        zero_d, zero_s = c["dims"][b, :k_] == 0, c["out_score"][b, :k_][finite] == 0
        assert (g["dims"][rows][zero_d] == 0).all() and (g["score"][rows][finite][zero_s] == 0).all()
        e["dims"] = max(e["dims"], float(rel_d[~zero_d].max()))
        e["score"] = max(e["score"], float(rel_s[~zero_s].max()))
        if ncols:
            e["aux"] = max(e["aux"], float(np.abs(g["aux"][rows] - c["out_aux"][b, :k_]).max()) / AUX_SCALE)
        for r in range(k_):
            row = b * S + r
            fc, fx, fd, ok = fit64(g["verts"][row])
            if not ok:
                assert g["size"][row] == 1 and (g["dims"][row] == 0).all() and (g["axes"][row] == 0).all() and (g["centre"][row] == 0).all()
                continue
            e["refit_c"] = max(e["refit_c"], float(np.abs(fc - g["centre"][row]).max()))
            e["refit_d"] = max(e["refit_d"], float(np.abs(fd - g["dims"][row]).max()))
            e["refit_x"] = max(e["refit_x"], float(np.abs(fx - g["axes"][row]).max() * g["dims"][row].min()))
            X = g["axes"][row].astype(np.float64)
            e["ortho"] = max(e["ortho"], float(np.abs(X @ X.T - np.eye(3)).max()))
    print("agnostic=%d views=%d A=%d: iou %.2e | verts %.2e | centre %.2e | dims rel %.2e | axes %.2e | score rel %.2e | aux/%g %.2e | "
          "refit centre %.2e dims %.2e axes x dmin %.2e | orthonormal %.2e"
          % (agnostic, views, ncols, e["iou"], e["verts"], e["centre"], e["dims"], e["axes"], e["score"], AUX_SCALE, e["aux"], e["refit_c"],
             e["refit_d"], e["refit_x"], e["ortho"]))
    assert e["iou"] <= IOU_TOL and e["verts"] <= POS_TOL and e["centre"] <= POS_TOL
    assert e["dims"] <= REL_TOL and e["axes"] <= REL_TOL and e["score"] <= REL_TOL and e["aux"] <= REL_TOL
    assert e["ortho"] <= ORTHO_TOL
    assert e["refit_c"] <= 1e-5 and e["refit_d"] <= 2 * np.sqrt(3.0) * E32 and e["refit_x"] <= 4 * np.sqrt(3.0) * E32


@pytest.mark.parametrize("agnostic,views,ncols", RUNS)
def test_fuse3d_emulated(emu_lib, monkeypatch, agnostic, views, ncols):
    _run_case("cpu", agnostic, views, ncols, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("agnostic,views,ncols", RUNS)
def test_fuse3d_gpu(hip_lib, monkeypatch, agnostic, views, ncols):
    _run_case("cuda", agnostic, views, ncols, monkeypatch)


def _small_cases(L, dev):
    from omni3d_amd import lib
    from omni3d_amd.kernels import det
    rng = np.random.default_rng(5)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)                           # noqa: E731
    # S = 1: the box comes back bit for bit with its own score (views = 1) or half of it (views = 2)
    one = torch.from_numpy(boxgen.random_boxes(rng, 1)).to(dev)
    aux = torch.tensor([[3.0, -4.0]], device=dev)
    for views in (1, 2):
        o = det.fuse3d(one, torch.tensor([0.75], device=dev), i32([4]), i32([1]), 0.5, views=views, aux=aux)
        assert torch.equal(_bits(o.verts), _bits(one)) and torch.equal(o.aux, aux) and o.score.tolist() == [0.75 / views]
        assert o.cls.tolist() == [4] and o.size.tolist() == [1] and o.head.tolist() == [0] and o.count.tolist() == [1] and o.cluster.tolist() == [[0]]
        c, X, d, ok = fit64(one[0].cpu().numpy())
        assert ok and np.abs(o.centre[0].cpu().numpy() - c).max() <= 1e-6 and np.abs(o.axes[0].cpu().numpy() - X).max() <= 1e-6
        assert np.abs(o.dims[0].cpu().numpy() - d).max() <= 1e-6
    # all counts 0: every row zero, every head and cluster entry -1, although real boxes and scores sit in the slots
    boxes = torch.from_numpy(boxgen.random_boxes(rng, 8)).to(dev)
    score = torch.from_numpy(rng.uniform(0.1, 0.9, 8).astype(np.float32)).to(dev)
    o = det.fuse3d(boxes, score, i32([0] * 8), i32([0, 0]), 0.5, aux=torch.ones(8, 3, device=dev))
    assert o.count.tolist() == [0, 0] and (o.head == -1).all() and (o.cluster == -1).all() and (o.iou == 0).all()
    for t in (o.verts, o.centre, o.axes, o.dims, o.score, o.cls, o.aux, o.size):
        assert (t == 0).all()
    # B = 0 and S = 0: nothing to launch
    for B_ in (0, 2):
        o = det.fuse3d(boxes[:0], score[:0], i32([]), i32([0] * B_), 0.5)
        assert o.verts.shape == (0, 8, 3) and o.count.shape == (B_,) and o.iou.shape == (B_, 0, 0) and o.aux.shape == (0, 0) and int(o.invalid) == 0
    # a threshold >= 1: every slot is a cluster of its own and comes back as itself, in score order -- even four copies of one box
    same = boxes[:1].repeat(4, 1, 1)
    sc4 = torch.tensor([0.2, 0.9, 0.9, 0.4], device=dev)
    for thr in (1.0, 1.5):
        o = det.fuse3d(same, sc4, i32([0] * 4), i32([4]), thr)
        assert o.head.tolist() == [1, 2, 3, 0] and o.size.tolist() == [1] * 4 and o.count.tolist() == [4] and o.cluster.tolist() == [[0, 1, 2, 3]]
        assert torch.equal(_bits(o.verts), _bits(same)) and torch.equal(o.score, sc4[[1, 2, 3, 0]])
        assert abs(float(o.iou[0, 0, 1]) - 1.0) <= IOU_TOL
    o = det.fuse3d(same, sc4, i32([0] * 4), i32([4]), 0.5, views=2)                           # and below it they are one, seen 4 times in 2 views
    assert o.count.tolist() == [1] and o.size.tolist() == [4, 0, 0, 0] and o.head.tolist() == [1, -1, -1, -1]
    assert abs(float(o.score[0]) - 2.4 / 4) <= 1e-6 and float((o.verts[0] - same[0]).abs().max()) <= POS_TOL
    # sizes and view counts the kernel refuses: the launcher raises before anything is launched, the C entry point returns the status
    big = torch.from_numpy(boxgen.random_boxes(rng, 1025)).to(dev)
    ones, zeros, cnt = torch.ones(1025, device=dev), torch.zeros(1025, dtype=torch.int32, device=dev), i32([1025])
    with pytest.raises(ValueError):
        det.fuse3d(big, ones, zeros, cnt, 0.5)
    for views in (0, -1, 1.5):
        with pytest.raises(ValueError):
            det.fuse3d(boxes, score, i32([0] * 8), i32([8]), 0.5, views=views)
    outs = [torch.full(shape, POISON, dtype=dt, device=dev) for shape, dt in
            (((1, 8, 8), torch.float32), ((1, 8), torch.int32), ((8, 8, 3), torch.float32), ((8, 3), torch.float32), ((8, 3, 3), torch.float32),
             ((8, 3), torch.float32), ((8,), torch.float32), ((8,), torch.int32), ((8, 1), torch.float32), ((8,), torch.int32), ((8,), torch.int32),
             ((1,), torch.int32), ((1,), torch.int32))]
    P = [t.data_ptr() for t in outs]
    ins = (boxes.data_ptr(), score.data_ptr(), zeros.data_ptr(), cnt.data_ptr())
    f, st = L._fn["omni_fuse3d"], lib.stream_of(boxes)
    assert f(big.data_ptr(), ones.data_ptr(), zeros.data_ptr(), cnt.data_ptr(), None, 1, 1025, 0, 1, 0.5, 1, EPS_COPLANAR, EPS_NONZERO, *P, st) == 1
    assert f(*ins, None, 1, 8, 0, 0, 0.5, 1, EPS_COPLANAR, EPS_NONZERO, *P, st) == 1          # views = 0
    assert f(*ins, None, 1, 8, -1, 1, 0.5, 1, EPS_COPLANAR, EPS_NONZERO, *P, st) == 1         # A < 0
    assert f(*ins, None, -1, 8, 0, 1, 0.5, 1, EPS_COPLANAR, EPS_NONZERO, *P, st) == 1         # B < 0
    assert f(*ins, None, 1, 8, 1, 1, 0.5, 1, EPS_COPLANAR, EPS_NONZERO, *P, st) == 1          # A = 1 without aux
    assert f(None, *ins[1:], None, 1, 8, 0, 1, 0.5, 1, EPS_COPLANAR, EPS_NONZERO, *P, st) == 1
    assert f(None, None, None, None, None, 0, 8, 0, 1, 0.5, 1, EPS_COPLANAR, EPS_NONZERO, *([None] * 13), st) == 0
    if dev == "cuda":
        torch.cuda.synchronize()
    assert all(bool((o == POISON).all()) for o in outs)


def test_small_cases_emulated(emu_lib):
    _small_cases(emu_lib, "cpu")


@pytest.mark.gpu
def test_small_cases_gpu(hip_lib):
    _small_cases(hip_lib, "cuda")


def test_launcher_checks_shapes_and_dtypes(emu_lib):
    from omni3d_amd.kernels import det
    v, s, c, n = torch.zeros(8, 8, 3), torch.zeros(8), torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    det.fuse3d(v, s, c, n, 0.5, aux=torch.zeros(8, 2))
    for bad in ((v[:7], s, c, n), (v.double(), s, c, n), (v.view(8, 24), s, c, n), (v, s[:7], c, n), (v, s.double(), c, n),
                (v, s, c.long(), n), (v, s, c[:1], n), (v, s, c, n.long()), (v, s, c, n.view(2, 1))):
        with pytest.raises(ValueError):
            det.fuse3d(*bad, 0.5)
    for aux in (torch.zeros(7, 2), torch.zeros(8, 2).double(), torch.zeros(8), torch.zeros(2, 8).t()):
        with pytest.raises(ValueError):
            det.fuse3d(v, s, c, n, 0.5, aux=aux)
