"""csrc/vis_errors.hip (omni_match_errors, `kernels.viserr.match_errors`) against a float64 reference written here from the
definitions: a plain double loop over the predictions and the ground truths of every image for the match (largest 2D IoU among the
same-category boxes of the image, the lowest row among equal ones, valid at IoU >= 0.5; IoU 0 where the union is not positive) and
the seven error terms [xy, z, w, h, l, dim, ry] of the matched pairs.  ry = pi / 2 - (trace(R_dt R_gt^T) - 1) / 2, skipped where the
trace lies outside [-1 - 1e-4, 3 + 1e-4]: a reading of pytorch3d's `so3_relative_angle(..., cos_bound=1)`, which is not installed, so
that parity cannot be pinned.

`match` must equal the reference exactly.  A detection is left out of the comparison only when, in the float64 reference, its best
IoU lies within 1e-6 of 0.5, or its two best same-category IoUs differ by less than 1e-6 (identical boxes excepted: there the lower
row must win), or its trace lies within 1e-6 of a bound; at most 0.5 % of the detections of a case (asserted; the chosen seeds leave
out none).  `err` is held, per term, to max(3 x the distance of the SAME reference evaluated in float32 from the float64 one, one
float32 ulp of the largest value of the term), distances measured as |a - b| / (1 + |b|); `sums / counts` to the same bound against
the float64 means; `counts` must be exact.  Two launches give the same bits.

Measured largest distances to float64 over both cases, kernel | float32 reference, under the host emulator (the kernel's float32
operations are the reference's there, so the two columns agree; no MI355X figures have been taken yet):
xy 1.6e-05 | 1.6e-05, z 4.8e-08 | 4.8e-08, w / h / l 3.9e-08 | 3.9e-08, dim 5.8e-08 | 5.8e-08, ry 6.5e-08 | 6.5e-08.
"""
import functools

import numpy as np
import pytest
import torch

I_IMAGES, N_CATS = 37, 5
DT_COUNTS, GT_COUNTS = (0, 1, 5, 100, 300), (0, 1, 7, 70)      # 300: more than one 256-thread pass; 70: more than one LDS chunk of 64
IOU_TOL, TIE_TOL, TRACE_TOL, LEFT_OUT_CAP = 1e-6, 1e-6, 1e-6, 0.005
TRACE_LO, TRACE_HI = -1.0 - 1e-4, 3.0 + 1e-4
SEEDS = (3, 8)
FAR = 3000.0                                                    # hand-placed boxes live here, away from the random ones (< 700)


def _rot_y(a, b=0.0):
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return Ry @ Rx


def _random_gt(rs):
    z = rs.uniform(2.0, 20.0)
    return dict(box=[rs.uniform(0, 500), rs.uniform(0, 500), rs.uniform(20, 150), rs.uniform(20, 150)], cat=int(rs.randint(N_CATS)),
                center=[rs.uniform(-0.3, 0.3) * z, rs.uniform(-0.3, 0.3) * z, z], dims=list(rs.uniform(0.3, 3.0, 3)),
                pose=_rot_y(rs.uniform(-np.pi, np.pi), rs.uniform(-0.2, 0.2)))


def _project(K, c):
    p = K @ np.asarray(c, np.float64)
    return p[:2] / c[2]


def _copy_of(rs, g, K, jitter):
    """a detection derived from ground truth g: the box shifted / scaled by up to `jitter` of its size, the 3D fields perturbed"""
    x, y, w, h = g["box"]
    box = [x + rs.uniform(-jitter, jitter) * w, y + rs.uniform(-jitter, jitter) * h, w * (1 + rs.uniform(-jitter, jitter)),
           h * (1 + rs.uniform(-jitter, jitter))]
    return dict(box=box, cat=g["cat"], c2d=list(_project(K, g["center"]) + rs.uniform(-6, 6, 2)), z=g["center"][2] + rs.uniform(-1, 1),
                dims=list(np.asarray(g["dims"]) + rs.uniform(-0.3, 0.3, 3)), pose=_rot_y(rs.uniform(-0.8, 0.8)) @ g["pose"])


def _random_dt(rs):
    return dict(box=[rs.uniform(0, 500), rs.uniform(0, 500), rs.uniform(20, 150), rs.uniform(20, 150)], cat=int(rs.randint(N_CATS)),
                c2d=list(rs.uniform(0, 600, 2)), z=rs.uniform(2, 20), dims=list(rs.uniform(0.3, 3.0, 3)),
                pose=_rot_y(rs.uniform(-np.pi, np.pi), rs.uniform(-0.2, 0.2)))


def _far_gt(k, cat, **kw):
    g = dict(box=[FAR + 400.0 * k, 100.0, 80.0, 60.0], cat=cat, center=[0.4, -0.2, 6.0 + k], dims=[1.0, 1.5, 2.0], pose=_rot_y(0.3 * k))
    g.update(kw)
    return g


def _exact_dt(g, K, **kw):
    d = dict(box=list(g["box"]), cat=g["cat"], c2d=list(_project(K, g["center"]) + [1.5, -2.0]), z=g["center"][2] + 0.25,
             dims=[g["dims"][0] + 0.1, g["dims"][1] - 0.2, g["dims"][2] + 0.3], pose=_rot_y(0.2) @ g["pose"])
    d.update(kw)
    return d


def _scene(seed):
    """-> per-image lists of ground truths and detections, the intrinsics, and the hand-placed detections as {name: (image, position)}"""
    rs = np.random.RandomState(seed)
    dt_n = [100, 5, 300] + list(rs.choice(DT_COUNTS, I_IMAGES - 3))
    gt_n = [70, 0, 70] + list(rs.choice(GT_COUNTS, I_IMAGES - 3))
    assert set(dt_n) == set(DT_COUNTS) and set(gt_n) == set(GT_COUNTS)
    Ks = [np.array([[rs.uniform(400, 700), 0.0, rs.uniform(250, 350)], [0.0, rs.uniform(400, 700), rs.uniform(200, 300)], [0.0, 0.0, 1.0]])
          for _ in range(I_IMAGES)]
    gts, dts = [], []
    for i in range(I_IMAGES):
        g = [_random_gt(rs) for _ in range(gt_n[i])]
        d = []
        for _ in range(dt_n[i]):
            if g and rs.rand() < 0.5:                     # about half: jittered copies, IoUs on both sides of 0.5
                d.append(_copy_of(rs, g[rs.randint(len(g))], Ks[i], 0.25))
            else:
                d.append(_random_dt(rs))
        gts.append(g)
        dts.append(d)
    # ---- hand-placed rows, all in image 0 (70 ground truths, 100 detections) ----
    K, g, d, names = Ks[0], gts[0], dts[0], {}
    g[10], g[11] = _far_gt(0, 1), _far_gt(0, 1, center=[0.1, 0.1, 9.0])       # two identical boxes: the lower row must win
    g[12] = _far_gt(1, 2)                                                     # the only overlap of "other_cat" has another category
    g[13] = _far_gt(2, 3)                                                     # holds the zero-area detection
    g[14] = _far_gt(3, 4, box=[FAR + 1200.0, 300.0, 0.0, 0.0])                # zero area, under a zero-area detection: union 0
    g[15] = _far_gt(4, 0, pose=np.eye(3))                                     # pose pair with trace 3.01
    g[63], g[64] = _far_gt(5, 1), _far_gt(6, 1)                               # last slot of the first LDS chunk, first slot of the next
    hand = [("identical", _exact_dt(g[10], K)), ("other_cat", _exact_dt(g[12], K, cat=3)),
            ("zero_area", _exact_dt(g[13], K, box=[FAR + 830.0, 120.0, 0.0, 0.0])),
            ("zero_union", _exact_dt(g[14], K)), ("trace", _exact_dt(g[15], K, pose=np.eye(3) * (3.01 / 3.0))),
            ("slot63", _exact_dt(g[63], K)), ("slot64", _exact_dt(g[64], K))]
    for k, (name, row) in enumerate(hand):
        d[20 + k] = row
        names[name] = (0, 20 + k)
    return gts, dts, Ks, names


def _flatten(gts, dts, Ks):
    f = lambda rows, key, width: np.asarray([np.asarray(r[key], np.float64).reshape(-1) for rows_i in rows for r in rows_i],     # noqa: E731
                                            np.float32).reshape(-1, width)
    off = lambda rows: np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int32)                                # noqa: E731
    cat = lambda rows: np.asarray([r["cat"] for rows_i in rows for r in rows_i], np.int32)                                      # noqa: E731
    return dict(dt_box=f(dts, "box", 4), dt_cat=cat(dts), dt_c2d=f(dts, "c2d", 2), dt_z=f(dts, "z", 1).reshape(-1), dt_dims=f(dts, "dims", 3),
                dt_pose=f(dts, "pose", 9), dt_off=off(dts), gt_box=f(gts, "box", 4), gt_cat=cat(gts), gt_center=f(gts, "center", 3),
                gt_dims=f(gts, "dims", 3), gt_pose=f(gts, "pose", 9), gt_off=off(gts),
                K=np.asarray(Ks, np.float32).reshape(-1, 9))


ARGS = ("dt_box", "dt_cat", "dt_c2d", "dt_z", "dt_dims", "dt_pose", "dt_off", "gt_box", "gt_cat", "gt_center", "gt_dims", "gt_pose",
        "gt_off", "K")


def _match_reference(a):
    """float64, a plain double loop -> match (D,), best IoU (D,), whether the row is left out of the comparison (D,)"""
    D = len(a["dt_cat"])
    match, best_iou, unsure = np.full(D, -1, np.int32), np.full(D, -1.0), np.zeros(D, bool)
    dt_box, gt_box = a["dt_box"].astype(np.float64).tolist(), a["gt_box"].astype(np.float64).tolist()
    dt_cat, gt_cat = a["dt_cat"].tolist(), a["gt_cat"].tolist()
    for i in range(len(a["dt_off"]) - 1):
        for d in range(a["dt_off"][i], a["dt_off"][i + 1]):
            x1, y1, w, h = dt_box[d]
            x2, y2 = x1 + w, y1 + h
            best, second, bj, second_j = -1.0, -1.0, -1, -1
            for g in range(a["gt_off"][i], a["gt_off"][i + 1]):
                if gt_cat[g] != dt_cat[d]:
                    continue
                gx1, gy1, gw, gh = gt_box[g]
                gx2, gy2 = gx1 + gw, gy1 + gh
                inter = max(min(x2, gx2) - max(x1, gx1), 0.0) * max(min(y2, gy2) - max(y1, gy1), 0.0)
                union = (x2 - x1) * (y2 - y1) + (gx2 - gx1) * (gy2 - gy1) - inter
                iou = inter / union if union > 0 else 0.0
                if iou > best:
                    best, second, bj, second_j = iou, best, g, bj
                elif iou > second:
                    second, second_j = iou, g
            best_iou[d] = best
            if bj >= 0 and best >= 0.5:
                match[d] = bj
            if bj >= 0:
                unsure[d] |= abs(best - 0.5) <= IOU_TOL
                if second_j >= 0 and best - second < TIE_TOL and best >= 0.5 - IOU_TOL and gt_box[bj] != gt_box[second_j]:
                    unsure[d] = True
    return match, best_iou, unsure


def _errors(a, match, dt):
    """the seven error terms of the pairs (d, match[d]) with every operation in `dt` -> err (D,7) (NaN where unmatched / ry skipped),
    trace (D,) in float64"""
    D = len(match)
    err, trace = np.full((D, 7), np.nan, dt), np.full(D, np.nan)
    d = np.flatnonzero(match >= 0)
    if len(d) == 0:
        return err, trace
    g = match[d]
    img = np.searchsorted(a["dt_off"], d, side="right") - 1
    K = a["K"].astype(dt)[img].reshape(-1, 3, 3)
    c = a["gt_center"].astype(dt)[g]
    u = (K[:, 0, 0] * c[:, 0] + K[:, 0, 1] * c[:, 1] + K[:, 0, 2] * c[:, 2]) / c[:, 2]
    v = (K[:, 1, 0] * c[:, 0] + K[:, 1, 1] * c[:, 1] + K[:, 1, 2] * c[:, 2]) / c[:, 2]
    c2d = a["dt_c2d"].astype(dt)[d]
    du, dv = c2d[:, 0] - u, c2d[:, 1] - v
    err[d, 0] = np.sqrt(du * du + dv * dv)
    err[d, 1] = np.abs(a["dt_z"].astype(dt)[d] - c[:, 2])
    dd = a["dt_dims"].astype(dt)[d] - a["gt_dims"].astype(dt)[g]
    err[d, 2:5] = np.abs(dd)
    err[d, 5] = np.sqrt(dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1] + dd[:, 2] * dd[:, 2])
    trace[d] = (a["dt_pose"].astype(np.float64)[d] * a["gt_pose"].astype(np.float64)[g]).sum(1)
    tr = trace[d].astype(dt)
    ry = dt(np.pi / 2) - dt(0.5) * (tr - dt(1.0))
    err[d, 6] = np.where((trace[d] >= TRACE_LO) & (trace[d] <= TRACE_HI), ry, dt(np.nan))
    return err, trace


@functools.lru_cache(maxsize=None)
def _case(seed):
    """the arrays and their references, computed once and shared (never written to)"""
    gts, dts, Ks, names = _scene(seed)
    a = _flatten(gts, dts, Ks)
    match, best_iou, unsure = _match_reference(a)
    err64, trace = _errors(a, match, np.float64)
    err32, _ = _errors(a, match, np.float32)
    with np.errstate(invalid="ignore"):
        unsure = unsure | (np.abs(trace - TRACE_LO) <= TRACE_TOL) | (np.abs(trace - TRACE_HI) <= TRACE_TOL)
    rows = {n: int(a["dt_off"][i]) + k for n, (i, k) in names.items()}
    out = dict(a, match=match, best_iou=best_iou, unsure=unsure, err64=err64, err32=err32, trace=trace, rows=rows)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@pytest.mark.parametrize("seed", SEEDS)
def test_reference_alone_meets_the_conditions(seed):
    """conditions on the chosen seeds and on the hand-placed rows, checked with the float64 reference alone"""
    c = _case(seed)
    D = len(c["match"])
    assert len(c["dt_off"]) - 1 == I_IMAGES
    assert c["unsure"].sum() <= LEFT_OUT_CAP * D, (int(c["unsure"].sum()), D)
    m, iou, r, g0 = c["match"], c["best_iou"], c["rows"], int(c["gt_off"][0])
    matched = m >= 0
    assert matched.sum() > 100 and ((iou > 0.2) & (iou < 0.5)).sum() > 100                   # matches on both sides of 0.5
    assert m[r["identical"]] == g0 + 10 and iou[r["identical"]] == 1.0
    assert m[r["other_cat"]] == -1 and iou[r["other_cat"]] <= 0.0                            # no same-category candidate overlaps ...
    assert m[r["zero_area"]] == -1 and iou[r["zero_area"]] == 0.0                            # ... IoU 0 with the box that holds it
    assert m[r["zero_union"]] == -1 and iou[r["zero_union"]] == 0.0
    assert m[r["trace"]] == g0 + 15 and abs(c["trace"][r["trace"]] - 3.01) < 1e-6
    assert np.isnan(c["err64"][r["trace"], 6]) and np.isfinite(c["err64"][r["trace"], :6]).all()
    assert m[r["slot63"]] == g0 + 63 and m[r["slot64"]] == g0 + 64
    per_image = np.diff(c["dt_off"])
    no_gt = (np.diff(c["gt_off"]) == 0) & (per_image > 0)
    assert no_gt[1] and per_image.max() == 300 and np.diff(c["gt_off"]).max() == 70
    assert np.isfinite(c["err64"][matched, 6]).sum() == matched.sum() - 1                    # every other matched pair has a valid ry


def _dist(a, b):
    return float((np.abs(a - b) / (1.0 + np.abs(b))).max()) if len(a) else 0.0


def _launch(dev, a):
    from omni3d_amd.kernels import viserr
    return viserr.match_errors(*[torch.from_numpy(np.array(a[k])).to(dev) for k in ARGS])


def _bits(t):
    return t.cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def _run_case(dev, seed):
    c = _case(seed)
    outs = [_launch(dev, c) for _ in range(2)]
    for x, y in zip(*outs):
        assert torch.equal(_bits(x), _bits(y))                                                # two launches are bit-identical
    match, err, sums, counts = [o.cpu().numpy() for o in outs[0]]
    D, keep = len(c["match"]), ~c["unsure"]
    assert c["unsure"].sum() <= LEFT_OUT_CAP * D
    assert np.array_equal(match[keep], c["match"][keep]), int((match != c["match"])[keep].sum())
    # the left-out rows: whatever the kernel decided among the admissible outcomes enters the expected sums
    used = np.where(keep, c["match"], match)
    for d in np.flatnonzero(~keep & (match >= 0)):
        i = np.searchsorted(c["dt_off"], d, side="right") - 1
        assert c["gt_off"][i] <= match[d] < c["gt_off"][i + 1] and c["gt_cat"][match[d]] == c["dt_cat"][d]
    err64, _ = (c["err64"], None) if np.array_equal(used, c["match"]) else _errors(c, used, np.float64)
    err32, _ = (c["err32"], None) if np.array_equal(used, c["match"]) else _errors(c, used, np.float32)
    matched = used >= 0
    assert np.isnan(err[~matched]).all()
    ry_ok = np.where(keep, np.isfinite(err64[:, 6]), np.isfinite(err[:, 6])) & matched
    assert np.array_equal(np.isfinite(err[:, 6])[keep], np.isfinite(err64[:, 6])[keep])
    assert counts.tolist() == [int(matched.sum()), int(ry_ok.sum())]
    worst = {}
    for q, name in enumerate(("xy", "z", "w", "h", "l", "dim", "ry")):
        rows = ry_ok if q == 6 else matched
        want, ref32 = err64[rows, q], err32[rows, q].astype(np.float64)
        e_hip, e_ref = _dist(err[rows, q].astype(np.float64), want), _dist(ref32, want)
        ulp = float(np.spacing(np.float32(want.max()))) / (1.0 + float(want.max()))
        n = counts[1 if q == 6 else 0]
        m_hip, m_ref = _dist(np.array([sums[q] / n]), np.array([want.mean()])), _dist(np.array([ref32.mean()]), np.array([want.mean()]))
        m_ulp = float(np.spacing(np.float32(want.mean()))) / (1.0 + float(want.mean()))
        print("seed %d %-3s: |hip-fp64| %.2e  |ref32-fp64| %.2e  ulp %.2e   means: %.2e | %.2e  ulp %.2e" % (seed, name, e_hip, e_ref, ulp, m_hip, m_ref, m_ulp))
        assert e_hip <= max(3.0 * e_ref, ulp), (name, e_hip, e_ref, ulp)
        assert m_hip <= max(3.0 * m_ref, m_ulp), (name, m_hip, m_ref, m_ulp)
        worst[name] = (e_hip, e_ref)
    return worst


@pytest.mark.parametrize("seed", SEEDS)
def test_match_errors_emulated(emu_lib, seed):
    _run_case("cpu", seed)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_match_errors_gpu(hip_lib, seed):
    _run_case("cuda", seed)


# ---- empty inputs ------------------------------------------------------------------------------------------------------------------

def _subset(c, images, keep_dt=True, keep_gt=True):
    """the first `images` images of a case, optionally without their detections / ground truths"""
    a = {k: np.array(c[k]) for k in ARGS}
    D, G = int(a["dt_off"][images]) if keep_dt else 0, int(a["gt_off"][images]) if keep_gt else 0
    for k in ARGS:
        if k.startswith("dt_") and k != "dt_off":
            a[k] = a[k][:D]
        elif k.startswith("gt_") and k != "gt_off":
            a[k] = a[k][:G]
    a["dt_off"] = a["dt_off"][:images + 1] if keep_dt else np.zeros(images + 1, np.int32)
    a["gt_off"] = a["gt_off"][:images + 1] if keep_gt else np.zeros(images + 1, np.int32)
    a["K"] = a["K"][:images]
    return a


def _run_empty(dev):
    c = _case(SEEDS[0])
    for images, keep_dt, keep_gt in ((0, True, True), (3, False, True), (3, True, False), (3, False, False)):
        a = _subset(c, images, keep_dt, keep_gt)
        match, err, sums, counts = [o.cpu().numpy() for o in _launch(dev, a)]
        assert match.shape == (len(a["dt_cat"]),) and err.shape == (len(a["dt_cat"]), 7)
        assert (match == -1).all() and np.isnan(err).all()
        assert sums.tolist() == [0.0] * 7 and counts.tolist() == [0, 0]
    # the first three images alone give what the reference gives for them
    a = _subset(c, 3)
    match, err, sums, counts = [o.cpu().numpy() for o in _launch(dev, a)]
    D = len(a["dt_cat"])
    keep = ~c["unsure"][:D]
    assert np.array_equal(match[keep], c["match"][:D][keep]) and counts[0] == (match >= 0).sum()


def test_empty_inputs_emulated(emu_lib):
    _run_empty("cpu")


@pytest.mark.gpu
def test_empty_inputs_gpu(hip_lib):
    _run_empty("cuda")


# ---- launcher contracts ------------------------------------------------------------------------------------------------------------

def test_launcher_rejects_bad_inputs(emu_lib, monkeypatch):
    """a wrong dtype, a non-contiguous input, offsets that decrease or do not end at D / G: ValueError before any launch"""
    from omni3d_amd.kernels import viserr
    c = _case(SEEDS[0])
    good = {k: torch.from_numpy(np.array(v)) for k, v in _subset(c, 3).items()}
    monkeypatch.setattr(emu_lib, "call", lambda *a, **k: pytest.fail("launched"))

    def bad(**changes):
        with pytest.raises(ValueError):
            viserr.match_errors(*[changes.get(k, good[k]) for k in ARGS])

    bad(dt_box=good["dt_box"].double())
    bad(dt_cat=good["dt_cat"].long())
    bad(gt_off=good["gt_off"].long())
    bad(K=good["K"].half())
    bad(gt_box=good["gt_box"].repeat(1, 2)[:, ::2])                                           # right shape, strided
    bad(dt_pose=good["dt_pose"].t().contiguous().t())
    bad(dt_dims=good["dt_dims"][:-1])
    dec = good["dt_off"].clone()
    dec[1], dec[2] = dec[2].item(), dec[1].item() - 1
    bad(dt_off=dec)
    short = good["gt_off"].clone()
    short[-1] -= 1
    bad(gt_off=short)
    bad(dt_off=good["dt_off"] + 1)
    bad(dt_off=good["dt_off"][:-1])
