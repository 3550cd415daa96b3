"""csrc/annotate.hip `omni_box_annotate` (`kernels.annotate.box_annotate`) against tests/golden/box_annotate.npz -- the recorded
results of the reference's own `get_cuboid_verts`, `convert_3d_box_to_2d(..., XYWH=False)` and `estimate_truncation` for 377 boxes
over 9 images (tools/make_annotate_golden.py) -- and against a float64 evaluation of the same formulas written here.

`behind`, `fully_behind` and the [-1, -1, -1, -1] marker of `trunc` must be exact (the fixture holds no box with a vertex within 1e-4
of min_z or a behind vertex within 1e-4 of x = 0 / y = 0, so every decision is unambiguous).  `verts3d`, `verts2d`, `proj` are held,
per output and as |a - b| / (1 + |b|), to max(3 x the distance of the reference's recorded float32 result from the float64
evaluation, one float32 ulp of the largest value); the factor 3 leaves room for another order of the three-term sums and for FMA
contraction.  `truncation` must equal the float64 formula applied to the kernel's OWN float32 `proj` to 1e-12, be NaN exactly where
the reference's is and exactly 1.0 where the box is fully behind; against the recorded reference it is held to the `proj` bound
propagated through the formula (see `_truncation_bound`).  Two launches give the same bits.

Measured largest distances to float64, kernel | float32 reference:
  host emulator  verts3d 1.5e-07 | 1.5e-07, verts2d 2.9e-05 | 2.9e-05, proj 1.2e-06 | 1.2e-06 (the same float32 operations as the reference)
  MI355X         no figures have been taken yet
"""
import functools
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "box_annotate.npz")
REFERENCE = os.environ.get("OMNI3D_REFERENCE", "/root/reference")
ARGS = ("box3d", "R", "box_off", "K", "size")
OUTS = ("verts3d", "verts2d", "proj", "trunc", "truncation", "behind", "fully_behind")
SX = np.array([-1, 1, 1, -1, -1, 1, 1, -1]) * 0.5
SY = np.array([-1, -1, 1, 1, -1, -1, 1, 1]) * 0.5
SZ = np.array([-1, -1, -1, -1, 1, 1, 1, 1]) * 0.5


def _truncation64(proj, xmax, ymax, fully):
    """the formula of the issue in float64 on a (N,4) XYXY box: 1 where fully behind, else 1 - area(box ^ frame) / area(box)"""
    p = proj.astype(np.float64)
    iw = np.clip(np.minimum(p[:, 2], xmax) - np.maximum(p[:, 0], 0.0), 0.0, None)
    ih = np.clip(np.minimum(p[:, 3], ymax) - np.maximum(p[:, 1], 0.0), 0.0, None)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = 1.0 - iw * ih / ((p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1]))
    return np.where(fully, 1.0, t)


@functools.lru_cache(maxsize=None)
def _case():
    """the fixture and the float64 evaluation of its inputs, computed once and shared (never written to)"""
    g = dict(np.load(GOLDEN))
    box, R = g["box3d"].astype(np.float64), g["R"].astype(np.float64).reshape(-1, 3, 3)
    N = len(box)
    img = np.searchsorted(g["box_off"], np.arange(N), side="right") - 1
    K = g["K"].astype(np.float64).reshape(-1, 3, 3)[img]
    xmax, ymax = (g["size"][img, 0] - 1).astype(np.float64), (g["size"][img, 1] - 1).astype(np.float64)
    local = np.stack((box[:, 5:6] * SX, box[:, 4:5] * SY, box[:, 3:4] * SZ), axis=1)            # (N,3,8)
    v3 = (R @ local).transpose(0, 2, 1) + box[:, None, :3]
    h = np.einsum("nij,nkj->nki", K, v3)
    with np.errstate(invalid="ignore", divide="ignore"):
        v2 = np.stack((h[:, :, 0] / h[:, :, 2], h[:, :, 1] / h[:, :, 2], h[:, :, 2]), axis=2)
    vb = v2[:, :, 2] <= float(g["min_z"])
    u, v = v2[:, :, 0].copy(), v2[:, :, 1].copy()
    sub = vb & (v3[:, :, 0] != 0) & (v3[:, :, 1] != 0)
    u[sub] = np.where(v3[:, :, 0] > 0, xmax[:, None], 0.0)[sub]
    v[sub] = np.where(v3[:, :, 1] > 0, ymax[:, None], 0.0)[sub]
    proj = np.stack((u.min(1), v.min(1), u.max(1), v.max(1)), axis=1)
    fully = vb.all(1)
    cut = np.stack((np.maximum(proj[:, 0], 0), np.maximum(proj[:, 1], 0), np.minimum(proj[:, 2], xmax), np.minimum(proj[:, 3], ymax)), axis=1)
    marker = fully | ~((cut[:, 2] > cut[:, 0]) & (cut[:, 3] > cut[:, 1]))
    out = dict(g, img=img, xmax=xmax, ymax=ymax, v3=v3, v2=v2, vb=vb, proj64=proj, behind64=vb.any(1), fully64=fully, marker=marker, cut64=cut)
    for a in out.values():
        a.setflags(write=False)
    return out


def test_fixture_alone_meets_the_conditions():
    """what the issue asks of the fixture, checked on the file and the float64 evaluation alone"""
    c = _case()
    N, sizes = len(c["box3d"]), c["size"].tolist()
    assert 350 <= N <= 450 and len(sizes) == 9 and int(c["rejected"]) >= 0
    assert all(s in sizes for s in ([33, 17], [50, 40], [16, 16], [640, 480]))
    assert 0 in np.diff(c["box_off"])                                                          # one image without a box
    assert (np.abs(c["v2"][:, :, 2] - float(c["min_z"])) >= 1e-4).all()
    assert (np.abs(c["v3"][:, :, 0][c["vb"]]) >= 1e-4).all() and (np.abs(c["v3"][:, :, 1][c["vb"]]) >= 1e-4).all()
    assert np.array_equal(c["ref_behind"], c["behind64"]) and np.array_equal(c["ref_fully"], c["fully64"])
    nb = c["vb"].sum(1)
    for k in range(1, 8):                                                                      # k vertices behind, in every sign quadrant
        for qx in (-1, 1):
            for qy in (-1, 1):
                rows = (nb == k) & (np.sign(c["v3"][:, :, 0]) == qx).all(1) & (np.sign(c["v3"][:, :, 1]) == qy).all(1)
                assert rows.any(), (k, qx, qy)
    t = c["ref_truncation"]
    assert c["fully64"].sum() >= 8 and (t[c["fully64"]] == 1.0).all()
    assert ((t > 0) & (t < 1)).sum() >= 30 and ((t == 1.0) & ~c["fully64"]).sum() >= 8 and (t == 0).sum() >= 30
    flat = np.flatnonzero(np.isnan(t))
    assert len(flat) == 1 and c["box3d"][flat[0], 3] == 0.0
    p = c["ref_proj"][flat[0]]
    assert (p[2] - p[0]) * (p[3] - p[1]) == 0.0
    assert c["marker"].sum() > c["fully64"].sum() and (~c["marker"]).sum() > 100


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "cubercnn")), reason="needs the reference checkout")
def test_fixture_is_what_the_reference_returns():
    """re-runs the reference's three functions on the recorded inputs (CPU) and compares with the file, bit for bit"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_annotate_golden", os.path.join(ROOT, "tools", "make_annotate_golden.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    c = _case()
    inp = tool.make_inputs()
    for k in ARGS + ("min_z", "rejected"):
        assert np.array_equal(inp[k], c[k]), k
    for k, v in tool.record({k: np.array(c[k]) for k in ARGS + ("min_z",)}).items():
        assert np.array_equal(v, c[k], equal_nan=True), k


def _dist(a, b):
    ok = np.isfinite(b)
    assert np.array_equal(np.isfinite(a), ok)
    return float((np.abs(a[ok] - b[ok]) / (1.0 + np.abs(b[ok]))).max())


def _launch(dev, c, **changes):
    from omni3d_amd.kernels import annotate
    args = [changes[k] if k in changes else torch.from_numpy(np.array(c[k])).to(dev) for k in ARGS]
    return annotate.box_annotate(*args, min_z=float(c["min_z"]))


def _bits(t):
    return t.cpu().contiguous().view({1: torch.uint8, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _truncation_bound(c, proj, b_proj):
    """|truncation - recorded reference| allowed per box.  t = 1 - I / A with A = w h the area of proj and I <= A that of its part in
    the frame.  When every coordinate moves by at most d, w and h move by at most 2 d, so |dA| and |dI| <= 2 d (w + h) + 4 d^2, and
    |dt| <= |dI| / A + I |dA| / A^2 <= 2 (2 d (w + h) + 4 d^2) / A.  d: the kernel's and the reference's proj each lie within b_proj
    (1 + |coordinate|) of the float64 one, and the reference goes through XYWH in float32 (w = fl(x2 - x1), read back as x1 + w), one
    more rounding of w / h: d = 2 b_proj (1 + max |coordinate|) + 2^-24 max(w, h).  1e-12 for the float64 arithmetic itself."""
    p = proj.astype(np.float64)
    w, h = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    d = 2.0 * b_proj * (1.0 + np.abs(p).max(1)) + 2.0 ** -24 * np.maximum(w, h)
    with np.errstate(invalid="ignore", divide="ignore"):
        return 2.0 * (2.0 * d * (w + h) + 4.0 * d * d) / (w * h) + 1e-12


def _run(dev):
    c = _case()
    outs = [_launch(dev, c) for _ in range(2)]
    for x, y in zip(*outs):
        assert torch.equal(_bits(x), _bits(y))                                                 # two launches are bit-identical
    o = {k: v.cpu().numpy() for k, v in zip(OUTS, outs[0])}
    N = len(c["box3d"])
    assert o["verts3d"].shape == (N, 8, 3) and o["verts2d"].shape == (N, 8, 3) and o["proj"].shape == (N, 4) and o["trunc"].shape == (N, 4)
    assert o["truncation"].dtype == np.float64 and o["behind"].dtype == np.uint8 and o["fully_behind"].dtype == np.uint8
    # decisions: exact
    assert np.array_equal(o["behind"].astype(bool), c["ref_behind"]) and np.array_equal(o["fully_behind"].astype(bool), c["ref_fully"])
    is_marker = (o["trunc"] == -1).all(1)
    assert np.array_equal(is_marker, c["marker"]), np.flatnonzero(is_marker != c["marker"])
    p, keep = o["proj"], ~c["marker"]
    own_cut = np.stack((np.maximum(p[:, 0], 0), np.maximum(p[:, 1], 0), np.minimum(p[:, 2], c["xmax"].astype(np.float32)),
                        np.minimum(p[:, 3], c["ymax"].astype(np.float32))), axis=1)
    assert np.array_equal(o["trunc"][keep], own_cut[keep])                                     # the cut of its own proj, bit for bit
    # values
    worst = {}
    for name, want, ref in (("verts3d", c["v3"], c["ref_verts3d"]), ("verts2d", c["v2"], c["ref_verts2d"]), ("proj", c["proj64"], c["ref_proj"])):
        e_hip, e_ref = _dist(o[name].astype(np.float64), want), _dist(ref.astype(np.float64), want)
        big = float(np.abs(want[np.isfinite(want)]).max())
        ulp = float(np.spacing(np.float32(big))) / (1.0 + big)
        print("%-7s |kernel-fp64| %.2e  |ref32-fp64| %.2e  ulp %.2e" % (name, e_hip, e_ref, ulp))
        assert e_hip <= max(3.0 * e_ref, ulp), (name, e_hip, e_ref, ulp)
        worst[name] = max(3.0 * e_ref, ulp)
    # truncation: the float64 formula on the kernel's own proj; NaN and 1.0 where the reference has them
    t, fully = o["truncation"], c["ref_fully"]
    own = _truncation64(p, c["xmax"], c["ymax"], fully)
    assert np.array_equal(np.isnan(t), np.isnan(c["ref_truncation"])) and np.array_equal(np.isnan(t), np.isnan(own))
    ok = ~np.isnan(t)
    assert np.abs(t[ok] - own[ok]).max() <= 1e-12 and (t[fully] == 1.0).all()
    bound = _truncation_bound(c, p, worst["proj"])
    diff = np.abs(t[ok & ~fully] - c["ref_truncation"][ok & ~fully])
    print("truncation: largest |kernel - reference| %.2e, largest bound / diff margin %.2e" % (diff.max(), (diff - bound[ok & ~fully]).max()))
    assert (diff <= bound[ok & ~fully]).all(), float((diff - bound[ok & ~fully]).max())


def test_box_annotate_emulated(emu_lib):
    _run("cpu")


@pytest.mark.gpu
def test_box_annotate_gpu(hip_lib):
    _run("cuda")


# ---- empty inputs ------------------------------------------------------------------------------------------------------------------

def _run_empty(dev):
    c = _case()
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)                              # noqa: E731
    for I in (0, 3):
        outs = _launch(dev, c, box3d=z((0, 6), torch.float32), R=z((0, 9), torch.float32), box_off=z((I + 1,), torch.int32),
                       K=torch.from_numpy(np.array(c["K"][:I])).to(dev), size=torch.from_numpy(np.array(c["size"][:I])).to(dev))
        assert [tuple(t.shape) for t in outs] == [(0, 8, 3), (0, 8, 3), (0, 4), (0, 4), (0,), (0,), (0,)]
    # the first two images alone give the rows of the whole
    n = int(c["box_off"][2])
    sub = _launch(dev, c, box3d=torch.from_numpy(np.array(c["box3d"][:n])).to(dev), R=torch.from_numpy(np.array(c["R"][:n])).to(dev),
                  box_off=torch.from_numpy(np.array(c["box_off"][:3])).to(dev), K=torch.from_numpy(np.array(c["K"][:2])).to(dev),
                  size=torch.from_numpy(np.array(c["size"][:2])).to(dev))
    for a, b in zip(sub, _launch(dev, c)):
        assert torch.equal(_bits(a), _bits(b[:n]))


def test_empty_inputs_emulated(emu_lib):
    _run_empty("cpu")


@pytest.mark.gpu
def test_empty_inputs_gpu(hip_lib):
    _run_empty("cuda")


# ---- launcher contracts ------------------------------------------------------------------------------------------------------------

def test_launcher_rejects_bad_inputs(emu_lib, monkeypatch):
    """a wrong dtype, shape or stride, offsets that do not start at 0, decrease or do not end at N, inputs on two devices: ValueError
    before any launch, from both launchers"""
    from omni3d_amd.kernels import annotate
    c = _case()
    good = {k: torch.from_numpy(np.array(c[k])) for k in ARGS}
    monkeypatch.setattr(emu_lib, "call", lambda *a, **k: pytest.fail("launched"))

    def bad(**changes):
        for fn in (annotate.box_annotate, annotate.visibility_ragged):
            with pytest.raises(ValueError):
                fn(*[changes.get(k, good[k]) for k in ARGS])

    bad(box3d=good["box3d"].double())
    bad(R=good["R"].half())
    bad(box_off=good["box_off"].long())
    bad(size=good["size"].long())
    bad(K=good["K"].double())
    bad(box3d=good["box3d"].repeat(1, 2)[:, ::2])                                              # right shape, strided
    bad(R=good["R"].t().contiguous().t())
    bad(box3d=good["box3d"][:-1])
    bad(K=good["K"][:-1])
    bad(size=good["size"].t().contiguous())
    dec = good["box_off"].clone()
    dec[1], dec[2] = dec[2].item(), dec[1].item() - 1
    bad(box_off=dec)
    short = good["box_off"].clone()
    short[-1] -= 1
    bad(box_off=short)
    bad(box_off=good["box_off"] + 1)
    bad(box_off=good["box_off"][:-1])
    bad(K=torch.empty(tuple(good["K"].shape), dtype=torch.float32, device="meta"))             # two devices
    with pytest.raises(ValueError):
        annotate.visibility_ragged(*[good[k] for k in ARGS], zplane=0.0)
    with pytest.raises(ValueError):
        annotate.visibility_ragged(*[torch.zeros_like(good[k]) if k == "size" else good[k] for k in ARGS])
