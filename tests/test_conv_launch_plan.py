"""The launch decisions of csrc/conv_gemm.hip's host code, pinned (tools/make_conv_plan_golden.py, tests/golden/conv_launch_plan.npz).

  * the `plan` mode of every deterministic launcher -- {tile, splits, counters, workspace floats} and the status code -- over a grid of
    some thousands of problems is recomputed with the host-emulated library and compared EXACTLY with the record;
  * one small launch per branch the plan does not show (zero-fill, statistics attach and *nblk_out, classic or deep-prefetch body,
    workgroup order, follow-up ReLU pass, grid shape) runs on the emulator, which is sequential and so bit-reproducible even for the
    atomic forms: the CRC-32 of the output bytes and *nblk_out equal the record;
  * the record alone covers what it is for: every tile of every launcher, split counts on both levels of split_reduce.h's group
    table, a refusal per launcher;
  * GPU: the same launches against a float64 einsum of the same inputs, with the tolerances of tests/test_conv.py for that kernel
    family (GPU bits are not pinned: the atomic forms are not reproducible there by design)."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT


@functools.lru_cache(maxsize=None)
def _tool():
    spec = importlib.util.spec_from_file_location("make_conv_plan_golden", os.path.join(ROOT, "tools", "make_conv_plan_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _gold():
    with np.load(os.path.join(ROOT, "tests", "golden", "conv_launch_plan.npz")) as z:
        return {k: z[k] for k in z.files}


def test_plans_equal_the_record(emu_lib):
    T, gold = _tool(), _gold()
    rows = T.plan_rows()
    assert np.array_equal(rows, gold["rows"]), "the grid of the tool is not the recorded one"
    plans, status = T.compute_plans(emu_lib, rows)
    bad = np.flatnonzero((plans != gold["plans"]).any(axis=1) | (status != gold["status"]))
    assert bad.size == 0, [(T.LAUNCHERS[rows[i, 0]], rows[i, 1:].tolist(), (int(status[i]), plans[i].tolist()),
                            (int(gold["status"][i]), gold["plans"][i].tolist())) for i in bad[:5]]


def test_launches_equal_the_record(emu_lib):
    T, gold = _tool(), _gold()
    assert [n for n, _, _ in T.LAUNCHES] == gold["launch_names"].tolist()
    got = T.compute_launches(emu_lib)
    bad = [(n, g.tolist(), w.tolist()) for (n, _, _), g, w in zip(T.LAUNCHES, got, gold["launches"]) if not np.array_equal(g, w)]
    assert not bad, bad          # [CRC-32 of the output bytes, *nblk_out, tile, splits, counters, workspace floats]: got, recorded


def test_the_record_covers_what_it_is_for():
    T, gold = _tool(), _gold()
    rows, plans, status = gold["rows"], gold["plans"], gold["status"]
    reported = (status == 0) & (plans[:, 0] != T.UNTOUCHED)
    assert not ((status != 0) & (plans != T.UNTOUCHED).any(axis=1)).any()       # a refusal reports nothing
    assert set(status.tolist()) == {0, 1}
    for kind, name in enumerate(T.LAUNCHERS):
        mine = rows[:, 0] == kind
        assert (mine & (status != 0)).any(), name                                # at least one refusal each
        ids = set(plans[mine & reported, 0].tolist())
        want = {1, 2, 3, 4} if kind <= T.WGRAD_MULTI else {1, 2} if kind == T.BWGRAD else {2}      # tile ids; algorithm ids of the batched forms
        assert want <= ids, (name, ids)
    conv = reported & (rows[:, 0] != T.BWGRAD_MULTI)                             # (the multi-problem form reports 0 splits)
    for lo, hi in ((1, 1), (2, 8), (9, 16), (17, 1 << 40)):                      # no group level, 4-wide groups, 8-wide and beyond
        hit = conv & (plans[:, 1] >= lo) & (plans[:, 1] <= hi)
        assert hit.any(), (lo, hi)
        if lo > 1:
            assert (plans[hit, 2] > 0).all() and (plans[hit, 3] > 0).all()
    names = gold["launch_names"].tolist()
    assert len(names) >= 12 and gold["launches"][names.index("fwd_ordered_stats"), 1] > 0       # a statistics attach is in the record


# ---- GPU twin: the same launches against float64 -----------------------------------------------------------------------------
def _cols(x, R, s, p):
    """NHWC input -> (N, C * R * R, OH * OW) patches in float64, channel-major like a (K, C, R, R) filter"""
    return F.unfold(x.permute(0, 3, 1, 2).double(), R, padding=p, stride=s)


def _check_launch(T, kind, q, r):
    out = r["out"][0].double()
    if kind in (T.BWGRAD, T.BWGRAD_MULTI):
        for x, dy, dw in zip(r["xs"], r["dys"], r["out"]):
            ref = torch.einsum("bmk,bmc->bkc", dy.double(), x.double())
            assert (dw.double() - ref).abs().max() <= 1e-4 * ref.abs().max(), q          # (an empty problem: exact zeros)
        return
    N, H, C, K, R, s, p = q["g"]
    x, w, dy = r["x"], r["w"], r["dy"]
    w2 = w.permute(0, 3, 1, 2).reshape(K, C * R * R).double()
    if kind in (T.FWD, T.FWD_MULTI):
        ref = torch.einsum("kq,nql->nlk", w2, _cols(x, R, s, p))
        scale = float(torch.einsum("kq,nql->nlk", w2.abs(), _cols(x.abs(), R, s, p)).max())
        if r["bias"] is not None:
            ref = ref + r["bias"].double()
        if q["relu"]:
            ref = ref.clamp(min=0)
        err = 2e-5 * scale + 1e-6
        assert (out.reshape(ref.shape) - ref).abs().max() <= err, q
        if len(r["out"]) > 1:                    # BatchNorm partial statistics [m-tile][2][K]: column sums and sums of squares of the output
            st = r["out"][1].double().sum(0)
            M = ref.shape[0] * ref.shape[1]
            bm = {1: 128, 2: 64, 3: 128, 4: 256}[r["plan"][0]]
            assert r["nblk"] == (M + bm - 1) // bm
            flat = ref.reshape(M, K)
            assert (st[:K] - flat.sum(0)).abs().max() <= M * err + 1e-6 * float(flat.abs().sum(0).max())
            assert (st[K:] - (flat * flat).sum(0)).abs().max() <= M * (2 * float(flat.abs().max()) * err + err * err) + 1e-6 * float((flat * flat).sum(0).max())
        else:
            assert r["nblk"] == 0
        return
    before = r["before"][0].double()
    if kind == T.DGRAD:
        ref = F.fold(torch.einsum("kq,nlk->nql", w2, dy.reshape(N, -1, K).double()), (H, H), R, padding=p, stride=s).permute(0, 2, 3, 1)
        if q["acc"]:
            ref = ref + before[..., :C]
        assert (out[..., :C] - ref).abs().max() <= 2e-5 * (float(ref.abs().max()) * 4 + 1) + 1e-6, q
        assert torch.equal(out[..., C:], before[..., C:])        # the pitch padding is not written
        return
    if N == 0:
        ref = torch.zeros(K, R, R, C, dtype=torch.float64)
    else:
        ref = torch.einsum("nlk,nql->kq", dy.reshape(N, -1, K).double(), _cols(x, R, s, p)).reshape(K, C, R, R).permute(0, 2, 3, 1)
    if q["acc"]:
        ref = ref + before
    assert (out - ref).abs().max() <= 2e-5 * (float(ref.abs().max()) * 4 + 1) + 1e-6, q


def test_launch_references_emulated(emu_lib):
    """the float64 references of the GPU twin, exercised on the emulator's results"""
    T = _tool()
    for _, kind, q in T.LAUNCHES:
        _check_launch(T, kind, q, T.run_launch(emu_lib, kind, q))


@pytest.mark.gpu
def test_launches_gpu(hip_lib):
    T = _tool()
    for _, kind, q in T.LAUNCHES:
        _check_launch(T, kind, q, T.run_launch(hip_lib, kind, q, dev="cuda"))
