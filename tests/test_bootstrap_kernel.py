"""csrc/eval_bootstrap.hip (`kernels.bootstrap`: omni_eval_bootstrap_counts, omni_eval_bootstrap) against its definition: the result
of a replicate with image multiplicities w IS what the existing evaluate() / accumulate() give on the split in which image i is
physically present w[i] times.  `ar` must be equal, `ap` within 1e-12 of `precision.mean(axis=1)` (the kernel sums the same 101 doubles
in another order: <= 100 x 2^-53 x 101 = 1.1e-12 on the sum, 1.1e-14 on the mean), -1 in exactly the same places.

Largest |ap - precision.mean(axis=1)| over the six replicates (3D | 2D), printed by every run under `-s`:
    host emulator   1.9e-15 | 8.9e-16
    MI355X          1.9e-15 | 8.9e-16
"""
import numpy as np
import pytest
import torch

import bootstrap_scene as S


def _run_duplication():
    gts, dts = S.scene()
    W = S.weight_rows()
    assert sum(1 for d in dts if d["category_id"] == 1) == 130
    assert max(sum(1 for d in dts if d["category_id"] == 2 and d["image_id"] == i) for i in S.IMGS) == 14
    assert sum(g["ignore3D"] for g in gts) >= 3
    depth = np.array([g["depth"] for g in gts])
    assert (depth < 10).sum() >= 3 and ((depth > 10) & (depth < 35)).sum() >= 3 and (depth > 35).sum() >= 3
    worst = {}
    for mode in ("3D", "2D"):
        ev = S.evaluate(gts, dts, mode=mode, accumulate=False)
        got = ev.bootstrap(weights=W)
        assert got["ap"].shape == got["ar"].shape == (6, 10, 3, 4, 3) and got["ap"].dtype == np.float64
        worst[mode] = 0.0
        for b, w in enumerate(W):
            g2, d2, imgs = S.duplicated(gts, dts, w)
            ref = S.evaluate(g2, d2, imgs=imgs, mode=mode)
            want_ap, want_ar = ref.eval["precision"].mean(axis=1), ref.eval["recall"]
            assert np.array_equal(got["ap"][b] == -1, want_ap == -1) and np.array_equal(got["ar"][b] == -1, want_ar == -1), (mode, b)
            assert np.array_equal((ref.eval["precision"] == -1).all(axis=1), want_ap == -1)               # -1 for all r or for none
            assert np.array_equal(got["ar"][b], want_ar), (mode, b)
            err = float(np.abs(got["ap"][b] - want_ap).max())
            worst[mode] = max(worst[mode], err)
            assert err <= 1e-12, (mode, b, err)
            assert (want_ap > 0).any() and (want_ap[want_ap > -1] < 1).any()                            # something matched, not everything
            if b == 3:                                                                                  # the replicate without category 3
                assert (want_ap[:, 2] == -1).all() and (got["ap"][b][:, 2] == -1).all() and (want_ap[:, 0, 0] > -1).all()
        # the cuts at maxDets and the ranges really differ
        assert not np.array_equal(got["ap"][0][..., 0], got["ap"][0][..., 1]) and not np.array_equal(got["ap"][0][..., 1], got["ap"][0][..., 2])
        assert not np.array_equal(got["ap"][0][:, :, 1], got["ap"][0][:, :, 2])
    print("|ap - precision.mean(axis=1)| 3D %.2e 2D %.2e" % (worst["3D"], worst["2D"]))


def test_equals_physical_duplication_emulated(emu_lib):
    _run_duplication()


@pytest.mark.gpu
def test_equals_physical_duplication_gpu(hip_lib):
    _run_duplication()


def _run_long_category(dev):
    """one category longer than the staged chunk of the kernel (4096 elements) against a numpy transcription of the definition"""
    from omni3d_amd.kernels import bootstrap as kb
    rng = np.random.default_rng(9)
    D, I, A, T, B, R = 9001, 37, 2, 2, 5, 101
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                   # noqa: E731
    det_img = rng.integers(0, I, D).astype(np.int32)
    rank = rng.integers(0, 12, D).astype(np.int32)
    order = rng.permutation(D).astype(np.int32)
    dt_match = np.where(rng.uniform(size=(A, T, D)) < 0.45, 0, -1).astype(np.int32)
    dt_ignore = (rng.uniform(size=(A, T, D)) < 0.1).astype(np.uint8)
    W = rng.multinomial(I, np.full(I, 1.0 / I), size=B).astype(np.int32)
    W[0] = 1
    grp_npig = rng.integers(60, 200, (I, A)).astype(np.int32)                           # one group per image, one category
    thr, md = np.linspace(0.0, 1.0, R), np.array([3, 100], np.int32)
    npig_b, has_e_b = kb.bootstrap_counts(t(np.array([0, I], np.int32)), t(np.arange(I, dtype=np.int32)), t(grp_npig), t(W))
    assert np.array_equal(npig_b.cpu().numpy()[:, 0], W.astype(np.int64) @ grp_npig) and (has_e_b.cpu().numpy() == 1).all()
    ap, ar = kb.bootstrap_accumulate(t(order), t(np.array([0, D], np.int32)), t(rank), t(dt_match), t(dt_ignore), t(det_img), t(W), npig_b,
                                     has_e_b, t(thr), t(md))
    ap, ar = ap.cpu().numpy(), ar.cpu().numpy()
    eps = np.spacing(1)
    for b in range(B):
        for a in range(A):
            npig = int(W[b] @ grp_npig[:, a])
            for ti in range(T):
                for m, maxdet in enumerate(md):
                    d = order[rank[order] < maxdet]
                    w = W[b][det_img[d]]
                    ig, mt = dt_ignore[a, ti, d] != 0, dt_match[a, ti, d] >= 0
                    tp, fp = np.cumsum(np.where(mt & ~ig, w, 0)), np.cumsum(np.where(~mt & ~ig, w, 0))
                    keep = w > 0
                    tp, fp, is_tp = tp[keep], fp[keep], (mt & ~ig)[keep]
                    pr = tp / (fp + tp + eps)
                    env = np.maximum.accumulate(pr[::-1])[::-1]
                    q = np.zeros(R)
                    rc = tp / npig
                    inds = np.searchsorted(rc, thr, side="left")           # as accumulate(): the first position that reaches r
                    for j, pos in enumerate(inds):
                        if pos < len(env):
                            q[j] = env[pos]
                    assert is_tp.any()
                    assert ar[b, ti, 0, a, m] == tp[-1] / npig
                    assert abs(ap[b, ti, 0, a, m] - q.mean()) <= 1e-12, (b, a, ti, m, ap[b, ti, 0, a, m], q.mean())


def test_category_longer_than_the_staged_chunk_emulated(emu_lib):
    _run_long_category("cpu")


@pytest.mark.gpu
def test_category_longer_than_the_staged_chunk_gpu(hip_lib):
    _run_long_category("cuda")


def _run_abi(L, dev):
    from omni3d_amd import lib
    from omni3d_amd.kernels import bootstrap as kb
    OK, ERR_ARG = 0, 1
    boot, counts = L._fn["omni_eval_bootstrap"], L._fn["omni_eval_bootstrap_counts"]
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device=dev)                   # noqa: E731
    order, cat_off, rank, img = i32(0, 1), i32(0, 2), i32(0, 0), i32(0, 1)
    dtm, dtg = i32(0, -1).view(1, 1, 2), torch.zeros((1, 1, 2), dtype=torch.uint8, device=dev)
    w, npig_b, has_e_b = i32(1, 1).view(1, 2), i32(2).view(1, 1, 1), i32(1).view(1, 1)
    thr, md = torch.linspace(0, 1, 101, dtype=torch.float64, device=dev), i32(100)
    ap, ar = torch.full((5,), -1.0, dtype=torch.float64, device=dev), torch.full((5,), -1.0, dtype=torch.float64, device=dev)
    p = lib.ptr

    def call(K=1, A=1, M=1, T=1, R=101, sumD=2, B=1, I=2, wmax=1):
        return boot(p(order), p(cat_off), p(rank), p(dtm), p(dtg), p(img), p(w), wmax, p(npig_b), p(has_e_b), p(thr), p(md), K, A, M, T, R,
                    sumD, B, I, p(ap), p(ar), lib.stream_of(ap))

    for bad in (dict(B=0), dict(B=-1), dict(A=0), dict(M=0), dict(T=0), dict(R=0), dict(K=-1), dict(sumD=-1), dict(I=-1), dict(wmax=-1),
                dict(I=1 << 29)):
        assert call(**bad) == ERR_ARG, bad
    assert (ap == -1).all() and (ar == -1).all()
    # the empty case: nothing is launched, the -1 of the caller stays
    assert call(K=0) == OK and call(K=0, sumD=0) == OK and (ap == -1).all() and (ar == -1).all()
    # the overflow rule: refused when sumD x max_weight >= 2^31, before anything else is looked at
    assert call(K=0, sumD=1 << 20, wmax=(1 << 11) - 1) == OK and call(K=0, sumD=1 << 20, wmax=1 << 11) == ERR_ARG
    assert counts(p(cat_off), p(img), p(npig_b), p(w), 1 << 11, 0, 1, 0, 1 << 20, 1, 2, p(npig_b), p(has_e_b), None) == ERR_ARG
    assert counts(p(cat_off), p(img), p(npig_b), p(w), (1 << 11) - 1, 0, 1, 0, 1 << 20, 1, 2, p(npig_b), p(has_e_b), None) == OK
    assert counts(p(cat_off), p(img), p(npig_b), p(w), 1, 1, 1, 1, 1, 0, 2, p(npig_b), p(has_e_b), None) == ERR_ARG       # B = 0
    # one true positive of two ground truths, one false positive behind it: precision 1 up to recall 0.5
    assert call() == OK
    assert float(ar[0]) == 0.5 and abs(float(ap[0]) - 51 / 101) <= 1e-15 and (ap[1:] == -1).all()
    # sumD == 0: a category with ground truth and no detection scores 0
    ap.fill_(-1.0)
    ar.fill_(-1.0)
    cat_off0 = i32(0, 0)
    assert boot(p(order), p(cat_off0), p(rank), p(dtm), p(dtg), p(img), p(w), 1, p(npig_b), p(has_e_b), p(thr), p(md), 1, 1, 1, 1, 101,
                0, 1, 2, p(ap), p(ar), lib.stream_of(ap)) == OK
    assert float(ap[0]) == 0.0 and float(ar[0]) == 0.0
    # the launcher refuses the same in Python, and a negative weight
    big = torch.full((1, 2), (1 << 31) - 1, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="2\\^31"):
        kb.bootstrap_accumulate(order, cat_off, rank, dtm, dtg, img, big, npig_b, has_e_b, thr, md)
    with pytest.raises(ValueError, match="2\\^31"):
        kb.bootstrap_counts(i32(0, 1), i32(0), i32(3).view(1, 1), big)
    with pytest.raises(ValueError, match=">= 0"):
        kb.bootstrap_accumulate(order, cat_off, rank, dtm, dtg, img, i32(1, -1).view(1, 2), npig_b, has_e_b, thr, md)


def test_abi_emulated(emu_lib):
    _run_abi(emu_lib, "cpu")


@pytest.mark.gpu
def test_abi_gpu(hip_lib):
    _run_abi(hip_lib, "cuda")


def test_header_and_integration_list_the_entries():
    import os
    from conftest import ROOT
    from omni3d_amd import lib
    decls = lib.parse_header()
    assert decls["omni_eval_bootstrap"] == "pppppppipppp" + "iiiiiiii" + "ppp" and decls["omni_eval_bootstrap_counts"] == "ppppiiiiiiippp"
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "omni_eval_bootstrap" in text and "omni_eval_bootstrap_counts" in text
