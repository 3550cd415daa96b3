"""Time of the bootstrap kernel (csrc/eval_bootstrap.hip), run by hand on an MI355X; not part of bench.py.
On hand-made tables of 20 categories x 10 000 detections x 4 depth ranges x 3 maxDets x 10 thresholds over 2 000 images (about half of
the detections are true positives, a tenth ignored; ranks 0 .. 124, so that every maxDets cuts the lists differently):
 1. omni_eval_bootstrap at B = 1000 replicates (row 0 all ones, the others multinomial draws of 2 000 images), npig_b / has_e_b taken
    once beforehand by omni_eval_bootstrap_counts (timed on its own);
 2. ONE omni_eval_accumulate call (csrc/eval_match.hip) on the same, unduplicated tables.
The yardstick: scoring the 1000 replicates through the existing entry would cost at least 1000 x (2) in device time alone, so (1) must
be below that; the tool asserts it.  Device events around 20 calls, 5 alternating blocks after warm-up calls of each, the medians and
the spread are reported with the clocks the device reported right after the loops.  Row 0 of the timed launch is checked against the
`precision` and `recall` of (2): equal recall, |ap - precision.mean over r| <= 1e-12.
Measured (MI355X, sclk 2398 MHz, profiles/bootstrap_timing.txt): omni_eval_bootstrap at B = 1000 132.4 ms per call (min 132.3, max
133.5), omni_eval_accumulate 944 us per call (min 942, max 945): bootstrap / (1000 x accumulate) = 0.140; omni_eval_bootstrap_counts 442 us.
    python tools/bench_bootstrap.py [output file]"""
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from omni3d_amd import lib  # noqa: E402

CATS, PER_CAT, RANGES, THRS, MAX_DETS, IMAGES, REPLICATES = 20, 10_000, 4, 10, (1, 10, 100), 2_000, 1_000
BLOCKS, CALLS, WARMUP = 5, 20, 2


def tables(rng):
    """hand-made match tables (those of tools/bench_let.py) plus the image of every detection, the (category, image) group tables and
    the replicates"""
    sumD = CATS * PER_CAT
    kind = rng.uniform(size=(RANGES, THRS, sumD))
    dt_match = np.where(kind < 0.5, 0, -1).astype(np.int32)
    dt_ignore = (kind > 0.9).astype(np.uint8)
    score = rng.uniform(size=sumD)
    cat = np.repeat(np.arange(CATS), PER_CAT)
    order = np.lexsort((np.arange(sumD), -score, cat)).astype(np.int32)
    grp_npig = rng.integers(0, 7, (CATS * IMAGES, RANGES)).astype(np.int32)              # about 6 000 ground truths per (category, range)
    weights = rng.multinomial(IMAGES, np.full(IMAGES, 1.0 / IMAGES), size=REPLICATES).astype(np.int32)
    weights[0] = 1
    return dict(order=order, cat_off=(np.arange(CATS + 1) * PER_CAT).astype(np.int32), rank=rng.integers(0, 125, sumD).astype(np.int32),
                score=score, dt_match=dt_match, dt_ignore=dt_ignore, det_img=rng.integers(0, IMAGES, sumD).astype(np.int32),
                grp_off=(np.arange(CATS + 1) * IMAGES).astype(np.int32), grp_img=np.tile(np.arange(IMAGES, dtype=np.int32), CATS),
                grp_npig=grp_npig, npig=np.ascontiguousarray(grp_npig.reshape(CATS, IMAGES, RANGES).sum(axis=1).astype(np.int32)),
                has_e=np.ones(CATS, np.int32), weights=weights, max_dets=np.array(MAX_DETS, np.int32), rec_thrs=np.linspace(0.0, 1.0, 101))


def clocks():
    """the sclk / mclk lines of `rocm-smi --showclocks` (read only), or a note that they could not be read"""
    try:
        text = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        rows = [" ".join(ln.split()) for ln in text.splitlines() if "sclk" in ln or "mclk" in ln]
        return "; ".join(rows[:2]) if rows else "clocks not reported"
    except Exception as exc:      # noqa: BLE001
        return "clocks not read (%s)" % type(exc).__name__


def fmt(t):
    return "median %.1f us (min %.1f, max %.1f)" % (statistics.median(t), min(t), max(t))


def block(call, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        call()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / calls


def main(out=None):
    assert torch.cuda.is_available(), "needs the GPU"
    tab = tables(np.random.default_rng(0))
    dv = {k: torch.from_numpy(v).cuda() for k, v in tab.items()}
    p = {k: v.data_ptr() for k, v in dv.items()}
    K, A, M, T, R, sumD, B, I = CATS, RANGES, len(MAX_DETS), THRS, 101, CATS * PER_CAT, REPLICATES, IMAGES
    G, wmax = CATS * IMAGES, int(tab["weights"].max())
    full = lambda shape: torch.full(shape, -1.0, dtype=torch.float64, device="cuda")      # noqa: E731
    prec, rec, scr = full((T, R, K, A, M)), full((T, K, A, M)), full((T, R, K, A, M))
    ap, ar = full((B, T, K, A, M)), full((B, T, K, A, M))
    npig_b = torch.zeros((B, K, A), dtype=torch.int32, device="cuda")
    has_e_b = torch.zeros((B, K), dtype=torch.int32, device="cuda")
    L, st = lib.get(), lib.stream_of(ap)

    def counts():
        L.call("omni_eval_bootstrap_counts", p["grp_off"], p["grp_img"], p["grp_npig"], p["weights"], wmax, K, A, G, int(tab["grp_npig"].sum(axis=0).max()),
               B, I, npig_b.data_ptr(), has_e_b.data_ptr(), st)

    def bootstrap():
        L.call("omni_eval_bootstrap", p["order"], p["cat_off"], p["rank"], p["dt_match"], p["dt_ignore"], p["det_img"], p["weights"], wmax,
               npig_b.data_ptr(), has_e_b.data_ptr(), p["rec_thrs"], p["max_dets"], K, A, M, T, R, sumD, B, I, ap.data_ptr(), ar.data_ptr(), st)

    def accumulate():
        L.call("omni_eval_accumulate", p["order"], p["cat_off"], p["rank"], p["score"], p["dt_match"], p["dt_ignore"], p["npig"], p["has_e"],
               p["rec_thrs"], p["max_dets"], K, A, M, T, R, sumD, prec.data_ptr(), rec.data_ptr(), scr.data_ptr(), st)

    counts()
    for _ in range(WARMUP):
        bootstrap()
        accumulate()
    torch.cuda.synchronize()
    t_boot, t_acc, t_cnt = [], [], []
    for _ in range(BLOCKS):                                        # alternating: both see the same clocks and neighbours
        t_boot.append(block(bootstrap, CALLS))
        t_acc.append(block(accumulate, CALLS))
        t_cnt.append(block(counts, CALLS))
    during = clocks()
    assert np.array_equal(npig_b[0].cpu().numpy(), tab["npig"]) and bool((has_e_b == 1).all())
    assert np.array_equal(npig_b.cpu().numpy()[:, 3, 1], tab["weights"].astype(np.int64) @ tab["grp_npig"][3 * IMAGES:4 * IMAGES, 1])
    want_ap, want_ar = prec.cpu().numpy().mean(axis=1), rec.cpu().numpy()
    got_ap, got_ar = ap.cpu().numpy(), ar.cpu().numpy()
    worst = float(np.abs(got_ap[0] - want_ap).max())
    assert np.array_equal(got_ar[0], want_ar) and worst <= 1e-12, worst
    assert (got_ap > -1).all() and got_ap[1:, :, :, 0, -1].std(axis=0).min() > 0            # the replicates differ
    med_b, med_a = statistics.median(t_boot), statistics.median(t_acc)
    lines = ["csrc/eval_bootstrap.hip -- %d categories x %d detections x %d ranges x %d maxDets x %d thresholds over %d images, %d replicates "
             "(largest weight %d); replicate 0 (all ones) against omni_eval_accumulate: recall equal, worst |ap - mean precision| %.1e"
             % (CATS, PER_CAT, RANGES, len(MAX_DETS), THRS, IMAGES, REPLICATES, wmax, worst),
             "omni_eval_bootstrap, B = %d: %s per call = %.1f us per replicate" % (B, fmt(t_boot), med_b / B),
             "omni_eval_accumulate, one call on the same tables: %s per call" % fmt(t_acc),
             "    bootstrap / (%d x accumulate) = %.3f (%d alternating blocks of %d calls between device events after %d warm-up calls of each)"
             % (B, med_b / (B * med_a), BLOCKS, CALLS, WARMUP),
             "omni_eval_bootstrap_counts, B = %d: %s per call" % (B, fmt(t_cnt)),
             "clocks right after the timed loops: %s" % during]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)
    assert med_b < B * med_a, "the weighted kernel costs more than %d calls of omni_eval_accumulate" % B


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
