"""Time of the accumulation over many workgroups (csrc/eval_accumulate_par.hip) against the one-wave kernel (csrc/eval_match.hip), run by
hand on an MI355X; not part of bench.py.
On hand-made K = 1 tables (the one list of a class-agnostic evaluation) of 10^4, 10^5 and 10^6 detections x 4 ranges x 3 maxDets x 10
thresholds, R = 101, built like those of tools/bench_bootstrap.py (about half of the detections are true positives, a tenth ignored;
ranks 0 .. 124, so that every maxDets cuts the list differently):
 1. omni_eval_accumulate (unchanged, one 64-lane wave per (range, maxDets, threshold): 120 waves);
 2. omni_eval_accumulate_par at each block size of BLOCKS_TESTED.
Device events around CALLS[n] calls, 5 alternating blocks in one process after warm-up calls of each; the medians with min and max are
reported with the clocks the device reported right after the loops.  At every size the three tables of every block size are checked to
be EQUAL to those of (1).  Reported: PAR_BLOCK = the fastest tested block at 10^6, PAR_MIN_LIST = the smallest tested length at which the median of (2) at that block
is not above that of (1); `kernels/accumulate.py` carries both.
    python tools/bench_accumulate_par.py [output file]"""
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from omni3d_amd import lib  # noqa: E402

SIZES, RANGES, THRS, MAX_DETS, R = (10_000, 100_000, 1_000_000), 4, 10, (1, 10, 100), 101
BLOCKS_TESTED = (256, 1024, 4096, 16384)
CALLS = {10_000: 50, 100_000: 20, 1_000_000: 5}
TIMED_BLOCKS, WARMUP = 5, 2


def tables(rng, n):
    """hand-made match tables of one list of n detections (those of tools/bench_bootstrap.py with one category)"""
    kind = rng.uniform(size=(RANGES, THRS, n))
    score = rng.uniform(size=n)
    return dict(order=np.lexsort((np.arange(n), -score)).astype(np.int32), cat_off=np.array([0, n], np.int32),
                rank=rng.integers(0, 125, n).astype(np.int32), score=score, dt_match=np.where(kind < 0.5, 0, -1).astype(np.int32),
                dt_ignore=(kind > 0.9).astype(np.uint8), npig=np.full((1, RANGES), int(0.6 * n), np.int32), has_e=np.ones(1, np.int32),
                rec_thrs=np.linspace(0.0, 1.0, R), max_dets=np.array(MAX_DETS, np.int32))


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


def timed(call, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        call()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / calls


def launchers(tab, device):
    """-> ({name: call}, {name: its three output tables}, the device tables) for the one-wave kernel ("seq") and every tested block ("par <block>")"""
    from omni3d_amd.kernels import accumulate as ka
    dv = {k: torch.from_numpy(v).to(device) for k, v in tab.items()}
    p = {k: v.data_ptr() for k, v in dv.items()}
    K, A, M, T, n = 1, RANGES, len(MAX_DETS), THRS, int(tab["cat_off"][1])
    full = lambda shape: torch.full(shape, -1.0, dtype=torch.float64, device=device)      # noqa: E731
    L = lib.get()
    args = (p["order"], p["cat_off"], p["rank"], p["score"], p["dt_match"], p["dt_ignore"], p["npig"], p["has_e"], p["rec_thrs"], p["max_dets"],
            K, A, M, T, R, n)
    calls, outs = {}, {"seq": (full((T, R, K, A, M)), full((T, K, A, M)), full((T, R, K, A, M)))}
    st = lib.stream_of(outs["seq"][0])
    calls["seq"] = lambda o=outs["seq"]: L.call("omni_eval_accumulate", *args, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), st)
    for b in BLOCKS_TESTED:
        name = "par %d" % b
        outs[name] = (full((T, R, K, A, M)), full((T, K, A, M)), full((T, R, K, A, M)))
        nbytes = ka.workspace_bytes(K, A, M, T, n, b)
        ws = torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device=device)
        calls[name] = lambda o=outs[name], b=b, ws=ws, nbytes=nbytes: L.call(
            "omni_eval_accumulate_par", *args, b, ws.data_ptr(), nbytes, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), st)
    return calls, outs, dv                                          # the launchers hold pointers: the tables must outlive them


def check_equal(outs):
    for name, o in outs.items():
        for got, want in zip(o, outs["seq"]):
            assert torch.equal(got, want), name
    assert bool((outs["seq"][0] > 0).any()) and bool((outs["seq"][1] > 0).all())


def main(out=None):
    assert torch.cuda.is_available(), "needs the GPU"
    lines = ["csrc/eval_accumulate_par.hip against omni_eval_accumulate -- one list (K = 1) x %d ranges x %d maxDets x %d thresholds, R = %d; "
             "%d alternating blocks of calls between device events after %d warm-up calls of each; every table of every block size equal "
             "to the one-wave kernel's" % (RANGES, len(MAX_DETS), THRS, R, TIMED_BLOCKS, WARMUP)]
    med = {}
    for n in SIZES:
        calls, outs, held = launchers(tables(np.random.default_rng(0), n), "cuda")
        names = list(calls)
        for _ in range(WARMUP):
            for name in names:
                calls[name]()
        torch.cuda.synchronize()
        check_equal(outs)
        t = {name: [] for name in names}
        for _ in range(TIMED_BLOCKS):                               # alternating: all see the same clocks and neighbours
            for name in names:
                t[name].append(timed(calls[name], CALLS[n]))
        check_equal(outs)
        med[n] = {name: statistics.median(t[name]) for name in names}
        lines.append("%d detections (%d calls per block):" % (n, CALLS[n]))
        lines.append("    omni_eval_accumulate: %s per call" % fmt(t["seq"]))
        for b in BLOCKS_TESTED:
            name = "par %d" % b
            lines.append("    omni_eval_accumulate_par, block %5d (%d workgroups per launch): %s per call = %.2f x" %
                         (b, RANGES * len(MAX_DETS) * THRS * ((n + b - 1) // b), fmt(t[name]), med[n]["seq"] / med[n][name]))
        del calls, outs, held
    during = clocks()
    best = min(BLOCKS_TESTED, key=lambda b: med[SIZES[-1]]["par %d" % b])
    pays = [n for n in SIZES if med[n]["par %d" % best] <= med[n]["seq"]]
    lines.append("PAR_MIN_LIST = %s; PAR_BLOCK = %d (the fastest tested block at %d)" %
                 (pays[0] if pays else "none of the tested lengths: the parallel form is not faster", best, SIZES[-1]))
    lines.append("clocks right after the timed loops: %s" % during)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
