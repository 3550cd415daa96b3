"""Record the launch decisions of csrc/conv_gemm.hip's host code: tests/golden/conv_launch_plan.npz.

The `plan` mode of the deterministic entry points answers {tile, splits, counters, workspace floats} without launching and without
touching a pointer -- the whole decision surface of the launchers, computed in microseconds by the host-emulated library.  This
tool enumerates a fixed grid of problems, asks every launcher for its plan, and stores the argument rows, the four plan values
and the status code.  What the plan does not show (zero-fill, statistics attach and *nblk_out, prefetch-or-classic body, XCD
order, follow-up ReLU pass, grid shape) is pinned by RUNNING one small launch per branch on the emulator, which is sequential and
therefore bit-reproducible even for the atomic forms: a CRC of the output bytes and *nblk_out are stored with the plans.

tests/test_conv_launch_plan.py recomputes all of it and asserts equality; its GPU twin checks the same launches against float64.

The fixture is a record of the launchers BEFORE a host-code change: run this tool on the commit the change starts from
(`python tools/make_conv_plan_golden.py`, which builds tests/hipemu first), commit the file, then change the code."""
import argparse
import ctypes
import itertools
import os
import subprocess
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_launch_plan.npz")

LAUNCHERS = ("omni_conv2d_fwd_det", "omni_conv2d_fwd_multi_det", "omni_conv2d_dgrad_det", "omni_conv2d_wgrad_det",
             "omni_conv2d_wgrad_multi_det", "omni_gemm_batched_wgrad_det", "omni_gemm_batched_wgrad_multi")
FWD, FWD_MULTI, DGRAD, WGRAD, WGRAD_MULTI, BWGRAD, BWGRAD_MULTI = range(7)
WIDTH = 22            # launcher id + up to 21 integer arguments (zero padded)
FAKE = 1 << 20        # a non-null address: the plan mode checks pointers against null and never follows them
UNTOUCHED = -1        # what the plan cells hold when the launcher returned without reporting


def emulated_library():
    from omni3d_amd import lib as L
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "hipemu"), "-j8"])
    return L.HipLibrary(os.path.join(ROOT, "tests", "hipemu", "libomni3d_emu.so"), emulated=True)


# ---------------------------------------------------------------------------------------------------- the plan table
def _mix(i):
    """a fixed scramble of the row index, so that the thinned (tile, splits) requests do not follow any axis of the grid"""
    return ((i + 1) * 2654435761 % (1 << 32)) >> 9


def plan_rows():
    """int32 (rows, WIDTH): [launcher, arguments...].  Argument order per launcher:
    FWD          N H W C K R stride pad ldx ldo relu tile splits_req
    FWD_MULTI    N H W K ldo relu tile splits_req nsrc cs[0..5]
    DGRAD        N H W C K R stride pad lddy lddx accumulate tile splits_req
    WGRAD        N H W C K R stride pad ldx lddy accumulate tile
    WGRAD_MULTI  N H W K lddy accumulate tile nsrc cs[0..5]
    BWGRAD       batch M C K algo
    BWGRAD_MULTI n (batch M C K)[0..4]"""
    rows = []

    def add(kind, *a):
        assert len(a) < WIDTH
        rows.append([kind, *a] + [0] * (WIDTH - 1 - len(a)))

    def out_hw(h, r, s, p):
        return (h + 2 * p - r) // s + 1

    def conv3(N, H, C, K, R, s, p, tile=0, sreq=0, order=0, acc=0, ldo_pad=0, ldx_pad=0):
        """the three launchers of one convolution: forward, data gradient, weight gradient (tile + order: its workgroup-order request)"""
        add(FWD, N, H, H, C, K, R, s, p, C, K + ldo_pad, 0, tile, sreq)
        add(DGRAD, N, H, H, C, K, R, s, p, K, C + ldx_pad, acc, tile, sreq)
        add(WGRAD, N, H, H, C, K, R, s, p, C, K, acc, tile + order)

    chans = (4, 16, 32, 64, 128, 256, 512)
    rsp = ((1, 1, 0), (1, 2, 0), (3, 1, 1), (3, 2, 1), (7, 1, 3))
    grid = list(itertools.product((1, 4), (1, 7, 8, 32, 128, 512), chans, chans, rsp))
    for i, (N, H, C, K, (R, s, p)) in enumerate(grid):
        h = _mix(i)
        if h % 3 == 0:                       # a third of the grid: the launcher's own choice
            conv3(N, H, C, K, R, s, p)
        elif h % 3 == 1 and (h // 3) % 2:    # a sixth: a forced tile / split request / workgroup order
            conv3(N, H, C, K, R, s, p, tile=(h // 6) % 5, sreq=(0, 1, 3)[(h // 30) % 3], order=(0, 16, 32)[(h // 90) % 3])
    # every forced tile with every split request on one mid-sized layer per filter shape
    for (R, s, p), tile, sreq, order in itertools.product(rsp, range(5), (0, 1, 3), (0, 16, 32)):
        if order == 0 or sreq == 0:
            conv3(4, 32, 128, 128, R, s, p, tile=tile, sreq=sreq, order=order)
    # the fc heads: box head on 4 x 512 ROIs, cube head on 4 x 128 (fc1: 12544 -> 1024, fc2: 1024 -> 1024)
    for rows_, (C, K) in itertools.product((2048, 512), ((12544, 1024), (1024, 1024))):
        for tile in range(5):
            conv3(rows_, 1, C, K, 1, 1, 0, tile=tile, order=(0, 16, 32)[tile % 3])
    # pitches larger than the channel count (a Root child's slice of the concatenated tensor, a fan-in carry), with and without accumulate
    for (C, K), (R, s, p), sreq, acc in itertools.product(((64, 64), (256, 256), (64, 256)), ((3, 1, 1), (1, 1, 0), (3, 2, 1)), (0, 3), (0, 1)):
        conv3(4, 32, C, K, R, s, p, tile=2 * (sreq > 0), sreq=sreq, acc=acc, ldo_pad=64, ldx_pad=64)
        conv3(1, 8, C, K, R, s, p, sreq=sreq, acc=acc, ldx_pad=32)
    # multi-source inputs (the DLA Root): 2, 3 and 6 sources; (64, 48) breaks the forward's width rule, (64, 6) the weight gradient's too
    for cs, (N, H), K, tile in itertools.product(((64, 64), (128, 64, 32), (32,) * 6, (256, 256, 128, 128, 64, 64), (64, 48), (64, 6)),
                                                 ((1, 8), (4, 32), (4, 128)), (64, 256), range(5)):
        pad = list(cs) + [0] * (6 - len(cs))
        add(FWD_MULTI, N, H, H, K, K, 0, tile, (0, 1, 3)[tile % 3], len(cs), *pad)
        add(WGRAD_MULTI, N, H, H, K, K, tile % 2, tile + (0, 16, 32)[tile % 3], len(cs), *pad)
    add(FWD_MULTI, 4, 32, 32, 64, 64, 0, 0, 0, 7, 32, 32, 32, 32, 32, 32)          # seven sources
    add(WGRAD_MULTI, 4, 32, 32, 64, 64, 0, 0, 0, 32, 32, 0, 0, 0, 0)               # none
    # empty problems
    for R, s, p in rsp:
        conv3(0, 32, 64, 64, R, s, p)
    add(FWD_MULTI, 0, 32, 32, 64, 64, 0, 0, 0, 2, 64, 64, 0, 0, 0, 0)
    add(WGRAD_MULTI, 0, 32, 32, 64, 64, 0, 0, 2, 64, 64, 0, 0, 0, 0)
    # an operand at or above 2 GiB: refused where 32-bit byte offsets are the only addressing, the classic body elsewhere
    conv3(4, 512, 512, 64, 3, 1, 1)             # x is exactly 2 GiB
    conv3(4, 512, 64, 512, 3, 1, 1)             # dy is
    conv3(4, 512, 508, 64, 3, 1, 1)             # x just below it
    conv3(1, 1, 32768, 16384, 1, 1, 0)          # the weights are
    add(FWD_MULTI, 4, 512, 512, 64, 64, 0, 0, 0, 2, 512, 32, 0, 0, 0, 0)
    add(WGRAD_MULTI, 4, 512, 512, 64, 64, 0, 0, 2, 512, 32, 0, 0, 0, 0)
    # arguments every launcher refuses
    add(FWD, 1, 8, 8, 6, 16, 3, 1, 1, 6, 16, 0, 0, 0)            # C % 4
    add(FWD, 1, 8, 8, 16, 16, 3, 1, 1, 16, 16, 0, 5, 0)          # tile 5
    add(FWD, 1, 8, 8, 16, 16, 3, 1, 1, 12, 16, 0, 0, 0)          # ldx < C
    add(DGRAD, 1, 8, 8, 16, 6, 3, 1, 1, 6, 16, 0, 0, 0)          # K % 4
    add(DGRAD, 1, 8, 8, 16, 16, 3, 1, 1, 16, 16, 0, 0, -1)       # splits_req < 0
    add(WGRAD, 1, 8, 8, 16, 16, 3, 1, 1, 16, 16, 0, 5)           # tile 5
    add(WGRAD, 1, 8, 8, 16, 16, 3, 1, 1, 16, 16, 0, 37)          # tile 32 + 5
    add(WGRAD, 1, 8, 8, 16, 16, 3, 1, 1, 16, 14, 0, 0)           # lddy < K
    # the batched weight gradients of the Winograd path
    for batch, M, C, K, algo in itertools.product((16, 36), (0, 256, 1024, 16384), (64, 128, 256, 512), (64, 128, 256, 512), (0, 1, 2)):
        add(BWGRAD, batch, M, C, K, algo)
    for algo in (0, 1, 2, 3):
        add(BWGRAD, 16, 1 << 20, 512, 64, algo)       # x is 2 GiB: algo 2 refused, the automatic choice falls back to algo 1; algo 3 does not exist
        add(BWGRAD, 16, 600, 6, 64, algo)             # C % 4
    add(BWGRAD_MULTI, 5, 16, 1024, 256, 256, 36, 256, 128, 128, 16, 0, 64, 64, 36, 16384, 64, 128, 16, 600, 512, 512)
    add(BWGRAD_MULTI, 1, 16, 600, 64, 64)
    add(BWGRAD_MULTI, 2, 16, 0, 64, 64, 36, 0, 128, 128)
    add(BWGRAD_MULTI, 2, 16, 1 << 20, 512, 64, 16, 600, 64, 64)      # 2 GiB member
    add(BWGRAD_MULTI, 0)
    return np.asarray(rows, dtype=np.int32)


def plan_call(lib, row):
    """-> (status, [tile, splits, counters, workspace floats]) of one row's plan call"""
    kind, a = int(row[0]), [int(v) for v in row[1:]]
    plan = (ctypes.c_longlong * 4)(*[UNTOUCHED] * 4)
    tail = (None, 0, None, 0, ctypes.addressof(plan), None)       # ws, ws_floats, ctr, n_ctr, plan, stream
    keep = []

    def ints(v):
        arr = (ctypes.c_int * max(len(v), 1))(*v)
        keep.append(arr)
        return ctypes.addressof(arr)

    def ptrs(n):
        arr = (ctypes.c_void_p * max(n, 1))(*[FAKE] * n)
        keep.append(arr)
        return ctypes.addressof(arr)

    if kind == FWD:
        N, H, W, C, K, R, s, p, ldx, ldo, relu, tile, sreq = a[:13]
        args = (FAKE, FAKE, None, FAKE, N, H, W, C, K, R, R, s, p, ldx, ldo, relu, tile, sreq, None, 0, None)
    elif kind == FWD_MULTI:
        N, H, W, K, ldo, relu, tile, sreq, nsrc = a[:9]
        args = (ptrs(nsrc), ints(a[9:9 + nsrc]), nsrc, FAKE, None, FAKE, N, H, W, K, ldo, relu, tile, sreq, None, 0, None)
    elif kind == DGRAD:
        N, H, W, C, K, R, s, p, lddy, lddx, acc, tile, sreq = a[:13]
        args = (FAKE, FAKE, FAKE, N, H, W, C, K, R, R, s, p, lddy, lddx, acc, tile, sreq)
    elif kind == WGRAD:
        N, H, W, C, K, R, s, p, ldx, lddy, acc, tile = a[:12]
        args = (FAKE, FAKE, FAKE, N, H, W, C, K, R, R, s, p, ldx, lddy, acc, tile)
    elif kind == WGRAD_MULTI:
        N, H, W, K, lddy, acc, tile, nsrc = a[:8]
        args = (ptrs(nsrc), ints(a[8:8 + nsrc]), nsrc, FAKE, FAKE, N, H, W, K, lddy, acc, tile)
    elif kind == BWGRAD:
        args = (FAKE, FAKE, FAKE, *a[:5])
    else:
        n = a[0]
        prob = [a[1 + 4 * i:5 + 4 * i] for i in range(n)]
        args = (ptrs(n), ptrs(n), ptrs(n), *[ints([q[j] for q in prob]) for j in range(4)], n)
    status = lib._fn[LAUNCHERS[kind]](*args, *tail)
    return int(status), [int(v) for v in plan]


def compute_plans(lib, rows):
    out = [plan_call(lib, r) for r in rows]
    return np.asarray([p for _, p in out], dtype=np.int64), np.asarray([s for s, _ in out], dtype=np.int32)


# ---------------------------------------------------------------------------------------------------- one launch per branch
def _values(n, seed):
    """n floats in [-1, 1): a counter scrambled by integer multiplication -- the same bits wherever this runs"""
    i = np.arange(n, dtype=np.uint64)
    u = ((i + np.uint64(seed * 7919 + 1)) * np.uint64(2654435761)) % np.uint64(1 << 32)
    u = (u ^ (u >> np.uint64(15))) * np.uint64(2246822519) % np.uint64(1 << 32)
    return torch.from_numpy(((u >> np.uint64(8)).astype(np.float64) / float(1 << 23) - 1.0).astype(np.float32))


def _t(shape, seed, scale=1.0):
    n = int(np.prod(shape))
    return (_values(n, seed) * scale).reshape(shape)


# name -> (launcher, parameters).  conv parameters: N H C K R stride pad; common keys: tile, sreq, det (counters given), acc.
LAUNCHES = (
    ("fwd_split_atomic_relu", FWD, dict(g=(1, 8, 64, 64, 3, 1, 1), tile=2, sreq=3, det=False, bias=True, relu=1)),
    ("fwd_ordered_bias_relu_stats_asked", FWD, dict(g=(1, 8, 64, 64, 3, 1, 1), tile=2, sreq=3, det=True, bias=True, relu=1, stats=True)),
    ("fwd_ordered_stats", FWD, dict(g=(1, 12, 32, 64, 3, 1, 1), tile=2, sreq=2, det=True, bias=False, relu=0, stats=True)),
    ("fwd_multi_source", FWD_MULTI, dict(g=(1, 8, 96, 32, 1, 1, 0), cs=(32, 64), tile=0, sreq=2, det=True, bias=True, relu=1)),
    ("dgrad_s2_split_atomic", DGRAD, dict(g=(1, 8, 64, 64, 3, 2, 1), tile=2, sreq=2, det=False, acc=0)),
    ("dgrad_accumulate_pitched", DGRAD, dict(g=(1, 8, 64, 32, 3, 1, 1), tile=2, sreq=2, det=True, acc=1, ldx_pad=32)),
    ("dgrad_tile4_classic", DGRAD, dict(g=(1, 8, 32, 32, 3, 1, 1), tile=4, sreq=1, det=False, acc=0)),
    ("wgrad_ordered", WGRAD, dict(g=(1, 24, 64, 64, 1, 1, 0), tile=0, det=True, acc=0)),
    ("wgrad_accumulate_unsplit_rmw", WGRAD, dict(g=(1, 8, 32, 64, 3, 1, 1), tile=0, det=True, acc=1)),
    ("wgrad_multi_source_classic", WGRAD_MULTI, dict(g=(1, 8, 68, 32, 1, 1, 0), cs=(32, 36), tile=0, det=False, acc=0)),
    ("wgrad_no_pixels", WGRAD, dict(g=(0, 8, 32, 32, 3, 1, 1), tile=0, det=False, acc=0)),
    ("bwgrad_algo1_ordered", BWGRAD, dict(b=(2, 600, 64, 64), algo=1, det=True)),
    ("bwgrad_algo2_ordered", BWGRAD, dict(b=(2, 600, 64, 64), algo=2, det=True)),
    ("bwgrad_multi", BWGRAD_MULTI, dict(probs=((2, 300, 64, 64), (1, 0, 8, 8), (1, 520, 32, 64)), det=True)),
)


def run_launch(lib, kind, q, dev="cpu"):
    """Runs one entry of LAUNCHES on `dev` -> dict of the CPU tensors involved: inputs, `out` (list of output tensors, in launch
    layout), `before` (their content before the launch, for the accumulating forms), `nblk`, `plan`."""
    from omni3d_amd import lib as L
    fn = lib._fn[LAUNCHERS[kind]]
    stream = torch.cuda.current_stream().cuda_stream if dev != "cpu" else None
    plan = (ctypes.c_longlong * 4)(*[UNTOUCHED] * 4)
    nblk = ctypes.c_int(-1)
    keep, r = [], {}

    def dv(t):
        t = t.to(dev)
        keep.append(t)
        return t

    def two_calls(head, late=()):
        """plan call, then the launch with the workspace the plan asks for (det) or without counters"""
        rc = fn(*head, *((None, 0, None) if late else ()), None, 0, None, 0, ctypes.addressof(plan), stream)
        assert rc == 0, rc
        ws = dv(torch.zeros(max(int(plan[3]), 1)))
        ctr = dv(torch.zeros(max(int(plan[2]), 1), dtype=torch.int32))
        det = (ws.data_ptr(), int(plan[3]), ctr.data_ptr(), max(int(plan[2]), 1)) if q["det"] else (None, 0, None, 0)
        rc = fn(*head, *late, *det, None, stream)
        assert rc == 0, rc
        if dev != "cpu":
            torch.cuda.synchronize()
        assert int(ctr.abs().sum()) == 0          # the arrival counters go back to zero
        r["plan"] = [int(v) for v in plan]

    if kind in (FWD, FWD_MULTI, DGRAD, WGRAD, WGRAD_MULTI):
        N, H, C, K, R, s, p = q["g"]
        OH = (H + 2 * p - R) // s + 1
        x, w, dy = _t((N, H, H, C), 1), _t((K, R, R, C), 2, 0.2), _t((N, OH, OH, K), 3)
        r.update(x=x, w=w, dy=dy)
        if "cs" in q:
            srcs = [dv(v.contiguous()) for v in torch.split(x, list(q["cs"]), dim=3)]
            pa = (ctypes.c_void_p * len(srcs))(*[v.data_ptr() for v in srcs])
            ca = (ctypes.c_int * len(srcs))(*q["cs"])
            src_head = (ctypes.addressof(pa), ctypes.addressof(ca), len(srcs))
    if kind in (FWD, FWD_MULTI):
        bias = _t((K,), 4) if q["bias"] else None
        out = dv(_t((N, OH, OH, K), 5))                      # garbage the launch has to overwrite
        stats = dv(_t((64, 2 * K), 6)) if q.get("stats") else None
        bd, wd = (dv(bias) if bias is not None else None), dv(w)
        late = (L.ptr(stats), 64 if stats is not None else 0, ctypes.addressof(nblk))
        if kind == FWD:
            head = (dv(x).data_ptr(), wd.data_ptr(), L.ptr(bd), out.data_ptr(), N, H, H, C, K, R, R, s, p, C, K, q["relu"], q["tile"], q["sreq"])
        else:
            head = (*src_head, wd.data_ptr(), L.ptr(bd), out.data_ptr(), N, H, H, K, K, q["relu"], q["tile"], q["sreq"])
        two_calls(head, late)
        r.update(bias=bias, out=[out.cpu()], nblk=nblk.value)
        if stats is not None and nblk.value > 0:
            r["out"].append(stats[:nblk.value].cpu())
    elif kind == DGRAD:
        ldx = C + q.get("ldx_pad", 0)
        dx = dv(_t((N, H, H, ldx), 5))
        r["before"] = [dx.cpu().clone()]
        two_calls((dv(dy).data_ptr(), dv(w).data_ptr(), dx.data_ptr(), N, H, H, C, K, R, R, s, p, K, ldx, q["acc"], q["tile"], q["sreq"]))
        r.update(out=[dx.cpu()], nblk=0)
    elif kind in (WGRAD, WGRAD_MULTI):
        dw = dv(_t((K, R, R, C), 5))
        r["before"] = [dw.cpu().clone()]
        if kind == WGRAD:
            head = (dv(x).data_ptr(), dv(dy).data_ptr(), dw.data_ptr(), N, H, H, C, K, R, R, s, p, C, K, q["acc"], q["tile"])
        else:
            head = (*src_head, dv(dy).data_ptr(), dw.data_ptr(), N, H, H, K, K, q["acc"], q["tile"])
        two_calls(head)
        r.update(out=[dw.cpu()], nblk=0)
    else:
        probs = q["probs"] if kind == BWGRAD_MULTI else (q["b"],)
        xs = [_t((b, M, C), 11 + 3 * i) for i, (b, M, C, K) in enumerate(probs)]
        dys = [_t((b, M, K), 12 + 3 * i) for i, (b, M, C, K) in enumerate(probs)]
        dws = [dv(_t((b, K, C), 13 + 3 * i)) for i, (b, M, C, K) in enumerate(probs)]
        xd, dyd = [dv(v) for v in xs], [dv(v) for v in dys]
        if kind == BWGRAD:
            two_calls((xd[0].data_ptr(), dyd[0].data_ptr(), dws[0].data_ptr(), *q["b"], q["algo"]))
        else:
            n = len(probs)
            arrs = [(ctypes.c_void_p * n)(*[v.data_ptr() for v in vs]) for vs in (xd, dyd, dws)]
            cols = [(ctypes.c_int * n)(*[pr[j] for pr in probs]) for j in range(4)]
            two_calls((*[ctypes.addressof(v) for v in arrs], *[ctypes.addressof(v) for v in cols], n))
        r.update(xs=xs, dys=dys, out=[v.cpu() for v in dws], nblk=0)
    return r


def crc_of(tensors):
    c = 0
    for t in tensors:
        c = zlib.crc32(t.contiguous().numpy().tobytes(), c)
    return c


def compute_launches(lib):
    """-> int64 (len(LAUNCHES), 6): CRC-32 of the output bytes, *nblk_out, the four plan values"""
    rec = []
    for _, kind, q in LAUNCHES:
        r = run_launch(lib, kind, q)
        rec.append([crc_of(r["out"]), r["nblk"], *r["plan"]])
    return np.asarray(rec, dtype=np.int64)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    lib = emulated_library()
    rows = plan_rows()
    plans, status = compute_plans(lib, rows)
    launches = compute_launches(lib)
    np.savez_compressed(a.out, rows=rows, plans=plans, status=status, launches=launches,
                        launch_names=np.asarray([n for n, _, _ in LAUNCHES]))
    print(f"{a.out}: {len(rows)} plan rows ({int((status != 0).sum())} refused), {len(launches)} launches, {os.path.getsize(a.out)} bytes")
    for k, name in enumerate(LAUNCHERS):
        m = rows[:, 0] == k
        ok = m & (status == 0) & (plans[:, 0] != UNTOUCHED)
        print(f"  {name}: {int(m.sum())} rows, {int((m & (status != 0)).sum())} refused, tiles {sorted(set(plans[ok, 0].tolist()))}, "
              f"splits 1 / 2-8 / 9-16 / >16: {[int((ok & (plans[:, 1] >= lo) & (plans[:, 1] <= hi)).sum()) for lo, hi in ((1, 1), (2, 8), (9, 16), (17, 1 << 40))]}")
    for (name, _, _), rec in zip(LAUNCHES, launches):
        print(f"  {name}: crc {int(rec[0]):08x} nblk {int(rec[1])} plan {rec[2:].tolist()}")


if __name__ == "__main__":
    main()
