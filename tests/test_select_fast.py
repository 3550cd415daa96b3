"""The selection kernels' fast paths (csrc/select_nms.hip): the scan's two-deep prefetch and fixed-point chunk resolution, the mask
kernel's division-free decision, the register stages of the top-k sort, and the masked-score output of the scan.  Every result is
index-exact against the oracle (oracle/upstream.py nms, torch stable sort); emulated and GPU variants share the case functions."""
import numpy as np
import pytest
import torch

from oracle import upstream as U

NEG_INF = float("-inf")


def _rand_boxes(g, n, size=100.0):
    xy = torch.rand(n, 2, generator=g) * size
    wh = torch.rand(n, 2, generator=g) * size * 0.4 + 1.0
    return torch.cat([xy, xy + wh], dim=1)


def _oracle_keep(boxes, n, valid, thr):
    """keep (n) 0/1 of one score-sorted problem: the oracle sees the boxes that take part, in their order"""
    sel = torch.arange(n) if valid is None else torch.where(valid[:n] != 0)[0]
    ref = torch.zeros(n, dtype=torch.int32)
    if sel.numel():
        scores = torch.arange(sel.numel(), 0, -1, dtype=torch.float32)
        ref[sel[U.nms(boxes[:n][sel], scores, thr)]] = 1
    return ref


def _check_nms(dev, boxes, thr, counts=None, valid=None):
    from omni3d_amd.kernels import select
    Q, nmax, _ = boxes.shape
    to = lambda t: None if t is None else t.to(dev)
    keep = select.nms_sorted(to(boxes), thr, to(counts), to(valid), _poison=True).cpu()
    for q in range(Q):
        n = nmax if counts is None else int(counts[q])
        ref = _oracle_keep(boxes[q], n, None if valid is None else valid[q], thr)
        assert torch.equal(keep[q, :n], ref), (q, n, torch.where(keep[q, :n] != ref)[0])
        assert (keep[q, n:] == 0).all()
    return keep


# ---- scan: prefetch depth ------------------------------------------------------------------------------------------------
def _scan_prefetch(dev):
    g = torch.Generator().manual_seed(11)
    for n in (1, 63, 64, 65, 128, 129, 193):                       # 1, 2, 3 and 4 chunks, ragged tails
        _check_nms(dev, _rand_boxes(g, n).unsqueeze(0), 0.5)
    boxes = torch.stack([_rand_boxes(g, 130), _rand_boxes(g, 130)])
    _check_nms(dev, boxes, 0.5, counts=torch.tensor([0, 130], dtype=torch.int32))
    _check_nms(dev, boxes, 0.5, counts=torch.tensor([130, 0], dtype=torch.int32))
    _check_nms(dev, boxes, 0.4, counts=torch.tensor([129, 65], dtype=torch.int32),
               valid=(torch.rand(2, 130, generator=g) > 0.2).int())


# ---- scan: chunk resolution ----------------------------------------------------------------------------------------------
def _unit(x, y):
    return [float(x), float(y), float(x) + 1.0, float(y) + 1.0]


def _scan_resolution(dev):
    thr = 0.5
    disjoint = torch.tensor([_unit(2 * i, 0) for i in range(64)])
    k = _check_nms(dev, disjoint.unsqueeze(0), thr)
    assert int(k.sum()) == 64                                       # every box survives
    copies = torch.tensor([_unit(0, 0)] * 64)
    k = _check_nms(dev, copies.unsqueeze(0), thr)
    assert k[0].tolist() == [1] + [0] * 63                          # only the first
    pairs = torch.tensor([_unit(2 * (i // 2), 0) for i in range(64)])
    k = _check_nms(dev, pairs.unsqueeze(0), thr)
    assert k[0].tolist() == [1, 0] * 32                             # survivors alternate: independent pairs
    # a chain: box i overlaps i + 1 only (IoU 0.6; 1/3 with i + 2), so box i is kept iff box i - 1 is not -- the longest
    # dependency a chunk can hold, and it runs on into a second and a ragged third chunk
    chain = torch.tensor([[0.25 * i, 0.0, 0.25 * i + 1.0, 1.0] for i in range(150)])
    k = _check_nms(dev, chain.unsqueeze(0), thr)
    assert k[0].tolist() == [1, 0] * 75
    # the only survivor of the second chunk is its lane 63: everything before it repeats box 0
    tail = torch.tensor([_unit(0, 0)] * 127 + [_unit(5, 5)])
    k = _check_nms(dev, tail.unsqueeze(0), thr)
    assert torch.where(k[0] != 0)[0].tolist() == [0, 127]
    # valid = 0 on the would-be survivors: the second box of every pair survives instead, and lane 63 alone in a chunk of copies
    valid = torch.tensor([[0, 1] * 32], dtype=torch.int32)
    k = _check_nms(dev, pairs.unsqueeze(0), thr, valid=valid)
    assert k[0].tolist() == [0, 1] * 32
    valid = torch.tensor([[0] * 63 + [1]], dtype=torch.int32)
    k = _check_nms(dev, copies.unsqueeze(0), thr, valid=valid)
    assert torch.where(k[0] != 0)[0].tolist() == [63]


# ---- mask: the division-free decision -------------------------------------------------------------------------------------
def _iou(a, b):
    """the kernel's expression, one float32 rounding per operation: a (n, 1, 4), b (1, m, 4) -> inter / (ai + aj - inter)"""
    a, b, f = a.astype(np.float32), b.astype(np.float32), np.float32
    with np.errstate(all="ignore"):
        w = np.fmax(np.fmin(a[..., 2], b[..., 2]) - np.fmax(a[..., 0], b[..., 0]), f(0))
        h = np.fmax(np.fmin(a[..., 3], b[..., 3]) - np.fmax(a[..., 1], b[..., 1]), f(0))
        inter = w * h
        ai = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
        aj = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
        iou = inter / (ai + aj - inter)
    assert iou.dtype == np.float32
    return iou


def _iou_gt(a, b, thr):
    return _iou(a, b) > np.float32(thr)


def _threshold_pairs(thr):
    """three pairs ([-1, 0, 0, 1], [-x, 0, 0, y]) whose float32 IoU is one ulp below thr, thr, and one ulp above it"""
    t = np.float32(thr)
    want = [np.nextafter(t, np.float32(-1)), t, np.nextafter(t, np.float32(2))]
    big = np.array([-1.0, 0.0, 0.0, 1.0], np.float32)
    # inter = x and union = 1 + x (y - 1) in exact arithmetic: x within a few ulps of the wanted quotient, y = 1 + m 2^-23 moves the
    # union in steps below an ulp of the quotient, and the float32 evaluation of the grid of candidates says which of them hit
    xs = np.unique(np.float32(np.float64(t) * (1.0 + np.arange(-64, 65) * 2.0 ** -25)))
    ys = np.float32(1.0 + np.arange(16) * 2.0 ** -23)
    cand = np.zeros((len(xs) * len(ys), 4), np.float32)
    cand[:, 0] = -np.repeat(xs, len(ys))
    cand[:, 3] = np.tile(ys, len(xs))
    iou = _iou(big[None, None, :], cand[None, :, :])[0]
    out = []
    for target in want:
        hit = np.where(iou == target)[0]
        assert hit.size, (thr, target)
        out.append((big, cand[hit[0]]))
    dec = [bool(_iou_gt(b[None, None], s[None, None], thr)[0, 0]) for b, s in out]
    assert dec == [False, False, True], (thr, dec)                   # the reference's decision differs across the three
    return out


def _mask_shortcut(dev):
    from omni3d_amd.kernels import select
    Q, nmax = 3, 200
    rng = np.random.default_rng(5)
    for thr in (0.5, 0.25, 0.75, float(np.float32(1.0) / np.float32(3.0)), float(np.float32(0.7))):
        # integer grid of side 8, integer widths: IoUs are exact ratios of small integers, many of them exactly at thr
        xy = rng.integers(0, 8, size=(Q, nmax, 2)).astype(np.float32) + 100.0
        wh = rng.integers(1, 9, size=(Q, nmax, 2)).astype(np.float32)
        boxes = np.concatenate([xy, xy + wh], axis=2)
        valid = np.ones((Q, nmax), np.int32)
        pairs = _threshold_pairs(thr)
        for q in range(Q):
            boxes[q, 0], boxes[q, 1] = pairs[q]                      # alone in their quadrant: box 1 is decided by box 0 only
            boxes[q, 180] = [103.0, 103.0, 103.0, 107.0]             # zero area
            boxes[q, 181] = [104.0, 104.0, 104.0, 104.0]
            boxes[q, 182] = [106.0, 102.0, 103.0, 105.0]             # x2 < x1: negative area
            boxes[q, 183] = [107.0, 107.0, 101.0, 101.0]             # both reversed: positive "area", no intersection
            boxes[q, 192:] = [[np.inf, 0.0, np.inf, 1.0], [np.nan, 100.0, 104.0, 104.0], [100.0, 100.0, np.inf, 104.0],
                              [100.0, np.nan, 104.0, np.nan], [-np.inf, -np.inf, np.inf, np.inf], [np.nan] * 4,
                              [101.0, 101.0, 105.0, np.nan], [np.inf, np.inf, np.inf, np.inf]]
            valid[q, 192:] = 0                                       # as in production: non-finite boxes take no part
        tb, tv = torch.from_numpy(boxes), torch.from_numpy(valid)
        ws = []
        keep = select.nms_sorted(tb.to(dev), thr, None, tv.to(dev), _poison=True, _ws_out=ws).cpu()
        got1 = []
        for q in range(Q):
            ref = _oracle_keep(tb[q], nmax, tv[q], thr)
            assert torch.equal(keep[q], ref), (thr, q, torch.where(keep[q] != ref)[0])
            got1.append(int(keep[q, 1]))
        assert got1 == [1, 1, 0], (thr, got1)                        # one ulp below / at thr: kept; one ulp above: suppressed
        # the mask words the scan reads: rows < n, the diagonal word (every column but the row's own) and the words above it
        words = (nmax + 63) // 64
        mask = ws[0].cpu().numpy().view(np.uint64).reshape(Q, nmax, words)
        for q in range(Q):
            over = _iou_gt(boxes[q][:, None, :], boxes[q][None, :, :], thr)
            np.fill_diagonal(over, False)
            padded = np.zeros((nmax, words * 64), bool)
            padded[:, :nmax] = over
            want = (padded.reshape(nmax, words, 64).astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=2, dtype=np.uint64)
            for i in range(nmax):
                c = i // 64
                assert np.array_equal(mask[q, i, c:], want[i, c:]), (thr, q, i)


# ---- top-k ---------------------------------------------------------------------------------------------------------------
def _check_topk(dev, keys, k):
    from omni3d_amd.kernels import select
    vals, idx = select.topk_rows(keys.to(dev), k)
    sv, si = torch.sort(keys, dim=1, descending=True, stable=True)
    kk = min(k, keys.shape[1])
    assert torch.equal(idx.cpu()[:, :kk].long(), si[:, :kk]), (keys.shape, k)
    assert torch.equal(vals.cpu()[:, :kk], sv[:, :kk]), (keys.shape, k)
    assert (idx.cpu()[:, kk:] == -1).all() and (vals.cpu()[:, kk:] == NEG_INF).all()
    return idx.cpu()


def _topk_equal_keys(dev):
    keys = torch.full((1, 3000), 0.5)
    for k in (64, 65, 2000):                                         # every lane of every wave passes; the order is the index order
        idx = _check_topk(dev, keys, k)
        assert torch.equal(idx[0].long(), torch.arange(k))


def _topk_k_boundaries(dev):
    g = torch.Generator().manual_seed(21)
    keys = torch.randn(2, 5000, generator=g)
    keys[1] = (keys[1] * 4).round() / 4                              # and with ties
    for k in (1, 2, 63, 64, 65, 1024, 2048, 2049):                   # kpad boundaries; 2048 / 2049: register sort / LDS sort
        _check_topk(dev, keys, k)


def _topk_n_boundaries(dev):
    g = torch.Generator().manual_seed(22)
    for n in (1023, 1024, 1025, 16384, 16385):
        keys = torch.randn(1, n, generator=g)
        if n == 16385:
            keys = (keys * 2).round() / 2
        _check_topk(dev, keys, 300)


def _topk_small_segments(dev):
    from omni3d_amd.kernels import select
    g = torch.Generator().manual_seed(23)
    seg_n = [768, 192, 48, 12, 3]                                    # the step's five levels, 64 x smaller
    keys = torch.randn(2, sum(seg_n), generator=g)
    keys[:, ::5] = keys[:, 2:3]
    keys = keys.to(dev)
    off = [sum(seg_n[:i]) for i in range(len(seg_n))]
    v, i = select.topk_segments(keys, off, seg_n, 100)
    for s, (o, m) in enumerate(zip(off, seg_n)):
        rv, ri = select.topk_rows(keys[:, o:o + m], 100)
        assert torch.equal(v[:, s], rv) and torch.equal(i[:, s], ri), s
        sv, si = torch.sort(keys[:, o:o + m].cpu(), dim=1, descending=True, stable=True)
        kk = min(100, m)
        assert torch.equal(ri.cpu()[:, :kk].long(), si[:, :kk]) and (ri.cpu()[:, kk:] == -1).all()


# ---- the masked scores written by the scan ---------------------------------------------------------------------------------
def _fold(dev):
    from omni3d_amd.kernels import select
    g = torch.Generator().manual_seed(31)
    Q, nmax = 3, 150
    boxes = torch.stack([_rand_boxes(g, nmax) for _ in range(Q)])
    scores = torch.sort(torch.randn(Q, nmax, generator=g), dim=1, descending=True)[0]
    scores[:, 140:] = NEG_INF                                        # padding slots of a level with few anchors
    scores[1, 3] = NEG_INF
    valid = (torch.rand(Q, nmax, generator=g) > 0.1).int()
    valid[:, 140:] = 0
    counts = torch.tensor([150, 97, 0], dtype=torch.int32)
    for cnt in (None, counts):
        c = None if cnt is None else cnt.to(dev)
        keep = select.nms_sorted(boxes.to(dev), 0.5, c, valid.to(dev), _poison=True)
        keep2, masked = select.nms_sorted_masked(boxes.to(dev), scores.to(dev), 0.5, c, valid.to(dev), _poison=True)
        assert torch.equal(keep, keep2)
        want = torch.where(keep.cpu() != 0, scores, torch.full_like(scores, NEG_INF))
        assert torch.equal(masked.cpu(), want)
        assert int(keep.sum()) > 0


CASES = [_scan_prefetch, _scan_resolution, _mask_shortcut, _topk_equal_keys, _topk_k_boundaries, _topk_n_boundaries,
         _topk_small_segments, _fold]


@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__.lstrip("_"))
def test_emulated(emu_lib, case):
    case("cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__.lstrip("_"))
def test_gpu(hip_lib, case):
    case("cuda")
