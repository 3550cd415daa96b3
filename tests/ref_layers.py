"""The memory-bound layer kernels of csrc/bn_pool.hip (below the BatchNorm section), csrc/pool3.hip and csrc/depthwise.hip written
from their definitions in float64 (the references of tests/test_layer_kernels.py), the launch arithmetic of their launchers, and
the a-priori error bounds of the kernels that add.  Everything is torch on the device of its input, so the one large case per
kernel stays on the GPU.  Only strided slices, F.pad, unfold and elementwise arithmetic: no library pooling or convolution.

All tensors are NHWC.  Window scan order is row-major ((0,0), (0,1), ..., (R-1,R-1)); in both max-pools the first maximum in that
order wins and padding counts as -inf.

Bounds.  A sum of terms t_j whose longest sequential path has L fp32 roundings satisfies

    |got - ref64| <= gamma(L) * sum_j |t_j|,       gamma(L) = L u / (1 - L u),  u = 2^-24

(Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1 and section 4.2: any summation order, L the depth of the
deepest path).  A product that is rounded before it is added counts as one rounding of its term; a fused multiply-add has one
fewer, so the bound covers both.  The first addition onto a zero accumulator is exact and is not counted.  The L of every kernel is
derived from its source in the docstring of its *_chain function below.  fp64 additions inside a kernel (the finalize of
omni_bias_grad) are counted apart at 2^-53 each.
"""
import math

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24        # unit roundoff of fp32
U64 = 2.0 ** -53

EW_CAP = 2048 * 256     # ew_grid (bn_pool.hip, pool3.hip): at most 2048 workgroups of 256 threads
DW_CAP = 8192 * 256     # dw_grid (depthwise.hip), grid_for (resize.hip): at most 8192 workgroups of 256 threads


def gamma(L):
    """L u / (1 - L u): the relative error bound of L successive fp32 roundings"""
    return L * U32 / (1.0 - L * U32)


def f64(t, absolute=False):
    t = t.detach().double()
    return t.abs() if absolute else t


# ---- launch arithmetic ------------------------------------------------------------------------------------------------------
def out_hw(H, W):
    """output extent of the stride-2 subsample and of the 3x3/s2/p1 max-pool"""
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def items_pool2(N, H, W, C):
    """work items of maxpool2_fwd/bwd, avgpool2_fwd/bwd, upsample2_bwd: one per (2x2 window, channel quad)"""
    return N * (H // 2) * (W // 2) * (C // 4)


def items_sub(N, H, W, C):
    """work items of subsample2_fwd/bwd and maxpool3s2_fwd: one per (output pixel, channel quad)"""
    OH, OW = out_hw(H, W)
    return N * OH * OW * (C // 4)


def items_full(N, H, W, C):
    """work items of subsample2_bwd_carry, maxpool3s2_bwd, upsample2_add, dwconv_dgrad: one per (input pixel, channel quad)"""
    return N * H * W * (C // 4)


def dw_out(H, W, R, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1


def items_dw_fwd(N, H, W, C, R, stride, pad):
    OH, OW = dw_out(H, W, R, stride, pad)
    return N * OH * OW * (C // 4)


def grid(total, cap):
    """workgroups of 256 threads of an elementwise launch over `total` work items"""
    return max(1, min(cap // 256, (total + 255) // 256))


def assert_two_uneven_trips(total, cap, C=None):
    """the premise of a 'large' case: the grid-stride loop runs at least twice, some threads once more than others, and the channel
    quads per pixel are no power of two (an index decomposition by shifts or masks would be wrong)"""
    assert total > cap, (total, cap)
    assert total % cap != 0, (total, cap)
    assert grid(total, cap) * 256 == cap
    if C is not None:
        c4 = C // 4
        assert c4 & (c4 - 1), C


def red_grid(P, C):
    """workgroups of the column reduction behind omni_bias_grad (red_grid in bn_pool.hip): >= 4 pixel rows per thread, <= 512"""
    rows = 1 if (C >> 2) >= 256 else 256 // (C >> 2)
    return max(1, min(512, (P + 4 * rows - 1) // (4 * rows)))


def bias_grad_chain(P, C, accumulate, atomic):
    """(L32, L64) of omni_bias_grad's bound (gamma(L32) + L64 * 2^-53) * (sum_p |dy[p, c]| + |db0[c]|).

    bn_reduce_tile<0> walks the C/4 channel quads in tiles of at most 256.  In a tile of width C4 a workgroup has rows = 256 / C4
    pixel rows (threads past rows * C4 idle); a thread adds the pixels p = blk * rows + row + k * nblk * rows one after the other
    onto a zero accumulator: n = ceil(P / (nblk * rows)) terms, n - 1 roundings.  Thread t < C4 then adds the rows one after the
    other from LDS: rows - 1 roundings.  colsum_finalize_kernel adds the nblk partial rows in fp64 (L64 = nblk), rounds once to
    fp32 (+1) and with accumulate adds that to db (+1, db0 one more term).
    atomic (accumulate == 1 and nblk <= 64, GPU only): bias_grad_atomic_kernel keeps the same thread walk (its 4-deep tree
    (v0 + v1) + (v2 + v3) only shortens a path) and the same LDS fold, then every workgroup adds its sum to db with one float
    atomic: nblk more roundings, no fp64 and no final cast."""
    nblk = red_grid(P, C)
    worst = 0
    C4 = C >> 2
    for cbase in range(0, C4, 256):
        width = min(256, C4 - cbase)
        rows = 256 // width
        n = (P + nblk * rows - 1) // (nblk * rows)
        worst = max(worst, (n - 1) + (rows - 1))
    if atomic:
        assert accumulate == 1 and nblk <= 64
        return worst + nblk, 0
    return worst + 1 + (1 if accumulate else 0), nblk


def dw_wgrad_slices(N, H, W, C, R, stride, pad):
    """blockIdx.y extent of dwconv_wgrad_kernel (omni_dwconv_wgrad): ~2048 workgroups, at least 64 output pixels per lane"""
    OH, OW = dw_out(H, W, R, stride, pad)
    P = N * OH * OW
    cb = (C // 4 + 63) // 64
    return max(1, min(2048 // cb, P // 256))


def dw_wgrad_chain(N, H, W, C, R, stride, pad):
    """L of omni_dwconv_wgrad's bound gamma(L) * sum |x| |dy| per (tap, channel).

    A lane owns a channel quad and every (4 * slices)-th output pixel: n = ceil(P / (4 * slices)) products, each rounded (1) and
    added one after the other onto a zero accumulator (n - 1) -- n roundings on the path of the first term.  The 4 pixel slices of
    a workgroup are folded through LDS one after the other (3), and each of the `slices` workgroups of a channel block adds its
    sum to the zeroed dw with one float atomic (slices)."""
    OH, OW = dw_out(H, W, R, stride, pad)
    P = N * OH * OW
    slices = dw_wgrad_slices(N, H, W, C, R, stride, pad)
    n = (P + 4 * slices - 1) // (4 * slices)
    return n + 3 + slices


def dw_fwd_chain(R):
    """L of omni_dwconv_fwd: R^2 products, each rounded and added in scan order onto a zero accumulator -> R^2 roundings on the
    path of the first tap"""
    return R * R


def dw_dgrad_chain(R, stride):
    """L of omni_dwconv_dgrad: an input pixel is read by at most ceil(R / stride)^2 (tap, output pixel) pairs, each product rounded
    and added one after the other onto a zero accumulator"""
    return math.ceil(R / stride) ** 2


AVGPOOL_CHAIN = 3       # ((a + b) + c) + d, then * 0.25 (exact)
MAXPOOL3_BWD_CHAIN = 3  # an input pixel lies in at most 4 windows; g += d one after the other onto zero
UPSAMPLE_BWD_CHAIN = 2  # (a + b) + (c + d)
CARRY_CHAIN = 1         # + carry: one more rounding, the carry one more term


# ---- 2x2 / stride 2 pools ------------------------------------------------------------------------------------------------------
def _windows2(x):
    """x (N,H,W,C) -> the 4 window positions in scan order, each (N,H/2,W/2,C); an odd last row / column is in no window"""
    H2, W2 = x.shape[1] // 2 * 2, x.shape[2] // 2 * 2
    return [x[:, r:H2:2, s:W2:2] for r in (0, 1) for s in (0, 1)]


def _first_max(vals):
    """(maximum, index of the first maximum) over a list of equally shaped tensors, in list order"""
    m = vals[0].clone()
    k = torch.zeros(m.shape, dtype=torch.int64, device=m.device)
    for j in range(1, len(vals)):
        gt = vals[j] > m
        m = torch.where(gt, vals[j], m)
        k = torch.where(gt, torch.full_like(k, j), k)
    return m, k


def maxpool2_fwd(x):
    return _first_max(_windows2(f64(x)))[0]


def maxpool2_bwd(x, dy, absolute=False):
    """dx: dy routed to the first maximum of every window, zero elsewhere (also in an odd last row / column)"""
    _, k = _first_max(_windows2(f64(x)))
    dx = torch.zeros(x.shape, dtype=torch.float64, device=x.device)
    g = f64(dy, absolute)
    for j, v in enumerate(_windows2(dx)):
        v.copy_(torch.where(k == j, g, torch.zeros_like(g)))
    return dx


def avgpool2_fwd(x, absolute=False):
    a, b, c, d = _windows2(f64(x, absolute))
    return (a + b + c + d) * 0.25


def avgpool2_bwd(dy, H, W):
    N, _, _, C = dy.shape
    dx = torch.zeros((N, H, W, C), dtype=torch.float64, device=dy.device)
    for v in _windows2(dx):
        v.copy_(f64(dy) * 0.25)
    return dx


# ---- stride-2 subsample --------------------------------------------------------------------------------------------------------
def subsample2_fwd(x):
    return f64(x)[:, ::2, ::2]


def subsample2_bwd(dy, H, W, absolute=False):
    N, _, _, C = dy.shape
    dx = torch.zeros((N, H, W, C), dtype=torch.float64, device=dy.device)
    dx[:, ::2, ::2] = f64(dy, absolute)
    return dx


# ---- 3x3 / stride 2 / padding 1 max-pool -----------------------------------------------------------------------------------------
def _windows3(x):
    """x (N,H,W,C) float64 -> the 9 window positions in scan order, each (N,OH,OW,C); padding is -inf"""
    xp = F.pad(x, (0, 0, 1, 1, 1, 1), value=float("-inf"))
    win = xp.unfold(1, 3, 2).unfold(2, 3, 2)            # (N,OH,OW,C,3,3)
    return [win[..., r, s] for r in range(3) for s in range(3)]


def maxpool3s2_fwd(x):
    return _first_max(_windows3(f64(x)))[0]


def maxpool3s2_bwd(x, dy, absolute=False):
    """dx[pixel] = sum of dy over the (at most 4) windows whose first maximum is that pixel"""
    N, H, W, C = x.shape
    OH, OW = out_hw(H, W)
    _, k = _first_max(_windows3(f64(x)))
    g = f64(dy, absolute)
    dxp = torch.zeros((N, 2 * OH + 1, 2 * OW + 1, C), dtype=torch.float64, device=x.device)
    for j in range(9):
        r, s = divmod(j, 3)
        dxp[:, r:r + 2 * OH:2, s:s + 2 * OW:2] += torch.where(k == j, g, torch.zeros_like(g))
    return dxp[:, 1:H + 1, 1:W + 1]


# ---- FPN top-down --------------------------------------------------------------------------------------------------------------
def upsample2(top):
    return f64(top).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def upsample2_add(lat, top):
    """exact in float64 for fp32 operands of comparable magnitude; the kernel's one rounding is the cast of this to fp32"""
    return f64(lat) + upsample2(top)


def upsample2_bwd(dout, absolute=False):
    a, b, c, d = _windows2(f64(dout, absolute))
    return a + b + c + d


# ---- elementwise ---------------------------------------------------------------------------------------------------------------
def relu_bwd(dy, y):
    return torch.where(y > 0, f64(dy), torch.zeros((), dtype=torch.float64, device=dy.device))


def preprocess(imgs, mean, std, PH, PW, image_hw=None):
    """imgs (N,3,H,W) uint8 -> (N,PH,PW,4) fp32: (v - mean) / std inside the valid region (image_hw rows clamped to the slot, the
    whole slot without image_hw), exactly zero outside it, in channel 3 and in the padding up to (PH, PW).
    The fp32 expression (img.float() - mean) / std evaluated through float64: the difference of two fp32 values is exact in
    float64, so its cast is the correctly rounded fp32 difference, and a float64 quotient of two fp32 values rounds to the correctly
    rounded fp32 quotient (53 >= 2 * 24 + 2) -- bit-equal to IEEE fp32 arithmetic on any device."""
    N, _, H, W = imgs.shape
    dev = imgs.device
    m = torch.tensor([float(v) for v in mean], dtype=torch.float32, device=dev).double().view(1, 3, 1, 1)
    s = torch.tensor([float(v) for v in std], dtype=torch.float32, device=dev).double().view(1, 3, 1, 1)
    v = ((imgs.double() - m).float().double() / s).float()
    if image_hw is not None:
        hw = image_hw.to(dev).long()
        vh, vw = hw[:, 0].clamp(max=H).view(N, 1, 1, 1), hw[:, 1].clamp(max=W).view(N, 1, 1, 1)
        inside = (torch.arange(H, device=dev).view(1, 1, H, 1) < vh) & (torch.arange(W, device=dev).view(1, 1, 1, W) < vw)
        v = torch.where(inside, v, torch.zeros_like(v))
    out = torch.zeros((N, PH, PW, 4), dtype=torch.float32, device=dev)
    out[:, :H, :W, :3] = v.permute(0, 2, 3, 1)
    return out


def bias_grad(dy2d, absolute=False):
    return f64(dy2d, absolute).sum(0)


# ---- depthwise convolution: x (N,H,W,C), w (R,R,C), y (N,OH,OW,C) -------------------------------------------------------------------
def _taps(xp, R, stride, OH, OW):
    """the R^2 strided views of the padded input that tap (r, s) multiplies, in scan order"""
    return [(r, s, xp[:, r:r + stride * (OH - 1) + 1:stride, s:s + stride * (OW - 1) + 1:stride]) for r in range(R) for s in range(R)]


def dwconv_fwd(x, w, stride, pad, absolute=False):
    R = w.shape[0]
    OH, OW = dw_out(x.shape[1], x.shape[2], R, stride, pad)
    xp = F.pad(f64(x, absolute), (0, 0, pad, pad, pad, pad))
    wd = f64(w, absolute)
    y = torch.zeros((x.shape[0], OH, OW, x.shape[3]), dtype=torch.float64, device=x.device)
    for r, s, v in _taps(xp, R, stride, OH, OW):
        y += v * wd[r, s]
    return y


def dwconv_dgrad(dy, w, H, W, stride, pad, absolute=False):
    R = w.shape[0]
    N, OH, OW, C = dy.shape
    g, wd = f64(dy, absolute), f64(w, absolute)
    dxp = torch.zeros((N, H + 2 * pad, W + 2 * pad, C), dtype=torch.float64, device=dy.device)
    for r, s, v in _taps(dxp, R, stride, OH, OW):
        v += g * wd[r, s]
    return dxp[:, pad:pad + H, pad:pad + W]


def dwconv_wgrad(x, dy, R, stride, pad, absolute=False):
    _, OH, OW, C = dy.shape
    xp = F.pad(f64(x, absolute), (0, 0, pad, pad, pad, pad))
    g = f64(dy, absolute)
    dw = torch.zeros((R, R, C), dtype=torch.float64, device=x.device)
    for r, s, v in _taps(xp, R, stride, OH, OW):
        dw[r, s] = (v * g).sum((0, 1, 2))
    return dw
