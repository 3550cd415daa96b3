"""The Winograd F(2x2,3x3) and F(4x4,3x3) transforms of csrc/winograd.hip written from their definitions in float64 (the
references of tests/test_winograd_transforms.py), the a-priori error bounds of the fp32 kernels, and the launch arithmetic the
statistics bounds need.  Everything is torch on the device of its input, so the one large case per kernel family stays on the GPU.

    Y = A^T [ (G g G^T) (.) (B^T d B) ] A        d: (tile+2)^2 input window, g: 3x3 filter, Y: tile^2 outputs

Layouts, P = (tile+2)^2, point p = (tile+2) r + s, tile index t = (n TH + ty) TW + tx, TH = H / tile, TW = W / tile:
    V[p][t][c] = (B^T d B)[r][s]       d = the window of x (NHWC) that starts at pixel (tile ty - 1, tile tx - 1), zeros outside
    dM[p][t][k] = (A dy A^T)[r][s]     dy = the tile x tile block of the output gradient at (tile ty, tile tx)
    Vd[p][t][k]                        = V of dy (the data gradient is the same convolution of dy)
    y = A^T M A                        M[p][t][k] -> the tile x tile block of y at (tile ty, tile tx)
    U[p][k][c] = (G g[k,c] G^T)[r][s]
    U'[p][c][k] = (G rot180(g[k,c]) G^T)[r][s]
    dw[k][c] = G^T dU[.][k][c] G       dU[p][k][c]

Every function takes absolute=True to evaluate the same transform with |matrix| on |input|: T_abs of the bound

    |got - ref64| <= 16 * 2^-24 * T_abs  (+ 2^-24 * (|ref| + |bias| + |carry|) where one more rounding adds those)

the a-priori bound of two passes of at most 6-term fp32 dot products whose coefficients are rounded once.
"""
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24        # unit roundoff of fp32


def _m(rows):
    return torch.tensor(rows, dtype=torch.float64)


BT = {
    2: _m([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]),
    4: _m([[1, -3 / 2, -2, 3 / 2, 1, 0], [0, -1, 1 / 2, 5 / 2, 1, 0], [0, 1, -5 / 2, 1 / 2, 1, 0], [0, -2, -1, 2, 1, 0],
           [0, 1 / 2, -1, -1 / 2, 1, 0], [0, 1, -3 / 2, -2, 3 / 2, 1]]),
}
G = {
    2: _m([[1, 0, 0], [1 / 2, 1 / 2, 1 / 2], [1 / 2, -1 / 2, 1 / 2], [0, 0, 1]]),
    4: _m([[1, 0, 0], [1 / 3, 1 / 3, 1 / 3], [-1 / 3, 1 / 3, -1 / 3], [-16 / 15, -8 / 15, -4 / 15], [1 / 15, -2 / 15, 4 / 15], [0, 0, 1]]),
}
AT = {
    2: _m([[1, 1, 1, 0], [0, 1, -1, -1]]),
    4: _m([[1, 1, 1, 1, 1, 0], [0, 1, -1, 1 / 2, -2, 0], [0, 1, 1, 1 / 4, 4, 0], [0, 1, -1, 1 / 8, -8, 1]]),
}


def _mat(table, tile, like, absolute):
    m = table[tile].to(like.device)
    return m.abs() if absolute else m


def _f64(t, absolute):
    t = t.detach().double()
    return t.abs() if absolute else t


def windows(x, tile):
    """x (N,H,W,C) -> (N,TH,TW,C,tile+2,tile+2): window (ty, tx) starts at pixel (tile ty - 1, tile tx - 1), zeros outside"""
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    return xp.unfold(1, tile + 2, tile).unfold(2, tile + 2, tile)


def input_transform(x, tile, absolute=False):
    """x (N,H,W,C) -> V (P,T,C) = B^T d B"""
    B = _mat(BT, tile, x, absolute)
    N, H, W, C = x.shape
    V = torch.einsum("ar,nyxcrs,bs->abnyxc", B, windows(_f64(x, absolute), tile), B)
    return V.reshape((tile + 2) ** 2, N * (H // tile) * (W // tile), C)


def dy_transform(dy, tile, absolute=False):
    """dy (N,H,W,K) -> dM (P,T,K) = A dy A^T"""
    A = _mat(AT, tile, dy, absolute)
    N, H, W, K = dy.shape
    d = _f64(dy, absolute).reshape(N, H // tile, tile, W // tile, tile, K)
    dM = torch.einsum("ra,nyrxsk,sb->abnyxk", A, d, A)
    return dM.reshape((tile + 2) ** 2, N * (H // tile) * (W // tile), K)


def output_transform(M, shape, absolute=False):
    """M (P,T,K), shape = (N,H,W) -> y (N,H,W,K) = A^T M A"""
    N, H, W = shape
    tile = 2 if M.shape[0] == 16 else 4
    A = _mat(AT, tile, M, absolute)
    m = _f64(M, absolute).reshape(tile + 2, tile + 2, N, H // tile, W // tile, M.shape[2])
    return torch.einsum("ir,rsnyxk,js->nyixjk", A, m, A).reshape(N, H, W, M.shape[2])


def weights_transform(g, tile, flip=False, absolute=False):
    """g (K,C,3,3) -> U (P,K,C) = G g G^T, or with flip U' (P,C,K) = G rot180(g) G^T"""
    Gm = _mat(G, tile, g, absolute)
    g = _f64(g, absolute)
    K, C = g.shape[:2]
    if flip:
        return torch.einsum("ar,kcrs,bs->abck", Gm, g.flip(2, 3), Gm).reshape((tile + 2) ** 2, C, K)
    return torch.einsum("ar,kcrs,bs->abkc", Gm, g, Gm).reshape((tile + 2) ** 2, K, C)


def dweights_transform(dU, absolute=False):
    """dU (P,K,C) -> dw (K,C,3,3) = G^T dU G"""
    tile = 2 if dU.shape[0] == 16 else 4
    Gm = _mat(G, tile, dU, absolute)
    d = _f64(dU, absolute).reshape(tile + 2, tile + 2, dU.shape[1], dU.shape[2])
    return torch.einsum("ar,abkc,bs->kcrs", Gm, d, Gm)


def transform_bound(t_abs, *rounded):
    """16 * 2^-24 * T_abs + 2^-24 * sum |r| over `rounded`: the terms of the one rounding a bias, a ReLU or a carry adds
    (the final reference, the bias, the carry)"""
    b = 16.0 * U32 * t_abs
    for r in rounded:
        b = b + U32 * r.detach().double().abs()
    return b


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound; an element whose bound is zero must be exact (it then counts as 0, else as inf)"""
    err = (got.detach().double() - ref).abs()
    bound = bound.expand_as(err)
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(ratio.max())


# ---- the launch of the output transforms with fused statistics (wino_out_impl in csrc/winograd.hip) ---------------------------
def natural_grid(N, H, W, K, tile):
    """workgroups of 256 threads, one (tile, channel group of 4) per thread and iteration, at most 4096"""
    total = N * (H // tile) * (W // tile) * (K // 4)
    return max(1, min(4096, (total + 255) // 256))


def stats_rows(N, H, W, K, tile, cap):
    """partial rows a statistics launch writes: one per workgroup, the grid cut down to the buffer's capacity"""
    return min(natural_grid(N, H, W, K, tile), cap)


def stats_chain(N, H, W, K, tile, rows):
    """L of the statistics bound L * 2^-24 * sum |term| per channel: the longest sequential fp32 chain a channel's sum goes through.
    A thread keeps one channel group and adds tile^2 values per iteration of its grid-stride walk over `rows` workgroups; the
    256 / (K/4) threads of a group are then added one after the other in LDS; the rows are added by the consumer.
        L = ceil(total / (256 rows)) * tile^2  +  256 / (K/4)  +  rows,       total = N (H/tile) (W/tile) (K/4)
    (A chain of n values has n - 1 roundings and the tests add the rows in float64, so the rounding of each term itself --
    the square, or dz * xhat with xhat = (x - mean) * rstd: at most 3 -- is inside L as well.)"""
    total = N * (H // tile) * (W // tile) * (K // 4)
    iters = (total + 256 * rows - 1) // (256 * rows)
    return iters * tile * tile + 256 // (K // 4) + rows
