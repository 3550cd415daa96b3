"""The argument checks the evaluation launchers, and the augmentation launchers (kernels/augment.py), share.  Nothing here launches
or allocates on a device; every check raises ValueError with the name of the argument and what was expected, and a launcher finishes all of them before it allocates or launches anything.
Read back from the device are only an offsets tensor (`offsets`, once) and the extremes of `order` (`merge_order`, once).
"""
import collections

import numpy as np
import torch


def empty(shape, dtype, like):
    return torch.empty(shape, dtype=dtype, device=like.device)


def shaped(t, name, dtype, shape):
    """t is a `dtype` tensor of `shape`, a None entry standing for any size -> its shape as a tuple"""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype:
        raise ValueError(f"{name} must be a {dtype} tensor")
    if t.dim() != len(shape) or any(want is not None and want != got for want, got in zip(shape, t.shape)):
        raise ValueError(f"{name} must have shape {str(tuple(shape)).replace('None', 'n')}, got {tuple(t.shape)}")
    return tuple(t.shape)


def tensor(t, name, dtype, shape):
    """`shaped`, and contiguous"""
    dims = shaped(t, name, dtype, shape)
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return dims


def nonempty(t, name, dtype):
    """t is a contiguous 1-D `dtype` tensor with at least one element -> its length"""
    n = tensor(t, name, dtype, (None,))[0]
    if n < 1:
        raise ValueError(f"{name} must be 1-D and not empty")
    return n


def integer(v, name, lo=None, hi=None):
    """v is an int (no bool, no float) with lo <= v <= hi where given -> v"""
    if isinstance(v, bool) or not isinstance(v, int) or (lo is not None and v < lo) or (hi is not None and v > hi):
        bound = "" if lo is None and hi is None else f" >= {lo}" if hi is None else f" <= {hi}" if lo is None else f" in [{lo}, {hi}]"
        raise ValueError(f"{name} must be an integer{bound}, got {v!r}")
    return v


def window(box, H, W, name="box"):
    """box = (x0, y0, w, h): four integers, a window of positive extent inside an H x W image -> the four"""
    if not isinstance(box, (tuple, list)) or len(box) != 4:
        raise ValueError(f"{name} must be four integers (x0, y0, w, h), got {box!r}")
    x0, y0, w, h = (integer(v, f"{name}[{i}]") for i, v in enumerate(box))
    if w <= 0 or h <= 0 or x0 < 0 or y0 < 0 or x0 + w > W or y0 + h > H:
        raise ValueError(f"{name} {tuple(box)} must be a window of positive extent inside the {H} x {W} image")
    return x0, y0, w, h


def matrix3(m, name):
    """nine finite numbers as a 3 x 3 -> them as a contiguous float64 array"""
    try:
        a = np.ascontiguousarray(np.asarray(m, dtype=np.float64))
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a 3 x 3 matrix of finite numbers, got {m!r}") from None
    if a.shape != (3, 3) or not np.isfinite(a).all():
        raise ValueError(f"{name} must be a 3 x 3 matrix of finite numbers, got {m!r}")
    return a


def one_device(tensors):
    if len({t.device for t in tensors}) != 1:
        raise ValueError("all inputs must live on one device")


def offset_count(off, name):
    """off holds the n + 1 int32 prefix offsets of n ranges -> n, with nothing read back"""
    return nonempty(off, name, torch.int32) - 1


def offsets(off, name, total=None, count=None):
    """off holds int32 prefix offsets (of `count` ranges when given) that start at 0, never decrease and end at `total` when given
    -> the offsets as a host list: the one read-back of a launcher that takes them"""
    if not tensor(off, name, torch.int32, (None if count is None else count + 1,))[0]:
        raise ValueError(f"{name} must hold at least one offset")
    o = off.tolist()
    if o[0] != 0 or any(b < a for a, b in zip(o, o[1:])) or (total is not None and o[-1] != total):
        raise ValueError(f"{name} must start at 0, never decrease" + ("" if total is None else f" and end at {total}"))
    return o


def pair_index(idx1, idx2):
    """idx1 / idx2: 1-D int32 or int64 tensors of equal length -> both as contiguous int32"""
    for i in (idx1, idx2):
        if not isinstance(i, torch.Tensor) or i.dim() != 1 or i.dtype not in (torch.int32, torch.int64):
            raise ValueError("idx1 / idx2 must be 1-D int32 or int64 tensors")
    if idx1.shape != idx2.shape:
        raise ValueError("idx1 / idx2 must be of equal length")
    return idx1.to(torch.int32).contiguous(), idx2.to(torch.int32).contiguous()


def all_pairs(N, M, device):
    """-> (idx1, idx2) int32 of the N x M grid, row-major: pair n * M + m is (n, m)"""
    rows, cols = torch.arange(N, dtype=torch.int32, device=device), torch.arange(M, dtype=torch.int32, device=device)
    return rows.repeat_interleave(M), cols.repeat(N)


def box_set(s, name, source, parts):
    """s is the tuple a launcher `source` returns for n boxes; parts: (member, dtype, the shape behind the leading n) of every member
    -> n"""
    if not isinstance(s, (tuple, list)) or len(s) != len(parts) or not all(isinstance(t, torch.Tensor) for t in s):
        raise ValueError(f"{name} must be the ({', '.join(p[0] for p in parts)}) of {source}")
    n = s[0].shape[0] if s[0].dim() else -1
    for t, (member, dtype, tail) in zip(s, parts):
        tensor(t, f"{name}: {member}", dtype, (n, *tail))
    return n


MergeOrder = collections.namedtuple("MergeOrder", "K A T R sumD off")


def merge_order(order, cat_off, dt_match, dt_ignore, rec_thrs, per_threshold=True):
    """The tables `Omni3Deval._device_tables` builds, as every accumulation takes them: order (N,) int32 indexing the sumD detections,
    cat_off (K+1,) int32 its ranges per category, dt_match (A, T, sumD) int32 / dt_ignore uint8 of the same shape -- (A, sumD) with
    per_threshold False --, rec_thrs (R,) float64 not empty, all on one device
    -> MergeOrder(K, A, T, R, sumD, off), off being cat_off as a host list (T = 1 with per_threshold False).  The caller checks its
    further tensors against these sizes, and then `one_device` over all of them."""
    K = offset_count(cat_off, "cat_off")
    tensor(order, "order", torch.int32, (None,))
    dims = tensor(dt_match, "dt_match", torch.int32, (None,) * (3 if per_threshold else 2))
    if min(dims[:-1]) < 1:
        raise ValueError("dt_match must have shape " + ("(A, T, sumD) with A >= 1 and T >= 1" if per_threshold else "(A, sumD) with A >= 1"))
    A, T, sumD = dims[0], dims[1] if per_threshold else 1, dims[-1]
    tensor(dt_ignore, "dt_ignore", torch.uint8, dims)
    R = nonempty(rec_thrs, "rec_thrs", torch.float64)
    one_device((order, cat_off, dt_match, dt_ignore, rec_thrs))
    off = offsets(cat_off, "cat_off", order.numel())
    if order.numel() and (int(order.min()) < 0 or int(order.max()) >= sumD):
        raise ValueError("order must index the sumD detections")
    return MergeOrder(K, A, T, R, sumD, off)


def corners(b, name):
    """b is an (N, 8, 3) float32 contiguous tensor of cuboid corners -> N"""
    return tensor(b, name, torch.float32, (None, 8, 3))[0]


def counter(counts, like):
    """the optional one-element int32 tensor a kernel adds a count to, on the device of `like`"""
    if counts is not None and (not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or counts.numel() != 1
                               or counts.device != like.device):
        raise ValueError("counts must be one int32 on the boxes' device")


def matrices(t, n, name):
    """t holds n 3 x 3 float32 matrices as (n, 3, 3) or (n, 9)"""
    tensor(t, name, torch.float32, (n, 3, 3) if isinstance(t, torch.Tensor) and t.dim() == 3 else (n, 9))


def up_vector(up):
    """three finite numbers, not all zero -> them as a float64 array"""
    u = np.asarray(up, dtype=np.float64).reshape(-1)
    if u.shape != (3,) or not np.isfinite(u).all() or not np.linalg.norm(u) > 0:
        raise ValueError("up must be three finite numbers, not all zero")
    return u
