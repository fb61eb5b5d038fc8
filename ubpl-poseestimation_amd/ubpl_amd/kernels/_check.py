"""Argument checks of the device wrappers: the only place that validates tensors.

The family modules read `_chk` as this module's attribute (`_check._chk(...)`), as the
helpers below do, so replacing that one attribute switches the tensor check for all of them.
"""
import torch

from .. import _lib
from .view_geometry import MAX_VIEWS

F32 = torch.float32


def _chk(t, name, dtype=F32):
    if t is None:
        return
    _lib.require_gpu(t)
    if t.dtype != dtype:
        raise TypeError("ubpl_amd: %s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("ubpl_amd: %s must be contiguous" % name)


def _chk_maps(t, name, counts, strides, plane, signed=True):
    """t (None: nothing to check) holds strided maps: counts[i] steps of strides[i] floats, then
    one block of `plane` floats.  signed=False: a negative stride is refused as well."""
    if t is None:
        return
    _chk(t, name)
    need = sum((n - 1) * st for n, st in zip(counts, strides)) + plane
    if t.numel() < need or not (signed or min(strides) >= 0):
        if len(counts) == 1:
            raise ValueError("ubpl_amd: %s holds %d floats, %d maps of stride %d need %d"
                             % (name, t.numel(), counts[0], strides[0], need))
        if len(counts) > 2:
            raise ValueError("ubpl_amd: %s holds %d floats, %s maps of strides %s need %d"
                             % (name, t.numel(), " x ".join(map(str, counts)), ", ".join(map(str, strides)), need))
        raise ValueError("ubpl_amd: %s holds %d floats, %d x %d maps of strides %d, %d need %d"
                         % (name, t.numel(), *counts, *strides, need))


def _chk_entries(perm, K, tinv, swap=None, V=None, N=None):
    """perm int32 [K], swap int32 [V] and tinv float64 ([N,6] where N is given), each or None."""
    _chk(swap, "swap", torch.int32)
    _chk(perm, "perm", torch.int32)
    _chk(tinv, "tinv", torch.float64)
    if swap is not None and swap.numel() != V:
        raise ValueError("ubpl_amd: swap has %d entries for %d views" % (swap.numel(), V))
    if perm is not None and perm.numel() != K:
        raise ValueError("ubpl_amd: perm has %d entries for %d joints" % (perm.numel(), K))
    if N is not None and tinv is not None and tinv.numel() != N * 6:
        raise ValueError("ubpl_amd: tinv has %d entries for %d samples" % (tinv.numel(), N))


def _outs(out, dev, *rows):
    """The outputs of a wrapper: `out` as given, or per (shape, wanted) row a fresh float32 tensor
    or None."""
    if out is not None:
        return tuple(out)
    return tuple(torch.empty(shape, device=dev, dtype=F32) if wanted else None for shape, wanted in rows)


def _same_shape(name, t, shape):
    if t is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("ubpl_amd: %s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))


def _members(name, M):
    if not 1 <= M <= 8:
        raise ValueError("ubpl_amd: %s takes 1 to 8 members, got %d" % (name, M))


def _views(name, V, lo):
    if not lo <= V <= MAX_VIEWS:
        raise ValueError("ubpl_amd: %s takes %d to %d views, got %d" % (name, lo, MAX_VIEWS, V))


def _one_float(t, name):
    """t (through _chk already) is one float: a threshold the kernel reads."""
    if t is None or t.numel() != 1:
        raise ValueError("ubpl_amd: %s is a device float32 tensor of one element" % name)


def _no_overlap(name, lo, hi, *outs):
    """No float32 output (None: not written) reaches into the input's bytes [lo, hi)."""
    for t in outs:
        if t is not None and t.numel() and t.data_ptr() < hi and lo < t.data_ptr() + t.numel() * 4:
            raise ValueError("ubpl_amd: %s writes %s its input" % (
                name, "a tensor that does not overlap" if len(outs) == 1 else "tensors that do not overlap"))


def _bn_tuple(name, bn, C):
    """bn is a BatchNorm's eight [C] tensors (rmean / rvar nullable)."""
    if bn is None or len(bn) != 8:
        raise ValueError("ubpl_amd: %s is (gamma, beta, rmean, rvar, mean, invstd, scale, shift)" % name)
    for i, t in enumerate(bn):
        _same_shape("%s[%d]" % (name, i), t, (C,))


def _plane(x):
    """x [B,C,...] -> (B, C, elements of one plane)."""
    B, C = x.shape[:2]
    return B, C, x[0, 0].numel()


def _crop_plan(table, gauss, off, hw, nbank, R):
    """Every index ubpl_crop_frames derives from a plan row stays inside its buffer: table int32
    [n,16] and gauss [n,2,gw] (host arrays: ubpl_amd.frames.crop_plan), off / hw the host copies of
    the bank's layout, nbank its bytes."""
    if table.ndim != 2 or table.shape[1] != 16 or table.dtype.kind != "i" or not len(table):
        raise ValueError("ubpl_amd: crop_frames: the plan is an int32 table [n,16], n >= 1")
    n = len(table)
    if gauss.ndim != 3 or gauss.shape[:2] != (n, 2) or gauss.shape[2] < 2:
        raise ValueError("ubpl_amd: crop_frames: gauss is [n,2,gw] with gw >= 2 for %d boxes" % n)
    t = table.astype("int64")
    hw = hw.reshape(-1, 2).astype("int64")
    off = off.astype("int64")
    f = t[:, 0]
    if len(off) != len(hw) or (f < 0).any() or (f >= len(hw)).any():
        raise ValueError("ubpl_amd: crop_frames: a frame index outside the bank's %d frames" % len(hw))
    if (hw < 1).any() or (off < 0).any() or (off + hw[:, 0] * hw[:, 1] * 3 > nbank).any():
        raise ValueError("ubpl_amd: crop_frames: a frame reaches past the end of the bank")
    for a in (1, 7):
        org, ls, lo, o, lb, r = (t[:, a + i] for i in range(6))
        if (ls < 1).any() or (lo < 1).any() or (lb < 1).any() or (r < 0).any() or (r + 2 > gauss.shape[2]).any() \
                or (abs(org) + ls >= 2 ** 30).any() or (abs(o) + lb >= 2 ** 30).any():
            raise ValueError("ubpl_amd: crop_frames: a plan row is out of range")
    first, rows = t[:, 13], t[:, 14]
    if (first < 0).any() or (rows < 1).any() or (first + rows > t[:, 8]).any() or int(rows.max()) * R >= 2 ** 31 \
            or R < 1 or R * R >= 2 ** 31:
        raise ValueError("ubpl_amd: crop_frames: a box's source rows leave its virtual source")
    # the kernel's second pass skips a tap outside [first, first + rows) for memory safety alone: a
    # range that misses a tap would give wrong pixels, so every tap is recomputed here
    for i in range(n):
        need = _crop_taps(t[i, 7:13], R)
        if need is not None and (need[0] < first[i] or need[1] >= first[i] + rows[i]):
            raise ValueError("ubpl_amd: crop_frames: box %d reads source rows %d..%d, its plan holds %d..%d"
                             % (i, need[0], need[1], first[i], first[i] + rows[i] - 1))


def _mirror(i, n):
    """ndimage 'mirror' of index array i into [0, n), continued periodically."""
    import numpy as np
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    m = np.mod(i, p)
    return np.where(m < n, m, p - m)


def _crop_taps(axis, R):
    """(lowest, highest) virtual-source index any of the R outputs of one plan axis (org, ls, lo,
    off, lb, r) taps, tap by tap as ubpl_crop_frames walks them; None when the box lies outside
    the zoom grid."""
    import numpy as np
    _, ls, lo, off, lb, r = (int(v) for v in axis)
    f = np.floor((np.arange(R) + 0.5) * (lb / R) - 0.5).astype(np.int64)
    g = off + np.concatenate([_mirror(f, lb), _mirror(f + 1, lb)])
    g = np.unique(g[(g >= 0) & (g < lo)])
    if not g.size:
        return None
    fq = np.floor((g + 0.5) * (ls / lo) - 0.5).astype(np.int64)
    idx = _mirror(fq[:, None] + np.arange(-r, r + 2)[None, :], ls)
    return int(idx.min()), int(idx.max())
