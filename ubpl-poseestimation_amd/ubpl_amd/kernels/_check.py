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
