"""Pooling, upsampling and the elementwise add of the hourglass."""
import torch

from .. import _lib
from ._check import F32


def maxpool2x2(x, out=None, stat_part=None):
    """stat_part: BatchNorm partials of the output (bn_partial_buffer; needs
    (H/2)*(W/2) % 64 == 0, see stats_ok)."""
    B, C, H, W = x.shape
    y = torch.empty((B, C, H // 2, W // 2), device=x.device, dtype=F32) if out is None else out
    if stat_part is not None:
        _lib.call("ubpl_maxpool2x2_forward_stats", x, B, C, H, W, y, stat_part)
    else:
        _lib.call("ubpl_maxpool2x2_forward", x, B * C, H, W, y)
    return y


def stats_ok(H, W):
    """Elementwise producers (max-pool, upsample-add) emit BatchNorm partials for planes of 64k pixels."""
    return (H * W) % 64 == 0


def maxpool2x2_backward(x, dy, dx, accumulate):
    B, C, H, W = x.shape
    _lib.call("ubpl_maxpool2x2_backward", x, dy, B * C, H, W, dx, int(accumulate))
    return dx


def avgpool2x2(x, out=None):
    B, C, H, W = x.shape
    y = torch.empty((B, C, H // 2, W // 2), device=x.device, dtype=F32) if out is None else out
    _lib.call("ubpl_avgpool2x2_forward", x, B * C, H, W, y)
    return y


def avgpool2x2_backward(dy, dx, accumulate):
    B, C, H, W = dx.shape
    _lib.call("ubpl_avgpool2x2_backward", dy, B * C, H, W, dx, int(accumulate))
    return dx


def upsample2x_add(up, low, out=None, stat_part=None):
    """stat_part: BatchNorm partials of the output (H*W % 64 == 0)."""
    B, C, H, W = up.shape
    y = torch.empty_like(up) if out is None else out
    if stat_part is not None:
        _lib.call("ubpl_upsample2x_add_forward_stats", up, low, B, C, H, W, y, stat_part)
    else:
        _lib.call("ubpl_upsample2x_add_forward", up, low, B * C, H, W, y)
    return y


def upsample2x_add_backward(dout, dlow, accumulate):
    B, C, H, W = dout.shape
    _lib.call("ubpl_upsample2x_add_backward", dout, B * C, H, W, dlow, int(accumulate))
    return dlow


def add(a, b, out=None):
    y = torch.empty_like(a) if out is None else out
    _lib.call("ubpl_add", a, b, a.numel(), y)
    return y
