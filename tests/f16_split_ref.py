"""A CPU statement of the 2xfp16 representation (csrc/common.h split2<2>, FP16_ACT_SCALE,
fp16_wscale), shared by the host and GPU range tests.

An f32 operand v travels as two IEEE fp16 pieces of v * scale, scale a power of two:
hi = fp16(v * scale), lo = fp16(v * scale - hi), both round-to-nearest-even with fp16
subnormals kept.  A conv sums hi.hi + hi.lo + lo.hi (lo.lo is dropped) and divides by the
two scales.  Everything here is float64 on exactly those pieces: a kernel that is right
equals it up to its own f32 accumulation error, at every operand magnitude — which the
true float64 conv of the unsplit operands is not, away from O(1) operands.
"""
import numpy as np
import torch
import torch.nn.functional as F

ACT_SCALE = 32.0                # common.h FP16_ACT_SCALE
FP16_MAX = 65504.0
FP16_MIN_NORMAL = 2.0 ** -14


def fp16_wscale(K):
    """csrc/common.h fp16_wscale: 2^(9 + ceil(log2 sqrt K)), K the contraction length."""
    e = 0
    while (1 << (2 * e)) < K:
        e += 1
    return float(1 << (9 + e))


def act_limit():
    """Largest |activation| the fixed scale carries: 2047 (2047 * 32 = 65504)."""
    return FP16_MAX / ACT_SCALE


def weight_limit(K):
    """Largest |w| of a K-long contraction: 65504 / fp16_wscale(K)."""
    return FP16_MAX / fp16_wscale(K)


def pieces(v, scale, flush=False):
    """(hi, lo) of v * scale as float64 arrays.  v holds f32 values (any float dtype) and
    scale is a power of two, so v * scale and v * scale - hi are exact in f32, as in the
    kernels, and each piece is one RNE rounding to fp16 (numpy's f32 -> f16 cast keeps
    subnormals).  Beyond the range hi is +-inf and lo -+inf.  flush: pieces below fp16's
    smallest normal become zero — what a flushing MFMA or denormal mode would see; the
    host test uses it to show that the GPU test can tell the two apart."""
    m, _ = np.frexp(float(scale))
    assert m == 0.5, "scale must be a power of two"
    a64 = np.asarray(v, dtype=np.float64) * float(scale)
    with np.errstate(over="ignore", invalid="ignore"):
        a = a64.astype(np.float32)
        assert np.array_equal(a.astype(np.float64), a64), "v * scale must be exact in f32"
        hi = a.astype(np.float16)
        lo = (a - hi.astype(np.float32)).astype(np.float16)
    hi, lo = hi.astype(np.float64), lo.astype(np.float64)
    if flush:
        hi = np.where(np.abs(hi) < FP16_MIN_NORMAL, np.copysign(0.0, hi), hi)
        lo = np.where(np.abs(lo) < FP16_MIN_NORMAL, np.copysign(0.0, lo), lo)
    return hi, lo


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _np(t):
    return t.detach().cpu().double().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)


def conv_2xfp16(x, w, bias=None, res=None, pad=0, act_scale=ACT_SCALE, wscale=None, flush=False):
    """The stride-1 conv as the 2xfp16 kernels carry it, in float64:
    (hi_w*hi_x + hi_w*lo_x + lo_w*hi_x) / (act_scale * wscale) + bias + res.
    x [B,Cin,H,W]: the f32 values the kernel splits (after the prologue); w [Cout,Cin,KS,KS]
    f32 values; wscale defaults to fp16_wscale(Cin*KS*KS).  Returns a float64 tensor."""
    x, w = _np(x), _np(w)
    if wscale is None:
        wscale = fp16_wscale(w.shape[1] * w.shape[2] * w.shape[3])
    xh, xl = pieces(x, act_scale, flush)
    wh, wl = pieces(w, wscale, flush)
    # hi_w * (hi_x + lo_x) + lo_w * hi_x: the sum of two fp16 values is exact in float64
    y = F.conv2d(_t(xh + xl), _t(wh), None, 1, pad) + F.conv2d(_t(xh), _t(wl), None, 1, pad)
    y = y / (float(act_scale) * float(wscale))
    if bias is not None:
        y = y + _t(_np(bias))[None, :, None, None]
    if res is not None:
        y = y + _t(_np(res))
    return y


def dgrad_2xfp16(dy, w, dy_scale, pad=0, flush=False):
    """The data gradient of a stride-1 conv on the 2xfp16 path: the conv of the dy pieces
    (power-of-two scale dy_scale, chosen on the device) with the mode-1 weights
    wd[ci][co][tap] = w[co][ci][T-1-tap], whose weight scale is fp16_wscale(Cout*KS*KS)."""
    w = _np(w)
    wd = np.flip(w, (2, 3)).transpose(1, 0, 2, 3)
    return conv_2xfp16(dy, wd, None, None, pad, dy_scale, fp16_wscale(w.shape[0] * w.shape[2] * w.shape[3]), flush)


def wgrad3_2xfp16(dy, x, dy_scale, act_scale=ACT_SCALE, flush=False):
    """The 3x3 (pad 1) weight gradient from the two images: dy pieces (scale dy_scale) times
    the forward's x pieces (scale act_scale), hi.hi + hi.lo + lo.hi, and the bias gradient
    sum (hi + lo) / dy_scale.  Returns (dw [Cout,Cin,3,3], db [Cout]) float64 tensors."""
    dy, x = _np(dy), _np(x)
    B, Cin = x.shape[:2]
    Cout = dy.shape[1]
    yh, yl = pieces(dy, dy_scale, flush)
    xh, xl = pieces(x, act_scale, flush)
    shape = (Cout, Cin, 3, 3)
    g = torch.nn.grad.conv2d_weight
    dw = g(_t(xh + xl), shape, _t(yh), 1, 1) + g(_t(xh), shape, _t(yl), 1, 1)
    db = _t((yh + yl).sum((0, 2, 3)))
    return dw / (float(dy_scale) * float(act_scale)), db / float(dy_scale)


def act_element_bound(v):
    """|hi + lo - v*32| / 32 <= max(2^-22 |v|, 2^-30) for |v| <= 2047: two 11-bit
    significands while lo is normal, the subnormal quantum 2^-24 (half of it, over 32)
    below."""
    return np.maximum(2.0 ** -22 * np.abs(v), 2.0 ** -30)


def weight_element_bound(w, s):
    """|hi + lo - w*s| / s <= max(2^-22 |w|, 2^-25 / s) for |w| <= 65504 / s."""
    return np.maximum(2.0 ** -22 * np.abs(w), 2.0 ** -25 / s)
