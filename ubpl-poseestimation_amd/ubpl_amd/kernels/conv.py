"""Convolution kernels: the exact-f32 convs, the split-operand (6xbf16 / 2xfp16 / bf16) convs
on pre-split or split-on-load operands, the operand splits and the weight gradients."""
import os

import torch

from .. import _lib
from ._check import F32
from .split_operands import SplitAct, SplitWeights


def _workspace(query, *sizes):
    """Floats of workspace the C-ABI size query `query` (a ubpl_*_workspace entry) asks for."""
    return int(getattr(_lib.lib(), query)(*sizes))


def _slab(query, device, *sizes, or_none=False):
    """The f32 workspace slab of _workspace(query, *sizes) floats (or_none: None when it asks for none)."""
    n = _workspace(query, *sizes)
    return None if or_none and n <= 0 else torch.empty(n, device=device, dtype=F32)


def conv_out_hw(H, W, KS, stride):
    pad = (KS - 1) // 2
    return (H + 2 * pad - KS) // stride + 1, (W + 2 * pad - KS) // stride + 1


def conv_weight_tapmajor(w):
    Cout, Cin, KS, _ = w.shape
    wt = torch.empty((Cout, KS * KS, Cin), device=w.device, dtype=F32)
    _lib.call("ubpl_conv_weight_tapmajor", w, Cout, Cin, KS, wt)
    return wt


def conv2d_forward(x, w, bias, stride=1, pscale=None, pshift=None, res=None, out=None, w_tap=None):
    """w: reference layout [Cout,Cin,KS,KS] (re-laid out here for KS > 1) — or
    pass w_tap, an already re-laid-out copy viewed as [Cout,KS*KS,Cin] (its
    element order is ubpl_conv_weight_tapmajor's grouped tap-major layout)."""
    B, Cin, H, W = x.shape
    if w_tap is not None:
        Cout, T, wc = w_tap.shape
        KS = int(round(T ** 0.5))
        wk = w_tap
    else:
        Cout, wc, KS, _ = w.shape
        wk = w if KS == 1 else conv_weight_tapmajor(w)
    if wc != Cin:
        raise AssertionError("{} {}".format(Cin, wc))  # models/base/layers.py:44
    Ho, Wo = conv_out_hw(H, W, KS, stride)
    y = torch.empty((B, Cout, Ho, Wo), device=x.device, dtype=F32) if out is None else out
    slab = _slab("ubpl_conv2d_forward_workspace", x.device, B, Cin, Cout, KS, Ho, Wo, or_none=True)
    _lib.call("ubpl_conv2d_forward", x, B, Cin, H, W, wk, bias, Cout, KS, stride, pscale, pshift, res, y, Ho, Wo, slab)
    return y


def conv1x1_kmajor_ok(x, cout):
    """Shapes / alignment the LDS-DMA 1x1 kernel takes (x: its B operand)."""
    return (x.shape[1] % 16 == 0 and cout % 4 == 0 and (x.shape[2] * x.shape[3]) % 4 == 0
            and x.data_ptr() % 16 == 0)


def conv1x1_forward_kmajor(x, wk, bias, pscale=None, pshift=None, res=None, out=None, stat_part=None):
    """1x1 stride-1 conv with k-major weights wk (Cin*Cout floats, [Cin][Cout]):
    y = conv(relu(x*pscale + pshift) or x) + bias (+ res; res may alias out);
    stat_part: BatchNorm partials of y (bn_partial_buffer)."""
    B, Cin, H, W = x.shape
    Cout = wk.numel() // Cin
    y = torch.empty((B, Cout, H, W), device=x.device, dtype=F32) if out is None else out
    slab = _slab("ubpl_conv1x1_kmajor_workspace", x.device, B, Cin, Cout, H * W, or_none=True)
    _lib.call("ubpl_conv1x1_forward_kmajor", x, B, Cin, H * W, wk, bias, Cout, pscale, pshift, res, y, slab, stat_part)
    return y


def conv2d_wgrad(dy, x, KS, stride, dw, db, pscale=None, pshift=None, accumulate=True):
    B, Cin, H, W = x.shape
    Cout, Ho, Wo = dy.shape[1], dy.shape[2], dy.shape[3]
    slab = _slab("ubpl_conv2d_wgrad_workspace", x.device, B, Cin, Cout, KS, Ho, Wo)
    _lib.call("ubpl_conv2d_wgrad", dy, x, B, Cin, H, W, Cout, KS, stride, pscale, pshift, Ho, Wo, slab, dw, db,
              int(accumulate))


def wgrad1x1_split_load_ok(dy, x):
    B, Cin, H, W = x.shape
    return (dy.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0
            and _workspace("ubpl_wgrad1x1_split_load_workspace", B, Cin, dy.shape[1], H * W) > 0)


def conv2d_wgrad1x1_split_load(dy, x, dw, db, pscale=None, pshift=None, accumulate=True, npieces=3):
    """1x1 weight (+ bias) gradient on the split path (npieces 3: 6xbf16; 1: bf16
    operands, f32 accumulation), f32 operands split on load (v = relu(x*pscale +
    pshift) when pscale is given)."""
    B, Cin, H, W = x.shape
    Cout = dy.shape[1]
    slab = _slab("ubpl_wgrad1x1_split_load_workspace", x.device, B, Cin, Cout, H * W)
    _lib.call("ubpl_wgrad1x1_split_load", dy, x, B, Cin, Cout, H * W, pscale, pshift, slab, dw, db, int(accumulate),
              int(npieces))


def conv_weight_flip(w):
    """Data-gradient weights (stride 1), viewed as [Cin, KS*KS, Cout]."""
    Cout, Cin, KS, _ = w.shape
    wt = torch.empty((Cin, KS * KS, Cout), device=w.device, dtype=F32)
    _lib.call("ubpl_conv_weight_flip", w, Cout, Cin, KS, wt)
    return wt


def conv_weights_relayout(src, dst, table, mode):
    """table: int64 [nseg,5] device tensor (src_off, dst_off, Cout, Cin, T)."""
    _lib.call("ubpl_conv_weights_relayout", src, dst, table, int(table.shape[0]), int(mode))


def conv_weights_split(src, dst, plane, table, mode, npieces):
    """Batched split re-layout (table as conv_weights_relayout, dst int16)."""
    _lib.call("ubpl_conv_weights_split", src, dst, int(plane), table, int(table.shape[0]), int(mode), int(npieces))


def conv_weight_split(w, mode, npieces):
    """Single conv: SplitWeights for the forward (mode 0) or data gradient (mode 1)."""
    Cout, Cin, KS, _ = w.shape
    n = w.numel()
    plane = (n + 7) // 8 * 8
    buf = torch.empty(npieces * plane, device=w.device, dtype=torch.int16)
    tbl = torch.tensor([[0, 0, Cout, Cin, KS * KS]], dtype=torch.int64).to(w.device)
    conv_weights_split(w.contiguous(), buf, plane, tbl, mode, npieces)
    shape = (Cout, KS * KS, Cin) if mode == 0 else (Cin, KS * KS, Cout)
    return SplitWeights(buf, plane, 0, shape, npieces)


def conv2d_forward_split(x, ws, bias, pscale=None, pshift=None, res=None, out=None):
    """Split-bf16 MFMA conv (stride 1, KS in {1, 3}, Cin % 16 == 0); ws: SplitWeights."""
    B, Cin, H, W = x.shape
    Cout, T, wc = ws.shape
    KS = int(round(T ** 0.5))
    if wc != Cin:
        raise AssertionError("{} {}".format(Cin, wc))
    Ho, Wo = conv_out_hw(H, W, KS, 1)
    y = torch.empty((B, Cout, Ho, Wo), device=x.device, dtype=F32) if out is None else out
    slab = _slab("ubpl_conv2d_forward_split_workspace", x.device, B, Cin, Cout, KS, Ho, Wo, ws.npieces, or_none=True)
    _lib.call("ubpl_conv2d_forward_split", x, B, Cin, H, W, ws.ptr(), int(ws.plane), bias, Cout, KS, 1, pscale, pshift,
              res, y, Ho, Wo, slab, int(ws.npieces))
    return y


def split_activation(x, npieces, pad, pscale=None, pshift=None, out=None, with3=False):
    """x [B,C,H,W] f32 -> SplitAct of relu(x*pscale + pshift) (or x), zero border `pad`.
    with3 (npieces 2): (the 2xfp16 image, the 3-piece 6xbf16 image) from one read — the
    2xfp16 forward's conv input and the 6xbf16 weight gradient's operand."""
    B, C, H, W = x.shape
    plane = B * C * (H + 2 * pad) * (W + 2 * pad)
    if out is None:
        out = torch.empty(npieces * plane, device=x.device, dtype=torch.int16)
    out3 = None
    if with3:
        if npieces != 2:
            raise ValueError("with3: the 2xfp16 split only")
        out3 = torch.empty(3 * plane, device=x.device, dtype=torch.int16)
    _lib.call("ubpl_split_activation", x, B, C, H, W, pscale, pshift, int(pad), int(npieces), out, int(plane), out3,
              int(plane))
    xs = SplitAct(out, plane, B, C, H, W, pad, npieces)
    return (xs, SplitAct(out3, plane, B, C, H, W, pad, 3)) if with3 else xs


def _bnb(bwd):
    """bwd = (x, coef, relu, part): backward BN partials from the epilogue (see
    ubpl_conv2d_forward_psa); coef = scale|shift|mean (3*C contiguous floats)."""
    if bwd is None:
        return None, None, 0, None
    x, coef, relu, part = bwd
    return x, coef, int(relu), part


def conv2d_forward_psa(xs, ws, bias, res=None, out=None, stat_part=None, bwd=None):
    """Stride-1 conv of pre-split activations xs (SplitAct) with SplitWeights ws;
    stat_part: BatchNorm partials of the output (bn_partial_buffer); bwd =
    (x, coef, relu, part): the output is dz of a BN with input x — its backward
    statistics partials into part."""
    Cout, T, wc = ws.shape
    KS = int(round(T ** 0.5))
    if wc != xs.C or ws.npieces != xs.npieces:
        raise AssertionError("{} {} / pieces {} {}".format(xs.C, wc, xs.npieces, ws.npieces))
    B, H, W = xs.B, xs.H, xs.W
    y = torch.empty((B, Cout, H, W), device=xs.buf.device, dtype=F32) if out is None else out
    slab = _slab("ubpl_conv2d_forward_psa_workspace", xs.buf.device, B, xs.C, Cout, KS, H, W, ws.npieces, or_none=True)
    _lib.call("ubpl_conv2d_forward_psa", xs.buf, int(xs.plane), B, xs.C, H, W, int(xs.pad), ws.ptr(), int(ws.plane),
              bias, Cout, KS, res, y, slab, int(ws.npieces), stat_part, *_bnb(bwd), xs.scale)
    return y


def stem_s2d_ok(x):
    B, C, H, W = x.shape
    return C <= 4 and H % 2 == 0 and W % 2 == 0 and (B * (H // 2) * (W // 2)) % 256 == 0


def stem_s2d_split(x, pad=2, npieces=3):
    """7x7/s2 stem input as the 16-channel PSA image of its 4 phase images
    (space-to-depth; channels c*4 + 2ph + pw, the rest zero), border `pad`;
    npieces 3 (6xbf16) or 1 (bf16)."""
    B, C, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    plane = B * (Ho + 2 * pad) * (Wo + 2 * pad) * 16
    buf = torch.empty(npieces * plane, device=x.device, dtype=torch.int16)
    _lib.call("ubpl_stem_s2d_split", x, B, C, H, W, int(pad), int(npieces), buf, int(plane))
    return SplitAct(buf, plane, B, 16, Ho, Wo, pad, npieces)


def stem_weight_s2d_split(w, npieces=3, out=None):
    """The stem's 7x7 weights as the split 4x4 weights of its space-to-depth conv
    (out: an earlier result of the same shape, rewritten in place)."""
    Cout, C, KS, _ = w.shape
    plane = Cout * 16 * 16
    if out is not None:
        if (out.plane, out.shape, out.npieces, out.off) != (plane, (Cout, 16, 16), npieces, 0):
            raise ValueError("ubpl_amd: stem split buffer of another shape")
        buf = out.buf
    else:
        buf = torch.empty(npieces * plane, device=w.device, dtype=torch.int16)
    _lib.call("ubpl_stem_weight_s2d_split", w.contiguous(), Cout, C, KS, int(npieces), buf, int(plane))
    return SplitWeights(buf, plane, 0, (Cout, 16, 16), npieces) if out is None else out


_NO_SOL = os.environ.get("UBPL_NO_SOL") == "1"      # diagnostic: every 1x1 on the exact-f32 kernels


# small=True (a model on the 2xfp16 precision): the split-load 1x1 also on grids below the chip's
# CU count, down to this many workgroups — the smaller planes' 1x1 convs were on the exact-f32
# kernel at 1/16 of the bf16 MFMA rate (-1 % step, profiles/r06_v8_sol_small_ab.txt); 0, and the
# other precisions: only grids that fill the chip (ubpl_conv1x1_split_load_preferred)
_SOL_MINWG = int(os.environ.get("UBPL_SOL_MINWG", "32"))


def conv1x1_split_load_ok(x, ws, small=False):
    """The split-on-load 1x1 kernel (6xbf16, 2xfp16 or bf16) takes this shape and fills the chip
    (small: on grids of >= _SOL_MINWG workgroups)."""
    B, Cin, H, W = x.shape
    ok = (not _NO_SOL and ws is not None and ws.npieces in (1, 2, 3) and ws.shape[1] == 1 and ws.shape[2] == Cin
          and x.data_ptr() % 16 == 0)
    if not ok:
        return False
    if small and _SOL_MINWG > 0 and ws.npieces in (2, 3):
        return bool(_lib.lib().ubpl_conv1x1_split_load_preferred_min(B, Cin, ws.shape[0], H * W, _SOL_MINWG))
    return bool(_lib.lib().ubpl_conv1x1_split_load_preferred(B, Cin, ws.shape[0], H * W))


def conv1x1_forward_split_load(x, ws, bias, pscale=None, pshift=None, res=None, out=None, stat_part=None,
                               bwd=None):
    """1x1 stride-1 conv on the split path (ws.npieces 3: 6xbf16; 2: 2xfp16; 1: bf16 operands)
    with x (NCHW f32) split while it is staged: y = conv(relu(x*pscale + pshift) or x, ws) + bias (+ res; res may
    alias out); ws = SplitWeights (rows, 1, Cin) — a forward (mode 0) or a data
    gradient (mode 1, x = dy) table; stat_part: BatchNorm partials of y."""
    B, Cin, H, W = x.shape
    Cout, T, wc = ws.shape
    if T != 1 or wc != Cin or ws.npieces not in (1, 2, 3) or (ws.npieces != 3 and (stat_part is not None or
                                                                               bwd is not None)):
        raise AssertionError("split-load 1x1: weights {} / pieces {} for {} input channels".format(
            ws.shape, ws.npieces, Cin))
    y = torch.empty((B, Cout, H, W), device=x.device, dtype=F32) if out is None else out
    _lib.call("ubpl_conv1x1_forward_split_load", x, B, Cin, H * W, ws.ptr(), int(ws.plane), bias, Cout, pscale, pshift,
              res, y, stat_part, *_bnb(bwd), int(ws.npieces))
    return y


def wgrad3_psa_ok(ys, xs):
    return (ys.npieces in (1, 2, 3) and xs.npieces == ys.npieces and (ys.npieces != 2 or ys.scale is not None) and ys.pad == 1 and xs.pad == 1 and xs.C % 64 == 0
            and ys.C % 64 == 0 and xs.W % 16 == 0 and (ys.B, ys.H, ys.W) == (xs.B, xs.H, xs.W))


def conv2d_wgrad3_psa(ys, xs, dw, db, accumulate=True):
    """3x3 weight (+ bias) gradient from PSA operands: ys = split(dy), xs = split(conv input), pad 1."""
    slab = _slab("ubpl_wgrad3_psa_workspace", xs.buf.device, xs.B, xs.C, ys.C, xs.H, xs.W)
    _lib.call("ubpl_wgrad3_psa", ys.buf, int(ys.plane), xs.buf, int(xs.plane), xs.B, xs.C, ys.C, xs.H, xs.W, slab, dw,
              db, int(accumulate), int(xs.npieces), ys.scale)


def wgrad_stem_psa_ok(ys, xs, w):
    Cout, C, KS = w.shape[0], w.shape[1], w.shape[2]
    return (ys.npieces in (1, 3) and xs.npieces == ys.npieces and ys.pad == 1 and xs.pad == 2 and xs.C == 16 and KS == 7
            and C <= 4 and Cout % 64 == 0 and ys.C == Cout and ys.W % 16 == 0
            and (ys.B, ys.H, ys.W) == (xs.B, xs.H, xs.W))


def conv2d_wgrad_stem_psa(ys, xs, dw, db, accumulate=True):
    """The 7x7/s2 stem's weight (+ bias) gradient from PSA operands: ys = split(dy) (pad 1),
    xs = the forward's space-to-depth phase image (stem_s2d_split, pad 2)."""
    Cout, C, KS = dw.shape[0], dw.shape[1], dw.shape[2]
    slab = _slab("ubpl_wgrad_stem_psa_workspace", ys.buf.device, ys.B, Cout, ys.H, ys.W)
    _lib.call("ubpl_wgrad_stem_psa", ys.buf, int(ys.plane), xs.buf, int(xs.plane), ys.B, C, Cout, ys.H, ys.W, KS, slab,
              dw, db, int(accumulate), int(ys.npieces))


def conv2d_dgrad(dy, w, res=None, out=None, wt=None):
    """dx of a stride-1 conv = conv(dy, flip(w)^T); res/out allow accumulation."""
    if wt is None:
        wt = conv_weight_flip(w)
    return conv2d_forward(dy, None, None, 1, res=res, out=out, w_tap=wt)
