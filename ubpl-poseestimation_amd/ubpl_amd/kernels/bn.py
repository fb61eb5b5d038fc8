"""BatchNorm kernels: statistics, coefficients, apply, backward — and the max-pool / upsample
passes folded into their BatchNorm neighbours."""
import torch

from .. import _lib
from . import _check
from ._check import F32, _bn_tuple, _plane, _same_shape
from .split_operands import SplitAct


def bn_part(B, C, device):
    """Zeroed BN scratch (partial sums + self-resetting arrival counters)."""
    return torch.zeros(int(_lib.lib().ubpl_bn_part_doubles(B, C)), dtype=torch.float64, device=device)


def bn_forward_stats(x, gamma, beta, eps, momentum, rmean, rvar, part, mean, invstd, scale, shift):
    B, C, HW = _plane(x)
    _lib.call("ubpl_bn_forward_stats", x, B, C, HW, gamma, beta, float(eps), float(momentum), rmean, rvar, part, mean,
              invstd, scale, shift)


def bn_eval_coeffs(gamma, beta, rmean, rvar, eps, scale, shift):
    _lib.call("ubpl_bn_eval_coeffs", gamma, beta, rmean, rvar, float(eps), gamma.numel(), scale, shift)


def bn_coeff_table(rows, n_params, n_stats, n_coef):
    """Host int64 [nbn,6] table of ubpl_bn_eval_coeffs_table from rows (gamma_off,
    beta_off, rmean_off, rvar_off, coef_off, C), every offset checked against the
    buffers' sizes (the kernel trusts the table)."""
    t = torch.tensor(rows, dtype=torch.int64).reshape(-1, 6)
    for g, b, rm, rv, co, c in t.tolist():
        if c < 1 or min(g, b, rm, rv, co) < 0 or max(g, b) + c > n_params or max(rm, rv) + c > n_stats \
                or co + 2 * c > n_coef:
            raise ValueError("ubpl_amd: BatchNorm table row %r reaches outside params[%d] / stats[%d] / coef[%d]"
                             % ((g, b, rm, rv, co, c), n_params, n_stats, n_coef))
    return t


def bn_eval_coeffs_table(params, stats, table, eps, coef):
    """scale | shift of every BatchNorm of `table` (bn_coeff_table(...).to(device)) in one launch."""
    _lib.call("ubpl_bn_eval_coeffs_table", params, stats, table, int(table.shape[0]), float(eps), coef)


def bn_apply(x, scale, shift, relu, out=None):
    B, C, HW = _plane(x)
    y = torch.empty_like(x) if out is None else out
    _lib.call("ubpl_bn_apply", x, B, C, HW, scale, shift, int(relu), y)
    return y


def bn_partial_buffer(C, N, device):
    return torch.empty(int(_lib.lib().ubpl_bn_partial_floats(C, N)), device=device, dtype=F32)


def bn_partials(y, part):
    B, C, HW = _plane(y)
    _lib.call("ubpl_bn_partials", y, B, C, HW, part)
    return part


def bn_stats_from_partials(part, C, N, gamma, beta, eps, momentum, rmean, rvar, mean, invstd, scale, shift_out):
    _lib.call("ubpl_bn_stats_from_partials", part, C, int(N), gamma, beta, float(eps), float(momentum), rmean, rvar,
              mean, invstd, scale, shift_out)


def bn_backward_split(dz, x, gamma, mean, invstd, scale, shift, relu, scratch, coef, dgamma, dbeta, npieces, pad,
                      part=None):
    """bn_backward with dx delivered as a SplitAct (PSA planes) only.  npieces 2
    (2xfp16): the pieces of dx times the power of two its bound asks for, kept on
    the device at coef[3C] — the SplitAct's `scale`, read by its consumers (so coef
    must not be reused before they are enqueued: stream order)."""
    B, C, H, W = x.shape
    plane = B * C * (H + 2 * pad) * (W + 2 * pad)
    out = torch.empty(npieces * plane, device=x.device, dtype=torch.int16)
    _lib.call("ubpl_bn_backward_split", dz, x, B, C, H, W, gamma, mean, invstd, scale, shift, int(relu), scratch, part,
              coef, dgamma, dbeta, int(pad), int(npieces), out, int(plane))
    return SplitAct(out, plane, B, C, H, W, pad, npieces, coef[3 * C:3 * C + 1] if npieces == 2 else None)


def bn_backward(dz, x, gamma, mean, invstd, scale, shift, relu, scratch, coef, dgamma, dbeta, add1=None, add2=None,
                out=None, part=None):
    """BatchNorm(+ReLU) backward.  scratch: bn_part(B, C) (zeroed double
    scratch of the one-launch statistics); part: the backward partials dz's
    producer wrote (bn_bwd_partials layout) — then only the finalize runs."""
    B, C, HW = _plane(x)
    dx = dz if out is None else out
    _lib.call("ubpl_bn_backward", dz, x, B, C, HW, gamma, mean, invstd, scale, shift, int(relu), scratch, part, coef,
              dgamma, dbeta, add1, add2, dx)
    return dx


def bn_bwd_partials(dz, x, scale, shift, mean, relu):
    """Backward statistics partials (S1, S2) per (channel, 64-pixel slice)."""
    B, C, HW = _plane(x)
    part = bn_partial_buffer(C, B * HW, x.device)
    _lib.call("ubpl_bn_backward_partials", dz, x, B, C, HW, scale, shift, mean, int(relu), part)
    return part


# ------------------------------------------------------------------ pool / upsample folded into BatchNorm
def pool_fuse_ok(H, W, C=1, *tensors):
    """Planes the fused resampling + BatchNorm kernels take (bn.h pool_geom): H and W
    even, W/4 a power of two <= 32 (the 2x2 windows' other row sits in lane ^ (W/4) of the
    same wave), H a power of two (planes divide, or are a power-of-two multiple of, a
    256-thread block's float4s), C <= 512 (the statistics scratch's tickets) and every
    tensor given 16-byte aligned."""
    if H < 2 or W < 4 or H & (H - 1) or W & 3:
        return False
    w4 = W >> 2
    if w4 & (w4 - 1) or w4 > 32 or not 1 <= C <= 512:
        return False
    return all(t is None or t.data_ptr() % 16 == 0 for t in tensors)


def _fuse_geometry(name, x):
    if x.dim() != 4:
        raise ValueError("ubpl_amd: %s takes a [B,C,H,W] tensor, got shape %s" % (name, tuple(x.shape)))
    B, C, H, W = x.shape
    if B < 1 or not pool_fuse_ok(H, W, C):
        raise ValueError("ubpl_amd: %s does not take planes of %dx%d with %d channels (pool_fuse_ok)" % (name, H, W, C))
    return B, C, H, W


def bn_forward_stats_maxpool(x, xbn, pbn, eps, momentum, part, out=None):
    """One launch: bn_forward_stats(x) for the BatchNorm xbn (None: x has none),
    y = maxpool2x2(x), and the statistics of y for the BatchNorm pbn (None: not taken; a new
    summation order, unlike everything else here).  xbn / pbn:
    (gamma, beta, rmean, rvar, mean, invstd, scale, shift), rmean / rvar nullable."""
    B, C, H, W = _fuse_geometry("bn_forward_stats_maxpool", x)
    for nm, bn in (("xbn", xbn), ("pbn", pbn)):
        if bn is not None:
            _bn_tuple(nm, bn, C)
    _same_shape("out", out, (B, C, H // 2, W // 2))
    _check._chk(x, "x")
    y = torch.empty((B, C, H // 2, W // 2), device=x.device, dtype=F32) if out is None else out
    _lib.call("ubpl_bn_forward_stats_maxpool", x, B, C, H, W, y, *(xbn if xbn is not None else (None,) * 8),
              *(pbn if pbn is not None else (None,) * 8), float(eps), float(momentum), part)
    return y


def upsample2x_add_bnstats(up, low, bn, eps, momentum, part, out=None):
    """One launch: out = upsample2x_add(up, low) (out=up: in place) and bn_forward_stats(out)
    for the BatchNorm bn = (gamma, beta, rmean, rvar, mean, invstd, scale, shift)."""
    B, C, H, W = _fuse_geometry("upsample2x_add_bnstats", up)
    _same_shape("low", low, (B, C, H // 2, W // 2))
    _same_shape("out", out, up.shape)
    _bn_tuple("bn", bn, C)
    _check._chk(up, "up")
    _check._chk(low, "low")
    y = torch.empty_like(up) if out is None else out
    gamma, beta, rmean, rvar, mean, invstd, scale, shift = bn
    _lib.call("ubpl_upsample2x_add_forward_bnstats", up, low, B, C, H, W, y, gamma, beta, float(eps), float(momentum),
              rmean, rvar, part, mean, invstd, scale, shift)
    return y


def bn_backward_pool(dz, x, gamma, mean, invstd, scale, shift, relu, scratch, coef, dgamma, dbeta, add1=None,
                     pool_dy=None, add2=None, out=None, part=None):
    """bn_backward with the gradient of maxpool2x2(x) folded into the apply:
    dx = ((dL/dx + add1) + maxpool2x2_backward(x, pool_dy)) + add2, bit-identical to
    bn_backward(add1), maxpool2x2_backward(accumulate=True) and add in turn."""
    if pool_dy is None:
        return bn_backward(dz, x, gamma, mean, invstd, scale, shift, relu, scratch, coef, dgamma, dbeta, add1=add1,
                           add2=add2, out=out, part=part)
    B, C, H, W = _fuse_geometry("bn_backward_pool", x)
    for nm, t in (("dz", dz), ("add1", add1), ("add2", add2), ("out", out)):
        _same_shape(nm, t, x.shape)
    _same_shape("pool_dy", pool_dy, (B, C, H // 2, W // 2))
    _check._chk(x, "x")
    _check._chk(dz, "dz")
    _check._chk(pool_dy, "pool_dy")
    dx = dz if out is None else out
    _lib.call("ubpl_bn_backward_pool", dz, x, B, C, H, W, gamma, mean, invstd, scale, shift, int(relu), scratch, part,
              coef, dgamma, dbeta, add1, pool_dy, add2, dx)
    return dx
