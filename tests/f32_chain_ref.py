"""A CPU statement of what the exact-f32 conv kernels promise (csrc/conv_f32.h, conv_f32_fwd.hip,
conv1x1_dma.hip, conv_f32_wgrad.hip, conv_reduce.hip), shared by the host
tests, the GPU yardstick test and the split / range tests that use those kernels as their bar.

The kernels run v_mfma_f32_32x32x2_f32: one f32 accumulator per output and one fused
multiply-add per K element.  The chain here is that, element for element:

    acc <- float32(float64(acc) + float64(w) * float64(x))

(the product of two f32 values is exact in float64, so this is the fma up to a double rounding
on ~2^-29 of the steps), over K in the order conv_f32.h documents — grouped tap-major,
k = (ci/G)*G*T + tap*G + ci%G with G = 16 when Cin % 16 == 0 and G = Cin otherwise (so the
stem's 3 and the heads' 17 channels run tap-major over the real channels) — from a zero
accumulator; bias, then the residual, are added in f32 afterwards.  The launches differ from
that in two documented ways, and chain_conv builds both: a launch without
split-K seeds the accumulator with float32(bias + res) (seeded=True: every partial sum then
carries the seed, which raises the error of a channel with a large bias up to 2x), and a
split-K launch runs `splits` chains from zero over whole 16-element K tiles and sums them in
split order before bias and residual (splits=n).  Splitting K or permuting the elements of a K
step cannot raise the expected error above one chain's, so the GPU test holds
e_kernel <= 1.5 * e_chain + 2^-24 per channel against the chain in the launch's order; every
exact f32 evaluation in any order obeys gamma_bound elementwise.  On the MI355X the forward,
k-major and data-gradient launches are bit-equal to these chains (recorded, not asserted).

The cap on the yardstick (yardstick_cap)
----------------------------------------
tests/test_gpu_split.py and tests/test_gpu_f16_range.py use the f32 kernels' own relative error
e32 as their bar; yardstick_cap holds it to C * sqrt(K) * 2^-24 (K the reduction length:
Cin*KS*KS for forward and dgrad, B*P for the weight and bias gradients), whole-tensor.  C is twice
the largest ratio e_chain / (sqrt(K) * 2^-24) the chain alone shows on those files' operand
distributions.  tools/f32_chain_table.py recomputes the table on the CPU: at most two images per
case, forward planes clipped to 16x16 (the stem's input to 32x32), K = B*P of the gradients to at
most 8192; the forward both as one chain from zero and seeded with bias + residual, the order of
a launch without split-K:

    distribution (file: cases)                                   K             ratio: from zero   seeded
    randn x, randn w / sqrt(K), randn bias, +- relu prologue,
      +- randn residual (split: CASES, SOL_CASES, 16-channel,
      HALO_CASES forward)                                        16 .. 2304    0.11 .. 0.25   0.25 .. 0.40
    randn dy through the flipped weights (split: every dgrad)    16 .. 2304    0.28 .. 0.31
    randn dy x relu-prologue or randn x (split: wgrad3, wgrad1x1,
      2xfp16 3x3 gradients)                                      128 .. 8192   0.22 .. 0.30
    uniform x - 0.5, randn w, randn bias (split: stem forward)   147           0.08           0.39 .. 0.41
    randn dy x (uniform x - 0.5) (split: stem weight gradient)   8192          0.29 .. 0.30
    sum of randn dy (split: stem bias gradient)                  8192          0.33 .. 0.35
    range file, every FWD_KERNELS shape x act, act_relu, act_top,
      w, w_top, both_top, mixed (and heatmap on sol_cin16)       16 .. 1152    0.14 .. 0.29   0.20 .. 0.37
    range file, 3x3 backward: dz uniform and spread over 2^-20,
      through a BN + ReLU backward; dgrad and wgrad              576 .. 2048   0.26 .. 0.38

    largest 0.41  ->  C = YARDSTICK_C = 0.82

The ratio does not grow with K: the chain's partial sums random-walk, so its error is about
0.3 * sqrt(K) * u on every zero-mean operand distribution in the two files.  (0.08 .. 0.14: the
reference carries a bias and a residual larger than the conv, which the chain from zero adds
once at the end; the seeded chain rounds against them at every step.  A cap only bounds from
above, so those cases keep it.)

Cases the chain model does not fit, which get no cap: none in the two files.  The near-zero
reference channel — the likely misfit — does not occur in them: test_gpu_f16_range.py refuses
more than 1 % zero channels and draws bias and residual at each channel's own magnitude, and the
cap is whole-tensor.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24                 # f32 unit roundoff
YARDSTICK_C = 0.82             # the docstring's table


def _np32(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    assert a.dtype == np.float32, "the chain runs on the f32 values the kernel sees"
    return a


def kgroup(cin):
    """csrc/common.h conv_kgroup."""
    return 16 if cin % 16 == 0 else cin


def k_order(cin, T, order="grouped"):
    """The (ci, tap) pairs of one output's K chain.  grouped: conv_f32.h's grouped tap-major
    order; ci: channel-major (torch's weight layout); rev: grouped, backwards."""
    if order == "ci":
        return [(ci, tap) for ci in range(cin) for tap in range(T)]
    G = kgroup(cin)
    ks = [(g + c, tap) for g in range(0, cin, G) for tap in range(T) for c in range(G)]
    return ks[::-1] if order == "rev" else ks


def prologue(x, sc, sh):
    """relu(float32(float64(x) * float64(sc) + float64(sh))): the kernels' fmaxf(fmaf(x, sc, sh), 0)
    per input channel, as a float32 tensor."""
    x, sc, sh = (torch.as_tensor(_np32(t)) for t in (x, sc, sh))
    v = x.double() * sc.double()[None, :, None, None] + sh.double()[None, :, None, None]
    return F.relu(v.float())


def gamma_bound(absprod, n):
    """n*u / (1 - n*u) * absprod, u = 2^-24: the bound on |computed - exact| of any evaluation
    of a sum of products by n exact f32 operations per output, in any order."""
    nu = n * U
    assert nu < 1
    return nu / (1 - nu) * absprod


def im2col(inp, KS, stride, pad):
    """float64 [B, Cin, KS*KS, Ho*Wo] patches of inp [B, Cin, H, W] (zeros outside)."""
    t = torch.as_tensor(np.asarray(inp, dtype=np.float64))
    B, C = t.shape[:2]
    return F.unfold(t, KS, 1, pad, stride).view(B, C, KS * KS, -1).numpy()


def _fma_chain(acc, tmp, a, b):
    """acc <- float32(float64(acc) + a * b), in place (a, b float64 arrays broadcasting to acc)."""
    np.multiply(a, b, out=tmp)
    tmp += acc
    np.copyto(acc, tmp, casting="same_kind")


def split_kchunk(K, splits):
    """K elements per split-K chain (csrc/conv_f32.h fwd_plan: whole 16-element K tiles, the
    same number in every split but the last)."""
    nkt = (K + 15) // 16
    return 16 * ((nkt + splits - 1) // splits)


def chain_conv(inp, w, bias=None, res=None, stride=1, pad=0, order="grouped", defect=None, seeded=False, splits=1):
    """The f32 fma chain of conv2d(inp, w, stride, pad) + bias + res.  inp [B,Cin,H,W]: the f32
    values the kernel multiplies (after prologue()); w [Cout,Cin,KS,KS], bias [Cout], res
    [B,Cout,Ho,Wo] f32.  Returns a float32 tensor.  defect(k, wk, xk) -> (wk, xk), when given,
    may alter the operands of step k (the host tests' planted defects).  seeded: the
    accumulator starts at float32(bias + res) and nothing is added afterwards — what a kernel
    launch without split-K does (csrc/common.h seed_acc).  splits > 1: what a split-K launch
    does — a chain from zero per split of split_kchunk(K, splits) elements, the partials summed
    in f32 in split order (conv_reduce.hip split_reduce_kernel), then bias, then the residual."""
    inp, w = _np32(inp), _np32(w)
    B, Cin, H, W = inp.shape
    Cout, _, KS, _ = w.shape
    T = KS * KS
    cols = im2col(inp, KS, stride, pad)                    # [B, Cin, T, P]
    P = cols.shape[-1]
    w64 = w.reshape(Cout, Cin, T).astype(np.float64)
    acc = np.zeros((B, Cout, P), np.float32)
    tmp = np.empty((B, Cout, P), np.float64)

    def add_bias_res():
        if bias is not None:
            acc[...] += _np32(bias)[None, :, None]
        if res is not None:
            acc[...] += _np32(res).reshape(B, Cout, P)

    assert not (seeded and splits > 1)
    if seeded:
        add_bias_res()
    kchunk = split_kchunk(Cin * T, splits)
    total = None
    for k, (ci, tap) in enumerate(k_order(Cin, T, order)):
        if splits > 1 and k > 0 and k % kchunk == 0:                # the next split's chain starts from zero
            total = acc.copy() if total is None else total + acc
            acc[...] = 0.0
        wk, xk = w64[None, :, ci, tap, None], cols[:, None, ci, tap, :]
        if defect is not None:
            wk, xk = defect(k, wk, xk)
        _fma_chain(acc, tmp, wk, xk)
    if total is not None:
        acc[...] = total + acc                                      # split_reduce_kernel: f32, in split order
    if not seeded:
        add_bias_res()
    Ho = (H + 2 * pad - KS) // stride + 1
    return torch.from_numpy(acc.reshape(B, Cout, Ho, P // Ho))


def flip_weights(w):
    """wd[ci][co][tap] = w[co][ci][T-1-tap]: the data gradient's weights (stride 1)."""
    return np.ascontiguousarray(np.flip(_np32(w), (2, 3)).transpose(1, 0, 2, 3))


def chain_dgrad(dy, w, pad=0, order="grouped", splits=1):
    """The data gradient of a stride-1 conv: the same chain through the flipped and transposed
    weights, K = Cout*KS*KS grouped over the output channels."""
    return chain_conv(dy, flip_weights(w), None, None, 1, pad, order, splits=splits)


def chain_wgrad(dy, inp, KS, stride, pad, skip_last=False):
    """dw[co,ci,kh,kw] and db[co] as one chain over k = (b, p) per element, from zero.
    dy [B,Cout,Ho,Wo], inp [B,Cin,H,W] f32 (after prologue()).  Returns float32 tensors.
    skip_last leaves the last pixel of the last image out (a planted defect)."""
    dy, inp = _np32(dy), _np32(inp)
    B, Cout = dy.shape[:2]
    Cin, T = inp.shape[1], KS * KS
    cols = im2col(inp, KS, stride, pad).reshape(B, Cin * T, -1)          # [B, Cin*T, P]
    P = cols.shape[-1]
    d64 = dy.reshape(B, Cout, P).astype(np.float64)
    acc = np.zeros((Cout, Cin * T), np.float32)
    tmp = np.empty((Cout, Cin * T), np.float64)
    db = np.zeros(Cout, np.float32)
    for b in range(B):
        ct, dt = np.ascontiguousarray(cols[b].T), np.ascontiguousarray(d64[b].T)
        for p in range(P - 1 if skip_last and b == B - 1 else P):
            _fma_chain(acc, tmp, dt[p][:, None], ct[p][None, :])
            db = (db.astype(np.float64) + dt[p]).astype(np.float32)
    return torch.from_numpy(acc.reshape(Cout, Cin, KS, KS)), torch.from_numpy(db)


def rel(a, ref):
    """||a - ref|| / ||ref|| over the whole tensor, in float64."""
    a, ref = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(ref).double()
    return float((a - ref).norm() / ref.norm())


def channel_errors(a, ref, cdim):
    """(||a_c - ref_c||, ||ref_c||) per channel along cdim, float64."""
    a, ref = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(ref).double()
    dims = tuple(i for i in range(ref.dim()) if i != cdim)
    return (a - ref).pow(2).sum(dims).sqrt(), ref.pow(2).sum(dims).sqrt()


def yardstick_ratio(e32, K):
    """e32 / (sqrt(K) * 2^-24)."""
    return e32 / (np.sqrt(K) * U)


def record(line):
    """Print a result line; with UBPL_YARDSTICK_LOG=<file> set, append it there too (how
    profiles/f32_yardstick_gpu_tests.txt is made from a run of the GPU tests)."""
    print(line)
    path = os.environ.get("UBPL_YARDSTICK_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def yardstick_cap(tag, e32, K):
    """The cap on an exact-f32 kernel's whole-tensor relative error e32 where a test uses it as
    a bar: e32 <= YARDSTICK_C * sqrt(K) * 2^-24 (the docstring's table).  Records the ratio with
    C beside it; returns e32."""
    r = yardstick_ratio(e32, K)
    record("cap   %-62s K %6d  e32 %.2e  e32/(sqrt(K) 2^-24) %.3f  C %.2f" % (tag, K, e32, r, YARDSTICK_C))
    assert np.isfinite(e32) and r <= YARDSTICK_C, \
        "%s: the exact-f32 yardstick is off its chain: e32 %.3e = %.3f sqrt(K) u > %.2f (K = %d)" % (
            tag, e32, r, YARDSTICK_C, K)
    return e32


CHAIN_BAR = 1.5                # e_kernel <= CHAIN_BAR * e_chain + U per channel (the module docstring)


def bars(y, true, chain, absref, n, cdim):
    """The yardstick's bars on a result y (f32) against the float64 truth, the chain reference and
    absref = conv(|inp|, |w|) + |bias| + |res| (float64), n f32 operations per output:
      a        worst |y - true| / gamma_bound(absref, n) over the elements (<= 1 passes; an element
               with absref == 0 must be exact), a_index its index
      b        worst e_k / (CHAIN_BAR * e_ch + U) over the channels along cdim whose truth is not
               exactly zero, e the channel's relative L2 error (<= 1 passes), b_channel its index,
               e_k / e_ch there as b_raw
      finite   nothing non-finite
      zero_ok  every channel whose truth is exactly zero is exactly zero"""
    y = torch.as_tensor(y).detach().cpu().double()
    true, absref = torch.as_tensor(true).double(), torch.as_tensor(absref).double()
    out = {"finite": bool(torch.isfinite(y).all())}
    bound = gamma_bound(absref, n)
    err = (y - true).abs()
    ra = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, np.inf), err))
    ra = torch.nan_to_num(ra, nan=np.inf)
    i = int(ra.argmax())
    out["a"], out["a_index"] = float(ra.reshape(-1)[i]), tuple(int(v) for v in np.unravel_index(i, tuple(ra.shape)))
    nk, d = channel_errors(y, true, cdim)
    nc, _ = channel_errors(chain, true, cdim)
    zero = d == 0
    out["zero_ok"] = bool((y.movedim(cdim, 0)[zero] == 0).all())
    out["zero_channels"] = int(zero.sum())
    nz = ~zero
    ek, ech = nk[nz] / d[nz], nc[nz] / d[nz]
    rb = torch.nan_to_num(ek / (CHAIN_BAR * ech + U), nan=np.inf)
    c = int(rb.argmax())
    out["b"], out["b_channel"] = float(rb[c]), int(torch.nonzero(nz).reshape(-1)[c])
    out["b_raw"] = float(ek[c] / ech[c]) if float(ech[c]) > 0 else float("inf")
    out["e_k"], out["e_ch"] = float(ek[c]), float(ech[c])
    return out


def assert_bars(tag, r):
    """Record and assert the bars() of one case."""
    record("bars  %-62s chain: worst e_k/(1.5 e_ch + u) %.3f (ch %d: e_k %.2e e_ch %.2e, e_k/e_ch %.2f) | "
           "elementwise: worst/gamma %.4f at %s | zero channels %d" % (
               tag, r["b"], r["b_channel"], r["e_k"], r["e_ch"], r["b_raw"], r["a"], r["a_index"], r["zero_channels"]))
    assert r["finite"], tag + ": non-finite output"
    assert r["zero_ok"], tag + ": a channel whose truth is exactly zero is not exactly zero"
    assert r["a"] <= 1.0, "%s: element %s is %.3f x gamma_bound from the truth" % (tag, r["a_index"], r["a"])
    assert r["b"] <= 1.0, "%s: channel %d: e_k %.3e > 1.5 * e_chain %.3e + 2^-24 (e_k/e_ch %.2f)" % (
        tag, r["b_channel"], r["e_k"], r["e_ch"], r["b_raw"])
