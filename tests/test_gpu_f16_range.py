"""The 2xfp16 conv kernels across their documented operand range, per output channel.

tests/test_gpu_split.py draws O(1) operands and weighs the whole output tensor at once; here
the operands go from the top of the range (|activation| = 2047, |w| = 65504 / fp16_wscale(K))
down to 2^-18 and 1e-6 of the init bound, where the lo pieces are fp16 subnormals, and every
output channel (input channel for the data gradient, output channel of dw for the weight
gradient) is held to the bar on its own.

The oracle is tests/f16_split_ref.py: the float64 conv of the operands as the fp16 pieces
carry them.  The kernel and the oracle differ by the kernel's f32 accumulation only, so

    ||y_c - oracle_c|| / ||oracle_c|| <= F16_BAR * e32_c + 2^-22

with e32_c the exact-f32 kernel's error against the true float64 conv on the same inputs (the
yardstick of test_gpu_split.py; 2^-22, one fp16-pair ulp, for channels where the f32 kernel
happens to be exact) — the bar does not loosen with magnitude.  A kernel that flushes
subnormal pieces misses it by more than 100x at activation magnitude 2^-10
(test_f16_split_host.py::test_conv_error_table_k1152).  The error against the true float64
conv follows (at most the oracle's own plus the bar) and is printed: the number users see.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import f16_split_ref as R
from f32_chain_ref import yardstick_cap

pytestmark = pytest.mark.gpu
DEV = "cuda"
F16_BAR = 4.0                # tests/test_gpu_split.py F16_BAR
PAIR_ULP = 2.0 ** -22


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ubpl_amd import _lib
    _lib.load()


@pytest.fixture()
def _lib_dispatch():
    """The C library for the halo-dispatch hook; the process's own dispatch is restored after."""
    from ubpl_amd import _lib
    lib = _lib.lib()
    yield lib
    assert lib.ubpl_set_psa_dispatch(-2, -2) == 0


def _d(t):
    return None if t is None else t.to(DEV)


def _norms(a, ref, cdim):
    dims = tuple(i for i in range(ref.dim()) if i != cdim)
    return (a - ref).pow(2).sum(dims).sqrt(), ref.pow(2).sum(dims).sqrt()


def _check(tag, y, y32, oracle, true, K, cdim=1):
    """Every channel along cdim of the kernel's y: against the oracle within the bar, against
    the true float64 result within the oracle's own error plus the bar, nothing non-finite; a
    channel whose float64 reference is exactly zero must be exactly zero (at most 1 % of
    them).  The yardstick y32 itself is capped first: its whole-tensor error within
    f32_chain_ref.yardstick_cap of a K-long f32 chain's.  Prints the worst ratios; returns the
    worst one against the bar."""
    y, y32 = y.detach().cpu().double(), y32.detach().cpu().double()
    yardstick_cap("range " + tag, float((y32 - true).norm() / true.norm()), K)
    assert torch.isfinite(true).all() and torch.isfinite(oracle).all(), tag + ": reference left the range"
    assert torch.isfinite(y).all(), tag + ": non-finite output inside the documented range"
    n_o, d_o = _norms(y, oracle, cdim)
    n_t, d_t = _norms(y, true, cdim)
    n_32, _ = _norms(y32, true, cdim)
    n_ot, _ = _norms(oracle, true, cdim)
    zero = d_t == 0
    assert int(zero.sum()) <= 0.01 * zero.numel(), (tag, int(zero.sum()))
    if zero.any():
        assert bool((y.movedim(cdim, 0)[zero] == 0).all()), tag
    nz = ~zero
    assert bool((d_o[nz] > 0).all()), tag
    e32, ek = n_32[nz] / d_t[nz], n_o[nz] / d_o[nz]
    et, eo = n_t[nz] / d_t[nz], n_ot[nz] / d_t[nz]
    bar = F16_BAR * e32 + PAIR_ULP
    r, rt = ek / bar, et / (eo + bar)
    c = int(r.argmax())
    print("%-46s worst/bar %.3f (ch %d of %d: kernel-oracle %.2e, f32 %.2e) | vs f64: kernel %.2e oracle %.2e "
          "worst/(oracle+bar) %.3f" % (tag, float(r.max()), c, int(nz.sum()), float(ek[c]), float(e32[c]),
                                       float(et.max()), float(eo.max()), float(rt.max())))
    assert float(r.max()) <= 1.0, (tag, c, float(ek[c]), float(e32[c]))
    assert float(rt.max()) <= 1.0, (tag, float(rt.max()))
    return float(r.max())


def _image(buf, plane, B, C, H, W, pad):
    """The two fp16 planes of a PSA image [B][C/16][H+2pad][W+2pad][16] as float64 (hi, lo)
    arrays [B,C,H+2pad,W+2pad]."""
    p = buf.view(2, plane).cpu()
    f = lambda q: (q.view(torch.float16).double().view(B, C // 16, H + 2 * pad, W + 2 * pad, 16)
                   .permute(0, 1, 4, 2, 3).reshape(B, C, H + 2 * pad, W + 2 * pad).numpy())
    return f(p[0]), f(p[1])


def _assert_image_is_pieces(tag, xs, v, scale):
    """The packing pass against the representation, bit for bit: the planes hold
    pieces(v, scale) inside and zeros on the border."""
    hi, lo = _image(xs.buf, xs.plane, xs.B, xs.C, xs.H, xs.W, xs.pad)
    rh, rl = R.pieces(F.pad(v, (xs.pad,) * 4).numpy(), scale)
    assert np.array_equal(hi, rh) and np.array_equal(lo, rl), tag


# ------------------------------------------------------------------ forward
# name, (B, Cin, H, Cout), KS, entry: each kernel at its smallest shape that reaches the path
FWD_KERNELS = [
    ("psa3x3", (2, 128, 16, 128), 3, "psa"),              # conv_psa_kernel, per-tap
    ("psa3x3_splitk", (4, 128, 8, 128), 3, "psa"),        # split-K slab + reduce
    ("sol_cin64", (3, 64, 32, 64), 1, "sol"),             # conv1x1_sol_kernel, split on load
    ("sol_cin256", (2, 256, 16, 128), 1, "sol"),
    ("sol_cout16", (4, 256, 32, 16), 1, "sol"),           # the 16-channel variants
    ("sol_cin16", (2, 16, 32, 256), 1, "sol"),
    ("psa1x1", (2, 256, 16, 128), 1, "psa"),              # the 1x1 through conv2d_forward_psa
]
FWD_CONDS = ([("act", e) for e in (-4, -10, -14, -18)] + [("act_relu", e) for e in (-4, -10, -14, -18)] +
             [("act_top", 0)] + [("w", f) for f in (1e-2, 1e-4, 1e-6)] + [("w_top", 0), ("both_top", 0), ("mixed", 0)])
FWD_CASES = [(k, c) for k in FWD_KERNELS for c in FWD_CONDS] + [(FWD_KERNELS[5], ("heatmap", 0))]


def _top_acts(u):
    """Uniform in [-2040, 2040] with +-2047 planted in the first and last pixel of the first
    and last channel group."""
    x = u * 2040.0
    C = x.shape[1]
    x[0, 0, 0, 0], x[0, 15, 0, 0] = 2047.0, -2047.0
    x[-1, C - 16, -1, -1], x[-1, C - 1, -1, -1] = 2047.0, -2047.0
    return x


def _top_weights(u, K):
    """Uniform within +-65504 / fp16_wscale(K), the limit itself planted at both ends."""
    w = u * R.weight_limit(K)
    w[0, 0, 0, 0], w[-1, -1, -1, -1] = R.weight_limit(K), -R.weight_limit(K)
    return w


def _forward_operands(shape, KS, cond, seed, ref_images=None):
    """The f32 operands of one case (bounded by construction: uniform draws times the
    magnitude, so nothing leaves the range) and the two float64 references (over the images
    ref_images only, when given).  Bias and residual are drawn at each output channel's own
    magnitude, or absent (post-ReLU cases)."""
    B, Cin, H, Cout = shape
    K, pad = Cin * KS * KS, (KS - 1) // 2
    gen = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64) * 2 - 1
    x, w = u(B, Cin, H, H), u(Cout, Cin, KS, KS) / np.sqrt(K)        # w at the default-init bound
    ps = ph = None
    kind, p = cond
    affine = kind != "act_relu"
    if kind == "act":
        x = x * 2.0 ** p
    elif kind == "act_relu":
        x = F.relu(x) * 2.0 ** p                                      # about half exact zeros
    elif kind in ("act_top", "both_top"):
        x = _top_acts(x)
    if kind == "w":
        w = w * p
    elif kind in ("w_top", "both_top"):
        w = _top_weights(u(Cout, Cin, KS, KS), K)
    if kind == "mixed":
        # exact prologue coefficients: relu(x * 2^k) with k per input channel, |.| <= 1024;
        # weights scaled per output channel by 2^-10 .. 1
        x = x * 4.0
        ps = 2.0 ** torch.randint(-12, 9, (Cin,), generator=gen).double()
        ph = torch.zeros(Cin, dtype=torch.float64)
        w = w * (2.0 ** torch.randint(-10, 1, (Cout,), generator=gen).double())[:, None, None, None]
    if kind == "heatmap":
        from oracle import render as OR
        kps = np.ones((B, Cin, 3), np.float32)
        kps[..., :2] = torch.randint(0, 4 * H, (B, Cin, 2), generator=gen).numpy()
        hm, _ = OR.render_batch(kps, (4 * H, 4 * H), 4 * H, H)
        x = torch.from_numpy(hm).double() + 1e-4 * x
    x32, w32 = x.float(), w.float()
    ps32, ph32 = (ps.float(), ph.float()) if ps is not None else (None, None)
    inp = F.relu(x32.double() * ps32.double()[None, :, None, None]) if ps is not None else x32.double()
    sl = list(range(B)) if ref_images is None else ref_images
    true = F.conv2d(inp[sl], w32.double(), None, 1, pad)
    b32 = res32 = None
    if affine:
        mag = true.pow(2).mean((0, 2, 3)).sqrt()
        b32, res32 = (u(Cout) * mag).float(), (u(B, Cout, H, H) * mag[None, :, None, None]).float()
        true = true + b32.double()[None, :, None, None] + res32[sl].double()
    oracle = R.conv_2xfp16(inp[sl], w32, b32, None if res32 is None else res32[sl], pad)
    return x32, w32, b32, res32, ps32, ph32, inp, true, oracle


def _cond_id(cond):
    kind, p = cond
    return kind + ("" if p == 0 else ("2^%d" % p if isinstance(p, int) else "%.0e" % p))


def _case_id(case):
    return "%s-%s" % (case[0][0], _cond_id(case[1]))


@pytest.mark.parametrize("case", FWD_CASES, ids=_case_id)
def test_2xfp16_forward_vs_oracle_per_channel(case):
    from ubpl_amd import _lib, kernels as Kn
    (name, shape, KS, entry), cond = case
    B, Cin, H, Cout = shape
    seed = 1000 + 37 * FWD_CASES.index(case)
    x32, w32, b32, res32, ps32, ph32, inp, true, oracle = _forward_operands(shape, KS, cond, seed)
    y32 = Kn.conv2d_forward(_d(x32), _d(w32), _d(b32), 1, _d(ps32), _d(ph32), res=_d(res32))
    ws = Kn.conv_weight_split(_d(w32), 0, 2)
    if entry == "psa":
        slab = int(_lib.lib().ubpl_conv2d_forward_psa_workspace(B, Cin, Cout, KS, H, H, 2))
        if name == "psa3x3_splitk":
            assert slab > 0, "the plan no longer splits K at this shape"
        xs = Kn.split_activation(_d(x32), 2, (KS - 1) // 2, _d(ps32), _d(ph32))
        _assert_image_is_pieces(_case_id(case), xs, inp, R.ACT_SCALE)
        y = Kn.conv2d_forward_psa(xs, ws, _d(b32), res=_d(res32))
    else:
        y = Kn.conv1x1_forward_split_load(_d(x32), ws, _d(b32), _d(ps32), _d(ph32), res=_d(res32))
    torch.cuda.synchronize()
    _check("fwd " + _case_id(case), y, y32, oracle, true, Cin * KS * KS)


@pytest.mark.parametrize("mode", [0, 1])
def test_2xfp16_weight_planes_are_the_pieces(mode):
    """The weight split (forward and data-gradient layouts) against the representation, bit
    for bit, from the top of the weight range down to 1e-6 of the init bound, per-channel
    powers of two included."""
    from ubpl_amd import kernels as Kn
    Cout, Cin, T = 32, 48, 9
    gen = torch.Generator().manual_seed(77 + mode)
    K = (Cin if mode == 0 else Cout) * T
    u = torch.rand(Cout, Cin, 3, 3, generator=gen, dtype=torch.float64) * 2 - 1
    spread = (2.0 ** torch.randint(-10, 1, (Cout,), generator=gen).double())[:, None, None, None]
    for tag, w in [("top", _top_weights(u.clone(), K))] + \
                  [("%.0e" % f, u * f / np.sqrt(K)) for f in (1.0, 1e-2, 1e-4, 1e-6)] + \
                  [("spread", u * spread / np.sqrt(K))]:
        w32 = w.float()
        ws = Kn.conv_weight_split(_d(w32), mode, 2)
        p = ws.buf.view(2, ws.plane)[:, :w32.numel()].cpu()
        hi, lo = (p[i].view(torch.float16).double().numpy() for i in (0, 1))
        if mode == 0:      # wt[co][ci/16][tap][ci%16] = w[co][ci][tap]
            ref = w32.reshape(Cout, Cin // 16, 16, T).permute(0, 1, 3, 2)
        else:              # wd[ci][co/16][tap][co%16] = w[co][ci][T-1-tap]
            ref = w32.flip((2, 3)).reshape(Cout // 16, 16, Cin, T).permute(2, 0, 3, 1)
        rh, rl = R.pieces(ref.reshape(-1).double().numpy(), R.fp16_wscale(K))
        assert np.isfinite(rh).all() and np.isfinite(rl).all()
        assert np.array_equal(hi, rh) and np.array_equal(lo, rl), (mode, tag)


# ------------------------------------------------------------------ the halo kernel
@pytest.mark.parametrize("cond", [("act", -18), ("act_top", 0)], ids=["act2^-18", "act_top"])
def test_2xfp16_halo_kernel_at_the_extremes(cond, _lib_dispatch):
    """conv_psah_kernel at the smallest HALO_CASES shape, at the two extreme activation
    magnitudes: bit for bit the per-tap kernel (forced through ubpl_set_psa_dispatch, both halo
    variants required), and the first / last image within the per-channel bar of the oracle."""
    from ubpl_amd import kernels as Kn
    lib = _lib_dispatch
    shape = (32, 128, 32, 128)
    sl = [0, shape[0] - 1]
    x32, w32, b32, res32, _, _, inp, true, oracle = _forward_operands(shape, 3, cond, 4242, ref_images=sl)
    xs = Kn.split_activation(_d(x32), 2, 1)
    ws = Kn.conv_weight_split(_d(w32), 0, 2)
    outs = {}
    for flag in (0, 2, 3):      # 0: conv_psa_kernel; 2: double-buffered halo; 3: one halo buffer (the default's)
        assert lib.ubpl_set_psa_dispatch(flag, 1) == 0
        outs[flag] = Kn.conv2d_forward_psa(xs, ws, _d(b32), res=_d(res32))
        torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[0], outs[3])
    y32 = Kn.conv2d_forward(_d(x32[sl].contiguous()), _d(w32), _d(b32), 1, res=_d(res32[sl].contiguous()))
    _check("halo %s %s" % (shape, _cond_id(cond)), outs[3][sl], y32, oracle, true, shape[1] * 9)


# ------------------------------------------------------------------ the 3x3 backward
def _spread(C):
    """Per-channel powers of two from 2^0 down to 2^-20 across the channels."""
    return 2.0 ** -torch.round(torch.arange(C, dtype=torch.float64) * 20.0 / (C - 1))


@pytest.mark.parametrize("mag", [1.0, 1e-5, 1e-10, "spread"], ids=lambda m: "dz_%s" % m)
def test_2xfp16_3x3_backward_vs_oracle_per_channel(mag):
    """dy through bn_backward_split (2 pieces, the scale chosen on the device and read back
    from ys.scale): the packed image is pieces(dy, scale) bit for bit; the data gradient on
    the mode-1 weights per input channel and the weight gradient per output channel of dw
    within the bar of the oracle, dz from O(1) to 1e-10 and spread over 2^-20 across the
    output channels; the bias gradient to f32 summation error."""
    from ubpl_amd import _lib, kernels as Kn
    B, Cin, Cout, H, W = 2, 64, 64, 32, 32
    gen = torch.Generator().manual_seed(613)
    u = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64) * 2 - 1
    x = u(B, Cin, H, W).float()
    w = (u(Cout, Cin, 3, 3) / np.sqrt(Cin * 9)).float()
    sc, sh = (torch.rand(Cin, generator=gen) + 0.5), u(Cin).float() * 0.5
    dz = u(B, Cout, H, W) * (_spread(Cout)[None, :, None, None] if mag == "spread" else mag)
    dz = dz.float()
    # the BN whose backward makes dy: |xb * bsc| reaches 1 and |bsh| < 0.73 in every channel, so
    # the ReLU mask passes part of every channel and none of dy's channels is exactly zero
    xb = (u(B, Cout, H, W) * 4.0).float()
    gamma = torch.rand(Cout, generator=gen) + 0.5
    mean, istd = u(Cout).float() * 0.1, torch.rand(Cout, generator=gen) + 0.5
    bsc, bsh = gamma * istd, u(Cout).float() * 0.5 - mean * gamma * istd
    part = torch.zeros(int(_lib.lib().ubpl_bn_part_doubles(B, Cout)), dtype=torch.float64, device=DEV)
    coef = torch.empty(3 * Cout + 1, device=DEV)
    dg, db_ = torch.zeros(Cout, device=DEV), torch.zeros(Cout, device=DEV)
    dy = Kn.bn_backward(_d(dz), _d(xb), _d(gamma), _d(mean), _d(istd), _d(bsc), _d(bsh), 1, part, coef, dg, db_,
                        out=torch.empty(B, Cout, H, W, device=DEV))
    ys = Kn.bn_backward_split(_d(dz), _d(xb), _d(gamma), _d(mean), _d(istd), _d(bsc), _d(bsh), 1, part, coef, None,
                              None, 2, 1)
    torch.cuda.synchronize()
    s = float(ys.scale.item())
    assert np.frexp(s)[0] == 0.5, s                                    # a power of two
    dy64 = dy.double().cpu()
    amax = float(dy64.abs().max())
    assert 2.0 ** 8 <= amax * s <= 2.0 ** 14, (amax, s)                # as test_bn_backward_split_2xfp16_scale
    tag = "dz %s (scale 2^%d)" % (mag, int(np.log2(s)))
    _assert_image_is_pieces(tag, ys, dy64, s)
    # data gradient, per input channel
    dx_true = torch.nn.grad.conv2d_input((B, Cin, H, W), w.double(), dy64, 1, 1)
    dx = Kn.conv2d_forward_psa(ys, Kn.conv_weight_split(_d(w), 1, 2), None)
    dx32 = Kn.conv2d_dgrad(dy, _d(w))
    _check("dgrad " + tag, dx, dx32, R.dgrad_2xfp16(dy64, w, s, 1), dx_true, Cout * 9)
    # weight gradient against the forward's 2xfp16 image, per output channel of dw
    inp = F.relu((x.double() * sc.double()[None, :, None, None] + sh.double()[None, :, None, None]).float()).double()
    dw_true = torch.nn.grad.conv2d_weight(inp, (Cout, Cin, 3, 3), dy64, 1, 1)
    xs = Kn.split_activation(_d(x), 2, 1, _d(sc), _d(sh))
    _assert_image_is_pieces(tag + " x", xs, inp, R.ACT_SCALE)
    assert Kn.wgrad3_psa_ok(ys, xs)
    dw, dbw = torch.zeros(Cout, Cin, 3, 3, device=DEV), torch.zeros(Cout, device=DEV)
    Kn.conv2d_wgrad3_psa(ys, xs, dw, dbw, accumulate=False)
    dw32, db32 = torch.zeros(Cout, Cin, 3, 3, device=DEV), torch.zeros(Cout, device=DEV)
    Kn.conv2d_wgrad(dy, _d(x), 3, 1, dw32, db32, _d(sc), _d(sh), accumulate=False)
    dw_or, db_or = R.wgrad3_2xfp16(dy64, inp, s)
    _check("wgrad " + tag, dw, dw32, dw_or, dw_true, B * H * W, cdim=0)
    # bias gradient: an f32 sum of the n = 2 * B*H*W pieces of a channel, in any order, is
    # within gamma_n * sum |piece| of the exact sum (gamma_n = n u / (1 - n u), u = 2^-24)
    n = 2 * B * H * W
    dbk = dbw.double().cpu()
    assert torch.isfinite(dbk).all()
    yh, yl = R.pieces(dy64.numpy(), s)
    nu = n * 2.0 ** -24
    slack = nu / (1 - nu) * torch.from_numpy((np.abs(yh) + np.abs(yl)).sum((0, 2, 3))) / s
    worst = float(((dbk - db_or).abs() / slack).max())
    print("%-46s worst/bound %.3f" % ("dbias " + tag, worst))
    assert worst <= 1.0
