"""The exact-f32 conv kernels against the f32 fma chain they are documented to be, per channel.

Kn.conv2d_forward, Kn.conv1x1_forward_kmajor, Kn.conv2d_dgrad and Kn.conv2d_wgrad (conv_f32_fwd.hip,
conv1x1_dma.hip, conv_f32_wgrad.hip, conv_reduce.hip) are the yardstick of every split-path
accuracy bar (tests/test_gpu_split.py, tests/test_gpu_f16_range.py) and still carry real work.
For each case, on the same f32 inputs: the float64 truth (F.conv2d / torch.nn.grad in double,
the input through f32_chain_ref.prologue) and the chain reference (tests/f32_chain_ref.py), then

  a. |y - true| <= gamma_bound(conv(|inp|, |w|) + |b| + |res|, K + 3) at every element: no
     order of exact f32 operations can break it; the failing element's index is in the message;
  b. per channel (output channel forward, input channel for the data gradient, output channel
     of dw), e_k <= 1.5 * e_ch + 2^-24, e the relative L2 error against the truth of the kernel
     and of the chain.  1.5: the kernel is this chain, possibly with the elements of a K step
     permuted or in shorter chains, which can only lower the expected error; on the CPU two
     orders of one chain differ per channel by 0.85 .. 1.13 where a channel has 128 outputs
     or more (test_f32_chain_host.py) — 1.5 covers that and stays below 2.  2^-24: one unit
     roundoff.  The bar is never taken from the kernel's output;
  c. |db - sum dy| <= gamma_bound(sum |dy|, K + 3);
  d. nothing non-finite; a channel whose truth is exactly zero (one is planted in every
     `spread` case) is exactly zero.

Which chain.  The reference of a launch is the chain in that launch's documented order
(DESIGN.md section 4, f32_chain_ref.chain_conv): seeded with float32(bias + res) without split-K
(csrc/common.h seed_acc), `splits` chains from zero summed in split order, then bias, then the
residual, with split-K (splits read from the ubpl_*_workspace query the launch itself uses;
conv_f32.h fwd_plan, conv_reduce.hip).  Against the plain chain — one chain from zero, bias and
residual afterwards — the same bar would say less and sometimes the wrong thing: on the CPU
the seeded chain's per-channel error is 1.05 .. 2.2 x the plain chain's when bias and residual are
as large as the conv (every partial sum carries the seed), and on a 2x2 plane (four outputs per
channel) two faithful orders of one chain differ per channel by up to 10 x.  Found on the
MI355X: every forward, k-major and data-gradient launch here is bit-equal to the chain in its
documented order (recorded with each case, not asserted), while against the plain chain the
worst e_k / (1.5 e_ch + 2^-24) is 1.095 (fwd 3x3 (1,256,2,256) spread: 48 split-K chains on
four pixels), which would have missed the bar with nothing wrong in the kernel.  The ratio against the plain
chain is recorded beside the asserted one.  The weight gradient runs chains from zero over
k = (b, p) slices, reduced in float64 and rounded once; accumulate=True adds that onto dw / db in
f32.  Its reference is the one chain over all of k: the slicing depends on two plans the
workspace query does not tell apart, it only shortens the chains, and the cases with few
elements per channel (K = 36 .. 75) run as a single slice, bit-equal to the chain.

Operand conditions, three per case where the entry takes a prologue: `uniform` (everything
uniform in [-1, 1], weights / sqrt(K), bias and residual at each channel's own output magnitude),
`prologue` (general coefficients, sc in [0.5, 1.5), sh = 0.5 * uniform: about half exact zeros)
and `spread` (per-input-channel scales 2^k, k in [-12, 8]; per-output-channel scales 2^-10 .. 1:
a small channel cannot hide behind a large one).

With UBPL_YARDSTICK_LOG=<file> every recorded line is appended to that file
(profiles/f32_yardstick_gpu_tests.txt).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import f32_chain_ref as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
CONDS = ["uniform", "prologue", "spread"]


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ubpl_amd import _lib
    _lib.load()


def _d(t):
    return None if t is None else t.to(DEV)


def _v(t):
    return t[None, :, None, None]


def _gen(seed):
    gen = torch.Generator().manual_seed(seed)
    return gen, lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64) * 2 - 1


def _pow2(gen, lo, hi, n):
    return 2.0 ** torch.randint(lo, hi + 1, (n,), generator=gen).double()


# ------------------------------------------------------------------ forward
# (B, Cin, H, Cout), KS, stride: the smallest shape that reaches each conv_fwd_kernel instantiation
# that is built (conv_f32_fwd.hip fwd_built, ubpl_conv2d_forward, conv_f32.h fwd_plan; PRO by the
# operand condition)
FWD_SHAPES = [
    ((2, 256, 16, 128), 1, 1),   # 1x1: VECB (P % 4 == 0) + AVEC, Cout > 64: the plan picks BM
    ((3, 64, 32, 64), 1, 1),     # Cout <= 64: BM = 64; three images per pixel-tile row
    ((4, 256, 32, 16), 1, 1),    # Cout 16: rows 16 .. 63 of the tile clamped on load, never stored
    ((2, 16, 32, 256), 1, 1),    # Cin 16: one K tile
    ((2, 17, 8, 256), 1, 1),     # Cin 17 (heads / merge): Ktot % 4 != 0, no AVEC; K tail of 1 masked
    ((3, 32, 5, 48), 1, 1),      # P = 25, P % 4 != 0: no VECB, the per-tap scalar loader on a 1x1; N = 75 < BN
    ((2, 128, 16, 128), 3, 1),   # 3x3: TAPK + AVEC, one tap per K tile, 8 channel groups
    ((4, 128, 8, 128), 3, 1),    # small grid: split-K slab + split_reduce_kernel (asserted)
    ((1, 256, 2, 256), 3, 1),    # 2x2 plane: N = 4, every tap but the centre partly outside
    ((2, 64, 6, 32), 3, 1),      # Cout 32, Wo = 6: output rows not float4-aligned
    ((2, 32, 6, 32), 3, 1),      # two channel groups, Wo = 6
    ((2, 3, 64, 64), 7, 2),      # stem: generic loader (a K tile straddles taps), scalar weight rows
    ((1, 3, 12, 64), 7, 2),      # stem, Wo = 6, N = 36
]
# conv1x1_dma_kernel through conv1x1_forward_kmajor (BM by the plan, PRO by the condition); the
# last with the residual aliasing the output
KMAJOR_SHAPES = [(2, 256, 16, 128), (2, 16, 8, 256), (2, 256, 8, 16), (2, 256, 4, 256)]
FWD_CASES = [(s, c) for s in FWD_SHAPES for c in CONDS]
KMAJOR_CASES = [(s, c) for s in KMAJOR_SHAPES for c in CONDS]


def _shape_id(shape, KS):
    return "%dx%d_%s" % (KS, KS, "x".join(str(v) for v in shape))


def _forward_operands(shape, KS, stride, cond, seed):
    """The f32 operands of one forward case and its float64 references (module docstring)."""
    B, Cin, H, Cout = shape
    K, pad = Cin * KS * KS, (KS - 1) // 2
    gen, u = _gen(seed)
    x, w = u(B, Cin, H, H), u(Cout, Cin, KS, KS) / np.sqrt(K)
    sc = sh = None
    if cond == "prologue":
        sc, sh = torch.rand(Cin, generator=gen, dtype=torch.float64) + 0.5, 0.5 * u(Cin)
    elif cond == "spread":
        x = x * 4.0
        sc, sh = _pow2(gen, -12, 8, Cin), torch.zeros(Cin, dtype=torch.float64)
        w = w * _pow2(gen, -10, 0, Cout)[:, None, None, None]
        w[1] = 0.0                                                  # the planted zero channel
    x32, w32 = x.float(), w.float()
    sc32, sh32 = (sc.float(), sh.float()) if sc is not None else (None, None)
    inp = C.prologue(x32, sc32, sh32) if sc is not None else x32
    true = F.conv2d(inp.double(), w32.double(), None, stride, pad)
    # bias and residual at each output channel's own magnitude (zero for the zero channel)
    mag = true.pow(2).mean((0, 2, 3)).sqrt()
    b32, res32 = (u(Cout) * mag).float(), (u(*true.shape) * _v(mag)).float()
    true = true + _v(b32.double()) + res32.double()
    absref = F.conv2d(inp.double().abs(), w32.double().abs(), None, stride, pad) + _v(b32.double().abs()) + \
        res32.double().abs()
    return dict(x=x32, w=w32, b=b32, res=res32, sc=sc32, sh=sh32, inp=inp, true=true, absref=absref, K=K, pad=pad)


def _splits(workspace, Cout, N):
    """The number of split-K chains of a launch, from its workspace query (splits * Cout * N floats)."""
    assert workspace % (Cout * N) == 0
    return max(1, workspace // (Cout * N))


def _check_forward(tag, y, o, stride, splits):
    """Bars a, b, d of a forward result against the chain in the launch's documented order:
    seeded with bias + res on a direct launch, `splits` zero-seeded chains and the reduce on a
    split-K launch.  The ratio against the plain chain (one chain from zero, bias and residual
    afterwards) is recorded beside it."""
    kw = dict(splits=splits) if splits > 1 else dict(seeded=True)
    chain = C.chain_conv(o["inp"], o["w"], o["b"], o["res"], stride, o["pad"], **kw)
    plain = C.chain_conv(o["inp"], o["w"], o["b"], o["res"], stride, o["pad"])
    r = C.bars(y, o["true"], chain, o["absref"], o["K"] + 3, 1)
    other = C.bars(y, o["true"], plain, o["absref"], o["K"] + 3, 1)
    C.record("      %-62s %s; bit-equal to it: %s; against the plain chain: worst e_k/(1.5 e_ch + u) %.3f" % (
        tag, "split-K, %d chains" % splits if splits > 1 else "direct, seeded chain",
        bool(torch.equal(y.detach().cpu(), chain)), other["b"]))
    C.assert_bars(tag, r)


@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: "%s-%s" % (_shape_id(c[0][0], c[0][1]), c[1]))
def test_conv2d_forward_vs_chain(case):
    from ubpl_amd import _lib, kernels as Kn
    (shape, KS, stride), cond = case
    B, Cin, H, Cout = shape
    o = _forward_operands(shape, KS, stride, cond, 7000 + 13 * FWD_CASES.index(case))
    Ho = o["true"].shape[-1]
    splits = _splits(int(_lib.lib().ubpl_conv2d_forward_workspace(B, Cin, Cout, KS, Ho, Ho)), Cout, B * Ho * Ho)
    if shape == (4, 128, 8, 128):
        assert splits > 1, "the plan no longer splits K at this shape"
    y = Kn.conv2d_forward(_d(o["x"]), _d(o["w"]), _d(o["b"]), stride, _d(o["sc"]), _d(o["sh"]), res=_d(o["res"]))
    torch.cuda.synchronize()
    _check_forward("fwd %s %s" % (_shape_id(shape, KS), cond), y, o, stride, splits)


@pytest.mark.parametrize("case", KMAJOR_CASES, ids=lambda c: "%s-%s" % (_shape_id(c[0], 1), c[1]))
def test_conv1x1_kmajor_vs_chain(case):
    from ubpl_amd import _lib, kernels as Kn
    shape, cond = case
    B, Cin, H, Cout = shape
    o = _forward_operands(shape, 1, 1, cond, 8000 + 13 * KMAJOR_CASES.index(case))
    splits = _splits(int(_lib.lib().ubpl_conv1x1_kmajor_workspace(B, Cin, Cout, H * H)), Cout, B * H * H)
    x = _d(o["x"])
    assert Kn.conv1x1_kmajor_ok(x, Cout)
    wk = Kn.conv_weight_flip(_d(o["w"]))
    alias = shape == (2, 256, 4, 256)
    r = _d(o["res"]).clone()
    y = Kn.conv1x1_forward_kmajor(x, wk, _d(o["b"]), _d(o["sc"]), _d(o["sh"]), res=r, out=r if alias else None)
    torch.cuda.synchronize()
    if alias:
        assert y.data_ptr() == r.data_ptr()
    _check_forward("kmajor %s %s%s" % (_shape_id(shape, 1), cond, " (res aliases y)" if alias else ""), y, o, 1, splits)


# ------------------------------------------------------------------ data gradient
# every stride-1 forward shape through conv2d_dgrad (conv_fwd_kernel on the flipped weights, no
# prologue: Cout plays Cin and the 17 / 16 / 48 input channels are the output rows); the three
# k-major shapes also through conv1x1_forward_kmajor(dy, w, None)
DGRAD_SHAPES = [(s, KS) for s, KS, st in FWD_SHAPES if st == 1] + [(s, 1) for s in KMAJOR_SHAPES[1:]]
DGRAD_CASES = [(s, c) for s in DGRAD_SHAPES for c in ("uniform", "spread")]


@pytest.mark.parametrize("case", DGRAD_CASES, ids=lambda c: "%s-%s" % (_shape_id(*c[0]), c[1]))
def test_conv2d_dgrad_vs_chain(case):
    from ubpl_amd import _lib, kernels as Kn
    (shape, KS), cond = case
    B, Cin, H, Cout = shape
    K, pad = Cout * KS * KS, (KS - 1) // 2
    lib = _lib.lib()
    gen, u = _gen(9000 + 13 * DGRAD_CASES.index(case))
    dy, w = u(B, Cout, H, H), u(Cout, Cin, KS, KS) / np.sqrt(K)
    if cond == "spread":
        dy = dy * _v(_pow2(gen, -12, 8, Cout))
        w = w * _pow2(gen, -10, 0, Cin)[None, :, None, None]
        w[:, 1] = 0.0                                               # the planted zero channel of dx
    dy32, w32 = dy.float(), w.float()
    g = torch.nn.grad.conv2d_input
    true = g((B, Cin, H, H), w32.double(), dy32.double(), 1, pad)
    absref = g((B, Cin, H, H), w32.double().abs(), dy32.double().abs(), 1, pad)
    tag = "dgrad %s %s" % (_shape_id(shape, KS), cond)
    # the data gradient is the forward with Cout as its input channels and Cin as its output rows
    runs = [("", lambda: Kn.conv2d_dgrad(_d(dy32), _d(w32)),
             int(lib.ubpl_conv2d_forward_workspace(B, Cout, Cin, KS, H, H)))]
    if KS == 1 and shape in KMAJOR_SHAPES[:3]:
        assert Kn.conv1x1_kmajor_ok(_d(dy32), Cin)
        runs.append(("kmajor ", lambda: Kn.conv1x1_forward_kmajor(_d(dy32), _d(w32), None),
                     int(lib.ubpl_conv1x1_kmajor_workspace(B, Cout, Cin, H * H))))
    chains = {}
    for name, run, workspace in runs:
        splits = _splits(workspace, Cin, B * H * H)
        if splits not in chains:
            chains[splits] = C.chain_dgrad(dy32, w32, pad, splits=splits)
        dx = run()
        torch.cuda.synchronize()
        C.record("      %-62s %s; bit-equal to it: %s" % (name + tag, "split-K, %d chains" % splits if splits > 1
                                                          else "direct", bool(torch.equal(dx.cpu(), chains[splits]))))
        C.assert_bars(name + tag, C.bars(dx, true, chains[splits], absref, K + 3, 1))


# ------------------------------------------------------------------ weight gradient
# (B, Cin, H, Cout), KS, stride, dy misaligned: K = B*P <= 2048 (at the workload's 32k pixels the
# split chains sit far below one chain and the bar would say little).  ubpl_conv2d_wgrad: v2
# (conv_wgrad2_kernel) needs P % 4 == 0, Wo % 4 == 0 on a spatial kernel and a 16-B aligned dy;
# else v1 (conv_wgrad_kernel), TAPN on 1x1 and on 3x3 with Cin % 64 == 0
WGRAD_SHAPES = [
    ((2, 64, 16, 64), 3, 1, False),     # v2, 3x3 generic rows (VEC1 off), K = 512
    ((2, 256, 16, 128), 1, 1, False),   # v2, 1x1 VEC1 (float4 rows of x)
    ((2, 128, 32, 128), 3, 1, False),   # v2, the larger tiles (Cout, Ntot > 64); the (8,128,32,128) case's first two images
    ((2, 64, 6, 32), 3, 1, False),      # Wo = 6: v1, TAPN (Cin % 64 == 0)
    ((2, 32, 6, 32), 3, 1, False),      # Wo = 6: v1, n tiles across taps
    ((3, 32, 5, 48), 1, 1, False),      # P = 25: v1, TAPN on 1x1; K = 75, a 32-k step tail
    ((2, 3, 64, 64), 7, 2, False),      # stem: v2, KS 7 stride 2, Ntot = 147
    ((1, 3, 12, 64), 7, 2, False),      # stem, Wo = 6: v1 generic; K = 36
    ((2, 64, 16, 64), 3, 1, True),      # dy at a 4-byte offset: v1 at a v2 shape
]
WGRAD_CASES = [(s, c) for s in WGRAD_SHAPES for c in CONDS]


def _wgrad_id(c):
    (shape, KS, stride, mis), cond = c
    return "%s%s-%s" % (_shape_id(shape, KS), "_misaligned" if mis else "", cond)


@pytest.mark.parametrize("case", WGRAD_CASES, ids=_wgrad_id)
def test_conv2d_wgrad_vs_chain(case):
    """accumulate False, then True onto a non-zero dw / db drawn at each channel's own magnitude."""
    from ubpl_amd import kernels as Kn
    (shape, KS, stride, misaligned), cond = case
    B, Cin, H, Cout = shape
    pad = (KS - 1) // 2
    Ho = (H + 2 * pad - KS) // stride + 1
    K = B * Ho * Ho
    assert K <= 2048
    gen, u = _gen(10000 + 13 * WGRAD_CASES.index(case))
    x, dy = u(B, Cin, H, H), u(B, Cout, Ho, Ho)
    sc = sh = None
    if cond == "prologue":
        sc, sh = torch.rand(Cin, generator=gen, dtype=torch.float64) + 0.5, 0.5 * u(Cin)
    elif cond == "spread":
        x = x * 4.0
        sc, sh = _pow2(gen, -12, 8, Cin), torch.zeros(Cin, dtype=torch.float64)
        dy = dy * _v(_pow2(gen, -10, 0, Cout))
        dy[:, 1] = 0.0                                              # the planted zero channel of dw / db
    x32, dy32 = x.float(), dy.float()
    sc32, sh32 = (sc.float(), sh.float()) if sc is not None else (None, None)
    inp = C.prologue(x32, sc32, sh32) if sc is not None else x32
    g = torch.nn.grad.conv2d_weight
    true = g(inp.double(), (Cout, Cin, KS, KS), dy32.double(), stride, pad)
    absref = g(inp.double().abs(), (Cout, Cin, KS, KS), dy32.double().abs(), stride, pad)
    dbt, dba = dy32.double().sum((0, 2, 3)), dy32.double().abs().sum((0, 2, 3))
    chain, _ = C.chain_wgrad(dy32, inp, KS, stride, pad)
    mag = true.pow(2).mean((1, 2, 3)).sqrt()
    dw0 = (u(Cout, Cin, KS, KS) * mag[:, None, None, None]).float()
    db0 = (u(Cout) * dbt.abs()).float()
    dyd = _d(dy32)
    if misaligned:
        buf = torch.empty(dy32.numel() + 1, device=DEV)
        dyd = buf[1:].view_as(dy32)
        dyd.copy_(dy32)
        assert dyd.data_ptr() % 16 == 4
    tag = "wgrad " + _wgrad_id(case)
    for acc in (False, True):
        dw, db = _d(dw0).clone(), _d(db0).clone()
        Kn.conv2d_wgrad(dyd, _d(x32), KS, stride, dw, db, _d(sc32), _d(sh32), accumulate=acc)
        torch.cuda.synchronize()
        t, a, ch = true, absref, chain
        bt, ba = dbt, dba
        if acc:
            t, a, ch = dw0.double() + true, dw0.double().abs() + absref, dw0 + chain
            bt, ba = db0.double() + dbt, db0.double().abs() + dba
        C.assert_bars(tag + (" accumulate" if acc else ""), C.bars(dw, t, ch, a, K + 3, 0))
        dbk = db.double().cpu()
        bound = C.gamma_bound(ba, K + 3)
        worst = float(((dbk - bt).abs() / bound.clamp_min(1e-300)).max())
        C.record("      %-62s dbias: worst/gamma %.4f; dw bit-equal to the one chain: %s" % (
            tag + (" accumulate" if acc else ""), worst, bool(torch.equal(dw.cpu(), ch))))
        assert torch.isfinite(dbk).all() and bool(((dbk - bt).abs() <= bound).all()), (tag, acc, worst)
