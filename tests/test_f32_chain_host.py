"""tests/f32_chain_ref.py against float64, and its bars against planted defects (no GPU).

The GPU yardstick test (tests/test_gpu_f32_yardstick.py) holds the exact-f32 conv kernels to the
f32 fma chain per channel and to gamma_bound elementwise.  Here: the chain obeys gamma_bound
itself; two K orders of it agree per channel within the bar; its gradients agree with the float64
torch.nn.grad results; and a CPU mock kernel with one planted defect — the chain with operands
truncated to a 10-bit mantissa, with one 16-wide K tile dropped at one pixel, with its split-K
partials rounded to bf16, or with the last pixel left out of the weight gradient — fails the
bars, while the unmodified chain in another K order passes them.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import f32_chain_ref as C


def _u(gen, *s):
    return torch.rand(*s, generator=gen, dtype=torch.float64) * 2 - 1


def _forward_case(shape, KS, seed, pro=True):
    """Uniform operands, general prologue coefficients, bias and residual at each channel's own
    output magnitude; the float64 truth and absref = conv(|inp|, |w|) + |b| + |res|."""
    B, Cin, H, Cout = shape
    K, pad = Cin * KS * KS, (KS - 1) // 2
    gen = torch.Generator().manual_seed(seed)
    x, w = _u(gen, B, Cin, H, H).float(), (_u(gen, Cout, Cin, KS, KS) / np.sqrt(K)).float()
    sc, sh = (torch.rand(Cin, generator=gen) + 0.5), (_u(gen, Cin) * 0.5).float()
    inp = C.prologue(x, sc, sh) if pro else x
    true = F.conv2d(inp.double(), w.double(), None, 1, pad)
    mag = true.pow(2).mean((0, 2, 3)).sqrt()
    b, res = (_u(gen, Cout) * mag).float(), (_u(gen, B, Cout, H, H) * mag[None, :, None, None]).float()
    true = true + b.double()[None, :, None, None] + res.double()
    absref = F.conv2d(inp.double().abs(), w.double().abs(), None, 1, pad) + b.double().abs()[None, :, None, None] + \
        res.double().abs()
    return inp, w, b, res, pad, K, true, absref


@pytest.fixture(scope="module")
def fwd3():
    """One 3x3 case (K = 288, two channel groups) with its references, shared and left unchanged."""
    inp, w, b, res, pad, K, true, absref = _forward_case((2, 32, 8, 24), 3, 101)
    return dict(inp=inp, w=w, b=b, res=res, pad=pad, K=K, true=true, absref=absref,
                chain=C.chain_conv(inp, w, b, res, 1, pad), other=C.chain_conv(inp, w, b, res, 1, pad, order="ci"))


@pytest.fixture(scope="module")
def wg3():
    """One 3x3 weight-gradient case (K = B*P = 512) with its references."""
    gen = torch.Generator().manual_seed(202)
    B, Cin, Cout, H = 2, 16, 24, 16
    x, dy = _u(gen, B, Cin, H, H).float(), _u(gen, B, Cout, H, H).float()
    inp = C.prologue(x, torch.rand(Cin, generator=gen) + 0.5, (_u(gen, Cin) * 0.5).float())
    g = torch.nn.grad.conv2d_weight
    true = g(inp.double(), (Cout, Cin, 3, 3), dy.double(), 1, 1)
    absref = g(inp.double().abs(), (Cout, Cin, 3, 3), dy.double().abs(), 1, 1)
    dw, db = C.chain_wgrad(dy, inp, 3, 1, 1)
    return dict(inp=inp, dy=dy, K=B * H * H, true=true, absref=absref, dw=dw, db=db)


def test_prologue_is_the_fma_then_relu():
    gen = torch.Generator().manual_seed(5)
    x, sc, sh = _u(gen, 2, 7, 5, 5).float(), torch.rand(7, generator=gen) + 0.5, (_u(gen, 7) * 0.5).float()
    got = C.prologue(x, sc, sh)
    assert got.dtype == torch.float32 and bool((got >= 0).all())
    ref = F.relu(x.double() * sc.double()[None, :, None, None] + sh.double()[None, :, None, None])
    assert float((got.double() - ref).abs().max()) <= 2.0 ** -24 * float(ref.abs().max())
    assert 0.3 < float((got == 0).double().mean()) < 0.7                # about half exact zeros
    # exact coefficients (powers of two, no shift) leave nothing to round
    p2 = 2.0 ** torch.randint(-12, 9, (7,), generator=gen).float()
    assert torch.equal(C.prologue(x, p2, torch.zeros(7)).double(), F.relu(x.double() * p2.double()[None, :, None, None]))


def test_k_order_is_conv_f32_h():
    """k = (ci/16)*16T + tap*16 + ci%16; Cin not a multiple of 16: tap-major over the real channels."""
    T = 9
    assert [(ci // 16) * 16 * T + tap * 16 + ci % 16 for ci, tap in C.k_order(32, T)] == list(range(32 * T))
    assert C.k_order(3, 2) == [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1)]
    assert C.k_order(17, 1) == [(c, 0) for c in range(17)]
    assert sorted(C.k_order(32, T, "ci")) == sorted(C.k_order(32, T)) == sorted(C.k_order(32, T, "rev"))


@pytest.mark.parametrize("shape,KS,stride", [((2, 32, 8, 24), 3, 1), ((2, 17, 6, 20), 1, 1), ((1, 3, 12, 8), 7, 2)])
def test_chain_within_gamma_bound_of_float64(shape, KS, stride):
    B, Cin, H, Cout = shape
    gen = torch.Generator().manual_seed(7 + Cin)
    pad, K = (KS - 1) // 2, Cin * KS * KS
    x, w = _u(gen, B, Cin, H, H).float(), (_u(gen, Cout, Cin, KS, KS) / np.sqrt(K)).float()
    b = _u(gen, Cout).float()
    true = F.conv2d(x.double(), w.double(), b.double(), stride, pad)
    res = _u(gen, *true.shape).float()
    true = true + res.double()
    absref = F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), stride, pad) + res.double().abs()
    for order, seeded in (("grouped", False), ("ci", False), ("rev", False), ("grouped", True)):
        y = C.chain_conv(x, w, b, res, stride, pad, order=order, seeded=seeded)
        assert y.dtype == torch.float32 and y.shape == true.shape
        assert bool(((y.double() - true).abs() <= C.gamma_bound(absref, K + 3)).all()), (order, seeded)
        # and it is an f32 computation, not float64 in disguise
        assert C.rel(y, true) > 2.0 ** -27


def test_two_k_orders_agree_per_channel(fwd3):
    """Each order passes the bars with the other as the reference (the scatter the bar of 1.5
    has to cover: the GPU test's docstring)."""
    f = fwd3
    for y, ref in ((f["other"], f["chain"]), (f["chain"], f["other"])):
        r = C.bars(y, f["true"], ref, f["absref"], f["K"] + 3, 1)
        assert r["finite"] and r["zero_ok"] and r["a"] <= 1.0 and r["b"] <= 1.0, r
    assert not torch.equal(f["chain"], f["other"])


def test_seeded_chain_is_its_own_order(fwd3):
    """Seeding the accumulator with bias + residual (a launch without split-K) keeps the
    elementwise bound but is a different chain: every partial sum carries the seed, so a
    channel with a large bias sits above the unseeded chain's error — the reason the GPU test
    builds the seeded chain for the launches that seed."""
    f = fwd3
    y = C.chain_conv(f["inp"], f["w"], f["b"], f["res"], 1, f["pad"], seeded=True)
    r = C.bars(y, f["true"], f["chain"], f["absref"], f["K"] + 3, 1)
    assert r["finite"] and r["a"] <= 1.0
    nk, d = C.channel_errors(y, f["true"], 1)
    nc, _ = C.channel_errors(f["chain"], f["true"], 1)
    assert float((nk / nc).median()) > 1.0


def test_chain_gradients_vs_float64(fwd3, wg3):
    f, g = fwd3, wg3
    gen = torch.Generator().manual_seed(9)
    dy = _u(gen, *f["true"].shape).float()
    w = f["w"]
    Kd = w.shape[0] * 9
    true = torch.nn.grad.conv2d_input(f["inp"].shape, w.double(), dy.double(), 1, 1)
    absref = torch.nn.grad.conv2d_input(f["inp"].shape, w.double().abs(), dy.double().abs(), 1, 1)
    dx = C.chain_dgrad(dy, w, 1)
    assert bool(((dx.double() - true).abs() <= C.gamma_bound(absref, Kd)).all())
    assert 2.0 ** -27 < C.rel(dx, true) <= C.YARDSTICK_C * np.sqrt(Kd) * C.U
    assert bool(((g["dw"].double() - g["true"]).abs() <= C.gamma_bound(g["absref"], g["K"])).all())
    assert 2.0 ** -27 < C.rel(g["dw"], g["true"]) <= C.YARDSTICK_C * np.sqrt(g["K"]) * C.U
    dbt, dba = g["dy"].double().sum((0, 2, 3)), g["dy"].double().abs().sum((0, 2, 3))
    assert bool(((g["db"].double() - dbt).abs() <= C.gamma_bound(dba, g["K"])).all())


def test_yardstick_cap_holds_the_chain_and_refuses_ten_times_it(fwd3):
    f = fwd3
    e = C.rel(f["chain"], f["true"])
    C.yardstick_cap("host chain", e, f["K"])
    with pytest.raises(AssertionError):
        C.yardstick_cap("host chain x10", 10 * e, f["K"])
    with pytest.raises(AssertionError):
        C.yardstick_cap("host nan", float("nan"), f["K"])


# ------------------------------------------------------------------ the bars bite
def _trunc10(a):
    """float64 values of f32 operands with the significand cut to 10 explicit bits."""
    b = np.ascontiguousarray(a, dtype=np.float64).astype(np.float32).view(np.uint32) & np.uint32(0xFFFFE000)
    return b.view(np.float32).astype(np.float64)


def _bf16(a):
    """f32 array rounded to bf16 (round to nearest even), as f32."""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32)


def _fails(r):
    return {k for k in ("a", "b") if not r[k] <= 1.0} | {k for k in ("finite", "zero_ok") if not r[k]}


def test_reordered_chain_passes_every_bar(fwd3, wg3):
    f = fwd3
    assert _fails(C.bars(f["other"], f["true"], f["chain"], f["absref"], f["K"] + 3, 1)) == set()
    C.assert_bars("host reordered", C.bars(f["other"], f["true"], f["chain"], f["absref"], f["K"] + 3, 1))


def test_planted_reduced_precision_operands_fail_the_chain_bar(fwd3):
    f = fwd3
    y = C.chain_conv(f["inp"], f["w"], f["b"], f["res"], 1, f["pad"], order="ci",
                     defect=lambda k, wk, xk: (_trunc10(wk), _trunc10(xk)))
    r = C.bars(y, f["true"], f["chain"], f["absref"], f["K"] + 3, 1)
    assert "b" in _fails(r) and r["b"] > 100, r                # 2^-11 per operand against ~2^-22: far off
    with pytest.raises(AssertionError):
        C.assert_bars("host trunc10", r)


def test_planted_dropped_k_tile_at_one_pixel_fails_both_bars(fwd3):
    """One 16-wide K tile (steps 16..31) dropped at one output pixel of one image, every channel."""
    f = fwd3

    def drop(k, wk, xk):
        if 16 <= k < 32:
            xk = xk.copy()
            xk[1, :, 37] = 0.0
        return wk, xk
    y = C.chain_conv(f["inp"], f["w"], f["b"], f["res"], 1, f["pad"], order="ci", defect=drop)
    assert int((y != f["other"]).reshape(2, 24, -1).any(1).sum()) == 1          # one pixel differs
    r = C.bars(y, f["true"], f["chain"], f["absref"], f["K"] + 3, 1)
    assert {"a", "b"} <= _fails(r), r
    assert r["a_index"][0] == 1 and r["a_index"][2:] == (37 // 8, 37 % 8), r    # the message names the element


def test_planted_bf16_split_k_partials_fail_the_chain_bar():
    """Split-K over four channel ranges of a 1x1 conv, the partials rounded to bf16 before the
    reduce; the same split with f32 partials passes."""
    inp, w, b, res, pad, K, true, absref = _forward_case((2, 64, 8, 24), 1, 303)
    chain = C.chain_conv(inp, w, b, res, 1, pad)
    parts = [C.chain_conv(inp[:, a:a + 16].contiguous(), w[:, a:a + 16].contiguous()).numpy() for a in range(0, 64, 16)]

    def reduce(ps):
        s = np.zeros_like(ps[0])
        for p in ps:
            s = s + p
        return torch.from_numpy(s + b.numpy()[None, :, None, None] + res.numpy())
    good = C.bars(reduce(parts), true, chain, absref, K + 3, 1)
    assert _fails(good) == set(), good
    bad = C.bars(reduce([_bf16(p) for p in parts]), true, chain, absref, K + 3, 1)
    assert "b" in _fails(bad) and bad["b"] > 100, bad


def test_planted_missing_last_pixel_fails_the_wgrad_bars(wg3):
    g = wg3
    dw, db = C.chain_wgrad(g["dy"], g["inp"], 3, 1, 1, skip_last=True)
    r = C.bars(dw, g["true"], g["dw"], g["absref"], g["K"] + 3, 0)
    assert {"a", "b"} <= _fails(r), r
    # the bias gradient's bound (c) sees it too
    dbt, dba = g["dy"].double().sum((0, 2, 3)), g["dy"].double().abs().sum((0, 2, 3))
    assert bool(((db.double() - dbt).abs() > C.gamma_bound(dba, g["K"] + 3)).any())
    assert bool(((g["db"].double() - dbt).abs() <= C.gamma_bound(dba, g["K"] + 3)).all())


def test_planted_nonzero_in_a_zero_channel_and_nan_fail(fwd3):
    """Bar (d): a channel whose truth is exactly zero must be exactly zero; nothing non-finite."""
    f = fwd3
    w, b, res = f["w"].clone(), f["b"].clone(), f["res"].clone()
    w[3], b[3], res[:, 3] = 0.0, 0.0, 0.0
    true = F.conv2d(f["inp"].double(), w.double(), b.double(), 1, 1) + res.double()
    absref = F.conv2d(f["inp"].double().abs(), w.double().abs(), b.double().abs(), 1, 1) + res.double().abs()
    chain = C.chain_conv(f["inp"], w, b, res, 1, 1)
    r = C.bars(chain, true, chain, absref, f["K"] + 3, 1)
    assert _fails(r) == set() and r["zero_channels"] == 1, r
    y = chain.clone()
    y[0, 3, 0, 0] = 1e-30
    assert {"zero_ok", "a"} <= _fails(C.bars(y, true, chain, absref, f["K"] + 3, 1))
    y = chain.clone()
    y[1, 5, 2, 2] = float("nan")
    assert "finite" in _fails(C.bars(y, true, chain, absref, f["K"] + 3, 1))
