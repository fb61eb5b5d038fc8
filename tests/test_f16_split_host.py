"""The 2xfp16 representation on the CPU (tests/f16_split_ref.py): the element bounds the
format implies, the edges of its range, and what they mean for one K = 1152 conv across
operand magnitudes — with fp16 subnormal pieces kept, as the MFMA keeps them, and flushed.
The bounds come from the format (two 11-bit significands, subnormal quantum 2^-24), not from
what the emulation gives."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import f16_split_ref as R

KS_ALL = [16, 64, 256, 576, 1152, 2304]


def _sweep(lo_exp, hi_exp, n, seed, top):
    """n f32 values of both signs, log-uniform in [2^lo_exp, 2^hi_exp], clipped to top."""
    rs = np.random.RandomState(seed)
    v = np.exp2(rs.uniform(lo_exp, hi_exp, n)) * rs.choice([-1.0, 1.0], n)
    return np.clip(v, -top, top).astype(np.float32).astype(np.float64)


def test_wscale_values():
    assert [R.fp16_wscale(K) for K in (1, 16, 17, 256, 576, 1152, 4096, 4097)] == \
        [2.0 ** e for e in (9, 11, 12, 13, 14, 15, 15, 16)]
    assert R.ACT_SCALE == 32.0 and R.act_limit() == 2047.0
    for K in KS_ALL:     # the default-init bound 1/sqrt(K) lands in [2^9, 2^10]: 64x headroom
        assert 2.0 ** 9 <= K ** -0.5 * R.fp16_wscale(K) <= 2.0 ** 10


def test_activation_element_bound():
    """|hi + lo - v*32| / 32 <= max(2^-22 |v|, 2^-30) for |v| <= 2047, at every magnitude
    down to where both pieces vanish."""
    v = np.concatenate([_sweep(-45, 11, 200000, 1, 2047.0),
                        np.float32([2047, -2047, 2046.9999, 1, -1, 2.0 ** -7, 2.0 ** -19, 2.0 ** -24, 2.0 ** -29,
                                    2.0 ** -30, 2.0 ** -31, 1e-30, 0.0, -0.0]).astype(np.float64)])
    hi, lo = R.pieces(v, R.ACT_SCALE)
    assert np.isfinite(hi).all() and np.isfinite(lo).all()
    err = np.abs(hi + lo - v * 32.0) / 32.0
    assert (err <= R.act_element_bound(v)).all(), float((err / R.act_element_bound(v)).max())
    # the absolute floor is reached (so 2^-30 is the right figure, not a loose one) and the
    # relative one nearly so
    assert err[np.abs(v) < 2.0 ** -8].max() > 0.9 * 2.0 ** -30
    big = np.abs(v) >= 2.0 ** -7
    assert (err[big] / np.abs(v[big])).max() > 0.4 * 2.0 ** -22
    # "full precision from |v| >= 2^-7": from there the relative bound is the larger one
    assert (R.act_element_bound(v[big]) == 2.0 ** -22 * np.abs(v[big])).all()


@pytest.mark.parametrize("K", KS_ALL)
def test_weight_element_bound(K):
    """|hi + lo - w*s| / s <= max(2^-22 |w|, 2^-25 / s) for |w| <= 65504 / s."""
    s, top = R.fp16_wscale(K), R.weight_limit(K)
    w = np.concatenate([_sweep(-50, 3, 100000, 2 + K, top), [top, -top, K ** -0.5, 1e-6 * K ** -0.5, 0.0, -0.0]])
    w = w.astype(np.float32).astype(np.float64)
    w = np.clip(w, -top, top)
    hi, lo = R.pieces(w, s)
    assert np.isfinite(hi).all() and np.isfinite(lo).all()
    err = np.abs(hi + lo - w * s) / s
    assert (err <= R.weight_element_bound(w, s)).all()


def test_range_edges():
    """2047 and 65504 / s are the last values with finite pieces; 2048 and the next fp16
    step above the weight limit (65536 / s) give hi = +-inf, lo = -+inf."""
    hi, lo = R.pieces(np.float64([2047.0, -2047.0]), R.ACT_SCALE)
    assert np.array_equal(hi, [65504.0, -65504.0]) and np.array_equal(lo, [0.0, 0.0])
    hi, lo = R.pieces(np.float64([2048.0, -2048.0]), R.ACT_SCALE)
    assert np.array_equal(hi, [np.inf, -np.inf]) and np.array_equal(lo, [-np.inf, np.inf])
    for K in KS_ALL:
        s = R.fp16_wscale(K)
        hi, lo = R.pieces(np.float64([65504.0 / s, -65504.0 / s]), s)
        assert np.array_equal(hi, [65504.0, -65504.0]) and np.array_equal(lo, [0.0, 0.0])
        hi, lo = R.pieces(np.float64([65536.0 / s, -65536.0 / s]), s)
        assert np.array_equal(hi, [np.inf, -np.inf]) and not np.isfinite(lo).any()
    # between the largest fp16 and the rounding boundary 65520 the hi piece is still finite
    hi, lo = R.pieces(np.float64([65519.0 / 32.0]), R.ACT_SCALE)
    assert hi[0] == 65504.0 and lo[0] == 15.0


def test_signs_and_zeros():
    v = _sweep(-30, 11, 50000, 5, 2047.0)
    hi, lo = R.pieces(v, R.ACT_SCALE)
    nh, nl = R.pieces(-v, R.ACT_SCALE)
    assert np.array_equal(nh, -hi) and np.array_equal(nl, -lo)            # RNE is symmetric
    assert (np.sign(hi) == np.sign(v)).all()
    # lo carries the rounding remainder of hi: either sign, at most half an ulp of hi
    assert (lo * hi < 0).any() and (lo * hi > 0).any()
    ulp = np.maximum(np.exp2(np.floor(np.log2(np.abs(hi))) - 10), 2.0 ** -24)
    assert (np.abs(lo) <= 0.5 * ulp).all()
    hi, lo = R.pieces(np.float64([0.0, -0.0]), R.ACT_SCALE)
    assert np.array_equal(hi, [0.0, 0.0]) and np.array_equal(lo, [0.0, 0.0])
    assert not np.signbit(hi[0]) and np.signbit(hi[1])                    # -0.0 stays -0.0 in hi
    # flushed variant: only pieces below 2^-14 change
    fh, fl = R.pieces(v, R.ACT_SCALE, flush=True)
    hi, lo = R.pieces(v, R.ACT_SCALE)
    assert np.array_equal(fh[np.abs(hi) >= 2.0 ** -14], hi[np.abs(hi) >= 2.0 ** -14])
    assert (fl[np.abs(lo) < 2.0 ** -14] == 0).all() and (fl != lo).any()


def _rel(a, ref):
    return float((a - ref).norm() / ref.norm())


ACT_MAGS = [0, -7, -10, -14, -18]
W_MAGS = [1.0, 1e-2, 1e-4, 1e-6]


def test_conv_error_table_k1152():
    """One 3x3 conv over 128 channels (K = 1152): conv_2xfp16 against the true float64 conv
    of the unsplit operands, post-ReLU activations relu(clip(randn, +-4)) * mag and weights
    uniform within the default-init bound 1/sqrt(K) (times a factor in the weight rows).

    Asserted, from the element bounds alone: with the other operand's errors independent
    of it, the output's relative L2 error is rms(dx)/rms(x) + rms(dw)/rms(w), and each
    element error is at most act_element_bound(max|x|) / weight_element_bound(max|w|); the
    dropped lo.lo products add at most 2^-22 of each product.  And: with subnormal pieces
    flushed the error at activation magnitude 2^-10 is >= 100x the kept one (every lo piece
    is then below 2^-14 and lost, leaving 11 bits) — the factor by which
    tests/test_gpu_f16_range.py tells a flushing kernel from a right one."""
    K, Cin, Cout, H = 1152, 128, 32, 16
    gen = torch.Generator().manual_seed(1152)
    x0 = F.relu(torch.randn(1, Cin, H, H, generator=gen, dtype=torch.float64).clamp(-4, 4)).float().double()
    w0 = ((torch.rand(Cout, Cin, 3, 3, generator=gen, dtype=torch.float64) * 2 - 1) / np.sqrt(K)).float().double()
    s = R.fp16_wscale(K)
    rows = [("act 2^%d" % e, 2.0 ** e, 1.0) for e in ACT_MAGS] + [("w %.0e" % f, 1.0, f) for f in W_MAGS[1:]]
    kept = {}
    print("\n%-10s %12s %12s %12s %8s" % ("operand", "kept", "flushed", "bound", "ratio"))
    for name, am, wf in rows:
        x = (x0 * am).float().double()
        w = (w0 * wf).float().double()
        true = F.conv2d(x, w, None, 1, 1)
        ek = _rel(R.conv_2xfp16(x, w, pad=1), true)
        ef = _rel(R.conv_2xfp16(x, w, pad=1, flush=True), true)
        bound = (float(R.act_element_bound(float(x.abs().max()))) / float(x.pow(2).mean().sqrt())
                 + float(R.weight_element_bound(float(w.abs().max()), s)) / float(w.pow(2).mean().sqrt())
                 + 2.0 ** -22)
        print("%-10s %12.2e %12.2e %12.2e %8.0f" % (name, ek, ef, bound, ef / ek))
        assert ek <= bound, (name, ek, bound)
        assert ef >= ek
        kept[name] = (ek, ef)
    ek, ef = kept["act 2^-10"]
    assert ef >= 100 * ek, (ek, ef)
    # inside "full precision" (|v| >= 2^-7, init-scale weights) a layer sits at the f32 level
    assert kept["act 2^0"][0] <= 2.0 ** -21 and kept["act 2^-7"][0] <= 2.0 ** -21


def test_gradient_oracles_are_the_adjoints():
    """dgrad_2xfp16 / wgrad3_2xfp16 on operands that split exactly (small integers, so lo = 0
    and nothing is dropped) equal the float64 gradients of the conv: the mode-1 weight
    order, the scales and the bias gradient are right."""
    gen = torch.Generator().manual_seed(7)
    x = torch.randint(-8, 9, (2, 16, 6, 6), generator=gen).double()
    w = (torch.randint(-8, 9, (32, 16, 3, 3), generator=gen).double() / 64.0)
    dy = torch.randint(-8, 9, (2, 32, 6, 6), generator=gen).double() * 2.0 ** -20
    assert torch.equal(R.conv_2xfp16(x, w, pad=1), F.conv2d(x, w, None, 1, 1))
    dx = R.dgrad_2xfp16(dy, w, 2.0 ** 30, pad=1)
    assert torch.equal(dx, torch.nn.grad.conv2d_input(x.shape, w, dy, 1, 1))
    dw, db = R.wgrad3_2xfp16(dy, x, 2.0 ** 30)
    assert torch.equal(dw, torch.nn.grad.conv2d_weight(x, w.shape, dy, 1, 1))
    assert torch.equal(db, dy.sum((0, 2, 3)))
