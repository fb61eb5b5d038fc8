"""The hourglass max-pool / upsample-add passes folded into the BatchNorm kernels
next to them (bn_fwd.hip: ubpl_bn_forward_stats_maxpool, ubpl_upsample2x_add_forward_bnstats; bn_bwd.hip:
ubpl_bn_backward_pool) against the launch sequences they replace.

Shapes (B, C, H=W): the smallest that reach every path — the flattened small-plane path
(8, 16) and the whole-row path with 1, 4 and 16 rows of 256 float4s per plane (32, 64,
128); an odd B (a short last slice); more than one slice per channel (64x64 with B=4);
channel counts that are a multiple of nothing; W/4 = 2 .. 32; and 4x4, the smallest plane
the kernels take (W/4 = 1, one float4 a row), which the model test reaches.

Everything that has an existing kernel to compare with is compared bit for bit.  The
statistics of the pooled tensor have a new summation order: their error against a float64
reference may be at most twice that of Kn.bn_forward_stats on the pooled tensor (both sum
f32 per thread and f64 across threads; the factor covers the different element count per
thread) and must stay within test_bn_forward_backward_vs_torch's bars.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(3, 5, 8), (2, 3, 16), (3, 2, 32), (4, 2, 64), (2, 2, 128), (2, 3, 4)]
EPS, MOM = 1e-5, 0.1


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b, what):
    assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), \
        "%s differs in %d of %d elements" % (what, int((_bits(a) != _bits(b)).sum()), a.numel())


_CASES = {}


def _case(shape):
    """Inputs of one shape, made once: x with a tie inside a window and a tie across the two
    rows of a window, BatchNorm parameters / running statistics for x and for the pooled
    tensor, gradients, and the float64 statistics of the pooled tensor."""
    if shape in _CASES:
        return _CASES[shape]
    B, C, H = shape
    gen = torch.Generator().manual_seed(11 + H)
    x = torch.randn(B, C, H, H, generator=gen) * 3 + 5
    x[0, 0, 0, 0:2] = 20.0            # a tie inside a window's row: the first maximum
    x[0, 1, 2:4, 2] = 21.0            # a tie across a window's two rows
    d = dict(x=x)
    for k in ("g", "b", "rm", "rv", "pg", "pb", "prm", "prv"):
        t = torch.randn(C, generator=gen)
        d[k] = t.abs() + 0.5 if k in ("g", "rv", "pg", "prv") else t
    for k in ("dz", "add1", "add2", "up"):
        d[k] = torch.randn(B, C, H, H, generator=gen)
    d["dpl"] = torch.randn(B, C, H // 2, H // 2, generator=gen)
    d["low"] = torch.randn(B, C, H // 2, H // 2, generator=gen) * 2 + 1
    # float64 reference of the pooled BatchNorm's six outputs
    pl = F.max_pool2d(x.double(), 2, 2)
    mean = pl.mean((0, 2, 3))
    var = pl.var((0, 2, 3), unbiased=False)
    n = pl.numel() // C
    istd = 1.0 / torch.sqrt(var + EPS)
    sc = istd * d["pg"].double()
    d["ref"] = dict(mean=mean, invstd=istd, scale=sc, shift=d["pb"].double() - mean * sc,
                    rmean=MOM * mean + (1 - MOM) * d["prm"].double(),
                    rvar=MOM * var * n / (n - 1) + (1 - MOM) * d["prv"].double())
    d = {k: (v.to(DEV) if torch.is_tensor(v) else {n: t.to(DEV) for n, t in v.items()}) for k, v in d.items()}
    _CASES[shape] = d
    return d


def _bn(d, C, pooled):
    """(gamma, beta, rmean, rvar, mean, invstd, scale, shift) with fresh outputs and fresh
    copies of the running statistics."""
    k = ("pg", "pb", "prm", "prv") if pooled else ("g", "b", "rm", "rv")
    return (d[k[0]], d[k[1]], d[k[2]].clone(), d[k[3]].clone()) + tuple(torch.empty(C, device=DEV) for _ in range(4))


def _stats_sep(x, bn, part):
    from ubpl_amd import kernels as Kn
    g, b, rm, rv, mean, istd, sc, sh = bn
    Kn.bn_forward_stats(x, g, b, EPS, MOM, rm, rv, part, mean, istd, sc, sh)


NAMES = ("rmean", "rvar", "mean", "invstd", "scale", "shift")


def _six(bn):
    return dict(zip(NAMES, bn[2:]))


def _err(bn, ref):
    """Largest error of the six outputs against float64, each relative to its largest reference value."""
    six = _six(bn)
    return max(float((six[k].double().cpu() - ref[k].cpu()).abs().max() / ref[k].abs().max()) for k in NAMES)


@pytest.mark.parametrize("shape", SHAPES)
def test_stats_maxpool_vs_separate_launches(shape):
    from ubpl_amd import kernels as Kn
    B, C, H = shape
    d = _case(shape)
    x = d["x"]
    part = Kn.bn_part(B, C, DEV)
    xs, ps = _bn(d, C, False), _bn(d, C, True)
    _stats_sep(x, xs, part)
    pl_ref = Kn.maxpool2x2(x)
    _stats_sep(pl_ref, ps, part)
    # twice in a row on one scratch (the tickets reset), fresh running statistics each time
    for rep in range(2):
        xf, pf = _bn(d, C, False), _bn(d, C, True)
        pl = Kn.bn_forward_stats_maxpool(x, xf, pf, EPS, MOM, part)
        _same(pl, pl_ref, "pooled tensor (call %d)" % rep)
        for k in NAMES:
            _same(_six(xf)[k], _six(xs)[k], "x %s (call %d)" % (k, rep))
        ef, es = _err(pf, d["ref"]), _err(ps, d["ref"])
        print("shape %s call %d: pooled BatchNorm error vs float64: fused %.3e, separate %.3e" % (shape, rep, ef, es))
        # (4x4, the shape added here: 8 pooled values a channel, both sums exact to a few f32
        # roundings, so what is compared is how the f32 outputs happen to round — shift alone
        # is two f32 roundings, a product and a difference — and a ratio of such errors is
        # noise; it gets one f32 ulp, 2^-23, beside the factor.  The five shapes above: no floor)
        floor = 2.0 ** -23 if shape == SHAPES[-1] else 0.0
        assert ef <= 2 * es + floor, "pooled BatchNorm vs float64: fused %.3e, separate launches %.3e" % (ef, es)
        # test_bn_forward_backward_vs_torch's bars
        r, six = d["ref"], _six(pf)
        y = pl_ref * six["scale"].view(1, C, 1, 1) + six["shift"].view(1, C, 1, 1)
        yr = (pl_ref.double() * r["scale"].view(1, C, 1, 1) + r["shift"].view(1, C, 1, 1)).float()
        torch.testing.assert_close(y, yr, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(six["rmean"], r["rmean"].float(), rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(six["rvar"], r["rvar"].float(), rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(six["mean"], r["mean"].float(), rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(six["invstd"], r["invstd"].float(), rtol=1e-5, atol=1e-6)
    # the x statistics left out (the stem's pool): same pooled tensor, same pooled statistics
    pn = _bn(d, C, True)
    pl = Kn.bn_forward_stats_maxpool(x, None, pn, EPS, MOM, part)
    _same(pl, pl_ref, "pooled tensor (no x statistics)")
    for k in NAMES:
        _same(_six(pn)[k], _six(pf)[k], "pooled %s (no x statistics)" % k)
    # the pooled statistics left out (the default model path): same pooled tensor, same x statistics
    xo = _bn(d, C, False)
    pl = Kn.bn_forward_stats_maxpool(x, xo, None, EPS, MOM, part)
    _same(pl, pl_ref, "pooled tensor (no pooled statistics)")
    for k in NAMES:
        _same(_six(xo)[k], _six(xs)[k], "x %s (no pooled statistics)" % k)
    # the scratch is back at rest: a plain statistics launch on it still agrees
    xa = _bn(d, C, False)
    _stats_sep(x, xa, part)
    for k in NAMES:
        _same(_six(xa)[k], _six(xs)[k], "x %s after the fused calls" % k)


@pytest.mark.parametrize("shape", SHAPES)
def test_stats_maxpool_nan_wins_like_maxpool(shape):
    from ubpl_amd import kernels as Kn
    B, C, H = shape
    d = _case(shape)
    x = d["x"].clone()
    x[1, 1, 1, 1] = float("nan")
    x[B - 1, C - 1, H - 2, H - 1] = float("nan")
    pl = Kn.bn_forward_stats_maxpool(x, None, _bn(d, C, True), EPS, MOM, Kn.bn_part(B, C, DEV))
    ref = Kn.maxpool2x2(x)
    assert int(torch.isnan(ref).sum()) == 2
    _same(pl, ref, "pooled tensor with NaNs")


@pytest.mark.parametrize("shape", SHAPES)
def test_upsample_add_bnstats_vs_separate_launches(shape):
    from ubpl_amd import kernels as Kn
    B, C, H = shape
    d = _case(shape)
    up, low = d["up"], d["low"]
    part = Kn.bn_part(B, C, DEV)
    out_ref = Kn.upsample2x_add(up, low)
    ref = _bn(d, C, False)
    _stats_sep(out_ref, ref, part)
    for inplace in (False, True):
        bn = _bn(d, C, False)
        src = up.clone()
        out = Kn.upsample2x_add_bnstats(src, low, bn, EPS, MOM, part, out=src if inplace else None)
        assert (out.data_ptr() == src.data_ptr()) == inplace
        _same(out, out_ref, "sum (in place: %s)" % inplace)
        if not inplace:
            _same(src, up, "up after the out-of-place call")
        for k in NAMES:
            _same(_six(bn)[k], _six(ref)[k], "%s (in place: %s)" % (k, inplace))


@pytest.mark.parametrize("shape", SHAPES)
def test_bn_backward_pool_vs_three_launches(shape):
    from ubpl_amd import kernels as Kn
    B, C, H = shape
    d = _case(shape)
    x = d["x"]
    part = Kn.bn_part(B, C, DEV)
    bn = _bn(d, C, False)
    _stats_sep(x, bn, part)
    g, _, _, _, mean, istd, sc, sh = bn
    coef = torch.empty(3 * C, device=DEV)

    def run(fused, a1, pd, a2, alias):
        dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        dz = d["dz"].clone()
        out = None if alias else torch.empty_like(dz)
        if fused:
            dx = Kn.bn_backward_pool(dz, x, g, mean, istd, sc, sh, 1, part, coef, dg, db, add1=a1, pool_dy=pd,
                                     add2=a2, out=out)
        else:
            dx = Kn.bn_backward(dz, x, g, mean, istd, sc, sh, 1, part, coef, dg, db, add1=a1, out=out)
            if pd is not None:
                Kn.maxpool2x2_backward(x, pd, dx, accumulate=True)
            if a2 is not None:
                Kn.add(dx, a2, out=dx)
        assert (dx.data_ptr() == dz.data_ptr()) == alias
        return dx, dg, db

    dg0 = None
    for a1, pd, a2, alias in [(d["add1"], d["dpl"], d["add2"], True), (d["add1"], d["dpl"], d["add2"], False),
                              (None, d["dpl"], d["add2"], True), (d["add1"], d["dpl"], None, True),
                              (None, d["dpl"], None, False), (d["add1"], None, d["add2"], True)]:
        what = "add1 %s pool_dy %s add2 %s alias %s" % (a1 is not None, pd is not None, a2 is not None, alias)
        dx, dg, db = run(True, a1, pd, a2, alias)
        rx, rg, rb = run(False, a1, pd, a2, alias)
        _same(dx, rx, "dx (%s)" % what)
        _same(dg, rg, "dgamma (%s)" % what)
        _same(db, rb, "dbeta (%s)" % what)
        if dg0 is None:
            dg0 = (dg, db)
        _same(dg, dg0[0], "dgamma across the variants")
        _same(db, dg0[1], "dbeta across the variants")


def _model_run(fuse, monkeypatch, imgs, dpreds):
    from ubpl_amd import _lib, hourglass as HG, hourglass_exec
    monkeypatch.setattr(hourglass_exec, "_POOL_FUSE", fuse)      # (the executor's module reads the flag)
    torch.manual_seed(0)
    model = HG.StackedHourglass(16, 2, "default")
    model.train()
    # the library calls of one forward + backward, counted at the wrappers' one way in
    real, log = _lib.call, []
    monkeypatch.setattr(_lib, "call", lambda name, *a: (log.append(name), real(name, *a))[1])
    preds = model(imgs.to(DEV))
    preds.backward(dpreds.to(DEV))
    torch.cuda.synchronize()
    monkeypatch.setattr(_lib, "call", real)
    grads = {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.grad is not None}
    return preds.detach().double().cpu(), grads, log


def _model_compare(monkeypatch, res):
    """One train-mode forward + backward (K=16, HG2, B=2, res x res input) at UBPL_POOL_FUSE
    levels 2, 1 and 0 and on the fp32 / fp64 oracle -> (figures printed, the runs)."""
    import seeds
    from oracle import hourglass as OH
    gen = torch.Generator().manual_seed(5)
    imgs = torch.rand(2, 3, res, res, generator=gen) - 0.5
    dpreds = torch.randn(2, 2, 16, res // 4, res // 4, generator=gen) / 64
    ref = {}
    for dt in (torch.float32, torch.float64):
        torch.manual_seed(0)
        params = {n: t.to(dt) for n, t in OH.init_params(16, 2).items()}
        o = OH.OracleHourglass(16, 2, "default", params=params).requires_grad_(True)
        o.buf = {n: (t.to(dt) if t.is_floating_point() else t) for n, t in o.buf.items()}
        p = o(imgs.to(dt))
        p.backward(dpreds.to(dt))
        ref[dt] = (p.detach().double(), {n: t.grad.double() for n, t in o.named_parameters() if t.grad is not None})
    p32, g32 = ref[torch.float32]
    p64, g64 = ref[torch.float64]
    runs = {f: _model_run(f, monkeypatch, imgs, dpreds) for f in (2, 1, 0)}
    names = [n for n, gg in g64.items() if not seeds.bn_cancelled(n) and float(gg.norm()) > 0]
    rel = lambda a, b, n: float((a[n] - b[n]).norm() / max(float(b[n].norm()), 1e-30))
    # what the fusion changes
    nl = {f: len(runs[f][2]) for f in runs}
    for f in (1, 2):
        pd = float((runs[f][0] - runs[0][0]).abs().max())
        gd = np.array([rel(runs[f][1], runs[0][1], n) for n in names])
        print("%dx%d fusion %d vs 0: max |dpred| %.3e (max |pred| %.3e), relative gradient difference median %.3e "
              "max %.3e; library calls per forward + backward: %d against %d"
              % (res, res, f, pd, float(p64.abs().max()), np.median(gd), gd.max(), nl[f], nl[0]))
    out = {}
    er = np.array([rel(g32, g64, n) for n in names])
    for f, (pr, grads, _) in runs.items():
        ok = np.abs(pr - p64).numpy() <= 3 * np.abs(p32 - p64).numpy() + 1e-4 * float(p64.abs().max()) + 1e-12
        eo = np.array([rel(grads, g64, n) for n in names])
        p90 = np.percentile(er, 90)
        bad = [(n, a, b) for n, a, b in zip(names, eo, er) if a > 3 * max(b, p90) + 1e-4]
        print("%dx%d fusion %d: max |pred - fp64| %.3e (fp32 oracle %.3e), %d of %d predictions over the bar; gradient "
              "error vs fp64 median %.3e (fp32 oracle %.3e), max %.3e (fp32 oracle %.3e), %d tensors over their bar"
              % (res, res, f, float((pr - p64).abs().max()), float((p32 - p64).abs().max()), int((~ok).sum()), ok.size,
                 np.median(eo), np.median(er), eo.max(), er.max(), len(bad)))
        out[f] = (ok, eo, er, bad)
    return out, runs


def test_model_fused_vs_unfused_train_step(monkeypatch):
    """K=16, HG2, B=2, 128x128 input, train mode, UBPL_POOL_FUSE levels 2, 1 and 0.

    Level 1, the default, folds only what is bit-identical to the separate launches: its
    predictions and every parameter gradient must EQUAL level 0's, bit for bit.  Level 2 also
    takes the pooled tensor's statistics in the pooling kernel, in a new summation order; it
    and the other two are held against the float64 oracle with the bars
    tests/test_gpu_train.py puts on the eager step (predictions: |ours - fp64| <= 3 |fp32
    oracle - fp64| + 1e-4 max|fp64|; gradients: check_full_grads' median and per-tensor
    bars).  Every figure is printed before the assertions.

    128x128 is the smallest input with a defined answer at B=2: at 64x64 the innermost
    hourglass planes are 1x1, BatchNorm there normalises two samples to +-1, and the
    network is a coin toss — the fp32 oracle itself sits 0.42 from the fp64 oracle on
    predictions of magnitude 1.9, and the separate launches miss the same bar on 1756 of
    16384 predictions.  Measured at 128x128 on MI355X, level 2 vs 0: max |dpred| 5.4e-5,
    relative gradient difference median 2.4e-2 (the fp32 oracle's own gradient error against
    fp64 is 1.9e-2 at this B=2: the backward amplifies any rounding); errors against fp64,
    level 2 / level 0 / fp32 oracle: predictions 1.31e-4 / 1.21e-4 / 2.07e-4, median gradient
    2.96e-2 / 1.51e-2 / 1.93e-2, worst tensor 4.1e-2 / 3.3e-2 / 3.5e-2; 557 against 591
    library calls per forward + backward."""
    out, runs = _model_compare(monkeypatch, 128)
    nl = {f: len(runs[f][2]) for f in runs}
    assert nl[2] < nl[1] < nl[0], nl
    for f in (1, 2):
        fused_calls = set(runs[f][2]) - set(runs[0][2])
        assert fused_calls == {"ubpl_bn_forward_stats_maxpool", "ubpl_upsample2x_add_forward_bnstats",
                               "ubpl_bn_backward_pool"}, (f, fused_calls)
    assert torch.equal(runs[1][0], runs[0][0]), "level 1 predictions differ from the separate launches'"
    for n, g in runs[0][1].items():
        assert torch.equal(runs[1][1][n], g), "level 1 gradient of %s differs from the separate launches'" % n
    for f, (ok, eo, er, bad) in out.items():
        assert ok.all(), ("predictions", f, int((~ok).sum()))
        assert np.median(eo) <= 3.5 * np.median(er) + 1e-5, (f, np.median(eo), np.median(er))
        assert not bad, (f, bad[:6])
