"""The guarded optimizer step's kernels (csrc/optim.hip): ubpl_grad_guard, the
guarded AdamW entries and ubpl_restore_if, at three sizes — one float4, a
partial last block, and just past the grid cap of 2048 blocks x 256 lanes x 4
floats, where the grid-stride loop takes a second pass."""
import numpy as np
import pytest
import torch

from guard_ref import guard_ref

pytestmark = pytest.mark.gpu
CAP = 2048 * 256 * 4
SIZES = [4, 1028, CAP + 1028]
HYPER = dict(lr=2.5e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2)
ALPHA = 0.5


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


_CLEAN = {}


def _clean(n):
    """A clean random gradient of n floats on the device, made once per size."""
    if n not in _CLEAN:
        _CLEAN[n] = (torch.randn(n, generator=torch.Generator().manual_seed(n % 9973)) * 0.01).cuda()
    return _CLEAN[n]


def _guard(g, max_norm):
    from ubpl_amd import kernels as Kn
    part = Kn.grad_guard_scratch(g.numel(), g.device)
    guard = torch.full((4,), -7.0, device=g.device)
    Kn.grad_guard_(g, max_norm, part, guard)
    return guard.cpu()


# ---------------------------------------------------------------- the guard
@pytest.mark.parametrize("n", SIZES)
def test_guard_clean(n):
    g = _clean(n)
    exact = float(g.double().norm())
    for max_norm in (0.5 * exact, 3.0 * exact, 0.0):
        out = _guard(g, max_norm)
        c, norm, skip = guard_ref(g, max_norm)
        assert out[2].item() == 0.0 and out[3].item() == 0.0 and not skip
        assert abs(out[1].item() - exact) <= 1e-6 * exact
        assert np.float32(out[0].item()).tobytes() == c.tobytes(), (out[0].item(), float(c))
    assert _guard(g, 3.0 * exact)[0].item() == 1.0 and _guard(g, 0.0)[0].item() == 1.0
    assert _guard(g, 0.5 * exact)[0].item() < 1.0


@pytest.mark.parametrize("n", SIZES)
def test_guard_nonfinite_planted(n):
    places = [0, n - 1, CAP + 500 if n > CAP else n // 2]
    for bad in (float("inf"), float("-inf"), float("nan")):
        for i in places:
            g = _clean(n).clone()
            g[i] = bad
            out = _guard(g, 1.0)
            assert out[2].item() == 1.0, (bad, i)
            assert out[0].item() == 1.0 and out[3].item() == 0.0


@pytest.mark.parametrize("n", SIZES)
def test_guard_large_finite_is_not_skipped(n):
    out = _guard(torch.full((n,), 1e30, device="cuda"), 1.0)
    assert out[2].item() == 0.0
    assert abs(out[1].item() - 1e30 * np.sqrt(n)) <= 1e-6 * 1e30 * np.sqrt(n)


@pytest.mark.parametrize("n", SIZES)
def test_guard_is_deterministic(n):
    g = _clean(n)
    exact = float(g.double().norm())
    assert _same(_guard(g, 0.37 * exact), _guard(g, 0.37 * exact))


def test_guard_empty_and_invalid_arguments():
    from ubpl_amd import kernels as Kn
    base = _clean(1028)
    assert _guard(base[:0], 1.0).tolist() == [1.0, 0.0, 0.0, 0.0]
    part = Kn.grad_guard_scratch(1028, base.device)
    guard = torch.zeros(4, device=base.device)
    with pytest.raises(RuntimeError):
        Kn.grad_guard_(base[1:5], 1.0, part, guard)          # 4 floats, 4 bytes off a 16-B boundary
    with pytest.raises(RuntimeError):
        Kn.grad_guard_(base[:6], 1.0, part, guard)           # aligned, n % 4 != 0
    torch.cuda.synchronize()
    assert guard.cpu().tolist() == [0.0] * 4                 # refused before anything ran


# ---------------------------------------------------------------- guarded steps
def _state(nlive, n):
    g = torch.Generator().manual_seed(nlive % 9973 + 1)
    dev = "cuda"
    return dict(p=torch.randn(n, generator=g).to(dev), g=(torch.randn(nlive, generator=g) * 0.01).to(dev),
                m=(torch.randn(nlive, generator=g) * 0.01).to(dev),
                v=(torch.rand(nlive, generator=g) * 1e-4).to(dev),
                ema=torch.randn(n, generator=g).to(dev), step=torch.full((), 3, dtype=torch.int64, device=dev),
                coef=torch.zeros(4, device=dev))


def _clone(s):
    return {k: v.clone() for k, v in s.items()}


def _run(s, fused, guard=None, skipped=None):
    """One AdamW step on state s in place: fused with the EMA or on the live prefix
    alone; guarded when guard is given."""
    from ubpl_amd import kernels as Kn
    h = (HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"], HYPER["weight_decay"])
    nlive = s["g"].numel()
    if fused:
        if guard is None:
            Kn.adamw_ema_step_dev_(s["p"], s["g"], s["m"], s["v"], nlive, *h, s["step"], s["coef"], s["ema"], ALPHA)
        else:
            Kn.adamw_ema_step_guarded_dev_(s["p"], s["g"], s["m"], s["v"], nlive, *h, s["step"], s["coef"],
                                           s["ema"], ALPHA, guard, skipped)
    elif guard is None:
        Kn.adamw_step_dev_(s["p"][:nlive], s["g"], s["m"], s["v"], *h, s["step"], s["coef"])
    else:
        Kn.adamw_step_guarded_dev_(s["p"][:nlive], s["g"], s["m"], s["v"], *h, s["step"], s["coef"], guard, skipped)
    torch.cuda.synchronize()


def _assert_state(a, b, keys=("p", "m", "v", "ema", "step", "coef")):
    for k in keys:
        if a[k].dtype == torch.int64:
            assert torch.equal(a[k], b[k]), k
        else:
            assert _same(a[k], b[k]), k


STEP_SIZES = [(1028, 1032), (CAP + 1028, CAP + 1032)]      # (nlive, n): a dead tail of one float4


@pytest.mark.parametrize("nlive,n", STEP_SIZES)
@pytest.mark.parametrize("fused", [True, False])
def test_guarded_step_c1_is_the_unguarded_step(nlive, n, fused):
    s0 = _state(nlive, n)
    ref, got = _clone(s0), _clone(s0)
    _run(ref, fused)
    skipped = torch.zeros(2, dtype=torch.int64, device="cuda")
    _run(got, fused, torch.tensor([1.0, 5.0, 0.0, 0.0], device="cuda"), skipped)
    _assert_state(got, ref)
    assert got["step"].item() == 4 and skipped.tolist() == [0, 0]
    assert not _same(got["p"], s0["p"])


@pytest.mark.parametrize("nlive,n", STEP_SIZES)
@pytest.mark.parametrize("fused", [True, False])
def test_guarded_step_clip_is_scale_then_step(nlive, n, fused):
    from ubpl_amd import kernels as Kn
    s0 = _state(nlive, n)
    ref, got = _clone(s0), _clone(s0)
    guard = torch.tensor([0.37, 5.0, 0.0, 0.0], device="cuda")
    Kn.scale_(ref["g"], guard[0].item())                    # the f32 coefficient, exactly
    _run(ref, fused)
    skipped = torch.zeros(2, dtype=torch.int64, device="cuda")
    _run(got, fused, guard, skipped)
    _assert_state(got, ref)
    assert _same(got["g"], s0["g"]) and not _same(ref["g"], s0["g"])       # g itself is not written
    assert skipped.tolist() == [0, 0]


@pytest.mark.parametrize("nlive,n", STEP_SIZES)
@pytest.mark.parametrize("fused", [True, False])
def test_guarded_step_skip(nlive, n, fused):
    from ubpl_amd import kernels as Kn
    s0 = _state(nlive, n)
    got = _clone(s0)
    got["g"][nlive // 2] = float("nan")
    skipped = torch.zeros(2, dtype=torch.int64, device="cuda")
    _run(got, fused, torch.tensor([1.0, float("nan"), 1.0, 0.0], device="cuda"), skipped)
    _assert_state(got, s0, ("p", "m", "v", "step", "coef"))
    ema = s0["ema"].clone()
    if fused:
        Kn.ema_update_(ema, s0["p"], ALPHA)                  # the teacher moves toward the unchanged student
    assert _same(got["ema"], ema)
    assert skipped.tolist() == [1, 1]
    # a clean step afterwards: it runs, and the consecutive count returns to zero
    got["g"].copy_(s0["g"])
    ref = _clone(got)
    _run(ref, fused)
    _run(got, fused, torch.tensor([1.0, 5.0, 0.0, 0.0], device="cuda"), skipped)
    _assert_state(got, ref)
    assert skipped.tolist() == [1, 0] and got["step"].item() == 4


# ---------------------------------------------------------------- restore_if
@pytest.mark.parametrize("n", [4, 1027, 1028, CAP + 1028])
def test_restore_if_both_ways(n):
    from ubpl_amd import kernels as Kn
    g = torch.Generator().manual_seed(5)
    dst0, saved = torch.randn(n, generator=g).cuda(), torch.randn(n, generator=g).cuda()
    dst = dst0.clone()
    Kn.restore_if_(dst, saved, torch.tensor([1.0, 2.0, 0.0, 0.0], device="cuda"))
    torch.cuda.synchronize()
    assert _same(dst, dst0)
    Kn.restore_if_(dst, saved, torch.tensor([1.0, float("inf"), 1.0, 0.0], device="cuda"))
    torch.cuda.synchronize()
    assert _same(dst, saved)
