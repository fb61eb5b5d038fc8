"""The guarded step inside train_mt_ubpl (args.maxGradNorm / skipNonFinite /
maxSkippedSteps) on the smallest MT_UBPL step: two 1-stack hourglasses and
their teachers at 128x128, B = 4 (2 unlabeled + 2 labeled rows), 4 keypoints,
seeded as test_gpu_train.py seeds its steps; at the end the NaN case once for each
of the other three train() flavours at the same size.

Everything compared here is compared bit for bit: the guard adds no arithmetic
to a step it lets through, and a skipped step writes nothing but the teachers
(the EMA toward the unchanged students) and the counters.
"""
import contextlib
import copy
import io

import pytest
import torch

import seeds
from guard_ref import guard_ref
from oracle import render as OR

pytestmark = pytest.mark.gpu
CFG = dict(seeds.step_cases()["mt_ubpl"], S=1, K=4, res=128, out=32, seed=611)
PLANT = "pre.1.conv2.conv.weight"          # 64 -> 64 channels, 3x3: K = 576, fp16_wscale = 2^14


def _factory(k, s, mode):
    from ubpl_amd.hourglass import StackedHourglass
    return StackedHourglass(k, s, mode)


_BATCH = {}


def _batch():
    """The seeded (batch, args) pair, rendered once."""
    if not _BATCH:
        loader, args = seeds.step_batch(CFG, OR.kps_heatmap_torch)
        _BATCH["v"] = (loader[0], args)
    batch, args = _BATCH["v"]
    return copy.deepcopy(batch), copy.copy(args)


def _poisoned(batch):
    imgs, hms, meta = copy.deepcopy(batch)
    imgs[0][1, 2, 5, 7] = float("nan")                     # one pixel of one image of view 0
    return imgs, hms, meta


def _setup(**opts):
    from ubpl_amd.optim import FlatAdamW
    models, emas, _ = seeds.step_models(_factory, CFG, device="cuda")
    optims = [FlatAdamW(m, lr=CFG["lr"], weight_decay=0) for m in models]
    batch, args = _batch()
    for k, v in opts.items():
        setattr(args, k, v)
    return models, emas, optims, batch, args


def _train(loader, models, emas, optims, args):
    from ubpl_amd import train as T
    with contextlib.redirect_stdout(io.StringIO()):
        rec = T.train_mt_ubpl(loader, models, emas, optims, args)
    torch.cuda.synchronize()
    return rec


def _state(models, emas, optims):
    st = {}
    for i, m in enumerate(models + emas):
        st["params%d" % i] = m.flat_params.detach().clone()
        st["stats%d" % i] = m.flat_stats.detach().clone()
    for i, o in enumerate(optims):
        st["m%d" % i], st["v%d" % i], st["step%d" % i] = o.exp_avg.clone(), o.exp_avg_sq.clone(), o._step_t.clone()
    return st


def _eq(a, b):
    if a.dtype.is_floating_point:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


@pytest.fixture
def eager(monkeypatch):
    from ubpl_amd import train as T
    monkeypatch.setenv("UBPL_STEP_GRAPH", "0")
    T._StepGraph.clear()
    yield
    T._StepGraph.clear()


@pytest.fixture
def graphed(monkeypatch):
    from ubpl_amd import train as T
    monkeypatch.setenv("UBPL_MODEL_STREAMS", "1")
    monkeypatch.setenv("UBPL_STEP_GRAPH", "1")
    T._StepGraph.clear()
    yield
    T._StepGraph.clear()


def _run_steps(nsteps, **opts):
    models, emas, optims, batch, args = _setup(**opts)
    _train([batch] * nsteps, models, emas, optims, args)
    return models, emas, optims, args


# (1) ------------------------------------------------------------------------
def test_guard_with_nothing_to_guard_changes_nothing_eager(eager):
    off = _state(*_run_steps(1)[:3])
    models, emas, optims, _ = _run_steps(1, maxGradNorm=1e9, skipNonFinite=True)
    on = _state(models, emas, optims)
    for k in off:
        assert _eq(off[k], on[k]), k
    for o in optims:
        assert o.guarded and (o.skipped_steps, o.consecutive_skipped, o.step_count) == (0, 0, 1)
        assert 0 < o.last_grad_norm < float("inf") and o.last_clip_coef == 1.0


def test_guard_with_nothing_to_guard_changes_nothing_captured(graphed):
    """Two eager warm-up steps, the capture with its first replay, one more replay."""
    from ubpl_amd import train as T
    off = _state(*_run_steps(4)[:3])
    T._StepGraph.clear()
    models, emas, optims, args = _run_steps(4, maxGradNorm=1e9, skipNonFinite=True)
    runner = T._StepGraph.get(T._mt_ubpl_core, models, emas, optims, args)
    assert runner.graph is not None and runner.n_eager == T._StepGraph.WARM
    on = _state(models, emas, optims)
    for k in off:
        assert _eq(off[k], on[k]), k
    for o in optims:
        assert (o.skipped_steps, o.consecutive_skipped, o.step_count) == (0, 0, 4)


# (2), (3) -------------------------------------------------------------------
def _check_skipped_branch(bi, before, after, models, emas, optims, args):
    """Branch bi after a skipped step: student, moments, step count and both networks'
    BatchNorm statistics as before; the teacher moved toward the unchanged student."""
    from ubpl_amd import kernels as Kn
    from ubpl_amd.parameters import ema_alpha
    M = len(models)
    for k in ("params%d" % bi, "m%d" % bi, "v%d" % bi, "step%d" % bi, "stats%d" % bi, "stats%d" % (M + bi)):
        assert _eq(before[k], after[k]), k
    want = before["params%d" % (M + bi)].clone()
    Kn.ema_update_(want, before["params%d" % bi], ema_alpha(args.epo, args.ema_decay))
    torch.cuda.synchronize()
    assert _eq(want, after["params%d" % (M + bi)])
    assert not _eq(before["params%d" % (M + bi)], after["params%d" % (M + bi)])
    assert (optims[bi].skipped_steps, optims[bi].consecutive_skipped) == (1, 1)


def _check_clean_step_after(bi, before, models, emas, optims):
    after = _state(models, emas, optims)
    M = len(models)
    for k in ("params%d" % bi, "m%d" % bi, "v%d" % bi, "stats%d" % bi, "params%d" % (M + bi), "stats%d" % (M + bi)):
        assert bool(torch.isfinite(after[k]).all()), k
    assert after["step%d" % bi].item() == before["step%d" % bi].item() + 1
    assert not _eq(before["params%d" % bi], after["params%d" % bi])
    assert not _eq(before["stats%d" % bi], after["stats%d" % bi])
    assert (optims[bi].skipped_steps, optims[bi].consecutive_skipped) == (1, 0)


def test_nan_input_skips_the_step_and_training_goes_on(eager):
    """One NaN pixel: on the parent commit every weight, moment, teacher and running
    statistic is NaN after this step."""
    models, emas, optims, batch, args = _setup(skipNonFinite=True)
    _train([batch], models, emas, optims, args)             # a clean step first: moments and counts set
    before = _state(models, emas, optims)
    _train([_poisoned(batch)], models, emas, optims, args)
    after = _state(models, emas, optims)
    for bi in range(len(models)):
        _check_skipped_branch(bi, before, after, models, emas, optims, args)
        assert optims[bi].step_count == 1
        assert not (optims[bi].last_grad_norm < float("inf"))
    _train([batch], models, emas, optims, args)
    for bi in range(len(models)):
        _check_clean_step_after(bi, after, models, emas, optims)


def test_fp16_weight_overflow_skips_that_branch(eager):
    """|w| * fp16_wscale(K) > 65504 in one 3x3 conv of the split path under 2xfp16:
    the fp16 piece is inf, the forward NaN.  (The plant's arithmetic is checked on the
    CPU in test_guard_host.py.)"""
    models, emas, optims, batch, args = _setup(skipNonFinite=True)
    for m in models + emas:
        m.set_conv_precision("2xfp16")
    s, n, shp = models[0]._offs[PLANT]
    assert tuple(shp) == (64, 64, 3, 3)
    with torch.no_grad():
        models[0].flat_params[s + 7] = 8.0                   # 8 * 2^14 = 131072 > 65504
    before = _state(models, emas, optims)
    _train([batch], models, emas, optims, args)
    after = _state(models, emas, optims)
    _check_skipped_branch(0, before, after, models, emas, optims, args)
    assert optims[0].step_count == 0
    # take the plant out of the student and of its teacher: the EMA still ran (alpha = 0.5
    # at epo 1), so the teacher's weight moved to about 4, the edge of its own fp16 range
    with torch.no_grad():
        models[0].flat_params[s + 7] = 0.01
        emas[0].flat_params[s + 7] = 0.01
    after = _state(models, emas, optims)
    _train([batch], models, emas, optims, args)
    _check_clean_step_after(0, after, models, emas, optims)


# (4) ------------------------------------------------------------------------
def test_clipped_step_is_the_unguarded_kernel_on_scaled_gradients(eager):
    from ubpl_amd import kernels as Kn
    first = _run_steps(1, maxGradNorm=1e9)[2]
    norms = [o.last_grad_norm for o in first]
    assert all(0 < v < float("inf") for v in norms)
    max_norm = 0.5 * min(norms)
    models, emas, optims, batch, args = _setup(maxGradNorm=max_norm)
    before = _state(models, emas, optims)
    _train([batch], models, emas, optims, args)
    for bi, (m, o) in enumerate(zip(models, optims)):
        g = m.flat_grads[:m.n_live]                          # the step leaves the gradients as they were
        c, norm, skip = guard_ref(g, max_norm)
        guard = o._guard.cpu()
        assert not skip and guard[2].item() == 0.0 and o.step_count == 1
        assert guard[0].item() == float(c) and float(c) <= 0.5 * (1 + 1e-6)
        assert abs(guard[1].item() - float(norm)) <= 1e-6 * float(norm)
        assert abs(guard[1].item() - norms[bi]) <= 1e-6 * norms[bi]     # the step is deterministic
        p, mm, vv = (before[k % bi].clone() for k in ("params%d", "m%d", "v%d"))
        step, coef = before["step%d" % bi].clone(), torch.zeros(4, device="cuda")
        gs = g.clone()
        Kn.scale_(gs, guard[0].item())
        h = o.param_groups[0]
        Kn.adamw_step_dev_(p[:m.n_live], gs, mm, vv, h["lr"], h["betas"][0], h["betas"][1], h["eps"],
                           h["weight_decay"], step, coef)
        torch.cuda.synchronize()
        assert _eq(p, m.flat_params.detach()) and _eq(mm, o.exp_avg) and _eq(vv, o.exp_avg_sq)
        assert not _eq(p, before["params%d" % bi])


# (5) ------------------------------------------------------------------------
def test_repeated_skips_stop_the_run(graphed):
    models, emas, optims, batch, args = _setup(skipNonFinite=True, maxSkippedSteps=2)
    before = _state(models, emas, optims)
    served = []

    def loader():
        for i in range(6):
            served.append(i)
            yield _poisoned(batch)
    with pytest.raises(FloatingPointError) as e:
        _train(loader(), models, emas, optims, args)
    assert len(served) <= 4                                  # the counts reach the host one step late
    msg = str(e.value)
    assert "2047" in msg and "65504 / fp16_wscale(K)" in msg and "UBPL_CONV_PRECISION=6xbf16" in msg
    torch.cuda.synchronize()
    after = _state(models, emas, optims)
    for bi, o in enumerate(optims):
        assert o.skipped_steps == o.consecutive_skipped >= 2 and o.step_count == 0
        for k in ("params%d" % bi, "m%d" % bi, "v%d" % bi, "stats%d" % bi, "stats%d" % (len(models) + bi)):
            assert _eq(before[k], after[k]), k


def test_guard_needs_flat_adamw(eager):
    models, emas, _, batch, args = _setup(maxGradNorm=1.0)
    torch_optims = [torch.optim.AdamW(m.parameters(), lr=CFG["lr"]) for m in models]
    with pytest.raises(TypeError, match="FlatAdamW"):
        _train([batch], models, emas, torch_optims, args)


# the other three train() flavours ---------------------------------------------
_SMALL = dict(S=1, K=4, res=128, out=32)
FLAVOURS = {"dualpose": dict(seeds.step_cases()["dualpose"], seed=612, **_SMALL),
            "mt": dict(seeds.step_cases()["mt"], seed=613, **_SMALL),
            "sup": dict(seeds.step_cases()["sup"], seed=614, **_SMALL)}


@pytest.mark.parametrize("name", sorted(FLAVOURS))
def test_nan_input_skips_in_every_flavour(name, eager):
    """train_dualpose_ubpl, train_mt and train_supervised read the same options: a NaN
    pixel in the student's image leaves the students, moments, step counts and every
    network's BatchNorm statistics bitwise alone, the teachers (where there are any) move
    toward the unchanged students, and the next clean step trains."""
    from ubpl_amd import kernels as Kn
    from ubpl_amd import train as T
    from ubpl_amd.optim import FlatAdamW
    from ubpl_amd.parameters import ema_alpha
    cfg = FLAVOURS[name]
    models, emas, _ = seeds.step_models(_factory, cfg, device="cuda")
    optims = [FlatAdamW(m, lr=cfg["lr"], weight_decay=0) for m in models]
    loader, args = seeds.step_batch(cfg, OR.kps_heatmap_torch)
    args.skipNonFinite = True
    clean = loader[0]
    bad = copy.deepcopy(clean)
    (bad[0][0] if name == "mt" else bad[0])[1, 2, 5, 7] = float("nan")

    def run(batch):
        with contextlib.redirect_stdout(io.StringIO()):
            if name == "dualpose":
                T.train_dualpose_ubpl([batch], models, emas, optims, args)
            elif name == "mt":
                T.train_mt([batch], models[0], emas[0], optims[0], args)
            else:
                T.train_supervised([batch], models[0], optims[0], args)
        torch.cuda.synchronize()
        return _state(models, emas, optims)

    before = run(clean)
    after = run(bad)
    M = len(models)
    for bi, o in enumerate(optims):
        for k in ("params%d" % bi, "m%d" % bi, "v%d" % bi, "step%d" % bi, "stats%d" % bi):
            assert _eq(before[k], after[k]), k
        assert (o.skipped_steps, o.consecutive_skipped, o.step_count) == (1, 1, 1)
        if emas:
            assert _eq(before["stats%d" % (M + bi)], after["stats%d" % (M + bi)])
            want = before["params%d" % (M + bi)].clone()
            Kn.ema_update_(want, before["params%d" % bi], ema_alpha(args.epo, args.ema_decay))
            torch.cuda.synchronize()
            assert _eq(want, after["params%d" % (M + bi)])
    last = run(clean)
    for bi, o in enumerate(optims):
        assert (o.skipped_steps, o.consecutive_skipped, o.step_count) == (1, 0, 2)
        for k in last:
            assert bool(torch.isfinite(last[k]).all()) if last[k].dtype.is_floating_point else True, k
        assert not _eq(after["params%d" % bi], last["params%d" % bi])
