"""Guarded optimizer step, host side: the guard's arithmetic as restated in
guard_ref against torch.nn.utils.clip_grad_norm_, and the new C-ABI entries as
the header's one parser sees them."""
import os

import numpy as np
import pytest
import torch

from f16_split_ref import fp16_wscale as _fp16_wscale
from guard_ref import guard_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ubpl_hip.h")


def _params(seed, dtype):
    g = torch.Generator().manual_seed(seed)
    ps = []
    for shape in [(64, 3, 7, 7), (64,), (128, 64), (17,), (3,)]:
        p = torch.zeros(shape, dtype=dtype, requires_grad=True)
        p.grad = (torch.randn(shape, generator=g) * 0.3).to(dtype)
        ps.append(p)
    return ps


@pytest.mark.parametrize("factor", [0.5, 0.013, 2.0, 100.0])
def test_restatement_matches_clip_grad_norm(factor):
    """max_norm = factor * norm, below and above the norm.  clip_grad_norm_ on float64
    gradients (the same values) applies the coefficient the restatement gives, to
    float64 rounding; on float32 gradients, to float32 rounding (torch forms the norm
    and the coefficient in float32 there)."""
    flat = torch.cat([p.grad.reshape(-1) for p in _params(7, torch.float32)])
    max_norm = factor * float(flat.double().norm())
    c, norm, skip = guard_ref(flat, max_norm)
    assert not skip
    assert (c == np.float32(1.0)) == (factor >= 1)
    for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 4 * 2.0 ** -24)):
        ps = _params(7, dtype)
        before = torch.cat([p.grad.reshape(-1) for p in ps]).clone()
        total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
        after = torch.cat([p.grad.reshape(-1) for p in ps])
        assert abs(float(total) - float(norm)) <= max(tol, 2.0 ** -24) * float(norm)
        applied = float((after.double() * before.double()).sum() / (before.double() ** 2).sum())
        assert abs(applied - float(c)) <= max(tol, 2.0 ** -24) * float(c), (dtype, applied, float(c))
        if factor >= 1:
            assert torch.equal(after, before)
    if factor < 1:
        # in float64 the applied coefficient rounds to the restatement's float32
        ps = _params(7, torch.float64)
        before = torch.cat([p.grad.reshape(-1) for p in ps]).clone()
        torch.nn.utils.clip_grad_norm_(ps, max_norm)
        k = int(before.abs().argmax())
        applied = float(torch.cat([p.grad.reshape(-1) for p in ps])[k] / before[k])
        assert abs(applied - float(c)) <= 2.0 ** -24 * float(c)


def test_restatement_flags_and_off():
    g = torch.randn(1028, generator=torch.Generator().manual_seed(1))
    assert guard_ref(g, 0.0)[0] == np.float32(1.0) and guard_ref(g, -1.0)[0] == np.float32(1.0)
    assert not guard_ref(torch.full((1028,), 1e30), 1.0)[2]          # finite: f32 squares fit f64
    for bad in (float("inf"), float("-inf"), float("nan")):
        h = g.clone()
        h[77] = bad
        c, _, skip = guard_ref(h, 1.0)
        assert skip and c == np.float32(1.0)
    assert guard_ref(torch.zeros(0), 1.0) == (np.float32(1.0), np.float32(0.0), False)


def test_header_declares_guard_entries():
    from ubpl_amd import _abi
    decls = {name: (ret, params, ann) for ret, name, params, ann in _abi.parse(open(HEADER).read())}
    ret, params, ann = decls["ubpl_grad_guard_scratch"]
    assert ret == "int64_t" and params == [("int64_t", "n")] and not any(map(_abi.is_stream, params))
    ret, params, ann = decls["ubpl_grad_guard"]
    assert [p for _, p in params] == ["g", "n", "max_norm", "part", "guard", "stream"]
    assert ann == {"g": ("f32", "n"), "part": ("f64", "ubpl_grad_guard_scratch(n)"), "guard": ("f32", "4")}
    assert dict((p, t) for t, p in params)["g"].startswith("const")
    for name, base in (("ubpl_adamw_step_guarded_dev", "ubpl_adamw_step_dev"),
                       ("ubpl_adamw_ema_step_guarded_dev", "ubpl_adamw_ema_step_dev")):
        _, params, ann = decls[name]
        _, bparams, bann = decls[base]
        # the unguarded entry's arguments, then guard and skipped, then the stream
        assert params == bparams[:-1] + [("const float*", "guard"), ("int64_t*", "skipped")] + bparams[-1:]
        assert ann == dict(bann, guard=("f32", "4"), skipped=("i64", "2"))
    _, params, ann = decls["ubpl_restore_if"]
    assert [p for _, p in params] == ["dst", "saved", "n", "guard", "stream"]
    assert ann == {"dst": ("f32", "n"), "saved": ("f32", "n"), "guard": ("f32", "4")}
    # the derived op layer: the guard is read-only, the counters are written
    src = _abi.gen(_abi.parse(open(HEADER).read()))
    assert 'm.def("grad_guard_scratch(int n) -> int");' in src
    assert "Tensor? guard, Tensor(a5!)? skipped) -> ()" in src


def test_fp16_overflow_plant_arithmetic():
    """What test_gpu_guard_train.py plants: w = 8 in a 64-channel 3x3 conv (K = 576)
    scales to 2^17, past fp16's largest finite value, so its fp16 piece is inf and the
    remainder -inf; the default-init bound 1/sqrt(K) stays far inside."""
    common = open(os.path.join(ROOT, "ubpl-poseestimation_amd", "csrc", "common.h")).read()
    assert "while ((1 << (2 * e)) < K) ++e;" in common and "(float)(1 << (9 + e))" in common
    assert "FP16_ACT_SCALE = 32.f" in common
    sc = _fp16_wscale(576)
    assert sc == 2.0 ** 14
    hi = torch.tensor(8.0 * sc).half()
    assert torch.isinf(hi) and torch.isinf((torch.tensor(8.0 * sc) - hi.float()).half())
    assert torch.isfinite(torch.tensor(3.99 * sc).half())          # |w| <= 65504 / 2^14 = 3.998
    assert torch.isfinite(torch.tensor(576 ** -0.5 * sc).half())
    assert torch.isfinite(torch.tensor(2047.0 * 32).half()) and torch.isinf(torch.tensor(2048.0 * 32).half())
