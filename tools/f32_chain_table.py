#!/usr/bin/env python
"""Recompute the table in tests/f32_chain_ref.py's docstring: e_chain / (sqrt(K) * 2^-24) of the
f32 fma chain alone, on the operand distributions of tests/test_gpu_split.py and
tests/test_gpu_f16_range.py.  CPU only; at most two images per case, forward planes clipped to
CLIP x CLIP and the gradients' K = B*P to at most 8192 (the ratio does not depend on either).

    python tools/f32_chain_table.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

_ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [os.path.join(_ROOT, "tests"), _ROOT]
import f32_chain_ref as C                                    # noqa: E402

CLIP = 16
rows = []


def note(group, tag, K, e):
    r = C.yardstick_ratio(e, K)
    rows.append((group, K, r))
    print("%-18s %-52s K %6d  ratio %.3f" % (group, tag, K, r), flush=True)


def fwd_randn(group, case, KS, pro, resid, seed, stem=False):
    B, Cin, H, Cout = case
    B, H = min(B, 2), min(H, CLIP * (2 if stem else 1))
    gen = torch.Generator().manual_seed(seed)
    K = Cin * KS * KS
    x = (torch.rand(B, Cin, H, H, generator=gen) - 0.5) if stem else torch.randn(B, Cin, H, H, generator=gen)
    w = torch.randn(Cout, Cin, KS, KS, generator=gen) / np.sqrt(K)
    b = torch.randn(Cout, generator=gen)
    sc, sh = torch.rand(Cin, generator=gen) + 0.5, torch.randn(Cin, generator=gen) * 0.5
    st, pad = (2, 3) if stem else (1, (KS - 1) // 2)
    inp = C.prologue(x, sc, sh) if pro else x
    y = F.conv2d(inp.double(), w.double(), b.double(), st, pad)
    res = torch.randn(y.shape, generator=gen) if resid else None
    if resid:
        y = y + res.double()
    for seeded in (False, True):      # a launch without split-K seeds its accumulators with bias + res
        note(group + (" seeded" if seeded else ""), "fwd %s KS %d pro %d res %d" % (case, KS, pro, resid), K,
             C.rel(C.chain_conv(inp, w, b, res, st, pad, seeded=seeded), y))
    if not stem:
        dy = torch.randn(B, Cout, H, H, generator=gen)
        dx = torch.nn.grad.conv2d_input((B, Cin, H, H), w.double(), dy.double(), 1, pad)
        note("dgrad", "dgrad %s KS %d" % (case, KS), Cout * KS * KS, C.rel(C.chain_dgrad(dy, w, pad), dx))


def wgrad_randn(group, case, KS, pro, seed, stem=False):
    B, Cin, Cout, H, W = case
    B = min(B, 2)
    while B * H * W > 8192 * (4 if stem else 1):
        H //= 2
        W //= 2
    gen = torch.Generator().manual_seed(seed)
    x = (torch.rand(B, Cin, H, W, generator=gen) - 0.5) if stem else torch.randn(B, Cin, H, W, generator=gen)
    st, pad = (2, 3) if stem else (1, (KS - 1) // 2)
    Ho, Wo = (H // 2, W // 2) if stem else (H, W)
    dy = torch.randn(B, Cout, Ho, Wo, generator=gen)
    sc, sh = torch.rand(Cin, generator=gen) + 0.5, torch.randn(Cin, generator=gen) * 0.5
    inp = C.prologue(x, sc, sh) if pro else x
    dwref = torch.nn.grad.conv2d_weight(inp.double(), (Cout, Cin, KS, KS), dy.double(), st, pad)
    dw, db = C.chain_wgrad(dy, inp, KS, st, pad)
    note(group, "wgrad %s KS %d pro %d" % (case, KS, pro), B * Ho * Wo, C.rel(dw, dwref))
    if stem:
        note("stem dbias", "dbias %s" % (case,), B * Ho * Wo, C.rel(db, dy.double().sum((0, 2, 3))))


def range_file():
    import test_gpu_f16_range as T
    kinds = [("act", -10), ("act_relu", -10), ("act_top", 0), ("w", 1e-4), ("w_top", 0), ("both_top", 0), ("mixed", 0)]
    for i, kern in enumerate(T.FWD_KERNELS):
        name, shape, KS, _ = kern
        conds = kinds + ([("heatmap", 0)] if name == "sol_cin16" else [])
        for cond in conds:
            B, Cin, H, Cout = shape
            x32, w32, b32, res32, ps32, ph32, inp, true, _ = T._forward_operands((min(B, 2), Cin, H, Cout), KS, cond,
                                                                                1000 + 37 * i)
            for seeded in (False, True):
                y = C.chain_conv(inp.float(), w32, b32, res32, 1, (KS - 1) // 2, seeded=seeded)
                note("range fwd" + (" seeded" if seeded else ""), "%s %s" % (name, T._cond_id(cond)), Cin * KS * KS,
                     C.rel(y, true))
    # the 3x3 backward: uniform dz through a training-mode BN + ReLU backward (float64 here)
    B, Cin, Cout, H, W = 2, 64, 64, 32, 32
    gen = torch.Generator().manual_seed(613)
    u = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64) * 2 - 1
    x, w = u(B, Cin, H, W).float(), (u(Cout, Cin, 3, 3) / np.sqrt(Cin * 9)).float()
    sc, sh = (torch.rand(Cin, generator=gen) + 0.5), u(Cin).float() * 0.5
    for mag in (1.0, "spread"):
        dz = u(B, Cout, H, W) * (T._spread(Cout)[None, :, None, None] if mag == "spread" else mag)
        xb = u(B, Cout, H, W) * 4.0
        gamma = (torch.rand(Cout, generator=gen) + 0.5).double()
        mean, istd = u(Cout) * 0.1, (torch.rand(Cout, generator=gen) + 0.5).double()
        bsc, bsh = gamma * istd, u(Cout) * 0.5 - mean * gamma * istd
        v = lambda t: t[None, :, None, None]
        g = dz * ((xb * v(bsc) + v(bsh)) > 0)
        xh = (xb - v(mean)) * v(istd)
        dy = (v(gamma * istd) * (g - g.mean((0, 2, 3), keepdim=True) - xh * (g * xh).mean((0, 2, 3), keepdim=True))).float()
        dx = torch.nn.grad.conv2d_input((B, Cin, H, W), w.double(), dy.double(), 1, 1)
        note("range bwd", "dgrad dz %s" % mag, Cout * 9, C.rel(C.chain_dgrad(dy, w, 1), dx))
        inp = C.prologue(x, sc, sh)
        dwref = torch.nn.grad.conv2d_weight(inp.double(), (Cout, Cin, 3, 3), dy.double(), 1, 1)
        note("range bwd", "wgrad dz %s" % mag, B * H * W, C.rel(C.chain_wgrad(dy, inp, 3, 1, 1)[0], dwref))


def main():
    split_cases = [(2, 128, 64, 128, 3, True, False), (4, 128, 8, 128, 3, True, False), (2, 64, 32, 64, 3, True, False),
                   (2, 256, 16, 128, 1, True, False), (2, 128, 16, 256, 1, True, True), (2, 256, 64, 16, 1, False, False),
                   (2, 16, 32, 256, 1, False, True), (3, 256, 4, 256, 1, True, True)]
    for i, (B, Cin, H, Cout, KS, pro, resid) in enumerate(split_cases):
        fwd_randn("split fwd", (B, Cin, H, Cout), KS, pro, resid, 11 + i)
    sol = [(2, 256, 64, 128, True, False), (2, 128, 64, 256, True, True), (3, 64, 32, 64, True, True),
           (5, 256, 8, 256, False, True), (3, 128, 6, 128, True, False), (4, 256, 32, 16, False, False),
           (8, 256, 16, 16, True, False), (2, 16, 32, 256, False, False)]
    for i, (B, Cin, H, Cout, pro, resid) in enumerate(sol):
        fwd_randn("split fwd", (B, Cin, H, Cout), 1, pro, resid, 50 + i)
    for i, case in enumerate([(32, 128, 64, 128), (32, 256, 32, 256), (32, 64, 128, 64)]):      # HALO_CASES
        fwd_randn("split fwd", case, 3, False, True, 80 + i)
    for i, H in enumerate((64, 32)):
        fwd_randn("stem fwd", (2, 3, H, 64), 7, False, False, 31 + i, stem=True)
    for i, case in enumerate([(2, 128, 128, 64, 64), (3, 128, 128, 16, 32), (2, 64, 64, 32, 32), (2, 128, 128, 8, 8)]):
        wgrad_randn("split wgrad", case, 3, True, 41 + i)
    for i, (B, Cin, Cout, H, pro) in enumerate([(2, 256, 128, 64, True), (3, 256, 256, 16, False), (2, 64, 64, 128, True)]):
        wgrad_randn("split wgrad", (B, Cin, Cout, H, H), 1, pro, 17 + i)
    for i, H in enumerate((256, 128)):
        wgrad_randn("stem wgrad", (2, 3, 64, H, H), 7, False, 37 + i, stem=True)
    range_file()
    print()
    for group in dict.fromkeys(g for g, _, _ in rows):
        sel = [(K, r) for g, K, r in rows if g == group]
        print("%-18s K %5d .. %5d   ratio %.2f .. %.2f" % (group, min(k for k, _ in sel), max(k for k, _ in sel),
                                                          min(r for _, r in sel), max(r for _, r in sel)))
    worst = max(r for _, _, r in rows)
    print("largest %.3f -> C = %.2f (tests/f32_chain_ref.py YARDSTICK_C = %.2f)" % (worst, 2 * worst, C.YARDSTICK_C))


if __name__ == "__main__":
    main()
