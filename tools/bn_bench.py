"""BatchNorm backward pieces at the hourglass planes (B=32): statistics
partials pass, finalize (via part_ready), apply, and the whole backward.

    python tools/bn_bench.py [B] [reps]
    python tools/bn_bench.py fused [B] [reps]

fused: the three fused pool / upsample-add + BatchNorm entries against the launch
sequences they replace, at the headline's planes (HG2 256x256, B=32), timed with HIP
events over inputs rotated through enough copies to exceed the 256 MB Infinity Cache (at
most 32 copies: the 8x8 and 16x16 planes stay cache-resident, as they are in the step,
and are launch-latency-bound either way).
"""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ubpl-poseestimation_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ubpl_amd import kernels as Kn  # noqa: E402
from conv_bench import timeit  # noqa: E402


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    for C, H in ((128, 128), (128, 64), (256, 64), (128, 32), (256, 16), (128, 16), (256, 8), (256, 4)):
        x = torch.randn(B, C, H, H, device=dev, generator=g)
        dz = torch.randn(B, C, H, H, device=dev, generator=g)
        gamma = torch.rand(C, device=dev, generator=g) + 0.5
        mean, istd = torch.randn(C, device=dev, generator=g) * 0.1, torch.rand(C, device=dev, generator=g) + 0.5
        sc, sh = gamma * istd, torch.randn(C, device=dev, generator=g)
        coef = torch.empty(3 * C, device=dev)
        dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        out = torch.empty_like(dz)
        part = Kn.bn_bwd_partials(dz, x, sc, sh, mean, 1)
        scratch = Kn.bn_part(B, C, dev)
        beta = torch.zeros(C, device=dev)
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        m_o, i_o, s_o, h_o = (torch.empty(C, device=dev) for _ in range(4))
        t_fwd = timeit(lambda: Kn.bn_forward_stats(x, gamma, beta, 1e-5, 0.1, rm, rv, scratch, m_o, i_o, s_o, h_o),
                       reps)
        t_part = timeit(lambda: Kn.bn_bwd_partials(dz, x, sc, sh, mean, 1), reps)
        t_ready = timeit(lambda: Kn.bn_backward(dz, x, gamma, mean, istd, sc, sh, 1, scratch, coef, dg, db, out=out,
                                                part=part), reps)
        t_all = timeit(lambda: Kn.bn_backward(dz, x, gamma, mean, istd, sc, sh, 1, scratch, coef, dg, db, out=out),
                       reps)
        mb = 3 * x.numel() * 4 / 1e6
        print("C=%3d H=%3d  fwd stats %7.1f us | bwd partials %7.1f us | finalize+apply %7.1f us | bwd all %7.1f us"
              " (apply %.0f MB)" % (C, H, t_fwd * 1e3, t_part * 1e3, t_ready * 1e3, t_all * 1e3, mb), flush=True)


def timeit_rot(fn, sets, reps):
    """ms per call of fn(set), the sets taken in turn."""
    for st in sets:
        fn(st)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(reps):
        fn(sets[i % len(sets)])
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main_fused():
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 60
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    tot = [0.0, 0.0]
    for C, H in ((128, 128), (256, 64), (256, 32), (256, 16), (256, 8)):
        per_set = 6.5 * B * C * H * H * 4
        nset = int(min(32, max(2, -(-600e6 // per_set))))
        rn = lambda *shape: torch.randn(*shape, device=dev, generator=g)
        sets = [dict(x=rn(B, C, H, H) * 3 + 5, up=rn(B, C, H, H), dz=rn(B, C, H, H), add1=rn(B, C, H, H),
                     add2=rn(B, C, H, H), dx=torch.empty(B, C, H, H, device=dev), low=rn(B, C, H // 2, H // 2) * 0.01,
                     dpl=rn(B, C, H // 2, H // 2), pl=torch.empty(B, C, H // 2, H // 2, device=dev))
                for _ in range(nset)]
        gamma, beta = torch.rand(C, device=dev, generator=g) + 0.5, torch.zeros(C, device=dev)
        bn = lambda: (gamma, beta, torch.zeros(C, device=dev), torch.ones(C, device=dev)) + tuple(
            torch.empty(C, device=dev) for _ in range(4))
        b1, b2 = bn(), bn()
        scratch, coef = Kn.bn_part(B, C, dev), torch.empty(3 * C, device=dev)
        dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        stats = lambda t, b: Kn.bn_forward_stats(t, b[0], b[1], 1e-5, 0.1, b[2], b[3], scratch, *b[4:])
        stats(sets[0]["x"], b1)
        mean, istd, sc, sh = b1[4:]

        def pool_sep(s):
            stats(s["x"], b1)
            Kn.maxpool2x2(s["x"], out=s["pl"])
            stats(s["pl"], b2)

        def up_sep(s):
            Kn.upsample2x_add(s["up"], s["low"], out=s["up"])
            stats(s["up"], b2)

        def bwd_sep(s):
            Kn.bn_backward(s["dz"], s["x"], gamma, mean, istd, sc, sh, 1, scratch, coef, dg, db, add1=s["add1"],
                           out=s["dx"])
            Kn.maxpool2x2_backward(s["x"], s["dpl"], s["dx"], accumulate=True)
            Kn.add(s["dx"], s["add2"], out=s["dx"])

        rows = [("stats+pool+stats", pool_sep,
                 lambda s: Kn.bn_forward_stats_maxpool(s["x"], b1, b2, 1e-5, 0.1, scratch, out=s["pl"])),
                ("upadd+stats", up_sep,
                 lambda s: Kn.upsample2x_add_bnstats(s["up"], s["low"], b2, 1e-5, 0.1, scratch, out=s["up"])),
                ("bn bwd+pool bwd+add", bwd_sep,
                 lambda s: Kn.bn_backward_pool(s["dz"], s["x"], gamma, mean, istd, sc, sh, 1, scratch, coef, dg, db,
                                               add1=s["add1"], pool_dy=s["dpl"], add2=s["add2"], out=s["dx"]))]
        line = "C=%3d H=%3d (%2d sets)" % (C, H, nset)
        for name, sep, fused in rows:
            ts, tf = timeit_rot(sep, sets, reps) * 1e3, timeit_rot(fused, sets, reps) * 1e3
            tot[0] += ts
            tot[1] += tf
            line += " | %s %7.1f -> %7.1f us" % (name, ts, tf)
        print(line, flush=True)
        del sets
    print("sum over the planes: separate %.1f us, fused %.1f us" % tuple(tot))


if __name__ == "__main__":
    main_fused() if len(sys.argv) > 1 and sys.argv[1] == "fused" else main()
