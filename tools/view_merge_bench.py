"""ubpl_merge_views_samples alone at the training step's shape, beside a device-to-device copy of
the same bytes as the floor.

The headline step's cross-view merge: A = 2 views, M = 2 teachers, B = 32, K = 16, 64x64 maps, a
random similarity per (view, sample) (tools/view_gate_bench.py's) — 33.5 MB read, 33.5 MB written.
Each variant is captured in a HIP graph of --launches launches; --replays replays are timed one by
one with device events after --warmup untimed ones, and the figure is the median replay over the
launches in it.  The floor is torch's copy of a tensor of the input's size (as many bytes read and
written).  One JSON line on stdout and in --out (default profiles/cross_view_kernel.json).  No GPU,
no number.

    python tools/view_merge_bench.py [--batch 32] [--views 2] [--launches 10] [--replays 20] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "ubpl-poseestimation_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--views", type=int, default=2)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_view_kernel.json"))
    a = ap.parse_args()

    from ubpl_amd import _lib, kernels as Kn
    from view_gate_bench import similarities
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    V, M, N, K, H, R = a.views, 2, a.batch, 16, 64, 256
    gen = torch.Generator().manual_seed(1388)
    hm = torch.rand((V, M, N, K, H, H), generator=gen).to(dev)
    pair = Kn.train_pair_matrices([similarities(N, R, gen, dev) for _ in range(V)], R, H)
    blk = K * H * H
    out = torch.empty_like(hm)
    cover = torch.empty((V, N, H, H), device=dev)
    dst = torch.empty_like(hm)

    def merge(include_self, want_cover):
        return lambda: Kn.merge_views_samples(hm.view(-1), M * N * blk, N * blk, blk, V, M, N, K, H, H, pair,
                                              include_self, out=(out, cover if want_cover else None))

    variants = {"merged": merge(True, False), "merged_cover": merge(True, True), "other": merge(False, False),
                "copy": lambda: dst.copy_(hm)}

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(a.launches):
                fn()
        for _ in range(a.warmup):
            g.replay()
        torch.cuda.synchronize()
        us = []
        for _ in range(a.replays):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            g.replay()
            t1.record()
            t1.synchronize()
            us.append(t0.elapsed_time(t1) * 1e3 / a.launches)
        us.sort()
        return us

    nbytes = 2 * hm.numel() * 4
    rows = {}
    for name, fn in variants.items():
        us = timed(fn)
        med = us[len(us) // 2]
        rows[name] = {"us": round(med, 2), "min_us": round(us[0], 2), "max_us": round(us[-1], 2),
                      "GB_per_s": round(nbytes / med * 1e-3, 1)}
    res = {"tool": "view_merge_bench", "shape": {"V": V, "M": M, "N": N, "K": K, "H": H, "W": H},
           "bytes_read_plus_written": nbytes, "launches_per_replay": a.launches, "replays": a.replays,
           "device": torch.cuda.get_device_name(0), "variants": rows,
           "merged_over_copy": round(rows["merged"]["us"] / rows["copy"]["us"], 3)}
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
