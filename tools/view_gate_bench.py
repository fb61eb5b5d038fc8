"""What a pseudo-label option of the training step costs on the headline step: the view-consistency
rule (--rule uncertainty, the default), the rank-based one (--rule rate) or cross-view targets
(--rule views).

The bench's MT_UBPL step (2 students + 2 EMA teachers, HG2, 256x256, B=32, synthetic
batches, captured in a HIP graph) with args.pseudoRule off ("score") and on
("uncertainty", Taylor peaks) — per view one strided decode and one refinement of both
teachers' last stacks, one ubpl_view_uncertainty_samples launch, the back matrices, and
kind 3 in place of kind 2 in the four pseudo-loss reductions — alternating in ONE
process, by the protocol of tools/guard_bench.py: both variants warmed up first, then
--repeats rounds in which they alternate, each timed over --steps replayed steps with a
host clock around work that ends in a device synchronise; per variant the median of the
rounds and the spread (max - min) / median across them.  The variants share the networks
and optimizers; switching re-captures the step (untimed).  The synthetic batches carry a
random similarity per (view, sample) as meta["viewmat"] (the rule's cost does not depend
on what the matrices say).  --rule rate times args.pseudoRule = "rate" (--sel-rate) instead: per
pseudo-loss call two ubpl_softmax_peak_scores reads (the student's stacks, the teachers' last
stacks), two ubpl_rank_threshold launches and ubpl_loss_finalize_ranked in ubpl_loss_finalize's
place.  --rule views times args.pseudoViews (--pseudo-views merged|other) under the score rule: one
stack of the teachers' last stacks, the pair matrices and one ubpl_merge_views_samples launch in
place of the per-view stacks of the teachers' full outputs.  One JSON line on stdout and in --out
(default profiles/view_gate_step.json, for --rule rate profiles/rate_rule_step.json, for --rule
views profiles/cross_view_step.json).  No GPU, no number.

    python tools/view_gate_bench.py [--rule uncertainty|rate|views] [--steps 10] [--repeats 5] [--dist-thr 4]
                                    [--sel-rate 0.5] [--pseudo-views merged] [--out FILE]
"""
import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "ubpl-poseestimation_amd"))
sys.path.insert(0, ROOT)


def similarities(B, res, gen, dev):
    """[B,6] float32: a random scale in [0.75, 1.25] and rotation in [-30, 30] degrees about the centre."""
    s = 0.75 + 0.5 * torch.rand(B, generator=gen, dtype=torch.float64)
    th = (torch.rand(B, generator=gen, dtype=torch.float64) * 60.0 - 30.0) * math.pi / 180.0
    c = (res - 1) / 2.0
    a, b = s * torch.cos(th), s * torch.sin(th)
    m = torch.stack([a, -b, c - a * c + b * c, b, a, c - b * c - a * c], 1)
    return m.float().to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="timed steps per variant per round")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rule", choices=("uncertainty", "rate", "views"), default="uncertainty")
    ap.add_argument("--dist-thr", type=float, default=4.0)
    ap.add_argument("--sel-rate", type=float, default=0.5)
    ap.add_argument("--pseudo-views", choices=("merged", "other"), default="merged")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", {"rate": "rate_rule_step.json", "views": "cross_view_step.json"}.get(
            a.rule, "view_gate_step.json"))

    import bench
    from ubpl_amd import _lib, kernels as Kn
    from ubpl_amd import train as T
    from ubpl_amd.hourglass import StackedHourglass
    from ubpl_amd.optim import FlatAdamW
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = bench.CONFIGS["mt_ubpl"]
    B, K, S, res = a.batch, cfg["K"], cfg["S"], cfg["res"]
    torch.manual_seed(1388)
    models, emas, optims = [], [], []
    for _ in range(2):
        m, e = StackedHourglass(K, S, "AvgPool"), StackedHourglass(K, S, "AvgPool")
        for p in e.parameters():
            p.detach_()
        models.append(m)
        emas.append(e)
        optims.append(FlatAdamW(m, lr=2.5e-4, weight_decay=0.0))
    plain = bench.make_batches(2, B, K, dev, 1388, res)
    gen = torch.Generator().manual_seed(1388)
    with_mats = [(imgs, hm, dict(meta, viewmat=[similarities(B, res, gen, dev) for _ in imgs]))
                 for imgs, hm, meta in plain]
    args_off = bench.make_args(B)
    args_off.nStack, args_off.outRes = S, res // 4
    args_on = bench.make_args(B)
    args_on.nStack, args_on.outRes = S, res // 4
    if a.rule == "rate":
        args_on.pseudoRule, args_on.pseudoSelRate = "rate", a.sel_rate
        rule_on = {"pseudoRule": "rate", "pseudoSelRate": a.sel_rate}
    elif a.rule == "views":
        args_on.pseudoViews = a.pseudo_views
        rule_on = {"pseudoViews": a.pseudo_views}
    else:
        args_on.pseudoRule, args_on.distThrMax = "uncertainty", a.dist_thr
        rule_on = {"pseudoRule": "uncertainty", "distThrMax": a.dist_thr, "pseudoRefine": "taylor"}

    def run(on, n):
        """n steps of one variant after two untimed ones (which re-capture the step) -> ms per step."""
        args, batches = (args_on, with_mats) if on else (args_off, plain)
        T.train_mt_ubpl([batches[i % 2] for i in range(2)], models, emas, optims, args, verbose=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        T.train_mt_ubpl([batches[i % 2] for i in range(n)], models, emas, optims, args, verbose=False)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    T._StepGraph.WARM = 2
    for on in (False, True):                       # warm-up: eager steps, first captures
        run(on, 2)
    ms = {False: [], True: []}
    for _ in range(a.repeats):
        for on in (False, True):
            ms[on].append(run(on, a.steps))
    runner = T._StepGraph.get(T._mt_ubpl_core, models, emas, optims, args_on)
    captured = runner.graph is not None
    row = {}
    for on, name in ((False, "off"), (True, "on")):
        v = sorted(ms[on])
        med = v[len(v) // 2]
        row[name + "_ms"] = round(med, 4)
        row[name + "_spread"] = round((v[-1] - v[0]) / med, 4)
        row[name + "_rounds_ms"] = [round(x, 4) for x in ms[on]]
    row["delta_ms"] = round(row["on_ms"] - row["off_ms"], 4)
    row["delta_rel"] = round(row["delta_ms"] / row["off_ms"], 5)
    row["outside_spread"] = bool(abs(row["delta_rel"]) > max(row["off_spread"], row["on_spread"]))
    out = {"tool": "view_gate_bench", "workload": "MT_UBPL train step, HG%d, K=%d, %dx%d, B=%d" % (S, K, res, res, B),
           "rule_on": rule_on,
           "captured": captured, "steps_per_round": a.steps, "repeats": a.repeats,
           "precision": Kn.conv_precision_name(), "device": torch.cuda.get_device_name(0),
           "images_per_sec": {"off": round(B / row["off_ms"] * 1e3, 2), "on": round(B / row["on_ms"] * 1e3, 2)}}
    out.update(row)
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
