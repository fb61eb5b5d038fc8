"""Inference latency: today's eager path against the Predictor's graph replay.

For one HG<n> teacher (default HG2, K=16, 256x256, the flagship network) and each
batch size (default 1, 8, 32), three ways of getting keypoints from images on the
device:

  (a) eager    model.eval()(x), then Kn.decode_heatmaps of the contiguous copy of the
               last stack — what train.validate does per batch;
  (b) replay   Predictor.predict(x, center, scale): copy into the static inputs,
               graph replay, clone of the outputs;
  (c) flip     the same with flip_test=True (a [2B] batch inside).

Timing: every variant warmed up (graphs captured) first; then REPEATS rounds in
which (a), (b), (c) alternate, each timed over enough calls for >= --window seconds
with a host clock around work that ends in a device synchronise.  Per variant the
median of the rounds is reported, with the spread (max - min) / median across them.
(b) and (a) must agree bit for bit before anything is timed.  One JSON line on
stdout (--out: also written to a file).  No GPU, no number: there is no CPU fallback.

    python tools/predict_bench.py [--stacks 2] [--res 256] [--batches 1,8,32] [--out FILE]

--mode pseudo times the ensemble pseudo-labels instead, on ONE Predictor of two teachers
with the flip test on:

  (p) pseudo    Predictor.pseudo_label(x, center, scale);
  (q) predict   Predictor.predict(x, center, scale) — what pseudo_label adds is (p) - (q);
  (r) compose   the same ensemble outputs by torch ops on predict(return_heatmaps=True) and
                one Kn.decode_heatmaps of the mean — what a user wrote before pseudo_label.

Same warm-up, rounds and report; (p) and (r) must select the same joints before anything
is timed.

--refine quarter|taylor (--blur-sigma S) builds the Predictors of either mode with the
sub-pixel decode on.  --mode refine times what it adds, on three Predictors of the same
teacher that differ in the option alone:

  (n) none      Predictor.predict(x, center, scale) with refine="none";
  (u) quarter   the same with refine="quarter" (one ubpl_refine_peaks launch more per replay);
  (t) taylor    the same with refine="taylor" at --blur-sigma.

Same warm-up, rounds and report; the integer outputs of the three must agree bit for bit
before anything is timed.

--mode tta times multi-view test-time augmentation, on Predictors of the same teacher that
differ in tta / flip_test alone:

  (none)  Predictor.predict(x, center, scale) with tta=None — the comparison;
  (v1)    tta=[(0, 1)]: one view through ubpl_decode_heatmaps_views;
  (v3)    three zooms;  (v5) three zooms + two rotations;  (v10) those five with flip_test.

Same warm-up, rounds and report; v1 and none must agree bit for bit before anything is timed.
A Predictor with tta keeps its forward batch within 2 max_batch images, so larger B run in chunks.

--mode unc times what the view-consistency uncertainty adds, on ONE pair of teachers and two
Predictors per view set that differ in the option alone:

  (v5_off / v5_on)    pseudo_label with tta = three zooms + two rotations, uncertainty off / on
                      (on: rule "uncertainty" at --dist-thr);
  (v10_off / v10_on)  the same views with flip_test;
  (p5_off / p5_on)    predict of ONE teacher on the five views, uncertainty off / on — p5_off is
                      --mode tta's v5.

Same warm-up, rounds and report; off and on must agree bit for bit on every key they share
before anything is timed.

--mode frames times the crop from raw frames (ubpl_amd.frames) beside the predict call it feeds:
per batch size (use --batches 32) and per sf = scale * 200 / res of 1, 1.5, 3 and 6, B boxes
out of four 1080x1920 uint8 frames:

  (crop)       FrameBank.crop(frame, center, scale, res), the whole call;
  (host_plan)  frames.crop_plan alone: the per-box plan in Python, no GPU work;
  (wrapper)    Kn.crop_frames on a plan already built: host check, two small uploads, the launches;
  (kernels)    the ubpl_crop_frames launches alone, plan and workspace already on the device;
  (predict)    Predictor.predict(crop, center, scale), the replay the crop feeds.

Same warm-up, rounds and report; two crops must give equal bits, the launches alone must give
the crop's bits and predict_frames must equal predict on the crop before anything is timed.  Each
row also records the bytes the crop must move: the frame pixels under the boxes' taps, the float32
output, and the intermediate it writes and reads once — kernels_stream_GBps says how far the HIP
path is from streaming them, crop_stream_GBps how far the whole call is.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ubpl-poseestimation_amd"))


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def measure(variants, a):
    """Warm-up, then a.repeats rounds in which the variants alternate -> {name_ms, name_spread,
    name_seconds_timed}."""
    calls = {}
    for name, fn in variants.items():        # warm-up, and the call count of a round's window
        timed(fn, 3)
        calls[name] = max(3, int(a.window * 1e3 / timed(fn, 5)) + 1)
    ms = {name: [] for name in variants}
    for _ in range(a.repeats):
        for name, fn in variants.items():
            ms[name].append(timed(fn, calls[name]))
    row = {}
    for name, v in ms.items():
        v = sorted(v)
        med = v[len(v) // 2]
        row[name + "_ms"] = round(med, 4)
        row[name + "_spread"] = round((v[-1] - v[0]) / med, 4)
        row[name + "_seconds_timed"] = round(sum(v) * calls[name] / 1e3, 2)
    return row


def refine_kw(a):
    """The Predictor arguments of --refine / --blur-sigma."""
    kw = {"refine": a.refine}
    if a.blur_sigma is not None:
        kw["blur_sigma"] = a.blur_sigma
    return kw if a.refine != "none" else {}


def teacher(a, seed, gen, dev):
    from ubpl_amd.hourglass import StackedHourglass
    torch.manual_seed(seed)
    m = StackedHourglass(a.k, a.stacks, "AvgPool")
    with torch.no_grad():
        for _ in range(2):                       # running statistics off their initial values
            m((torch.rand(4, 3, a.res, a.res, generator=gen) - 0.5).to(dev))
    return m.eval()


def refine_main(a):
    from ubpl_amd import Predictor, _lib, kernels as Kn
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    gen = torch.Generator().manual_seed(1)
    model = teacher(a, 0, gen, dev)
    sg = {} if a.blur_sigma is None else {"blur_sigma": a.blur_sigma}
    P = {"none": Predictor(model), "quarter": Predictor(model, refine="quarter"),
         "taylor": Predictor(model, refine="taylor", **sg)}
    rows = []
    for B in [int(b) for b in a.batches.split(",")]:
        x = (torch.rand(B, 3, a.res, a.res, generator=gen) - 0.5).to(dev)
        center = torch.full((B, 2), a.res / 2.0)
        scale = torch.full((B,), a.res / 200.0)
        outs = {n: p.predict(x, center, scale) for n, p in P.items()}
        for n in ("quarter", "taylor"):
            if not all(torch.equal(outs[n][k], outs["none"][k]) for k in outs["none"]):
                raise SystemExit("predict_bench: refine=%s changes the integer outputs at B=%d" % (n, B))
        row = {"B": B, "taylor_rule_2_fraction": round(float((outs["taylor"]["refine_rule"] == 2).float().mean()), 4)}
        row.update(measure({n: (lambda p=p: p.predict(x, center, scale)) for n, p in P.items()}, a))
        for n in ("quarter", "taylor"):
            row[n + "_added_us"] = round((row[n + "_ms"] - row["none_ms"]) * 1e3, 1)
        rows.append(row)
    out = {"tool": "predict_bench", "mode": "refine", "model": "HG%d" % a.stacks, "k": a.k, "res": a.res,
           "blur_sigma": P["taylor"].blur_sigma, "precision": Kn.conv_precision_name(), "repeats": a.repeats,
           "device": torch.cuda.get_device_name(0), "rows": rows}
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


TTA_ZOOMS = [(0, 1), (0, 0.85), (0, 1.15)]
TTA_ROTATIONS = [(15, 1), (-15, 1)]


def tta_main(a):
    from ubpl_amd import Predictor, _lib, kernels as Kn
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    gen = torch.Generator().manual_seed(1)
    model = teacher(a, 0, gen, dev)
    kw = refine_kw(a)
    P = {"none": Predictor(model, **kw), "v1": Predictor(model, tta=[(0, 1)], **kw),
         "v3": Predictor(model, tta=TTA_ZOOMS, **kw), "v5": Predictor(model, tta=TTA_ZOOMS + TTA_ROTATIONS, **kw),
         "v10": Predictor(model, tta=TTA_ZOOMS + TTA_ROTATIONS, flip_test=True, **kw)}
    rows = []
    for B in [int(b) for b in a.batches.split(",")]:
        x = (torch.rand(B, 3, a.res, a.res, generator=gen) - 0.5).to(dev)
        center = torch.full((B, 2), a.res / 2.0)
        scale = torch.full((B,), a.res / 200.0)
        outs = {n: p.predict(x, center, scale) for n, p in P.items()}
        if not all(torch.equal(outs["v1"][k], outs["none"][k]) for k in outs["none"]):
            raise SystemExit("predict_bench: tta=[(0, 1)] and tta=None disagree at B=%d" % B)
        row = {"B": B, "chunk": {n: min(B, p.max_batch) for n, p in P.items()}}
        row.update(measure({n: (lambda p=p: p.predict(x, center, scale)) for n, p in P.items()}, a))
        for n, p in P.items():
            if n != "none":
                row[n + "_over_none"] = round(row[n + "_ms"] / row["none_ms"], 3)
        rows.append(row)
    out = {"tool": "predict_bench", "mode": "tta", "model": "HG%d" % a.stacks, "k": a.k, "res": a.res,
           "views": {"v1": 1, "v3": 3, "v5": 5, "v10": 10}, "zooms": TTA_ZOOMS, "rotations": TTA_ROTATIONS,
           "refine": a.refine, "precision": Kn.conv_precision_name(), "repeats": a.repeats,
           "device": torch.cuda.get_device_name(0), "rows": rows}
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


def unc_main(a):
    from ubpl_amd import Predictor, _lib, kernels as Kn
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    gen = torch.Generator().manual_seed(1)
    models = [teacher(a, seed, gen, dev) for seed in (0, 1)]
    kw = refine_kw(a)
    views = TTA_ZOOMS + TTA_ROTATIONS
    P = {}
    for name, flip in (("v5", False), ("v10", True)):
        P[name + "_off"] = Predictor(models, tta=views, flip_test=flip, **kw)
        P[name + "_on"] = Predictor(models, tta=views, flip_test=flip, uncertainty=True, **kw)
    call = {n: (lambda x, c, s, p=p, on=n.endswith("_on"):
                p.pseudo_label(x, c, s, thr=a.thr, **({"rule": "uncertainty", "dist_thr": a.dist_thr} if on else {})))
            for n, p in P.items()}
    P["p5_off"] = Predictor(models[0], tta=views, **kw)
    P["p5_on"] = Predictor(models[0], tta=views, uncertainty=True, **kw)
    for n in ("p5_off", "p5_on"):
        call[n] = lambda x, c, s, p=P[n]: p.predict(x, c, s)
    rows = []
    for B in [int(b) for b in a.batches.split(",")]:
        x = (torch.rand(B, 3, a.res, a.res, generator=gen) - 0.5).to(dev)
        center = torch.full((B, 2), a.res / 2.0)
        scale = torch.full((B,), a.res / 200.0)
        outs = {n: f(x, center, scale) for n, f in call.items()}
        row = {"B": B, "chunk": {n: min(B, p.max_batch) for n, p in P.items()}}
        for v in ("v5", "v10", "p5"):
            off, on = outs[v + "_off"], outs[v + "_on"]
            if not all(torch.equal(on[k], off[k]) for k in off if k not in ("selected", "kps", "kps_sub")):
                raise SystemExit("predict_bench: uncertainty=True changes a shared output (%s, B=%d)" % (v, B))
            row[v + "_legal_fraction"] = round(float(on["view_legal"].float().mean()), 4)
            if "selected" in on:
                row[v + "_selected_fraction"] = round(float(on["selected"].float().mean()), 4)
        row.update(measure({n: (lambda f=f: f(x, center, scale)) for n, f in call.items()}, a))
        for v in ("v5", "v10", "p5"):
            row[v + "_added_us"] = round((row[v + "_on_ms"] - row[v + "_off_ms"]) * 1e3, 1)
            row[v + "_on_over_off"] = round(row[v + "_on_ms"] / row[v + "_off_ms"], 4)
        rows.append(row)
    out = {"tool": "predict_bench", "mode": "unc", "model": "HG%d" % a.stacks, "teachers": len(models), "k": a.k,
           "res": a.res, "views": {"v5": 5, "v10": 10, "p5": 5}, "zooms": TTA_ZOOMS, "rotations": TTA_ROTATIONS,
           "refine": a.refine, "thr": a.thr, "dist_thr": a.dist_thr, "precision": Kn.conv_precision_name(),
           "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "rows": rows}
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


FRAME_HW = (1080, 1920)
FRAME_SFS = [1.0, 1.5, 3.0, 6.0]


def frames_main(a):
    """--mode frames: the crop from raw frames (FrameBank.crop: host plan + ubpl_crop_frames) and
    the predict call it feeds, alternating, per sf = scale * 200 / res."""
    import numpy as np
    from ubpl_amd import Predictor, _lib, frames as F, kernels as Kn
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    gen = torch.Generator().manual_seed(1)
    P = Predictor(teacher(a, 0, gen, dev))
    rs = np.random.RandomState(2)
    ht, wd = FRAME_HW
    bank = F.FrameBank([rs.randint(0, 256, (ht, wd, 3)).astype(np.uint8) for _ in range(4)], [0.45, 0.45, 0.45], dev)
    R, rows = a.res, []
    for B in [int(b) for b in a.batches.split(",")]:
        for sf in FRAME_SFS:
            frame = rs.randint(0, len(bank), B)
            scale = torch.full((B,), sf * R / 200.0)
            half = 100.0 * float(scale[0])                           # boxes inside the frame where they fit
            center = torch.tensor(np.stack([rs.uniform(min(half, wd / 2), max(wd - half, wd / 2), B),
                                            rs.uniform(min(half, ht / 2), max(ht - half, ht / 2), B)], 1))
            plan = F.crop_plan(bank.sizes, frame, center, scale, R)

            def span(ax, length):                                    # frame pixels one axis of a box reads
                first, count = F._rows(tuple(int(v) for v in ax), R)
                return max(0, min(length, int(ax[0]) + first + count) - max(0, int(ax[0]) + first))
            src = sum(3 * span(t[1:7], wd) * span(t[7:13], ht) for t in plan.table)
            inter = int(sum(12 * int(t[14]) * R for t in plan.table))
            x = bank.crop(frame, center, scale, R)
            if not torch.equal(x, bank.crop(frame, center, scale, R)):
                raise SystemExit("predict_bench: two crops of the same boxes differ at B=%d sf=%g" % (B, sf))
            got, want = P.predict_frames(bank, center, scale, R, frame=frame), P.predict(x, center, scale)
            if not all(torch.equal(got[k], want[k]) for k in want):
                raise SystemExit("predict_bench: predict_frames and predict on the crop disagree at B=%d" % B)
            # the device part alone: the plan built, checked and uploaded once, then only the launches
            dplan = torch.from_numpy(plan.table).to(dev)
            dgauss = torch.from_numpy(plan.gauss.astype("float32")).to(dev)
            gw, chunks = plan.gauss.shape[2], Kn._crop_chunks(plan.rows, R)
            inters = [torch.empty(B * 3 * int(plan.rows[c0:c1].max()) * R, device=dev) for c0, c1 in chunks]
            xk = torch.empty_like(x)

            def kernels():
                for (c0, c1), inter_c in zip(chunks, inters):
                    Kn.call("ubpl_crop_frames", bank.bank, bank.off, bank.hw, dplan[c0:c1], dgauss[c0:c1], gw,
                            bank.chan_mean, c1 - c0, int(plan.rows[c0:c1].max()), R, inter_c, xk[c0:c1])
            kernels()
            if not torch.equal(xk, x):
                raise SystemExit("predict_bench: the launches alone and FrameBank.crop differ at B=%d sf=%g" % (B, sf))
            row = {"B": B, "sf": sf, "gauss_radius": int(plan.table[:, 6].max()),
                   "source_bytes": int(src), "output_bytes": B * 3 * R * R * 4, "intermediate_bytes": inter,
                   "chunks": len(chunks)}
            row.update(measure({"crop": lambda: bank.crop(frame, center, scale, R),
                                "host_plan": lambda: F.crop_plan(bank.sizes, frame, center, scale, R),
                                "wrapper": lambda: Kn.crop_frames(bank.bank, bank.off, bank.hw, plan.table, plan.gauss,
                                                                  bank.chan_mean, R, out=xk,
                                                                  layout=(bank.off_host, bank.hw_host)),
                                "kernels": kernels,
                                "predict": lambda: P.predict(x, center, scale)}, a))
            # the kernels must read the source once and write the output once, and they write and
            # read the intermediate once each
            moved = row["source_bytes"] + row["output_bytes"] + 2 * inter
            row["kernels_stream_GBps"] = round(moved / (row["kernels_ms"] * 1e-3) / 1e9, 1)
            row["crop_stream_GBps"] = round(moved / (row["crop_ms"] * 1e-3) / 1e9, 2)
            row["crop_over_predict"] = round(row["crop_ms"] / row["predict_ms"], 4)
            rows.append(row)
    out = {"tool": "predict_bench", "mode": "frames", "model": "HG%d" % a.stacks, "k": a.k, "res": R,
           "frame_hw": list(FRAME_HW), "frames": len(bank), "precision": Kn.conv_precision_name(),
           "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
           "note": "crop is FrameBank.crop end to end = host_plan (crop_plan alone) + wrapper (Kn.crop_frames on a "
                   "built plan: host check, two small uploads, the launches); kernels is the ubpl_crop_frames "
                   "launches alone on a plan already on the device; source_bytes are the frame pixels under the "
                   "boxes' taps",
           "rows": rows}
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


def pseudo_main(a):
    from ubpl_amd import Predictor, _lib, kernels as Kn
    from ubpl_amd.hourglass import StackedHourglass
    from ubpl_amd.process import inverse_transforms
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    gen = torch.Generator().manual_seed(1)
    models = []
    for seed in (0, 1):
        torch.manual_seed(seed)
        m = StackedHourglass(a.k, a.stacks, "AvgPool")
        with torch.no_grad():
            for _ in range(2):                   # running statistics off their initial values
                m((torch.rand(4, 3, a.res, a.res, generator=gen) - 0.5).to(dev))
        models.append(m.eval())
    P = Predictor(models, flip_test=True, **refine_kw(a))
    rows = []
    for B in [int(b) for b in a.batches.split(",")]:
        x = (torch.rand(B, 3, a.res, a.res, generator=gen) - 0.5).to(dev)
        center = torch.full((B, 2), a.res / 2.0)
        scale = torch.full((B,), a.res / 200.0)
        tinv = inverse_transforms(center, scale, [a.res // 4, a.res // 4]).to(dev)
        # seeded networks score low: the threshold that splits this batch's ensemble scores
        thr = float(P.pseudo_label(x, center, scale, thr=0.0)["ens_score"].median()) if a.thr <= 0 else a.thr

        def compose():
            o = P.predict(x, center, scale, return_heatmaps=True)
            hm = o["heatmaps"]
            T = hm.mean(0)
            raw, preds, score = Kn.decode_heatmaps(T, tinv)
            sel = (hm.flatten(3).amax(-1) >= thr) & (score >= thr)
            dis = ((hm - T) ** 2).flatten(3).mean(-1)
            spread = ((o["raw"] - raw) ** 2).sum(-1).sqrt().amax(0)
            return raw, preds, score, sel, dis, spread, sel.all(0)

        got, want = P.pseudo_label(x, center, scale, thr=thr), compose()
        if not (torch.equal(got["ens_raw"], want[0]) and torch.equal(got["member_select"], want[3])
                and torch.equal(got["selected"], want[6])):
            raise SystemExit("predict_bench: pseudo_label and the torch composition disagree at B=%d" % B)
        row = {"B": B, "thr": thr, "selected_fraction": round(float(got["selected"].float().mean()), 4)}
        row.update(measure({"pseudo": lambda: P.pseudo_label(x, center, scale, thr=thr),
                            "predict": lambda: P.predict(x, center, scale), "compose": compose}, a))
        row["pseudo_over_predict"] = round(row["pseudo_ms"] / row["predict_ms"], 3)
        row["compose_over_pseudo"] = round(row["compose_ms"] / row["pseudo_ms"], 3)
        rows.append(row)
    out = {"tool": "predict_bench", "mode": "pseudo", "model": "HG%d" % a.stacks, "teachers": len(models),
           "flip_test": True, "k": a.k, "res": a.res, "precision": Kn.conv_precision_name(), "repeats": a.repeats,
           "device": torch.cuda.get_device_name(0), "rows": rows}
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stacks", type=int, default=2)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of work per variant per round")
    ap.add_argument("--out", default=None)
    ap.add_argument("--mode", default="predict", choices=["predict", "pseudo", "refine", "tta", "unc", "frames"])
    ap.add_argument("--refine", default="none", choices=["none", "quarter", "taylor"])
    ap.add_argument("--blur-sigma", type=float, default=None, help="taylor's blur (default: the Predictor's)")
    ap.add_argument("--thr", type=float, default=0.95, help="--mode pseudo: the score threshold (<= 0: each batch's median ensemble score)")
    ap.add_argument("--dist-thr", type=float, default=8.0, help="--mode unc: the distance threshold, image pixels")
    a = ap.parse_args()
    if a.mode == "frames":
        return frames_main(a)
    if a.mode == "unc":
        return unc_main(a)
    if a.mode == "pseudo":
        return pseudo_main(a)
    if a.mode == "refine":
        return refine_main(a)
    if a.mode == "tta":
        return tta_main(a)

    from ubpl_amd import Predictor, _lib, kernels as Kn
    from ubpl_amd.hourglass import StackedHourglass
    from ubpl_amd.process import inverse_transforms
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    model = StackedHourglass(a.k, a.stacks, "AvgPool")
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for _ in range(2):                       # running statistics off their initial values
            model((torch.rand(4, 3, a.res, a.res, generator=gen) - 0.5).to(dev))
    model.eval()
    plain = Predictor(model, **refine_kw(a))
    flip = Predictor(model, flip_test=True, **refine_kw(a))
    rows = []
    for B in [int(b) for b in a.batches.split(",")]:
        x = (torch.rand(B, 3, a.res, a.res, generator=gen) - 0.5).to(dev)
        center = torch.full((B, 2), a.res / 2.0)
        scale = torch.full((B,), a.res / 200.0)
        tinv = inverse_transforms(center, scale, [a.res // 4, a.res // 4]).to(dev)

        def eager():
            with torch.no_grad():
                o = model(x)[0]
                return Kn.decode_heatmaps(o[:, -1].contiguous(), tinv)

        variants = {"eager": eager, "replay": lambda: plain.predict(x, center, scale),
                    "flip": lambda: flip.predict(x, center, scale)}
        ref = eager()
        got = plain.predict(x, center, scale)
        if not (torch.equal(ref[0], got["raw"][0]) and torch.equal(ref[1], got["preds"][0])
                and torch.equal(ref[2], got["scores"][0])):
            raise SystemExit("predict_bench: the replay and the eager path disagree at B=%d" % B)
        row = {"B": B}
        row.update(measure(variants, a))
        row["replay_speedup"] = round(row["eager_ms"] / row["replay_ms"], 3)
        row["flip_over_2x_replay"] = round(row["flip_ms"] / (2 * row["replay_ms"]), 3)
        rows.append(row)
    out = {"tool": "predict_bench", "model": "HG%d" % a.stacks, "k": a.k, "res": a.res,
           "precision": Kn.conv_precision_name(), "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
           "refine": a.refine, "rows": rows}
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
