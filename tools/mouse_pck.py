"""Real-data PCK@0.2 harness: the reference's MT_UBPL experiment on the Mouse
split (projects/MT_UBPL.py:27-154 main(): 2 students + 2 EMA teachers,
TwoStreamBatchSampler over 70 unlabeled / 30 labeled images, trainBS 4 with
2 labeled, AdamW lr 2.5e-4, two augmented views per sample, ramped loss
weights, validate() on the 500 validation images every few epochs), entirely
on the HIP path: device augmentation (augment.hip), device heatmap targets,
the fused train step, HIP decode + PCK.

    python tools/mouse_pck.py [--epochs 100] [--model HG2] [--out profiles/r02_mouse_pck.json]

--pseudo-rule uncertainty / score+uncertainty (with --dist-thr, source-image pixels) selects the
pseudo labels by the view-consistency rule of the training step; the loader then
hands the views' matrices on as meta["viewmat"].  --pseudo-rule rate (with --sel-rate R, a share in
(0, 1]) keeps the top share R of every batch's joints by softmax score (JointPseudoLoss2 in the
step, DESIGN.md §4 "Rank-based pseudo-label selection") and logs each epoch's selection count
("n_sel") and mean thresholds ("rate_thr1", "rate_thr2").  --pseudo-views merged / other takes the
pseudo loss' targets of a view from both views' teacher maps warped into its frame (DESIGN.md §4,
"Cross-view pseudo-label targets"; the matrices are handed on whenever it is not own); it combines
with every rule.  Every run logs the share of pseudo labels its rule selected per epoch
("sel_rate").

Reads tests/golden/mouse_100_500_0.3/ (tools/pack_mouse.py).
"""
import argparse
import json
import os
import random
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ubpl-poseestimation_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--model", default="HG2")
    ap.add_argument("--trainBS", type=int, default=4)
    ap.add_argument("--trainBS_labeled", type=int, default=2)
    ap.add_argument("--inferBS", type=int, default=128)
    ap.add_argument("--valid-every", type=int, default=5)
    ap.add_argument("--no-aug", action="store_true")
    ap.add_argument("--seed", type=int, default=1388)
    ap.add_argument("--pseudo-rule", default="score", choices=["score", "uncertainty", "score+uncertainty", "rate"])
    ap.add_argument("--dist-thr", type=float, default=None, help="distThrMax, source-image pixels")
    ap.add_argument("--sel-rate", type=float, default=None, help="pseudoSelRate of --pseudo-rule rate, in (0, 1]")
    ap.add_argument("--pseudo-views", default="own", choices=["own", "merged", "other"])
    ap.add_argument("--pseudo-refine", default=None, choices=["none", "quarter", "taylor"])
    ap.add_argument("--pseudo-blur-sigma", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "gpurun_out", "mouse_pck.json"))
    return ap


def main():
    log = run(parser().parse_args())
    print(json.dumps({"best_pck": log["best_pck"], "best_epoch": log["best_epoch"], "final_pck": log["final_pck"],
                      "sel_rate_last10": log["sel_rate_last10"], "wall_s": log["wall_s"]}))


def run(a, write=True, keep=None):
    """The experiment of main() with options `a` (parser() defaults); returns the log.
    keep: a dict that receives the trained networks ("models", "emas")."""

    from ubpl_amd import _lib, mouse
    from ubpl_amd import parameters as PR
    from ubpl_amd import train as T
    from ubpl_amd.augment import DeviceAugment
    from ubpl_amd.hourglass import pose_model
    from ubpl_amd.optim import FlatAdamW
    from ubpl_amd.sampler import TwoStreamBatchSampler
    _lib.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    random.seed(a.seed)
    np.random.seed(a.seed)
    torch.manual_seed(a.seed)                                          # projects/MT_UBPL.py:424-428

    data = mouse.MouseData.from_pack()
    semi, valid, lab, unlab, lidx, uidx, means, stds = data.getSemiData(100, 500, 0.3)
    args = types.SimpleNamespace(
        nStack=int(a.model[2:]), pseudoScoreThr=0.95, ensemblePseudoWeight=10.0, poseWeight=10.0,
        consWeight_max=10.0, consWeight_min=0.0, consWeight_rampup=5, FDLWeight_max=1.0, FDLWeight_min=1.0,
        FDLWeight_rampup=100, pseudoWeight_max=1.0, pseudoWeight_min=1.0, pseudoWeight_rampup=100,
        FDL_label="labeled", FDL_type="covariance", useEnsemblePseudo=True, ema_decay=0.999, lr=2.5e-4,
        outRes=data.outRes, pck_ref=data.pck_ref, pck_thr=data.pck_thr, feature_mode="AvgPool", epo=0)
    gated = a.pseudo_rule not in ("score", "rate")
    if a.pseudo_rule == "rate":
        args.pseudoRule, args.pseudoSelRate = "rate", a.sel_rate
    if gated:                                                          # (a default run sets none of these)
        args.pseudoRule, args.distThrMax = a.pseudo_rule, a.dist_thr
        if a.pseudo_refine is not None:
            args.pseudoRefine = a.pseudo_refine
        if a.pseudo_blur_sigma is not None:
            args.pseudoBlurSigma = a.pseudo_blur_sigma
    with_mats = gated or a.pseudo_views != "own"
    if a.pseudo_views != "own":
        args.pseudoViews = a.pseudo_views
    models, emas, optims = [], [], []
    for _ in range(2):                                                 # :43-50 student, teacher per branch
        models.append(pose_model(a.model, data.kpsCount, "AvgPool"))
        emas.append(pose_model(a.model, data.kpsCount, "AvgPool", nograd=True))
        optims.append(FlatAdamW(models[-1], lr=args.lr, weight_decay=0.0))
    aug = DeviceAugment(data.images("train"), means, inp_res=data.inpRes, use_flip=not a.no_aug,
                        use_noise=not a.no_aug, sf=0.0 if a.no_aug else 0.25, rf=0.0 if a.no_aug else 30.0,
                        device=dev)
    kps_all = np.array([it["kps"] for it in semi], np.float32)
    isl_all = np.array([it["islabeled"] for it in semi], bool)
    sampler = TwoStreamBatchSampler(uidx, lidx, a.trainBS, a.trainBS_labeled)
    vb = mouse.valid_batches(data, a.inferBS, dev)

    def loader():
        for idx in sampler:
            idx = list(idx)
            views, kps, mats = [], [], []
            for _ in range(2):                                         # DS_mds augCount = 2
                x, k, *m = aug.views(idx, kps_all[idx], with_mats=with_mats)
                views.append(x)
                kps.append(k)
                mats += m
            meta = {"kps": kps, "islabeled": [torch.tensor(isl_all[idx], device=dev)]}
            if with_mats:
                meta["viewmat"] = mats
            yield views, None, meta

    log = {"config": {"model": a.model, "trainBS": a.trainBS, "trainBS_labeled": a.trainBS_labeled,
                      "epochs": a.epochs, "augment": not a.no_aug, "seed": a.seed, "split": "Mouse_100_500_0.3",
                      "pck_ref": data.pck_ref, "pck_thr": data.pck_thr, "means": means,
                      "pseudo_rule": a.pseudo_rule, "dist_thr": a.dist_thr, "pseudo_refine": a.pseudo_refine,
                      "pseudo_blur_sigma": a.pseudo_blur_sigma, "pseudo_sel_rate": a.sel_rate,
                      "pseudo_views": a.pseudo_views},
           "epochs": []}
    best = (-1.0, -1)
    t0 = time.time()
    for epo in range(a.epochs):                                        # :68-152
        args.epo = epo
        args.consWeight = PR.consWeight_increase(epo, args)
        args.FDLWeight = PR.FDLWeight_decrease(epo, args)
        args.pseudoWeight = PR.pseudoWeight_increase(epo, args)
        te = time.time()
        picked = {}                                                    # the steps' pseudo-label counts
        pec, mtc, epc, fdc = T.train_mt_ubpl(loader(), models, emas, optims, args, verbose=False,
                                             pseudo_counts=picked)
        torch.cuda.synchronize()
        rec = {"epoch": epo + 1, "train_s": round(time.time() - te, 2), "pec": pec, "mtc": mtc, "epc": epc,
               "fdc": fdc, "sel_rate": round(picked["n_sel"] / picked["n_pseudo"], 4) if picked.get("n_pseudo") else None}
        if picked.get("steps"):                                        # the "rate" rule: count and thresholds
            rec["n_sel"] = picked["n_sel"]
            rec["rate_thr1"] = round(picked["rate_thr1"] / picked["steps"], 6)
            rec["rate_thr2"] = round(picked["rate_thr2"] / picked["steps"], 6)
        if (epo + 1) % a.valid_every == 0 or epo + 1 == a.epochs:
            _, accs, errs = T.validate(vb, emas, args)
            rec["pck"] = [round(v[-1], 4) for v in accs]               # teacher 1, teacher 2, mean
            rec["pck_per_kp_mean"] = [round(v, 4) for v in accs[-1][:-1]]
            m = max(rec["pck"])
            if m > best[0]:
                best = (m, epo + 1)
            print("epoch %3d  pck@0.2 t1 %.4f t2 %.4f mean %.4f  (%.1f s)" % (
                epo + 1, rec["pck"][0], rec["pck"][1], rec["pck"][2], time.time() - t0), flush=True)
        log["epochs"].append(rec)
    log["best_pck"], log["best_epoch"] = best
    tail = [e["sel_rate"] for e in log["epochs"][-10:] if e["sel_rate"] is not None]
    log["sel_rate_last10"] = round(sum(tail) / len(tail), 4) if tail else None
    log["final_pck"] = log["epochs"][-1]["pck"]
    log["wall_s"] = round(time.time() - t0, 1)
    if keep is not None:
        keep.update({"models": models, "emas": emas})
    if write:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(log, f, indent=1)
    return log


if __name__ == "__main__":
    main()
