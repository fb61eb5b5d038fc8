"""Label a pool with the teachers' UBPL ensemble pseudo-labels and see what was kept.

Loads the EMA teachers of a checkpoint (ubpl_amd.checkpoint schema: model<b>_ema_state), or
seeded, untrained networks when none is given, labels the Mouse fixture's validation split
with Predictor.label_pool, writes the result as JSON (checkpoint.save_pseudo_data: the
reference's predsArraies key plus the selection and its confidence figures) and, since that
split has ground truth, prints the selection rate and the share of valid joints within
pck_thr of the truth, for the selected joints and for all of them.

    python tools/pseudo_label.py [--ckpt ckpts/checkpoint_best.pth.tar] [--model HG2]
                                 [--thr 0.95] [--rule unanimous|ensemble|uncertainty] [--dist-thr a,b,c]
                                 [--flip] [--out FILE]
                                 [--refine none|quarter|taylor|all] [--blur-sigma S]
                                 [--train-epochs E] [--record FILE] [--tta rows|A:Z,A:Z,...]

--refine / --blur-sigma: the Predictor's sub-pixel decode (predsArraies then holds the
sub-pixel coordinates).  --refine all labels the split once per variant — none, quarter,
taylor at blur sigma 0, 1 and 2 — with the same weights, and --record writes, per variant, the
PCK@pck_thr of the ensemble peak, of the teachers' mean (Predictor.validate) and the mean
pixel error over the valid joints.  --train-epochs E: without --ckpt, train the teachers
first by E epochs of tools/mouse_pck.py's experiment (once, shared by every variant).

--tta: the Predictor's test-time augmentation, as angle_deg:zoom pairs whose first is 0:1
(with --flip every view also mirrored).  --tta rows labels the split once per row of views —
none; flip; three zooms; three zooms + two rotations; those five with flip — for every refine
variant asked for (--refine takes a comma-separated list too), with the same weights.

--rule uncertainty --dist-thr a,b,c: the view-consistency rule (Predictor(uncertainty=True), so
rows of fewer than 2 views are left out), labelled once per distance threshold (image pixels)
on the same Predictor.  --rule takes a comma-separated list, e.g. ensemble,uncertainty, to put
the score rule beside it with the same weights and views.

--frames DIR --boxes FILE.json: label one box per image of DIR instead — images of any and mixed
sizes, read with PIL; FILE.json holds one [x, y, scale] per image (a {file name: box} object, or a
list in the sorted order of DIR's images).  The crops are made on the device (ubpl_amd.frames);
there is no ground truth, so only the selection is printed.  The first --rule / --refine applies.

Reads tests/golden/mouse_100_500_0.3/ (tools/pack_mouse.py).  Untrained networks select
next to nothing at the default threshold; that is the expected output without --ckpt.
"""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ubpl-poseestimation_amd"))

import torch  # noqa: E402


def within_pck(preds, gts, ref, thr):
    """preds [N,K,2], gts [N,K,3] (host) -> (hit [N,K] bool, valid [N,K] bool): the distance
    rule of EvaluationUtils.acc_pck (utils/evaluation.py:118-139) per joint."""
    norm = (gts[:, ref[0], :2] - gts[:, ref[1], :2]).norm(dim=-1, keepdim=True)
    valid = (gts[..., 0] > 1) & (gts[..., 1] > 1)
    dist = (preds - gts[..., :2]).norm(dim=-1)
    return (dist / norm < thr) & valid, valid


TTA_ZOOMS = [(0.0, 1.0), (0.0, 0.85), (0.0, 1.15)]
TTA_ROTATIONS = [(15.0, 1.0), (-15.0, 1.0)]
TTA_ROWS = [("none", None, False), ("flip", None, True), ("3 zooms", TTA_ZOOMS, False),
            ("3 zooms + 2 rotations", TTA_ZOOMS + TTA_ROTATIONS, False),
            ("3 zooms + 2 rotations, flip", TTA_ZOOMS + TTA_ROTATIONS, True)]


def tta_rows(spec, flip):
    """--tta / --flip -> [(row name, views or None, flip_test)]."""
    if spec is None:
        return [("flip" if flip else "none", None, flip)]
    if spec == "rows":
        return TTA_ROWS
    views = [tuple(float(v) for v in item.split(":")) for item in spec.split(",")]
    return [(spec + (", flip" if flip else ""), views, flip)]


def read_frames(frames_dir, boxes_file):
    """--frames DIR --boxes FILE.json -> (names, uint8 BGR frames of any sizes, [[x, y, scale]]).
    FILE.json: {image file name: [x, y, scale]}, or a list of [x, y, scale] for DIR's images in
    sorted order — the box centre in pixels and the reference's scale (box side / 200)."""
    import numpy as np
    from PIL import Image
    with open(boxes_file) as f:
        boxes = json.load(f)
    names = sorted(boxes) if isinstance(boxes, dict) else sorted(
        n for n in os.listdir(frames_dir) if n.lower().endswith((".png", ".jpg", ".jpeg", ".bmp")))
    rows = [boxes[n] for n in names] if isinstance(boxes, dict) else boxes
    if len(rows) != len(names) or not names or any(len(r) != 3 for r in rows):
        raise SystemExit("pseudo_label: %d images in %s for %d boxes of [x, y, scale]" % (len(names), frames_dir, len(rows)))
    frames = [np.asarray(Image.open(os.path.join(frames_dir, n)).convert("RGB"), dtype=np.uint8)[:, :, ::-1].copy()
              for n in names]
    return names, frames, rows


def label_frames(a, teachers, data, rules, dev):
    """--frames: label one box per image of a directory (any image sizes) instead of the Mouse
    split: the crops come from the device (frames.FrameBank), there is no ground truth to score."""
    from ubpl_amd import Predictor, checkpoint
    from ubpl_amd.frames import FrameBank
    if not a.boxes:
        raise SystemExit("pseudo_label: --frames needs --boxes FILE.json")
    names, frames, rows = read_frames(a.frames, a.boxes)
    means = data.getSemiData(100, 500, 0.3)[6]
    bank = FrameBank(frames, means, dev)
    center = torch.tensor([r[:2] for r in rows], dtype=torch.float64)
    scale = torch.tensor([r[2] for r in rows], dtype=torch.float32)
    views = tta_rows(a.tta, a.flip)[0][1]
    rule, dist_thr = rules[0]
    P = Predictor(teachers, flip_test=a.flip, max_batch=a.inferBS, refine=a.refine.split(",")[0], tta=views,
                  uncertainty=rule == "uncertainty",
                  **({} if a.blur_sigma is None else {"blur_sigma": a.blur_sigma}))
    d = P.label_pool(bank.batches(center, scale, data.inpRes, a.inferBS), types.SimpleNamespace(outRes=data.outRes),
                     thr=a.thr, rule=rule, dist_thr=dist_thr)
    P.release()
    d["source"] = {"ckpt": a.ckpt, "model": a.model, "teachers": a.teachers, "flip_test": a.flip, "frames": a.frames,
                   "boxes": a.boxes, "images": names, "sizes": [list(s) for s in bank.sizes]}
    checkpoint.save_pseudo_data(d, a.out)
    print(json.dumps({"out": a.out, "images": len(names), "thr": a.thr, "rule": rule,
                      "selected_fraction": round(float(torch.tensor(d["selected"]).float().mean()), 4),
                      "selected_fraction_per_joint": [round(v, 4) for v in d["selected_fraction"]]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default=None, help="label the images of this directory (any sizes) instead of the "
                                                   "Mouse split; needs --boxes")
    ap.add_argument("--boxes", default=None, help="JSON: one [x, y, scale] per image of --frames")
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--model", default="HG2")
    ap.add_argument("--teachers", type=int, default=2)
    ap.add_argument("--thr", type=float, default=0.95)
    ap.add_argument("--rule", default="unanimous", help="unanimous, ensemble, uncertainty, or a comma-separated list")
    ap.add_argument("--dist-thr", default=None, help="rule uncertainty: distance thresholds in image pixels, a,b,c")
    ap.add_argument("--flip", action="store_true")
    ap.add_argument("--inferBS", type=int, default=32)
    ap.add_argument("--limit", type=int, default=0, help="label only the first batches up to this many images")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "pseudo_labels.json"))
    ap.add_argument("--refine", default="none", help="none, quarter, taylor, a comma-separated list of them, or all")
    ap.add_argument("--tta", default=None, help="angle:zoom,... (first 0:1), or rows")
    ap.add_argument("--blur-sigma", type=float, default=None, help="taylor's blur (default: the Predictor's)")
    ap.add_argument("--train-epochs", type=int, default=0, help="without --ckpt: train the teachers this long first")
    ap.add_argument("--record", default=None, help="write the per-variant accuracy figures here")
    a = ap.parse_args()

    from ubpl_amd import Predictor, _lib, checkpoint, mouse
    from ubpl_amd.hourglass import pose_model
    from ubpl_amd.predict_args import DEFAULT_BLUR_SIGMA, check_rule, view_count
    rules = []                                   # (rule, dist_thr or None), one labelling each
    for rule in a.rule.split(","):
        if check_rule(rule) != "uncertainty":
            rules.append((rule, None))
            continue
        if not a.dist_thr:
            ap.error("--rule uncertainty needs --dist-thr (the reference ships no default)")
        rules += [(rule, float(t)) for t in a.dist_thr.split(",")]
    unc = any(r == "uncertainty" for r, _ in rules)
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    data = mouse.MouseData.from_pack()
    teachers, trained = [], None
    if a.train_epochs > 0 and not a.ckpt:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        import mouse_pck
        keep = {}
        log = mouse_pck.run(mouse_pck.parser().parse_args(["--epochs", str(a.train_epochs), "--model", a.model,
                                                           "--valid-every", str(a.train_epochs)]), write=False, keep=keep)
        teachers = keep["emas"][:a.teachers]
        trained = {"epochs": a.train_epochs, "final_pck": log["final_pck"], "wall_s": log["wall_s"]}
    for b in range(len(teachers), a.teachers):
        torch.manual_seed(b)
        teachers.append(pose_model(a.model, data.kpsCount, "AvgPool", nograd=True))
    if a.ckpt:
        ck = torch.load(a.ckpt, map_location="cpu", weights_only=True)
        for b, m in enumerate(teachers):
            m.load_state_dict(ck["model{}_ema_state".format(b + 1)])
    if a.frames:
        return label_frames(a, teachers, data, rules, dev)
    loader = mouse.valid_batches(data, a.inferBS, dev)
    if a.limit:
        loader = loader[:max(1, a.limit // a.inferBS)]
    gts = torch.cat([m["kpsMap"] for _, _, m in loader])
    sigma = DEFAULT_BLUR_SIGMA if a.blur_sigma is None else a.blur_sigma
    variants = [(r, sigma) for r in a.refine.split(",")] if a.refine != "all" else \
        [("none", sigma), ("quarter", sigma), ("taylor", 0.0), ("taylor", 1.0), ("taylor", 2.0)]
    rows_of_views = tta_rows(a.tta, a.flip)
    vargs = types.SimpleNamespace(outRes=data.outRes, pck_ref=data.pck_ref, pck_thr=data.pck_thr)
    rows = []
    if unc:                                      # view consistency needs views to compare
        rows_of_views = [t for t in rows_of_views if view_count(t[1], t[2]) >= 2]
    several = len(variants) * len(rows_of_views) * len(rules) > 1
    for refine, sg, (row_name, views, flip), (rule, dist_thr) in [(r, g, t, u) for r, g in variants
                                                                  for t in rows_of_views for u in rules]:
        P = Predictor(teachers, flip_test=flip, max_batch=a.inferBS, refine=refine, blur_sigma=sg, tta=views,
                      uncertainty=unc)
        d = P.label_pool(loader, types.SimpleNamespace(outRes=data.outRes), thr=a.thr, rule=rule, dist_thr=dist_thr)
        d["source"] = {"ckpt": a.ckpt, "model": a.model, "teachers": a.teachers, "flip_test": flip,
                       "split": "Mouse_100_500_0.3 valid", "images": len(d["predsArraies"]), "trained": trained}
        out = a.out if not several else "%s.%s%s%s%s.json" % (
            os.path.splitext(a.out)[0], refine, "_s%g" % sg if refine == "taylor" else "",
            "" if len(rows_of_views) == 1 else ".v%d" % P.passes,
            "" if len(rules) == 1 else ".%s%s" % (rule, "" if dist_thr is None else "_%g" % dist_thr))
        checkpoint.save_pseudo_data(d, out)
        preds = torch.tensor(d["predsArraies"])
        sel = torch.tensor(d["selected"])
        hit, valid = within_pck(preds, gts, data.pck_ref, data.pck_thr)
        share = lambda mask: float(hit[mask].float().mean()) if bool(mask.any()) else None
        _, accs, _ = P.validate(loader, vargs)
        P.release()
        rows.append({"out": out, "refine": refine, "blur_sigma": sg if refine == "taylor" else None,
                     "views": row_name, "tta": views, "flip_test": flip,
                     "forward_passes_per_image": P.passes,
                     "images": len(preds), "thr": a.thr, "rule": rule, "dist_thr": dist_thr,
                     "selected_fraction": round(float(sel.float().mean()), 4),
                     "selected_fraction_per_joint": [round(v, 4) for v in d["selected_fraction"]],
                     "within_pck_thr_all": share(valid), "within_pck_thr_selected": share(valid & sel),
                     "mean_pixel_error": float((preds - gts[..., :2]).norm(dim=-1)[valid].mean()),
                     "validate_pck": [round(v[-1], 4) for v in accs],     # teacher 1, ..., their mean
                     "trained": a.ckpt is not None or trained is not None})
        if unc:                                  # how large the distances are, legal members only (image pixels)
            legal = torch.tensor(d["int_dist"]) < 999
            q = lambda t: [round(float(v), 3) for v in torch.quantile(t, torch.tensor([0.25, 0.5, 0.75]))] \
                if t.numel() else None
            rows[-1].update({"legal_member_fraction": round(float(legal.float().mean()), 4),
                             "int_dist_quartiles": q(torch.tensor(d["int_dist"])[legal]),
                             "ext_dist_quartiles": q(torch.tensor(d["ext_dist"])[torch.tensor(d["ext_dist"]) < 999])})
        print(json.dumps(rows[-1]))
    if a.record:
        os.makedirs(os.path.dirname(os.path.abspath(a.record)), exist_ok=True)
        with open(a.record, "w") as f:
            json.dump({"tool": "pseudo_label", "split": "Mouse_100_500_0.3 valid", "model": a.model,
                       "teachers": a.teachers, "flip_test": a.flip, "ckpt": a.ckpt, "training": trained,
                       "pck_thr": data.pck_thr, "pck_ref": data.pck_ref, "variants": rows}, f, indent=1)
            f.write("\n")

if __name__ == "__main__":
    main()
