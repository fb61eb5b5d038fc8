"""Label a pool with the teachers' UBPL ensemble pseudo-labels and see what was kept.

Loads the EMA teachers of a checkpoint (ubpl_amd.checkpoint schema: model<b>_ema_state), or
seeded, untrained networks when none is given, labels the Mouse fixture's validation split
with Predictor.label_pool, writes the result as JSON (checkpoint.save_pseudo_data: the
reference's predsArraies key plus the selection and its confidence figures) and, since that
split has ground truth, prints the selection rate and the share of valid joints within
pck_thr of the truth, for the selected joints and for all of them.

    python tools/pseudo_label.py [--ckpt ckpts/checkpoint_best.pth.tar] [--model HG2]
                                 [--thr 0.95] [--rule unanimous|ensemble] [--flip] [--out FILE]

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--model", default="HG2")
    ap.add_argument("--teachers", type=int, default=2)
    ap.add_argument("--thr", type=float, default=0.95)
    ap.add_argument("--rule", default="unanimous")
    ap.add_argument("--flip", action="store_true")
    ap.add_argument("--inferBS", type=int, default=32)
    ap.add_argument("--limit", type=int, default=0, help="label only the first batches up to this many images")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "pseudo_labels.json"))
    a = ap.parse_args()

    from ubpl_amd import Predictor, _lib, checkpoint, mouse
    from ubpl_amd.hourglass import pose_model
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    data = mouse.MouseData.from_pack()
    teachers = []
    for b in range(a.teachers):
        torch.manual_seed(b)
        teachers.append(pose_model(a.model, data.kpsCount, "AvgPool", nograd=True))
    if a.ckpt:
        ck = torch.load(a.ckpt, map_location="cpu", weights_only=True)
        for b, m in enumerate(teachers):
            m.load_state_dict(ck["model{}_ema_state".format(b + 1)])
    loader = mouse.valid_batches(data, a.inferBS, dev)
    if a.limit:
        loader = loader[:max(1, a.limit // a.inferBS)]
    P = Predictor(teachers, flip_test=a.flip, max_batch=a.inferBS)
    d = P.label_pool(loader, types.SimpleNamespace(outRes=data.outRes), thr=a.thr, rule=a.rule)
    d["source"] = {"ckpt": a.ckpt, "model": a.model, "teachers": a.teachers, "flip_test": a.flip,
                   "split": "Mouse_100_500_0.3 valid", "images": len(d["predsArraies"])}
    checkpoint.save_pseudo_data(d, a.out)

    preds = torch.tensor(d["predsArraies"])
    sel = torch.tensor(d["selected"])
    gts = torch.cat([m["kpsMap"] for _, _, m in loader])
    hit, valid = within_pck(preds, gts, data.pck_ref, data.pck_thr)
    share = lambda mask: float(hit[mask].float().mean()) if bool(mask.any()) else None
    print(json.dumps({"out": a.out, "images": len(preds), "thr": a.thr, "rule": a.rule,
                      "selected_fraction": round(float(sel.float().mean()), 4),
                      "selected_fraction_per_joint": [round(v, 4) for v in d["selected_fraction"]],
                      "within_pck_thr_all": share(valid), "within_pck_thr_selected": share(valid & sel),
                      "trained": a.ckpt is not None}))


if __name__ == "__main__":
    main()
