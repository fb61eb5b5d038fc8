"""Generate tests/golden/unc.npz by running the REFERENCE's own uncertainty code.

TEST INFRASTRUCTURE ONLY, as gen_golden.py (whose import recipe this uses): it runs where the
reference tree is present and writes a fixture; the tests read the fixture alone.

Per view count V in 2..5: seeded float32 points [2 members, V, bs 3, k 4, 2] in [0, 512) (the
reference moves coordinates around as float32 tensors and computes on their Python floats), and
what the reference makes of them:
  ProcessUtils.coord_avgDistance of every member's V points                      -> avg
  BusinessUtils.pseudo_cal_unc with empty lma caches (a first call), the member's view-0 point as
  its "coord" and all V points as its "coords_aug", distThrMax so large that every unc is kept
                                                     -> intDist, coord_aug, extDist, aExtDist, mixDist, unc
  the same with distThrMax = t, then pseudo_filter_mixUnc                        -> thr (the t used), enable
  BusinessUtils.assess_pseudo_unc2 of the same points                            -> extViews, intDist1/2
and for V = 3 once more with two planted negative coordinates (set "3neg": coord_legal, business.py:31)
through assess_pseudo_unc2 alone, the one of the three that looks at legality.

Usage:  python tests/golden/gen_unc_golden.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden  # noqa: E402

BS, K, M = 3, 4, 2


def point_set(V, seed):
    return np.random.RandomState(seed).uniform(0, 512, (M, V, BS, K, 2)).astype(np.float32)


def _args(V, thr):
    return types.SimpleNamespace(pck_ref=[0, 1], pck_thr=0.2, distThrMax=thr, kpsCount=K, br_inferAugNum=V,
                                 mds1_lma_cache=[], mds2_lma_cache=[])


def cal_unc(B, pts, thr):
    """pseudo_cal_unc on pts [M,V,BS,K,2] -> the two members' kSample lists (bs-major, then k)."""
    V = pts.shape[1]
    ids = ["img%d" % i for i in range(BS)]
    gt = torch.from_numpy(pts[0, 0] + 1.0)
    per = []
    for m in range(M):
        coord = torch.from_numpy(pts[m, 0])                                     # [bs,k,2]
        augs = torch.from_numpy(np.ascontiguousarray(pts[m].transpose(1, 2, 0, 3)))   # [bs,k,V,2]
        per += [coord, torch.ones(BS, K), augs, torch.ones(BS, K, V)]
    return B.pseudo_cal_unc(ids, gt, *per, _args(V, thr))


def assess(B, pts):
    V = pts.shape[1]
    ids = ["img%d" % i for i in range(BS)]
    gt = torch.from_numpy(np.abs(pts[0, 0]) + 1.0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    ori = [t(pts[0, 0]), t(pts[1, 0]), t((pts[0, 0] + pts[1, 0]) / 2)]
    augs = [[t(pts[m, v]) for v in range(V)] for m in range(M)]
    pseudo, _, _ = B.assess_pseudo_unc2(ids, gt, ori, augs, _args(V, 1.0))
    g = lambda key: np.array([p[key] for p in pseudo], np.float64).reshape(BS, K)
    return g("extDist"), g("intDist1"), g("intDist2"), g("coord_legal")


def main():
    R = gen_golden.import_reference()
    from utils.business import BusinessUtils as B
    import unc_ref as UR
    out = {}
    for V in (2, 3, 4, 5):
        pts = point_set(V, 70 + V)
        name = "%d" % V
        out[name + "/pts"] = pts
        out[name + "/avg"] = np.array([[[R["P"].coord_avgDistance(pts[m, :, b, k].tolist()) for k in range(K)]
                                        for b in range(BS)] for m in range(M)], np.float64)
        members = cal_unc(B, pts, 1e9)
        g = lambda key, shape=(): np.array([[s[key] for s in mem] for mem in members],
                                           np.float64).reshape((M, BS, K) + shape)
        for key in ("intDist", "extDist", "aExtDist", "mixDist", "unc"):
            out[name + "/" + key] = g(key)
        out[name + "/coord_aug"] = g("coord_aug", (2,))
        # a threshold between two distances (the float64 restatement picks it), then the filter
        ok = np.ones(pts.shape[:-1], bool)
        gaps = UR.gaps_between(UR.fold(pts.astype(np.float64), ok, 1e9, np.float64))
        thr = float(np.float32(gaps[3 * len(gaps) // 4]))                       # (some joints kept, some not)
        members = cal_unc(B, pts, thr)
        en = []
        for mem in members:
            sel = B.pseudo_filter_mixUnc(mem, _args(V, thr))[0]
            en.append([s["enable"] for s in sel])
        out[name + "/thr"] = np.array(thr, np.float64)
        out[name + "/enable"] = np.array(en, np.float64).reshape(M, BS, K)
        ev, i1, i2, _ = assess(B, pts)
        out[name + "/extViews"], out[name + "/intDist1"], out[name + "/intDist2"] = ev, i1, i2
    pts = point_set(3, 99)
    pts[0, 1, 0, 2, 0] = -3.5                                                  # member 0: one illegal view
    pts[1, 0, 2, 1, 1] = -0.25                                                 # member 1: its view-0 point
    ev, i1, i2, legal = assess(B, pts)
    out["3neg/pts"], out["3neg/extViews"], out["3neg/intDist1"], out["3neg/intDist2"] = pts, ev, i1, i2
    out["3neg/coord_legal"] = legal
    path = os.path.join(HERE, "unc.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
