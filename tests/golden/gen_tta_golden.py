"""Generate tests/golden/tta.npz by running the REFERENCE's own heatmap back-warp.

TEST INFRASTRUCTURE ONLY, as gen_golden.py (whose import recipe this uses): it runs where the
reference tree is present and writes a fixture; the tests read the fixture alone.

Per shape (N, K, H, W): maps of rendered Gaussians with the renderer's 0.01 cutoff (so the
background is exactly zero and the fixture stays small) and 2 % multiplicative noise on their
support; one transform per sample — theta [N,2,3] by affine_getWarpmat's formula
(utils/augment.py:158-164; cv2 is absent, so getRotationMatrix2D's inverse with the translation
column zeroed is written out: scale * [[cos, -sin], [sin, cos]], as float32) plus, on some, a
translation; isflip set on some.  Outputs: AugmentUtils.affine_back2 (utils/augment.py:36-47) of
the maps and of an all-ones map (the coverage), on float32 tensors and on float64 tensors.

Usage:  python tests/golden/gen_tta_golden.py   (prints the distances DESIGN.md quotes)
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "ubpl-poseestimation_amd"))
import gen_golden  # noqa: E402

# shape -> per sample (angle_deg, scale, tx, ty, isflip); tx, ty in affine_grid's normalised units
CASES = {
    (2, 3, 8, 8): [(20.0, 1.25, 0.0, 0.0, False), (-35.0, 0.8, 0.2, -0.1, True)],
    (2, 5, 24, 40): [(15.0, 1.0, 0.1, 0.05, True), (-30.0, 1.25, 0.0, 0.0, False)],
    (2, 4, 64, 64): [(30.0, 0.75, -0.15, 0.1, False), (-12.5, 1.1, 0.0, 0.0, True)],
}


def warpmat(angle, scale):
    """affine_getWarpmat without cv2: invertAffineTransform(getRotationMatrix2D(c, angle, 1/scale))
    with the translation column zeroed, as torch.Tensor (float32)."""
    a = math.radians(angle)
    alpha, beta = math.cos(a) / scale, math.sin(a) / scale          # getRotationMatrix2D's
    det = alpha * alpha + beta * beta
    inv = np.array([[alpha / det, -beta / det, 0.0], [beta / det, alpha / det, 0.0]])
    return torch.Tensor(inv)


def maps(shape, seed):
    N, K, H, W = shape
    rs = np.random.RandomState(seed)
    sigma = max(1.0, min(H, W) / 21.0)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros(shape, np.float64)
    for n in range(N):
        for k in range(K):
            for _ in range(1 + (n + k) % 2):
                cx, cy = rs.uniform(0.15, 0.85) * (W - 1), rs.uniform(0.15, 0.85) * (H - 1)
                g = np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * sigma * sigma))
                out[n, k] = np.maximum(out[n, k], np.where(g > 0.01, g, 0.0))
    out *= 1.0 + 0.02 * rs.standard_normal(shape)
    return out.astype(np.float32)


def main():
    gen_golden.import_reference()
    from utils.augment import AugmentUtils
    out = {}
    for si, (shape, rows) in enumerate(CASES.items()):
        N, K, H, W = shape
        hm = torch.from_numpy(maps(shape, 40 + si))
        theta = torch.stack([warpmat(a, s) for a, s, _, _, _ in rows])
        for n, (_, _, tx, ty, _) in enumerate(rows):
            theta[n, 0, 2], theta[n, 1, 2] = tx, ty
        isflip = [bool(r[4]) for r in rows]
        ones = torch.ones(N, 1, H, W)
        name = "%dx%dx%dx%d" % shape
        out[name + "/hm"] = hm.numpy()
        out[name + "/theta"] = theta.numpy()
        out[name + "/isflip"] = np.array(isflip)
        with torch.no_grad():
            for tag, t in (("32", torch.float32), ("64", torch.float64)):
                out[name + "/back" + tag] = AugmentUtils.affine_back2(hm.to(t), theta.to(t), isflip).numpy()
                out[name + "/cov" + tag] = AugmentUtils.affine_back2(ones.to(t), theta.to(t), isflip).numpy()
        assert out[name + "/back32"].dtype == np.float32 and out[name + "/back64"].dtype == np.float64
    path = os.path.join(HERE, "tta.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))
    # the figures of tests/test_tta_host.py, for DESIGN.md
    import tta_ref
    from test_tta_host import fixture_distances
    for name, d in fixture_distances(dict(np.load(path)), tta_ref).items():
        print(name, " ".join("%s %.3g" % kv for kv in d.items()))


if __name__ == "__main__":
    main()
