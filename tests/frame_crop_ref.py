"""Test infrastructure: the float64 restatement of the reference's evaluation crop,
AugmentUtils.affine_image(img, center, scale, [R, R]) with angle == 0 (utils/augment.py:91-137),
branch by branch — pre-resize the whole frame, then crop, then resize — on the scikit-image
restatements of oracle/augment_chain.py (crop_padded, sk_resize) and the product's crop_box.
It does not use the composite form the device kernel runs.  Parity with scikit-image itself is
unpinned (it is not installed here), as for the training augmentation."""
import math

import numpy as np
import torch

from oracle.augment_chain import crop_padded, sk_resize
from ubpl_amd import augment as A

F32 = torch.float32


def ref_geometry(ht, wd, center, scale, R):
    """The integers of utils/augment.py:91-110: (sf, new_ht, new_wd, ul, br); new_* None for
    sf < 2.  ValueError where the reference returns its mis-shaped zero image."""
    scale = torch.as_tensor(scale, dtype=F32).reshape(())
    sf = scale * 200.0 / R
    new_ht = new_wd = None
    center = [float(center[0]), float(center[1])]
    if not bool(sf < 2):
        new_size = int(math.floor(float(max(ht, wd) / sf)))
        new_ht = int(math.floor(float(ht / sf)))
        new_wd = int(math.floor(float(wd / sf)))
        if new_size < 2:
            raise ValueError("new_size < 2")
        center = torch.tensor(center, dtype=F32) * 1.0 / sf
        scale = scale / sf
    ul, br, _ = A.crop_box(center, scale, [R, R], 0)
    return float(sf), new_ht, new_wd, (int(ul[0]), int(ul[1])), (int(br[0]), int(br[1]))


def ref_crop(frame_bgr, center, scale, R, means):
    """frame uint8 BGR [ht,wd,3] -> float64 [3,R,R]: u8 / 255, the reference's pixel path,
    minus means[c] per channel."""
    ht, wd = frame_bgr.shape[:2]
    _, new_ht, new_wd, ul, br = ref_geometry(ht, wd, center, scale, R)
    image = frame_bgr.astype(np.float64) / 255.0
    if new_ht is not None:
        image = sk_resize(image, (new_ht, new_wd))
    new = crop_padded(image, ul, br)
    new = sk_resize(new, (R, R))
    return np.transpose(new, (2, 0, 1)) - np.asarray(means, np.float64).reshape(3, 1, 1)


CASE_RES = 32
CASE_MEANS = [0.41, 0.47, 0.53]
CASE_SIZES = [(37, 53), (20, 25), (150, 200), (301, 420), (3, 300)]
# (what it covers, frame, center (x, y), scale); sf = scale * 200 / 32
CASES = [
    ("up-scale: a 20 px box, sf 0.63", 0, (26.0, 18.0), 0.1),
    ("Gaussian radius 0, sf 1.1", 2, (100.3, 75.7), 0.176),
    ("Gaussian radius 1, sf 1.4", 2, (90.0, 70.0), 0.224),
    ("Gaussian radius 2, sf 1.95", 2, (101.5, 74.0), 0.312),
    ("pre-resize, sf 2.0", 3, (210.0, 150.0), 0.32),
    ("pre-resize, sf 2.7", 3, (200.0, 140.0), 0.432),
    ("pre-resize, sf 7.9", 3, (212.0, 151.0), 1.264),
    ("box over the left edge", 2, (5.0, 75.0), 0.224),
    ("box over the top edge", 2, (100.0, 4.0), 0.224),
    ("box over the right edge", 2, (196.0, 75.0), 0.224),
    ("box over the bottom edge", 2, (100.0, 147.0), 0.224),
    ("pre-resized box over the left and top edges", 3, (10.0, 12.0), 0.432),
    ("pre-resized box over the right and bottom edges", 3, (415.0, 295.0), 0.432),
    ("box wholly outside the frame", 1, (200.0, 200.0), 0.176),
    ("frame narrower than the Gaussian radius (3 rows, radius 4)", 4, (150.0, 1.0), 0.432),
    ("a 3-row frame inside a 62 px box", 4, (40.0, 1.0), 0.312),
    ("pre-resize of a small frame to 2 x 3, radius 18 of 20 rows", 1, (12.0, 10.0), 1.264),
    ("up-scale over a corner", 0, (2.0, 35.0), 0.1),
]


def case_frames():
    """The uint8 BGR frames of CASE_SIZES: seeded noise over a smooth ramp, the three channels
    different."""
    rs = np.random.RandomState(20)
    out = []
    for h, w in CASE_SIZES:
        ramp = (np.add.outer(np.arange(h) * 3, np.arange(w) * 2) % 200)[..., None] + np.array([0, 20, 40])
        out.append(np.clip(ramp + rs.randint(0, 56, (h, w, 3)), 0, 255).astype(np.uint8))
    return out


def plan_dense(plan, i, frame_bgr, means):
    """Box i of a frames.CropPlan evaluated densely in float64: per axis the composite weight
    matrix [R, frame length] the device kernel applies tap by tap (ubpl_hip.h ubpl_crop_frames),
    then out = Ay @ image @ Ax^T per channel, minus means."""
    from ubpl_amd.frames import _mirror
    R = plan.res

    def matrix(ax, gw, length):
        org, ls, lo, off, lb, r = (int(v) for v in ax)
        zoom = np.zeros((lo, length))                      # zoom grid <- frame pixels
        for g in range(lo):
            q = (g + 0.5) * (ls / lo) - 0.5
            f = int(np.floor(q))
            w = q - f
            for k in range(-r, r + 2):
                wk = (1 - w) * (gw[abs(k)] if abs(k) <= r else 0.0) + w * (gw[abs(k - 1)] if abs(k - 1) <= r else 0.0)
                x = org + int(_mirror(np.array(f + k), ls))
                if 0 <= x < length:
                    zoom[g, x] += wk
        out = np.zeros((R, length))
        for o in range(R):
            q = (o + 0.5) * (lb / R) - 0.5
            f = int(np.floor(q))
            w = q - f
            for t, wt in ((0, 1 - w), (1, w)):
                g = off + int(_mirror(np.array(f + t), lb))
                if 0 <= g < lo:
                    out[o] += wt * zoom[g]
        return out
    ht, wd = frame_bgr.shape[:2]
    Ax = matrix(plan.table[i, 1:7], plan.gauss[i, 0], wd)
    Ay = matrix(plan.table[i, 7:13], plan.gauss[i, 1], ht)
    img = frame_bgr.astype(np.float64) / 255.0
    out = np.stack([Ay @ img[:, :, c] @ Ax.T for c in range(3)])
    return out - np.asarray(means, np.float64).reshape(3, 1, 1)
