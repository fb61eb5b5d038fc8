"""Crop from raw frames: the reference's evaluation crop, on the device, for boxes in uint8
BGR frames of any and mixed sizes.

`Predictor.predict(images, center, scale)` uses center / scale only to map predictions back
into image coordinates; the forward half of that transform is AugmentUtils.affine_image(img,
center, scale, [R, R]) with angle = 0 (utils/augment.py:91-137), which the reference runs on
scikit-image.  Restated here:

* sf = scale * 200 / R in float32 (scale is a float32 value, as in augment.get_transform).
  sf < 2: no pre-resize.  sf >= 2: the WHOLE frame is resized to int(floor(ht / sf)) x
  int(floor(wd / sf)) (float32 divisions) by skimage.transform.resize, center := center * 1.0
  / sf and scale := scale / sf in float32.  Where the reference returns a mis-shaped zero
  image (both new sizes below 2) this raises; so does sf > 16.
* ul, br = augment.crop_box(center, scale, [R, R], 0); the box [ul, br) is cut out with zero
  fill and resized to R x R by skimage.transform.resize.
* skimage's resize: per shrinking axis a Gaussian of sigma = (in / out - 1) / 2 (truncate 4:
  radius int(4 sigma + 0.5), normalised weights, ndimage 'mirror' edges, periodic when the
  radius exceeds the length), then the bilinear sample at (o + 0.5) * in / out - 0.5 with
  mirrored indices; the clip is the identity (convex weights).
* channel c of the result is BGR channel c of u8 / 255, minus means[c]: the RGB-ordered means
  on BGR channels, the quirk mouse.to_device_images and the augment kernels keep.  On the device
  u8 / 255 is u8 * (1/255.f), the float32 value to_device_images computes there, so the identity
  crop (box = frame, sf = 1) is that function bit for bit.

`crop_plan` is the one statement of that branch logic: per box and axis the six ints
ubpl_crop_frames reads (include/ubpl_hip.h), the Gaussian weights in float64, and the source
rows the box needs.  Parity with scikit-image itself is unpinned (it is not installed where
this runs); the yardstick is the float64 restatement on scipy.ndimage in tests/frame_crop_ref.py.
"""
import math

import numpy as np
import torch

from . import kernels as Kn
from .augment import crop_box
from .kernels._check import _mirror

F32 = torch.float32
MAX_SF = 16.0
PLAN_INTS = 16


def gauss_weights(n_in, n_out):
    """The anti-aliasing Gaussian of skimage's resize n_in -> n_out along one axis:
    (radius, weights[0 .. radius] in float64, normalised over -radius .. radius)."""
    sigma = max(0.0, (n_in / n_out - 1) / 2)
    if not sigma > 1e-15:
        return 0, np.ones(1)
    r = int(4.0 * sigma + 0.5)
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return r, phi[r:]


def _axis(length, ul, br, new, R):
    """One axis of a box: (org, ls, lo, off, lb, r) and the Gaussian weights.  length: the frame's;
    [ul, br): the box; new: the pre-resized length (sf >= 2) or None (sf < 2)."""
    lb = int(br - ul)
    if lb < 1:
        raise ValueError("ubpl_amd: crop_plan: an empty box (%d pixels)" % lb)
    if new is None:
        org, ls, lo, off, lb = int(ul), lb, R, 0, R
    else:
        org, ls, lo, off = 0, int(length), int(new), int(ul)
        if gauss_weights(lb, R)[0] > 0:
            raise ValueError("ubpl_amd: crop_plan: a box of %d pixels after the pre-resize needs a second "
                             "anti-aliasing blur to reach %d, which the device crop does not run" % (lb, R))
    r, g = gauss_weights(ls, lo)
    return (org, ls, lo, off, lb, r), g


def _rows(ay, R):
    """(first, count) of the virtual-source rows the R output rows of axis ay read."""
    org, ls, lo, off, lb, r = ay
    if off == 0 and lo == R and lb == R:                  # sf < 2: the zoom grid is the output
        return 0, ls
    q = (np.arange(R) + 0.5) * (lb / R) - 0.5
    f = np.floor(q).astype(np.int64)
    g = off + np.concatenate([_mirror(f, lb), _mirror(f + 1, lb)])
    g = g[(g >= 0) & (g < lo)]
    if not g.size:
        return 0, 1
    fq = np.floor((np.array([g.min(), g.max()]) + 0.5) * (ls / lo) - 0.5).astype(np.int64)
    first, last = int(fq[0]) - r, int(fq[1]) + r + 1
    if first < 0 or last >= ls:                             # mirrored taps: anywhere in the source
        return 0, ls
    return first, last - first + 1


class CropPlan:
    """crop_plan's result: table int32 [n,16] (frame; x axis 1-6; y axis 7-12; first row, rows;
    0), gauss float64 [n,2,gw] (x, y; zero beyond each radius), rows [n] (= table[:, 14]), res,
    and per box the reference's own integers under `boxes`: sf (float32 value), branch
    ("crop" for sf < 2, "resize" for sf >= 2), ul, br (x, y), new_ht, new_wd (None for "crop")."""

    def __init__(self, table, gauss, res, boxes):
        self.table, self.gauss, self.res, self.boxes = table, gauss, int(res), boxes
        self.rows = table[:, 14].copy()

    def __len__(self):
        return self.table.shape[0]


def box_geometry(ht, wd, center, scale, R):
    """The reference's integers for one box: -> dict(sf, branch, ul, br, new_ht, new_wd)."""
    scale = torch.as_tensor(scale, dtype=F32).reshape(())
    sf = scale * 200.0 / R                                           # utils/augment.py:91 (float32)
    if bool(sf < 2):
        ul, br, _ = crop_box([float(center[0]), float(center[1])], scale, [R, R], 0)
        return {"sf": float(sf), "branch": "crop", "ul": (int(ul[0]), int(ul[1])), "br": (int(br[0]), int(br[1])),
                "new_ht": None, "new_wd": None}
    if not bool(sf <= MAX_SF):
        raise ValueError("ubpl_amd: crop_plan: sf = scale * 200 / res = %g is beyond the supported %g"
                         % (float(sf), MAX_SF))
    new_ht = int(math.floor(float(ht / sf)))                         # :96-97 (float32 divisions)
    new_wd = int(math.floor(float(wd / sf)))
    if max(new_ht, new_wd) < 2 or min(new_ht, new_wd) < 1:
        raise ValueError("ubpl_amd: crop_plan: a %dx%d frame pre-resized by sf = %g is %dx%d: too small "
                         "(the reference returns a zero image there)" % (ht, wd, float(sf), new_ht, new_wd))
    c = torch.as_tensor([float(center[0]), float(center[1])], dtype=F32) * 1.0 / sf   # :104
    ul, br, _ = crop_box(c, scale / sf, [R, R], 0)                   # :105, :108-110
    return {"sf": float(sf), "branch": "resize", "ul": (int(ul[0]), int(ul[1])), "br": (int(br[0]), int(br[1])),
            "new_ht": new_ht, "new_wd": new_wd}


def crop_plan(sizes, frame, center, scale, res):
    """Host-only and pure.  sizes: (ht, wd) per frame of the bank; frame [n] ints (None: box i
    reads frame i); center [n,2] (x, y); scale [n]; res: the output size R.  -> CropPlan."""
    R = int(res)
    if R < 1:
        raise ValueError("ubpl_amd: crop_plan: res must be positive")
    center = np.asarray(torch.as_tensor(center).cpu() if torch.is_tensor(center) else center, np.float64)
    scale = torch.as_tensor(scale, dtype=F32).reshape(-1).cpu()
    n = scale.numel()
    if frame is None:
        frame = np.arange(len(sizes))
    frame = np.asarray(torch.as_tensor(frame).cpu() if torch.is_tensor(frame) else frame)
    if center.ndim != 2 or center.shape != (n, 2) or frame.shape != (n,) or n < 1:
        raise ValueError("ubpl_amd: crop_plan: %s frames, centers of shape %s and %d scales do not describe one "
                         "set of boxes" % (frame.shape, center.shape, n))
    if frame.dtype.kind not in "iu" or (frame < 0).any() or (frame >= len(sizes)).any():
        raise ValueError("ubpl_amd: crop_plan: a frame index outside the bank's %d frames" % len(sizes))
    table = np.zeros((n, PLAN_INTS), np.int32)
    gs, boxes = [], []
    for i in range(n):
        ht, wd = (int(v) for v in sizes[int(frame[i])])
        b = box_geometry(ht, wd, center[i], scale[i], R)
        ax, gx = _axis(wd, b["ul"][0], b["br"][0], b["new_wd"], R)
        ay, gy = _axis(ht, b["ul"][1], b["br"][1], b["new_ht"], R)
        table[i, 0] = frame[i]
        table[i, 1:7], table[i, 7:13] = ax, ay
        table[i, 13:15] = _rows(ay, R)
        gs.append((gx, gy))
        boxes.append(b)
    gw = max(len(g) for pair in gs for g in pair) + 1
    gauss = np.zeros((n, 2, gw))
    for i, pair in enumerate(gs):
        for a, g in enumerate(pair):
            gauss[i, a, :len(g)] = g
    return CropPlan(table, gauss, R, boxes)


class FrameBank:
    """FrameBank(frames, means, device="cuda"): uint8 BGR frames resident on the device as one
    ragged byte bank (frame f is [H_f, W_f, 3] at bank + off[f]; the OcclusionBank layout).
    frames: a list of [H_i, W_i, 3] uint8 arrays (or tensors) of any sizes, or one [N,H,W,3]
    array; means: the RGB-ordered channel means (MouseData.getSemiData)."""

    def __init__(self, frames, means, device="cuda"):
        frames = [np.ascontiguousarray(f.cpu().numpy() if torch.is_tensor(f) else f) for f in frames]
        if not frames:
            raise ValueError("ubpl_amd: FrameBank: no frames")
        for f in frames:
            if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3 or f.shape[0] < 1 or f.shape[1] < 1:
                raise ValueError("ubpl_amd: FrameBank: frames are uint8 BGR [H, W, 3]")
        self.sizes = [tuple(int(v) for v in f.shape[:2]) for f in frames]
        self.off_host = np.concatenate([[0], np.cumsum([f.size for f in frames])[:-1]]).astype(np.int64)
        self.hw_host = np.array(self.sizes, np.int32)
        self.dev = torch.device(device)
        self.bank = torch.from_numpy(np.concatenate([f.reshape(-1) for f in frames])).to(self.dev)
        self.off = torch.from_numpy(self.off_host).to(self.dev)
        self.hw = torch.from_numpy(self.hw_host).to(self.dev)
        self.chan_mean = torch.tensor(means, dtype=F32, device=self.dev)

    def __len__(self):
        return len(self.sizes)

    def crop(self, frame, center, scale, res, out=None):
        """Box i = (frame[i], center[i] = (x, y), scale[i]) -> float32 [n,3,res,res] on the device
        (out: written in place and returned).  frame None: box i reads frame i.  Runs on torch's
        current stream, eagerly (frame sizes vary: not part of a captured graph)."""
        plan = crop_plan(self.sizes, frame, center, scale, res)
        return Kn.crop_frames(self.bank, self.off, self.hw, plan.table, plan.gauss, self.chan_mean, plan.res, out=out,
                              layout=(self.off_host, self.hw_host))

    def batches(self, center, scale, res, batch, frame=None, kps=None):
        """A generator of (imgMap, None, meta) in the shape mouse.valid_batches yields — meta
        center [B,2], scale [B] float32, kpsMap [B,K,3] (when kps is given), batch_index —
        for Predictor.label_pool / validate: the boxes cropped `batch` at a time."""
        center = torch.as_tensor(center).cpu()
        scale = torch.as_tensor(scale, dtype=F32).reshape(-1).cpu()
        frame = np.arange(len(self.sizes)) if frame is None else np.asarray(frame)
        n = scale.numel()
        if center.shape != (n, 2) or frame.shape != (n,) or (kps is not None and len(kps) != n):
            raise ValueError("ubpl_amd: FrameBank.batches: frames, centers, scales and kps differ in length")
        kps = None if kps is None else torch.as_tensor(kps, dtype=F32).cpu()
        for bi, s in enumerate(range(0, n, int(batch))):
            e = min(s + int(batch), n)
            meta = {"center": center[s:e].clone(), "scale": scale[s:e].clone(), "batch_index": bi}
            if kps is not None:
                meta["kpsMap"] = kps[s:e].clone()
            yield self.crop(frame[s:e], center[s:e], scale[s:e], res), None, meta
