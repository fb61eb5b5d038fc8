"""Device augmentation (f1): image means, the view warps, the occlusion pastes and the
evaluation crop from raw frames, with the host checks of their small tables."""
import torch

from .. import _lib
from . import _check
from ._check import F32


def image_mean_u8(imgs):
    """imgs uint8 [N,H,W,3] -> per-image mean / 255 (noisy_mean's mu), float32 [N]."""
    _check._chk(imgs, "imgs", torch.uint8)
    out = torch.empty(imgs.shape[0], device=imgs.device, dtype=F32)
    _lib.call("ubpl_image_mean_u8", imgs, imgs.shape[0], imgs[0].numel(), out)
    return out


def augment_warp(imgs, src_idx, mat, noise, img_mean, chan_mean, out):
    """One launch for V augmented views (see augment.hip): out [V,3,Ho,Wo]."""
    _check._chk(imgs, "imgs", torch.uint8)
    _check._chk(src_idx, "src_idx", torch.int32)
    for t, n in ((mat, "mat"), (noise, "noise"), (img_mean, "img_mean"), (chan_mean, "chan_mean"), (out, "out")):
        _check._chk(t, n)
    V, _, Ho, Wo = out.shape
    if mat.numel() != 6 * V or noise.numel() != 3 * V or src_idx.numel() != V:
        raise ValueError("augment_warp: per-view tables do not match %d views" % V)
    _lib.call("ubpl_augment_warp", imgs, imgs.shape[1], imgs.shape[2], src_idx, mat, noise, img_mean, chan_mean, V, Ho,
              Wo, out)
    return out


def augment_chain(imgs, geo, cs, noise, img_mean, chan_mean, Hm, Wm, out):
    """The reference's two resamplings per view (see augment.hip
    ubpl_augment_chain): geo int32 [V,8] (src, flip, ul_x, ul_y, Hp, Wp, Hc, Wc),
    cs float32 [V,2] (cos, sin); out [V,3,Ho,Wo].  Stage-1 scratch [V,3,Hm,Wm]."""
    _check._chk(imgs, "imgs", torch.uint8)
    _check._chk(geo, "geo", torch.int32)
    for t, n in ((cs, "cs"), (noise, "noise"), (img_mean, "img_mean"), (chan_mean, "chan_mean"), (out, "out")):
        _check._chk(t, n)
    V, _, Ho, Wo = out.shape
    if geo.numel() != 8 * V or cs.numel() != 2 * V or noise.numel() != 3 * V:
        raise ValueError("augment_chain: per-view tables do not match %d views" % V)
    g = geo.reshape(V, 8).cpu() if geo.is_cuda else geo.reshape(V, 8)
    if (g[:, 6] > Hm).any() or (g[:, 7] > Wm).any() or (g[:, 6] < 1).any() or (g[:, 7] < 1).any() or \
            (g[:, 0] < 0).any() or (g[:, 0] >= imgs.shape[0]).any():
        raise ValueError("augment_chain: a view's stripped crop exceeds %dx%d or its source index is out of range"
                         % (Hm, Wm))
    # skimage.transform.resize anti-aliases a downscale with a Gaussian of sigma = (s - 1) / 2
    # (s = crop / output); the device resize omits it, which is exact to f32 only while its
    # off-centre weight exp(-1 / (2 sigma^2)) stays below f32 rounding: s <= 1.3 (2e-10 there;
    # the loaders' defaults draw s <= 1.25).  A larger crop would silently leave the reference.
    s = max(float((g[:, 6].double() / Ho).max()), float((g[:, 7].double() / Wo).max()))
    if s > 1.3:
        raise ValueError("augment_chain: a crop %.3fx the output size needs skimage's anti-aliasing blur "
                         "(sigma %.3f px), which the device resize does not run; crops up to 1.3x are exact"
                         % (s, (s - 1) / 2))
    inter = torch.empty((V, 3, Hm, Wm), device=out.device, dtype=F32)
    _lib.call("ubpl_augment_chain", imgs, imgs.shape[1], imgs.shape[2], geo, cs, noise, img_mean, chan_mean, V, int(Hm),
              int(Wm), inter, Ho, Wo, out)
    return out


CROP_WORKSPACE_BYTES = 256 << 20
CROP_MAX_BOXES = 65535          # boxes of one ubpl_crop_frames launch (the box is the grid's y index)


def _crop_chunks(rows, R, budget=None):
    """[(first box, end box)] such that a chunk's intermediate — boxes x 3 x (its largest row
    count) x R floats — stays within budget bytes (default CROP_WORKSPACE_BYTES; a single box
    may exceed it) and a chunk holds at most CROP_MAX_BOXES boxes."""
    budget = CROP_WORKSPACE_BYTES if budget is None else budget
    chunks, a, top = [], 0, 0
    for i, r in enumerate(rows):
        if i > a and ((i + 1 - a) * 12 * max(top, int(r)) * R > budget or i - a >= CROP_MAX_BOXES):
            chunks.append((a, i))
            a, top = i, 0
        top = max(top, int(r))
    return chunks + [(a, len(rows))]


def crop_frames(bank, off, hw, table, gauss, chan_mean, res, out=None, layout=None):
    """The reference's evaluation crop of n boxes out of a ragged uint8 BGR frame bank (see
    frame_crop.hip): bank / off / hw on the device (frame f is [h,w,3] at bank + off[f]); table
    int32 [n,16] and gauss [n,2,gw] the HOST plan of ubpl_amd.frames.crop_plan; out float32
    [n,3,res,res].  layout: host copies of (off, hw) for the bounds check (else read back).
    The boxes run in chunks whose intermediate stays within CROP_WORKSPACE_BYTES."""
    _check._chk(bank, "bank", torch.uint8)
    _check._chk(off, "off", torch.int64)
    _check._chk(hw, "hw", torch.int32)
    _check._chk(chan_mean, "chan_mean")
    R = int(res)
    off_h, hw_h = layout if layout is not None else (off.cpu().numpy(), hw.cpu().numpy())
    _check._crop_plan(table, gauss, off_h, hw_h, bank.numel(), R)
    n, gw = gauss.shape[0], gauss.shape[2]
    if out is None:
        out = torch.empty((n, 3, R, R), device=bank.device, dtype=F32)
    _check._chk(out, "out")
    _check._same_shape("out", out, (n, 3, R, R))
    plan = torch.from_numpy(table.astype("int32")).to(bank.device)
    g = torch.from_numpy(gauss.astype("float32")).to(bank.device)
    for a, e in _crop_chunks(table[:, 14], R):
        rows = int(table[a:e, 14].max())
        inter = torch.empty(int(_lib.lib().ubpl_crop_frames_workspace(e - a, rows, R)), device=bank.device, dtype=F32)
        _lib.call("ubpl_crop_frames", bank, off, hw, plan[a:e], g[a:e], gw, chan_mean, e - a, rows, R, inter, out[a:e])
    return out


def _occlude_check(V, H, W, nbank, off, hw, pastes, view_first):
    """Every index occlude_kernel derives from a paste row stays inside its
    buffer (host copies of the small tables; occlusion is opt-in)."""
    if not pastes.numel():
        return
    noff = off.numel()
    pr = pastes.reshape(-1, 9).cpu().numpy().astype("int64")
    vf = view_first.cpu().numpy().astype("int64")
    hwh = hw.reshape(-1, 2).cpu().numpy().astype("int64")
    if vf[0] != 0 or (vf[1:] < vf[:-1]).any() or vf[-1] != len(pr):
        raise ValueError("occlude: view_first is not a running count of %d paste rows" % len(pr))
    v, oc, w1, h1, x0, y0, x1, y1 = (pr[:, i] for i in range(8))
    sx0, sy0 = pr[:, 8] & 0xFFFF, pr[:, 8] >> 16
    bad = ((v < 0) | (v >= V) | (oc < 0) | (oc >= min(noff, len(hwh))) | (w1 <= 0) | (h1 <= 0)
           | (x0 < 0) | (y0 < 0) | (x1 > W) | (y1 > H) | (x1 < x0) | (y1 < y0)
           | (sx0 + (x1 - x0) > w1) | (sy0 + (y1 - y0) > h1))
    if bad.any():
        raise ValueError("occlude: paste row %d is out of range for %dx%d views / %d occluders" % (
            int(bad.nonzero()[0][0]), H, W, noff))
    h, w = hwh[oc, 0], hwh[oc, 1]
    if (h <= 0).any() or (w <= 0).any():
        raise ValueError("occlude: an occluder of the bank has an empty size")
    offh = off.cpu().numpy().astype("int64")[oc]
    if (offh < 0).any() or (offh + h * w * 4 > nbank).any():
        raise ValueError("occlude: an occluder reaches past the end of the bank")


def occlude(out, bank, off, hw, pastes, view_first, chan_mean):
    """Random occlusion pastes onto augmented views in place (see augment.hip
    occlude_kernel): out [V,3,H,W]; bank / off / hw: the occluder bank;
    pastes int32 [P,9] sorted by view; view_first int32 [V+1]."""
    _check._chk(out, "out")
    _check._chk(bank, "bank")
    _check._chk(off, "off", torch.int64)
    _check._chk(hw, "hw", torch.int32)
    _check._chk(pastes, "pastes", torch.int32)
    _check._chk(view_first, "view_first", torch.int32)
    _check._chk(chan_mean, "chan_mean")
    V, _, H, W = out.shape
    if view_first.numel() != V + 1 or (pastes.numel() and pastes.shape[-1] != 9):
        raise ValueError("occlude: paste table does not match %d views" % V)
    _occlude_check(V, H, W, bank.numel(), off, hw, pastes, view_first)
    _lib.call("ubpl_occlude", out, V, H, W, bank, off, hw, pastes, view_first, chan_mean)
    return out
