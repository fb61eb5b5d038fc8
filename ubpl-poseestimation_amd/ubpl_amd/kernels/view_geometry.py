"""Host geometry of the multi-view kernels: 2x3 pixel matrices [...,6] (output pixel -> source
pixel), composed and inverted in float64 and rounded once to float32 (the convention: DESIGN.md
§4).  Pure torch — no library, no device needed; the train_* functions are tensor ops only and
run on whatever device their input is on."""
import math

import torch

MAX_VIEWS = 16
F32 = torch.float32
F64 = torch.float64


def _mat6(m):
    return torch.as_tensor(m, dtype=F64).reshape(-1, 6)


def _compose(a, b):
    """a o b of pixel matrices [...,6] (broadcast): b first, then a."""
    rows = []
    for r in (0, 3):
        rows += [a[..., r] * b[..., 0] + a[..., r + 1] * b[..., 3],
                 a[..., r] * b[..., 1] + a[..., r + 1] * b[..., 4],
                 a[..., r] * b[..., 2] + a[..., r + 1] * b[..., 5] + a[..., r + 2]]
    return torch.stack(rows, -1)


def _invert(m):
    """Pixel matrices [...,6] -> (their inverses, their determinants); non-finite where singular."""
    det = m[..., 0] * m[..., 4] - m[..., 1] * m[..., 3]
    i0, i1, i3, i4 = m[..., 4] / det, -m[..., 1] / det, -m[..., 3] / det, m[..., 0] / det
    i2 = -(i0 * m[..., 2] + i1 * m[..., 5])
    i5 = -(i3 * m[..., 2] + i4 * m[..., 5])
    return torch.stack([i0, i1, i2, i3, i4, i5], -1), det


def compose_pixels(a, b):
    """Pixel matrices [...,6] (output pixel -> source pixel) -> a o b: b first, then a, in float64."""
    return _compose(_mat6(a), _mat6(b))


def mirror_pixels(W):
    """m(x, y) = (W - 1 - x, y) as a pixel matrix [1,6] (float64)."""
    return torch.tensor([[-1.0, 0.0, W - 1.0, 0.0, 1.0, 0.0]], dtype=F64)


def affine_theta_to_pixels(theta, H, W):
    """theta [V,2,3] (or [2,3]) of F.affine_grid(..., align_corners=True) on [H,W] planes — the
    reference's affine_back2 convention, utils/augment.py:36-47: normalised output position ->
    normalised source position, -1 and 1 the centres of the first and last pixel — -> the pixel
    matrices [V,6] float64 (output pixel -> source pixel) that sample the same positions."""
    if H < 2 or W < 2:
        raise ValueError("ubpl_amd: align_corners=True normalises over H - 1 and W - 1; %dx%d has none" % (H, W))
    t = torch.as_tensor(theta, dtype=F64).reshape(-1, 2, 3)
    hx, hy = (W - 1) / 2.0, (H - 1) / 2.0
    m = torch.empty((t.shape[0], 6), dtype=F64)
    m[:, 0] = t[:, 0, 0]
    m[:, 1] = t[:, 0, 1] * (hx / hy)
    m[:, 2] = hx * (t[:, 0, 2] + 1.0 - t[:, 0, 0] - t[:, 0, 1])
    m[:, 3] = t[:, 1, 0] * (hy / hx)
    m[:, 4] = t[:, 1, 1]
    m[:, 5] = hy * (t[:, 1, 2] + 1.0 - t[:, 1, 0] - t[:, 1, 1])
    return m


def affine_pixels_to_theta(mat, H, W):
    """The inverse of affine_theta_to_pixels: pixel matrices [V,6] -> theta [V,2,3] float64."""
    if H < 2 or W < 2:
        raise ValueError("ubpl_amd: align_corners=True normalises over H - 1 and W - 1; %dx%d has none" % (H, W))
    m = _mat6(mat)
    hx, hy = (W - 1) / 2.0, (H - 1) / 2.0
    t = torch.empty((m.shape[0], 2, 3), dtype=F64)
    t[:, 0, 0] = m[:, 0]
    t[:, 0, 1] = m[:, 1] * (hy / hx)
    t[:, 0, 2] = m[:, 2] / hx - 1.0 + t[:, 0, 0] + t[:, 0, 1]
    t[:, 1, 0] = m[:, 3] * (hx / hy)
    t[:, 1, 1] = m[:, 4]
    t[:, 1, 2] = m[:, 5] / hy - 1.0 + t[:, 1, 0] + t[:, 1, 1]
    return t


def _about_centre(a, S):
    """q -> c + a (q - c), c = ((S-1)/2, (S-1)/2), a a 2x2 nested list -> one matrix row [6]."""
    c = (S - 1) / 2.0
    return [a[0][0], a[0][1], c - a[0][0] * c - a[0][1] * c, a[1][0], a[1][1], c - a[1][0] * c - a[1][1] * c]


def view_matrices(views, flip, R, H):
    """The matrices of test-time-augmentation views on square planes ("Multi-view
    decode").  views: [(angle_deg, zoom), ...]; A = R(angle) / zoom, R(a) = [[cos a, -sin a],
    [sin a, cos a]], y down, so zoom > 1 magnifies.  The view image is view(q) = img(c + A (q - c));
    the original frame's heatmap at p samples the view's at q = c_h + A^-1 (p - c_h).  flip: every
    view once more mirrored, after the plain ones — view_f(q) = view(m(q)), its heatmap sampled at
    m(q), m(x, y) = (S - 1 - x, y) — with swap = 1 (the joint permutation is not geometry).
    -> host (img_mat [V,6] on [R,R] planes, hm_mat [V,6] on [H,H] planes, both output pixel ->
    source pixel, float64 rounded to float32; swap [V] int32)."""
    img, hm = [], []
    for angle, zoom in views:
        a = math.radians(float(angle))
        co, si, z = math.cos(a), math.sin(a), float(zoom)
        img.append(_about_centre([[co / z, -si / z], [si / z, co / z]], R))
        hm.append(_about_centre([[co * z, si * z], [-si * z, co * z]], H))
    img, hm = _mat6(img), _mat6(hm)
    swap = [0] * len(img)
    if flip:
        # view_f(q) = img(M m(q)): M o m on the image; the heatmap is read at m(q(p)): m o M
        img = torch.cat([img, compose_pixels(img, mirror_pixels(R))])
        hm = torch.cat([hm, compose_pixels(mirror_pixels(H), hm)])
        swap = swap + [1] * len(swap)
    return img.to(F32), hm.to(F32), torch.tensor(swap, dtype=torch.int32)


# ---- view-consistency uncertainty (csrc/uncertainty.hip; the rule: include/ubpl_hip.h)
def view_back_matrices(hm_mat):
    """view_matrices' hm_mat [V,6] (original-frame heatmap pixel -> view heatmap pixel) -> host
    float32 [V,6], view heatmap pixel -> original-frame heatmap pixel: the inverse of each (float32)
    matrix taken in float64 and rounded once.  ValueError on a singular matrix."""
    inv, det = _invert(_mat6(hm_mat.detach().cpu() if torch.is_tensor(hm_mat) else hm_mat))
    if not bool(((det != 0) & torch.isfinite(det)).all()):
        raise ValueError("ubpl_amd: view_back_matrices takes invertible pixel matrices")
    return inv.to(F32)


def _viewmat(viewmat):
    """The training step's view matrices, [V,N,6] or a list of V [N,6], as one float64 [V,N,6]."""
    m = torch.stack(list(viewmat)) if isinstance(viewmat, (list, tuple)) else viewmat
    if m.dim() != 3 or m.shape[-1] != 6:
        raise ValueError("ubpl_amd: viewmat is [V,N,6], one pixel matrix per view and sample")
    return m.to(F64)


def train_back_matrices(viewmat, R, H):
    """The back matrices of the training step's views for view_uncertainty_samples.
    viewmat: [V,N,6] (or a list of V [N,6]) float32, DeviceAugment.views(with_mats=True)'s matrices
    (warp_matrix: 0-based view input pixel -> 0-based source-image pixel), on any device; R the
    views' input side, H the heatmaps'.  -> float32 [V,N,6] on viewmat's device: 0-based heatmap
    cell -> source-image pixel, back = viewmat o C.

    The cell convention C is the renderer's, inverted.  render_batch centres the Gaussian of a
    keypoint at view pixel x on the 0-based cell x / (R/H) (csrc/render.hip: cx = trunc(x) /
    stride), so C(c) = (R/H) c on both axes, and a decoded 1-based peak raw enters the kernel as
    c = raw - 1.  The keypoint coordinates the loader hands the renderer are taken as the view's
    pixel coordinates, as the renderer takes them; the reference's keypoint path (transform_point:
    p - 1, the float64 product truncated, + 1; kps_fliplr: W - x) lands within a pixel of where
    warp_matrix puts the same source pixel (DESIGN.md §4 has the measured offsets).
    Composed in float64 and rounded once to float32, as compose_pixels does, with tensor ops only:
    on the device it needs no host synchronisation and can be captured."""
    m = _viewmat(viewmat)
    s = float(R) / float(H)
    out = m * s                                                 # the linear part: a cell is R/H pixels
    out[..., 2::3] = m[..., 2::3]                               # C has no offset: the translation stays
    return out.to(F32).contiguous()


# ---- cross-view pseudo-label targets (csrc/view_merge.hip)
def train_pair_matrices(viewmat, R, H):
    """The pair matrices of the training step's views for merge_views_samples.  viewmat, R, H as
    train_back_matrices takes them (view v's matrix Mv: 0-based view input pixel -> 0-based
    source-image pixel).  -> float32 [V,V,N,6] on viewmat's device: P[a][v][n] maps a 0-based
    heatmap cell of view a to the 0-based heatmap cell of view v that shows the same source pixel,

        P[a][v] = C^-1 o inv(Mv) o Ma o C,    C(c) = (R/H) c

    — train_back_matrices' cell convention, so the gate and the targets agree.  In float64, in this
    order: inv(Mv) as view_back_matrices takes it; L = inv(Mv) o Ma as compose_pixels does; the
    linear part of P is L's, its translation L's divided by R/H; rounded once to float32.  The
    diagonal a == v is written as exactly (1,0,0,0,1,0).  A singular Mv gives non-finite entries,
    which the kernel's sampling rule counts as outside.  Tensor ops only: on the device it needs no
    host synchronisation and can be captured."""
    m = _viewmat(viewmat)
    V = m.shape[0]
    inv, _ = _invert(m)                                      # [V,N,6]
    out = _compose(inv.unsqueeze(0), m.unsqueeze(1))         # a o b at [target a][source v]: inv(Mv) o Ma
    out[..., 2::3] /= float(R) / float(H)
    out = out.to(F32)                                        # [V,V,N,6]
    eye = (torch.arange(6, device=out.device) % 4 == 0).to(F32)   # (1,0,0,0,1,0) without a host -> device copy
    diag = torch.eye(V, dtype=torch.bool, device=out.device).reshape(V, V, 1, 1)
    return torch.where(diag, eye, out).contiguous()
