"""A numpy restatement of kernels.train_pair_matrices and ubpl_merge_views_samples
(include/ubpl_hip.h), built on tta_ref.sample_plane — the one sampling rule — and shared by the
cross-view tests.  Every product, sum and quotient is one numpy operation in the dtype given, in
the kernel's order: the float32 instance gives the kernel's bits, the float64 one is a yardstick."""
import numpy as np

import tta_ref as TR

IDENTITY = np.array(TR.IDENTITY, np.float32)


def pair_matrices(viewmat, R, H):
    """viewmat [V,N,6] float32 (view pixel -> source pixel) -> P [V,V,N,6] float32: P[a][v][n]
    maps a 0-based heatmap cell of view a to view v's.  float64 in train_pair_matrices' op order:
    inv(Mv) (view_back_matrices' formula), L = inv(Mv) o Ma (compose_pixels' formula), the
    translation over R/H; rounded once; the diagonal exactly the identity."""
    m = np.asarray(viewmat, np.float32).astype(np.float64)
    V, N = m.shape[:2]
    s = float(R) / float(H)
    with np.errstate(all="ignore"):
        det = m[..., 0] * m[..., 4] - m[..., 1] * m[..., 3]
        inv = np.empty_like(m)
        inv[..., 0], inv[..., 1] = m[..., 4] / det, -m[..., 1] / det
        inv[..., 3], inv[..., 4] = -m[..., 3] / det, m[..., 0] / det
        inv[..., 2] = -(inv[..., 0] * m[..., 2] + inv[..., 1] * m[..., 5])
        inv[..., 5] = -(inv[..., 3] * m[..., 2] + inv[..., 4] * m[..., 5])
        P = np.empty((V, V, N, 6), np.float64)
        for a in range(V):
            for v in range(V):
                i, b = inv[v], m[a]
                for r in (0, 3):
                    P[a, v, :, r + 0] = i[:, r] * b[:, 0] + i[:, r + 1] * b[:, 3]
                    P[a, v, :, r + 1] = i[:, r] * b[:, 1] + i[:, r + 1] * b[:, 4]
                    P[a, v, :, r + 2] = (i[:, r] * b[:, 2] + i[:, r + 1] * b[:, 5] + i[:, r + 2]) / s
        P = P.astype(np.float32)
    for a in range(V):
        P[a, a] = IDENTITY
    return P


def merge_views_samples(hm, P, include_self, dtype=np.float32):
    """hm [V,M,N,K,H,W], P [V,V,N,6] -> (out [V,M,N,K,H,W], cover [V,N,H,W]): per target view a
    and sample n, the source views in ascending v — v == a as it is (skipped without include_self,
    its matrix never read), the others sampled under P[a][v][n] — num / den with sequential sums,
    0 where den is not > 0; cover = den."""
    hm = np.asarray(hm, dtype)
    V, M, N, K, H, W = hm.shape
    P = np.asarray(P, np.float32).reshape(V, V, N, 6)
    out = np.empty(hm.shape, dtype)
    cover = np.empty((V, N, H, W), dtype)
    with np.errstate(all="ignore"):
        for a in range(V):
            for n in range(N):
                num = den = None
                for v in range(V):
                    if v == a:
                        if not include_self:
                            continue
                        s, c = hm[v, :, n].copy(), np.ones((H, W), dtype)
                    else:
                        s, c = TR.sample_plane(hm[v, :, n], P[a, v, n], dtype)
                    num, den = (s, c) if num is None else (num + s, den + c)
                out[a, :, n] = np.where(den > 0, num / np.where(den > 0, den, dtype(1)), dtype(0))
                cover[a, n] = den
    return out, cover
