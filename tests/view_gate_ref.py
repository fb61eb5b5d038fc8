"""A numpy restatement of ubpl_view_uncertainty_samples (include/ubpl_hip.h): ubpl_view_uncertainty
with one back matrix per (view, sample), no joint swap and no tinv, and the gate.  The fold of the
points is unc_ref.fold itself; only the mapping of the points and the gate are stated here."""
import numpy as np

from unc_ref import KEYS, fold, gaps_between, thresholds_between  # noqa: F401

KEYS_GATE = KEYS + ("gate",)


def points(raw, back, dtype=np.float32):
    """raw [M,V,N,K,2] (1-based view-frame peaks), back [V,N,6] -> (pts [M,V,N,K,2] in the frame back
    maps to, ok [M,V,N,K] bool: the point is legal).  Each product and sum one operation in dtype,
    in the kernel's order."""
    raw = np.asarray(raw, np.float32)
    M, V, N, K, _ = raw.shape
    b = np.asarray(back, np.float32).reshape(V, N, 6).astype(dtype)[None, :, :, None, :]    # [1,V,N,1,6]
    with np.errstate(all="ignore"):
        rx, ry = raw[..., 0].astype(dtype), raw[..., 1].astype(dtype)
        u, w = rx - dtype(1), ry - dtype(1)
        ox = (b[..., 0] * u + b[..., 1] * w) + b[..., 2]
        oy = (b[..., 3] * u + b[..., 4] * w) + b[..., 5]
        px, py = ox + dtype(1), oy + dtype(1)
        peak = ~((raw[..., 0] == 0) & (raw[..., 1] == 0))
        ok = peak & np.isfinite(px) & np.isfinite(py)
    return np.stack([px, py], -1).astype(dtype), ok


def view_gate(raw, back, dist_thr, dtype=np.float32):
    """The kernel on raw [M,V,N,K,2], back [V,N,6] -> dict (KEYS_GATE); gate [N,K] = select.all(0)."""
    pts, ok = points(raw, back, dtype)
    out = fold(pts, ok, dist_thr, dtype)
    out["gate"] = (out["select"] > 0).all(0).astype(dtype)
    return out


def train_back(viewmat, R, H):
    """kernels.train_back_matrices in numpy: viewmat [V,N,6] (view pixel -> source pixel) composed
    with the cell convention C(c) = (R/H) c in float64, rounded once to float32."""
    m = np.asarray(viewmat, np.float32).astype(np.float64)
    out = m * (float(R) / float(H))
    out[..., 2::3] = m[..., 2::3]
    return out.astype(np.float32)
