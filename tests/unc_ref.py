"""A numpy restatement of ubpl_view_uncertainty (include/ubpl_hip.h), shared by the
view-consistency-uncertainty tests.  Every product, sum, quotient and square root is one numpy
operation in the dtype given, in the kernel's order: the float32 instance gives the kernel's bits
(unc up to the two exponentials' last place), the float64 instance is the yardstick that is
compared with the reference's own Python-float arithmetic (tests/golden/unc.npz)."""
from itertools import combinations

import numpy as np

SENTINEL = 999.0
KEYS = ("pts", "legal", "int_dist", "aug_coord", "ext_dist", "aext_dist", "ext_views", "mix_dist", "unc", "select")


def points(raw, back, swap=None, perm=None, tinv=None, dtype=np.float32):
    """raw [M,V,N,K,2] (1-based view-frame peaks, each view in its own joint order), back [V,6],
    swap [V] or None, perm [K] or None, tinv [N,6] float64 or None -> (pts [M,V,N,K,2] in the
    original frame and in output joint order, ok [M,V,N,K] bool: the point is legal)."""
    raw = np.asarray(raw, np.float32)
    M, V, N, K, _ = raw.shape
    back = np.asarray(back, np.float32).reshape(V, 6).astype(dtype)
    pts = np.empty((M, V, N, K, 2), dtype)
    ok = np.empty((M, V, N, K), bool)
    with np.errstate(all="ignore"):
        for v in range(V):
            r = raw[:, v]
            if swap is not None and swap[v] != 0 and perm is not None:
                pk = np.asarray(perm).astype(np.int64)
                pk = np.where((pk >= 0) & (pk < K), pk, np.arange(K))
                r = r[:, :, pk]
            rx, ry = r[..., 0].astype(dtype), r[..., 1].astype(dtype)
            u, w = rx - dtype(1), ry - dtype(1)
            b = back[v]
            ox = (b[0] * u + b[1] * w) + b[2]
            oy = (b[3] * u + b[4] * w) + b[5]
            if tinv is not None:
                t = np.asarray(tinv, np.float64).reshape(N, 6)[None, :, None, :]      # [1,N,1,6]
                du, dw = ox.astype(np.float64), oy.astype(np.float64)
                px = (((t[..., 0] * du + t[..., 1] * dw) + t[..., 2]) + 1.0).astype(dtype)
                py = (((t[..., 3] * du + t[..., 4] * dw) + t[..., 5]) + 1.0).astype(dtype)
            else:
                px, py = ox + dtype(1), oy + dtype(1)
            peak = ~((r[..., 0] == 0) & (r[..., 1] == 0))
            good = peak & np.isfinite(px) & np.isfinite(py)
            if tinv is not None:
                good &= (px >= 0) & (py >= 0)
            pts[:, v, ..., 0], pts[:, v, ..., 1], ok[:, v] = px, py, good
    return pts, ok


def _dist(p, q):
    dx, dy = p[..., 0] - q[..., 0], p[..., 1] - q[..., 1]
    return np.sqrt(dx * dx + dy * dy)


def fold(pts, ok, dist_thr, dtype=np.float32):
    """pts [M,V,N,K,2], ok [M,V,N,K], dist_thr -> the kernel's outputs as a dict (KEYS)."""
    pts = np.asarray(pts, dtype)
    M, V, N, K, _ = pts.shape
    S, zero = dtype(SENTINEL), dtype(0)
    t = dtype(np.float32(dist_thr))
    legal = np.asarray(ok, bool).all(1)                                 # [M,N,K]
    with np.errstate(all="ignore"):
        ds = np.zeros((M, N, K), dtype)
        for a, b in combinations(range(V), 2):
            ds = ds + _dist(pts[:, a], pts[:, b])
        int_dist = np.where(legal, ds / dtype(V * (V - 1) // 2), S)
        sm = np.zeros((M, N, K, 2), dtype)
        for v in range(V):
            sm = sm + pts[:, v]
        aug = np.where(legal[..., None], sm / dtype(V), dtype(-1))
        se, sa, sv = (np.zeros((N, K), dtype) for _ in range(3))
        cnt = np.zeros((N, K), np.int64)
        for a, b in combinations(range(M), 2):
            both = legal[a] & legal[b]
            dv = np.zeros((N, K), dtype)
            for v in range(V):
                dv = dv + _dist(pts[a, v], pts[b, v])
            se = se + np.where(both, _dist(pts[a, 0], pts[b, 0]), zero)
            sa = sa + np.where(both, _dist(aug[a], aug[b]), zero)
            sv = sv + np.where(both, dv / dtype(V), zero)
            cnt += both
        none = S if M >= 2 else zero
        den = np.maximum(cnt, 1).astype(dtype)
        ext, aext, extv = (np.where(cnt > 0, s / den, none).astype(dtype) for s in (se, sa, sv))
        mix = np.where(legal, int_dist + np.where(ext > 0, (ext + aext) / dtype(2), aext), S)
        unc = np.where(legal, dtype(1) - np.exp(-mix / dtype(5)), S)
        select = legal & (int_dist <= t) & (ext <= t) & (aext <= t) & (mix <= dtype(3) * t)
    out = {"pts": pts, "legal": legal.astype(dtype), "int_dist": int_dist, "aug_coord": aug, "ext_dist": ext,
           "aext_dist": aext, "ext_views": extv, "mix_dist": mix, "unc": unc, "select": select.astype(dtype)}
    assert all(v.dtype == dtype for v in out.values())
    return out


def view_uncertainty(raw, back, dist_thr, swap=None, perm=None, tinv=None, dtype=np.float32):
    """The kernel on raw [M,V,N,K,2] -> dict (KEYS)."""
    pts, ok = points(raw, back, swap, perm, tinv, dtype)
    return fold(pts, ok, dist_thr, dtype)


def gaps_between(out):
    """Every value midway between two neighbouring distinct values (0.1 % apart at least) of the
    restatement's distances — int_dist, ext_dist, aext_dist and mix_dist / 3, the sentinels aside —
    ascending: a dist_thr taken from here leaves no comparison of select on a rounding edge."""
    vals = np.concatenate([out[k].astype(np.float64).reshape(-1) for k in ("int_dist", "ext_dist", "aext_dist")]
                          + [out["mix_dist"].astype(np.float64).reshape(-1) / 3.0])
    vals = np.unique(vals[np.isfinite(vals) & (vals < SENTINEL / 3)])
    return [float((a + b) / 2) for a, b in zip(vals[:-1], vals[1:]) if b - a > 1e-3 * max(1.0, abs(b))]


def thresholds_between(out):
    """Of gaps_between the lowest, the middle and the highest, and a value above them all (at which
    every legal member with a legal partner is selected)."""
    gaps = gaps_between(out)
    top = 2.0 * gaps[-1] + 1.0 if gaps else 1.0
    return ([gaps[0], gaps[len(gaps) // 2], gaps[-1]] if gaps else []) + [top]
