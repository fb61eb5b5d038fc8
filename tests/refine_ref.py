"""A numpy restatement of ubpl_refine_peaks (include/ubpl_hip.h), shared by the refine
tests.  It loops in the kernel's order — rows then columns, each blur w[0] x(0) +
sum_j w[j] (x(-j) + x(+j)) in ascending j — in the dtype given: its float32 instance mirrors
the kernel, its float64 instance is the yardstick.  The sampled values are the decode's own
float32 bits in both."""
import numpy as np

QUARTER, TAYLOR = 1, 2


def merged_maps(hm, hm_flip=None, perm=None):
    """v of the header: hm [N,K,H,W] float32, or (hm + hm_flip[:, perm] mirrored) * 0.5f."""
    hm = np.asarray(hm, np.float32)
    if hm_flip is None:
        return hm
    f = np.asarray(hm_flip, np.float32)
    if perm is not None:
        f = f[:, np.asarray(perm)]
    return ((hm + f[..., ::-1]) * np.float32(0.5)).astype(np.float32)


def _window(v, r, c, half):
    """The (2 half + 1)^2 values around (r, c) of v [H,W], 0 outside the map."""
    H, W = v.shape
    out = np.zeros((2 * half + 1, 2 * half + 1), v.dtype)
    y0, y1, x0, x1 = max(r - half, 0), min(r + half + 1, H), max(c - half, 0), min(c + half + 1, W)
    out[y0 - (r - half):y1 - (r - half), x0 - (c - half):x1 - (c - half)] = v[y0:y1, x0:x1]
    return out


def _sign(d):
    return 1.0 if d > 0 else (-1.0 if d < 0 else 0.0)


def _at(v, y, x):
    return v[y, x] if 0 <= y < v.shape[0] and 0 <= x < v.shape[1] else v.dtype.type(0)


def refine_map(v, rx, ry, mode, taps, dtype):
    """One map v [H,W] float32 and its raw peak -> (ox, oy, how, dxx, det, omax); the last three
    are the float branch quantities of the Taylor step (nan where it was not tried)."""
    H, W = v.shape
    nan = float("nan")
    if not (rx >= 1 and rx <= W and ry >= 1 and ry <= H):
        return dtype(0), dtype(0), 0, nan, nan, nan
    c, r = int(rx) - 1, int(ry) - 1
    if not v[r, c] > 0:
        return dtype(0), dtype(0), 0, nan, nan, nan
    dxx = det = omax = nan
    if mode == TAYLOR and 2 <= c <= W - 3 and 2 <= r <= H - 3:
        w = np.asarray(taps, np.float32).astype(dtype)
        R = len(w) - 1
        win = _window(v, r, c, 2 + R).astype(dtype)
        rows = np.empty((5 + 2 * R, 5), dtype)
        for dx in range(5):
            acc = w[0] * win[:, R + dx]
            for j in range(1, R + 1):
                acc = acc + w[j] * (win[:, R + dx - j] + win[:, R + dx + j])
            rows[:, dx] = acc
        b = np.empty((5, 5), dtype)
        for dy in range(5):
            acc = w[0] * rows[R + dy]
            for j in range(1, R + 1):
                acc = acc + w[j] * (rows[R + dy - j] + rows[R + dy + j])
            b[dy] = acc
        L = np.log(np.fmax(b, dtype(1e-10)))
        h, q, two = dtype(0.5), dtype(0.25), dtype(2)
        gx, gy = h * (L[2, 3] - L[2, 1]), h * (L[3, 2] - L[1, 2])
        dxx = q * (L[2, 4] - two * L[2, 2] + L[2, 0])
        dyy = q * (L[4, 2] - two * L[2, 2] + L[0, 2])
        dxy = q * (L[3, 3] - L[1, 3] - L[3, 1] + L[1, 1])
        det = dxx * dyy - dxy * dxy
        if dxx < 0 and det > 0:
            ox, oy = -(dyy * gx - dxy * gy) / det, -(dxx * gy - dxy * gx) / det
            omax = max(abs(float(ox)), abs(float(oy))) if ox == ox and oy == oy else nan
            if abs(ox) <= 1 and abs(oy) <= 1:
                return dtype(ox), dtype(oy), 2, float(dxx), float(det), omax
    ex, ey = 1 <= c <= W - 2, 1 <= r <= H - 2
    ox = 0.25 * _sign(_at(v, r, c + 1) - _at(v, r, c - 1)) if ex else 0.0
    oy = 0.25 * _sign(_at(v, r + 1, c) - _at(v, r - 1, c)) if ey else 0.0
    return dtype(ox), dtype(oy), 1 if (ex or ey) else 0, float(dxx), float(det), omax


def refine_ref(hm, raw, mode, taps, dtype, hm_flip=None, perm=None, tinv=None):
    """hm (and hm_flip) [N,K,H,W], raw [N,K,2] (the decode's 1-based peaks), taps the float32
    half kernel, tinv [N,6] float64 or None -> dict of raw_sub [N,K,2] (dtype), preds_sub
    [N,K,2] (float64 arithmetic in the decode's order on raw_sub, rounded to float32; None
    without tinv), how [N,K] and the branch quantities dxx, det, omax [N,K] (float64)."""
    v = merged_maps(hm, hm_flip, perm)
    N, K = v.shape[:2]
    raw = np.asarray(raw, np.float32)
    out = {"raw_sub": np.zeros((N, K, 2), dtype), "how": np.zeros((N, K), np.float32),
           "dxx": np.zeros((N, K)), "det": np.zeros((N, K)), "omax": np.zeros((N, K)), "preds_sub": None}
    with np.errstate(all="ignore"):
        for n in range(N):
            for k in range(K):
                ox, oy, how, dxx, det, omax = refine_map(v[n, k], raw[n, k, 0], raw[n, k, 1], mode, taps, dtype)
                out["raw_sub"][n, k] = (dtype(raw[n, k, 0]) + ox, dtype(raw[n, k, 1]) + oy)
                out["how"][n, k] = how
                out["dxx"][n, k], out["det"][n, k], out["omax"][n, k] = dxx, det, omax
        if tinv is not None:
            t = np.asarray(tinv, np.float64).reshape(N, 1, 6)
            u, w = out["raw_sub"][..., 0].astype(np.float64) - 1.0, out["raw_sub"][..., 1].astype(np.float64) - 1.0
            px = (t[..., 0] * u + t[..., 1] * w) + t[..., 2]
            py = (t[..., 3] * u + t[..., 4] * w) + t[..., 5]
            out["preds_sub"] = np.stack([px + 1.0, py + 1.0], -1).astype(np.float32)
    return out


def at_boundary(ref):
    """[N,K] bool: the float64 branch quantities of ref sit at a decision boundary of the
    Taylor step (the only maps a comparison with a float32 computation may leave out)."""
    with np.errstate(invalid="ignore"):
        return (np.abs(ref["dxx"]) < 1e-3) | (np.abs(ref["det"]) < 1e-4) | (np.abs(ref["omax"] - 1.0) < 1e-3)
