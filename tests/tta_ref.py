"""A numpy restatement of ubpl_warp_views and ubpl_decode_heatmaps_views (include/ubpl_hip.h),
shared by the test-time-augmentation tests.  Every product, sum and quotient is one numpy
operation in the dtype given, in the kernel's order: the float32 instance gives the kernel's
bits, the float64 instance is a yardstick."""
import numpy as np

IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def sample_plane(p, mat, dtype=np.float32):
    """Planes p [..., H, W] under one pixel matrix mat [6] (output pixel -> source pixel)
    -> (s, cov): s [..., H, W] the bilinear sample with zero taps outside, cov [H, W] the same
    formula over the in-bounds indicator."""
    p = np.asarray(p, dtype)
    H, W = p.shape[-2:]
    m = np.asarray(mat, np.float32).astype(dtype)
    if tuple(float(v) for v in m) == IDENTITY:
        return p.copy(), np.ones((H, W), dtype)
    y, x = np.meshgrid(np.arange(H, dtype=dtype), np.arange(W, dtype=dtype), indexing="ij")
    with np.errstate(all="ignore"):
        sx = (m[0] * x + m[1] * y) + m[2]
        sy = (m[3] * x + m[4] * y) + m[5]
        inside = (sx > -1) & (sx < W) & (sy > -1) & (sy < H)
        sx, sy = np.where(inside, sx, dtype(0)), np.where(inside, sy, dtype(0))
        x0f, y0f = np.floor(sx), np.floor(sy)
        ax, ay = sx - x0f, sy - y0f
        bx, by = dtype(1) - ax, dtype(1) - ay
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)

        def tap(yy, xx):
            ok = inside & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            v = p[..., np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
            return np.where(ok, v, dtype(0)), ok.astype(dtype)

        (v00, c00), (v01, c01) = tap(y0, x0), tap(y0, x0 + 1)
        (v10, c10), (v11, c11) = tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
        s = (v00 * bx + v01 * ax) * by + (v10 * bx + v11 * ax) * ay
        cov = (c00 * bx + c01 * ax) * by + (c10 * bx + c11 * ax) * ay
        s = np.where(inside, s, dtype(0))
        cov = np.where(inside, cov, dtype(0))
    return s.astype(dtype), cov.astype(dtype)


def warp_views(src, mats, dtype=np.float32):
    """src [N,C,H,W], mats [V,6] -> [V,N,C,H,W]."""
    return np.stack([sample_plane(src, m, dtype)[0] for m in np.asarray(mats).reshape(-1, 6)])


def merge_views(hm, mats, swap=None, perm=None, dtype=np.float32):
    """hm [V,N,K,H,W] (the views' maps), mats [V,6], swap [V] or None, perm [K] or None ->
    merged [N,K,H,W]: num / den over the views in ascending order, 0 where den is not > 0."""
    hm = np.asarray(hm, dtype)
    V, N, K = hm.shape[:3]
    mats = np.asarray(mats).reshape(V, 6)
    num = den = None
    with np.errstate(all="ignore"):
        for v in range(V):
            maps = hm[v]
            if swap is not None and swap[v] != 0 and perm is not None:
                pk = np.asarray(perm).astype(np.int64)
                pk = np.where((pk >= 0) & (pk < K), pk, np.arange(K))
                maps = maps[:, pk]
            s, c = sample_plane(maps, mats[v], dtype)
            c = np.broadcast_to(c, s.shape)
            num, den = (s, c) if v == 0 else (num + s, den + c)
        out = np.where(den > 0, num / np.where(den > 0, den, dtype(1)), dtype(0))
    return out.astype(dtype)


def decode(merged):
    """merged [N,K,H,W] without NaNs -> (raw [N,K,2] 1-based (col, row) of the first maximum, zeroed
    where it is not > 0; scores [N,K])."""
    N, K, H, W = merged.shape
    flat = merged.reshape(N, K, -1)
    idx = flat.argmax(-1)
    scores = np.take_along_axis(flat, idx[..., None], -1)[..., 0]
    raw = np.stack([idx % W + 1, idx // W + 1], -1).astype(np.float32) * (scores > 0)[..., None]
    return raw.astype(np.float32), scores
