"""ubpl_view_uncertainty against its numpy restatement (tests/unc_ref.py) in float32: bit for bit
on every output but unc, which the two exponentials leave within 2^-22."""
import numpy as np
import pytest
import torch

import unc_ref as UR

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = 64                                                               # the heatmaps' side
VIEWS = [(0, 1), (0, 1.25), (20, 0.8), (-35, 1.5), (10, 0.9), (-15, 1.1), (30, 1.0), (-5, 0.7)]


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ubpl_amd import _lib
    _lib.load()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(got, want, key):
    """Equal bits; a NaN stands where a NaN stands (its payload is the platform's)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, key
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), key
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan]), key


def _geometry(V, flip):
    """-> host (hm_mat [V,6], back [V,6], swap [V]): V views, with flip the second half mirrored."""
    from ubpl_amd import kernels as Kn
    _, hm_mat, swap = Kn.view_matrices(VIEWS[:V // 2 if flip else V], flip, 4 * S, S)
    return hm_mat, Kn.view_back_matrices(hm_mat), swap


def _peaks(M, V, N, K, hm_mat, swap, perm, rs, lo=12.0, hi=52.0):
    """Per-view peaks [M,V,N,K,2] that agree roughly: a true point per (n, k), where each view
    would see it (hm_mat maps original -> view), each member a pixel or two off, half of them on
    the lattice and half sub-pixel; a mirrored view stores joint k at its own index perm[k]."""
    true = rs.uniform(lo, hi, (N, K, 2))
    m = hm_mat.double().numpy()
    raw = np.empty((M, V, N, K, 2), np.float64)
    for v in range(V):
        p = true[None] + rs.normal(0, 1.0, (M, N, K, 2))
        q = np.stack([m[v, 0] * p[..., 0] + m[v, 1] * p[..., 1] + m[v, 2],
                      m[v, 3] * p[..., 0] + m[v, 4] * p[..., 1] + m[v, 5]], -1) + 1.0
        q = np.where(rs.uniform(size=(M, N, K, 1)) < 0.5, np.round(q), q)
        if swap is not None and swap[v] and perm is not None:
            own = np.empty_like(q)
            own[:, :, perm] = q                                     # output joint k is read at perm[k]
            q = own
        raw[:, v] = q
    return raw.astype(np.float32)


def _tinv(N, rs):
    t = rs.uniform(-0.3, 0.3, (N, 6)) + np.array([4.0, 0, 0, 0, 4.0, 0])
    t[:, [2, 5]] = rs.uniform(0, 20, (N, 2))
    return t


def _place(raw, strided):
    """Host [M,V,N,K,2] -> (device tensor as the kernel takes it, sm).  Strided: every member's
    block is followed by as many floats that would wreck every distance."""
    M = raw.shape[0]
    flat = raw.reshape(M, -1)
    if not strided:
        return torch.from_numpy(flat.copy()).to(DEV).reshape(-1), flat.shape[1]
    full = np.full((M, 2, flat.shape[1]), 1e3, np.float32)
    full[:, 0] = flat
    return torch.from_numpy(full).to(DEV).reshape(-1)[:(M - 1) * 2 * flat.shape[1] + flat.shape[1]], 2 * flat.shape[1]


def _run(raw, sm, shape, back, thr, swap, perm, tinv):
    from ubpl_amd import kernels as Kn
    M, V, N, K = shape
    dev = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)
    out = Kn.view_uncertainty(raw, sm, M, V, N, K, back.to(DEV), torch.full((1,), thr, device=DEV),
                              dev(swap, torch.int32), dev(perm, torch.int32), dev(tinv, torch.float64))
    return dict(zip(UR.KEYS, (o.cpu().numpy() for o in out)))


def _check(raw, shape, back, swap, perm, tinv, strided=False):
    """The kernel on raw against the restatement at three thresholds between the restatement's
    distances; twice, for equal bits.  -> the restatement's outputs at the last threshold."""
    dev_raw, sm = _place(raw, strided)
    want = UR.view_uncertainty(raw, back.numpy(), 1.0, swap, perm, tinv)
    thrs = UR.thresholds_between(want)
    for thr in thrs:
        want = UR.view_uncertainty(raw, back.numpy(), thr, swap, perm, tinv)
        got = _run(dev_raw, sm, shape, back, thr, swap, perm, tinv)
        for key in UR.KEYS:
            if key != "unc":
                _same_bits(got[key], want[key], key)
        err = np.abs(got["unc"].astype(np.float64) - want["unc"].astype(np.float64)).max()
        print(shape, "thr %.4g" % thr, "selected %d of %d" % (want["select"].sum(), want["select"].size),
              "unc err %.3g" % err)
        assert err <= 2.0 ** -22
        again = _run(dev_raw, sm, shape, back, thr, swap, perm, tinv)
        for key in UR.KEYS:
            assert np.array_equal(_bits(again[key]), _bits(got[key])), key
    return want, thrs


# (M, V, N, K), flip (mirrored views with swap and perm), strided sm, tinv
CASES = [((1, 2, 1, 1), False, False, True), ((2, 3, 2, 3), False, False, True), ((8, 16, 2, 17), True, True, True),
         ((2, 5, 2, 3), False, False, False)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "M%dV%dN%dK%d" % c[0])
def test_kernel_matches_the_restatement(case):
    (M, V, N, K), flip, strided, with_tinv = case
    rs = np.random.RandomState(M * 100 + V)
    hm_mat, back, swap = _geometry(V, flip)
    swap = swap.numpy() if flip else None
    perm = rs.permutation(K).astype(np.int32) if flip else None
    raw = _peaks(M, V, N, K, hm_mat, swap, perm, rs)
    tinv = _tinv(N, rs) if with_tinv else None
    want, thrs = _check(raw, (M, V, N, K), back, swap, perm, tinv, strided)
    assert want["legal"].all()                                      # (the planted case has the others)
    if M == 1:
        assert not want["ext_dist"].any() and not want["ext_views"].any()
    else:
        # members a pixel or two apart: the views agree within a few cells (or 4x that in pixels)
        assert 0 < want["ext_dist"].max() < (40 if with_tinv else 10)
        sel = [UR.view_uncertainty(raw, back.numpy(), t, swap, perm, tinv)["select"].sum() for t in thrs]
        assert sel[0] < sel[-1] and sel[-1] > 0                     # the thresholds bite
    if flip:                                                        # the joint order matters
        other = UR.view_uncertainty(raw, back.numpy(), 1.0, swap, None, tinv)
        assert not np.array_equal(other["int_dist"], want["int_dist"])


def test_illegal_points_and_the_sentinels():
    M, V, N, K = 3, 3, 2, 4
    rs = np.random.RandomState(9)
    hm_mat, back, _ = _geometry(V, False)
    raw = _peaks(M, V, N, K, hm_mat, None, None, rs, 20.0, 50.0)
    tinv = _tinv(N, rs)
    tinv[1] = [4.0, 0, -40.0, 0, 4.0, 5.0]
    raw[0, 1, 0, 0] = 0.0                                           # member 0: no peak in one view
    raw[1, 0, 0, 1, 0] = np.nan                                     # member 1: a NaN
    raw[2, 0, 1, 2] = (3.0, 20.0)                                   # member 2: x = 4 * 2 - 40 + 1 < 0
    raw[0, 0, 1, 3] = 0.0                                           # joint (1, 3): members 0 and 1 without
    raw[1, 2, 1, 3] = 0.0                                           # a peak somewhere: no legal pair
    want, _ = _check(raw, (M, V, N, K), back, None, None, tinv)
    legal = want["legal"] > 0
    assert legal.sum() == legal.size - 5
    assert not legal[0, 0, 0] and not legal[1, 0, 1] and not legal[2, 1, 2] and not legal[:2, 1, 3].any()
    assert want["pts"][2, 0, 1, 2, 0] < 0 and np.isnan(want["pts"][1, 0, 0, 1, 0])
    for key in ("int_dist", "mix_dist", "unc"):
        assert (want[key][~legal] == 999).all() and (want[key][legal] < 999).sum() > 0
    assert (want["aug_coord"][~legal] == -1).all() and not want["select"][~legal].any()
    # a joint with one illegal member keeps the pair of the other two; one with no legal pair has none
    assert want["ext_dist"][0, 0] < 999 and want["ext_dist"][1, 2] < 999
    for key in ("ext_dist", "aext_dist", "ext_views"):
        assert want[key][1, 3] == 999
    assert legal[2, 1, 3] and want["mix_dist"][2, 1, 3] > 999 and want["select"][2, 1, 3] == 0


def test_argument_errors():
    from ubpl_amd import _lib
    M, V, N, K = 2, 3, 1, 2
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    big = 9 * 17 * N * K * 2
    a = {"raw": z(big), "sm": V * N * K * 2, "M": M, "V": V, "N": N, "K": K, "back": z(17 * 6), "swap": None,
         "perm": None, "tinv": None, "dist_thr": z(1), "pts": z(big), "legal": z(9 * N * K), "int_dist": z(9 * N * K),
         "aug_coord": z(9 * N * K * 2), "ext_dist": z(N * K), "aext_dist": z(N * K), "ext_views": z(N * K),
         "mix_dist": z(9 * N * K), "unc": z(9 * N * K), "select": z(9 * N * K)}
    call = lambda **kw: _lib.call("ubpl_view_uncertainty", *[kw.get(n, v) for n, v in a.items()])
    call()
    call(M=8, sm=16 * N * K * 2, V=16)
    call(M=1, V=2)
    for bad in ({"M": 0}, {"M": 9}, {"V": 1}, {"V": 17}, {"K": 0}, {"sm": V * N * K * 2 - 1}, {"back": None},
                {"dist_thr": None}, {"select": None}):
        a["select"].fill_(7.0)
        with pytest.raises(RuntimeError, match="failed with hipError 1"):
            call(**bad)
        if "select" not in bad:
            assert (a["select"] == 7.0).all()                      # nothing was launched
    call(N=0)                                                       # no joints: nothing to do
    with pytest.raises(RuntimeError, match="raw holds"):            # the op's extent check
        call(raw=a["raw"][:(M - 1) * a["sm"] + V * N * K * 2 - 1])
    torch.cuda.synchronize()
