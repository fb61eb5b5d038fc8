"""ubpl_view_uncertainty_samples against its numpy restatement (tests/view_gate_ref.py) in float32:
bit for bit on every output but unc, which the two exponentials leave within 2^-22 (as
tests/test_gpu_unc_kernels.py treats ubpl_view_uncertainty), and bit for bit against
ubpl_view_uncertainty itself where the samples share their matrices."""
import numpy as np
import pytest
import torch

import view_gate_ref as VR

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ubpl_amd import _lib
    _lib.load()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(got, want, key):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, key
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), key
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan]), key


def _similarities(V, N, rs):
    """Per (view, sample) a random similarity, view pixel -> source pixel (scale 3 to 5, any
    rotation up to 40 degrees, every third one mirrored in x), float64 rounded to float32: [V,N,6]."""
    out = np.empty((V, N, 6))
    for i in range(V * N):
        s, th = rs.uniform(3.0, 5.0), np.deg2rad(rs.uniform(-40, 40))
        a = s * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        if i % 3 == 1:
            a = a @ np.diag([-1.0, 1.0])
        t = rs.uniform(-20, 20, 2) + 128.0 - a @ np.array([32.0, 32.0])
        out[i // N, i % N] = [a[0, 0], a[0, 1], t[0], a[1, 0], a[1, 1], t[1]]
    return out.astype(np.float32)


def _peaks(M, V, N, K, back, rs):
    """Peaks [M,V,N,K,2] that agree roughly: a true source point per (n, k), seen through the inverse
    of every (view, sample) matrix, each member a source pixel or two off; half on the lattice,
    half sub-pixel; a few (0,0) no-peak entries."""
    true = rs.uniform(60, 196, (N, K, 2))
    raw = np.empty((M, V, N, K, 2))
    for v in range(V):
        for n in range(N):
            b = back[v, n].astype(np.float64).reshape(2, 3)
            p = true[n][None] + rs.normal(0, 1.5, (M, K, 2))
            raw[:, v, n] = np.linalg.solve(b[:, :2], (p - b[:, 2]).reshape(-1, 2).T).T.reshape(M, K, 2) + 1.0
    raw = np.where(rs.uniform(size=(M, V, N, K, 1)) < 0.5, np.round(raw), raw)
    raw[0, 0, 0, 0] = 0.0                                               # no peak in one view of one member
    raw[M - 1, V - 1, N - 1, K - 1] = 0.0
    return raw.astype(np.float32)


def _place(raw, pad):
    """Host [M,V,N,K,2] -> (device tensor in [V][M][N][K][2] order, sm, sv); pad: every (view,
    member) block is followed by as many floats that would wreck every distance."""
    M, V, N, K, _ = raw.shape
    blk = N * K * 2
    vm = np.ascontiguousarray(raw.transpose(1, 0, 2, 3, 4)).reshape(V, M, blk)
    if not pad:
        return torch.from_numpy(vm.copy()).to(DEV).reshape(-1), blk, M * blk
    full = np.full((V, M + 1, 2, blk), 1e3, np.float32)                # sm = 2 blk, sv = (M + 1) * 2 blk
    full[:, :M, 0] = vm
    return torch.from_numpy(full).to(DEV).reshape(-1), 2 * blk, (M + 1) * 2 * blk


def _run(dev_raw, sm, sv, shape, back, thr):
    from ubpl_amd import kernels as Kn
    M, V, N, K = shape
    out = Kn.view_uncertainty_samples(dev_raw, sm, sv, M, V, N, K, torch.from_numpy(back).to(DEV),
                                      torch.full((1,), thr, device=DEV))
    return dict(zip(VR.KEYS_GATE, (o.cpu().numpy() for o in out)))


# M x V x N x K, padded strides
CASES = [((2, 2, 3, 5), False), ((1, 2, 2, 3), False), ((3, 2, 2, 4), False), ((2, 3, 2, 3), True)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "M%dV%dN%dK%d" % c[0])
def test_kernel_matches_the_restatement(case):
    (M, V, N, K), pad = case
    rs = np.random.RandomState(M * 100 + V * 10 + K)
    back = _similarities(V, N, rs)
    raw = _peaks(M, V, N, K, back, rs)
    dev_raw, sm, sv = _place(raw, pad)
    want = VR.view_gate(raw, back, 1.0)
    thrs = VR.thresholds_between(want)
    sel = []
    for thr in thrs:
        want = VR.view_gate(raw, back, thr)
        got = _run(dev_raw, sm, sv, (M, V, N, K), back, thr)
        for key in VR.KEYS_GATE:
            if key != "unc":
                _same_bits(got[key], want[key], key)
        err = np.abs(got["unc"].astype(np.float64) - want["unc"].astype(np.float64)).max()
        print((M, V, N, K), "thr %.4g" % thr, "gate %d of %d" % (want["gate"].sum(), want["gate"].size),
              "unc err %.3g" % err)
        assert err <= 2.0 ** -22
        assert np.array_equal(got["gate"], (got["select"] > 0).all(0).astype(np.float32))
        again = _run(dev_raw, sm, sv, (M, V, N, K), back, thr)       # two launches, equal bits
        for key in VR.KEYS_GATE:
            assert np.array_equal(_bits(again[key]), _bits(got[key])), key
        sel.append(want["gate"].sum())
    legal = want["legal"] > 0
    assert not legal[0, 0, 0] and not legal[M - 1, N - 1, K - 1] and legal.sum() == legal.size - (2 if M * N * K > 1 else 1)
    assert want["gate"][0, 0] == 0 and sel[0] < sel[-1] and 0 < sel[-1] < N * K   # the thresholds bite


def test_shared_matrices_equal_view_uncertainty():
    """The same matrix for every sample and the view-major member blocks: the existing entry's bits."""
    from ubpl_amd import kernels as Kn
    M, V, N, K = 3, 4, 3, 5
    rs = np.random.RandomState(77)
    back1 = _similarities(V, 1, rs)
    back = np.ascontiguousarray(np.repeat(back1, N, 1))
    raw = _peaks(M, V, N, K, back, rs)
    dev_raw = torch.from_numpy(raw).to(DEV).reshape(-1)               # [M][V][N][K][2]
    thr = torch.full((1,), VR.thresholds_between(VR.view_gate(raw, back, 1.0))[1], device=DEV)
    old = Kn.view_uncertainty(dev_raw, V * N * K * 2, M, V, N, K, torch.from_numpy(back1).to(DEV).reshape(V, 6), thr)
    new = Kn.view_uncertainty_samples(dev_raw, V * N * K * 2, N * K * 2, M, V, N, K, torch.from_numpy(back).to(DEV),
                                      thr)
    for key, a, b in zip(VR.KEYS, old, new):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), key
    assert 0 < new[-2].sum() < new[-2].numel()
    assert torch.equal(new[-1], (new[-2] > 0).all(0).float())


def test_argument_errors():
    from ubpl_amd import _lib
    from ubpl_amd import kernels as Kn
    M, V, N, K = 2, 3, 1, 2
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    big = 9 * 17 * N * K * 2
    blk = N * K * 2
    a = {"raw": z(big), "sm": blk, "sv": M * blk, "M": M, "V": V, "N": N, "K": K, "back": z(17 * N * 6),
         "dist_thr": z(1), "pts": z(big), "legal": z(9 * N * K), "int_dist": z(9 * N * K),
         "aug_coord": z(9 * N * K * 2), "ext_dist": z(N * K), "aext_dist": z(N * K), "ext_views": z(N * K),
         "mix_dist": z(9 * N * K), "unc": z(9 * N * K), "select": z(9 * N * K), "gate": z(N * K)}
    call = lambda **kw: _lib.call("ubpl_view_uncertainty_samples", *[kw.get(n, v) for n, v in a.items()])
    call()
    call(M=8, sv=8 * blk, V=16)
    call(M=1, V=2, gate=None)
    call(sm=V * blk, sv=blk)                                           # member-major nesting
    for bad in ({"M": 0}, {"M": 9}, {"V": 1}, {"V": 17}, {"K": 0}, {"sv": blk - 1}, {"sm": blk - 1},
                {"sv": M * blk - 1}, {"back": None}, {"dist_thr": None}, {"select": None}):
        a["select"].fill_(7.0)
        with pytest.raises(RuntimeError, match="failed with hipError 1"):
            call(**bad)
        if "select" not in bad:
            assert (a["select"] == 7.0).all()                          # nothing was launched
    call(N=0)
    with pytest.raises(RuntimeError, match="raw holds"):                # the op's extent check: a short raw
        call(raw=a["raw"][:(M - 1) * blk + (V - 1) * M * blk + blk - 1])
    with pytest.raises(RuntimeError, match="back holds"):
        call(back=a["back"][:V * N * 6 - 1])
    # the wrapper refuses the same before the call
    thr = z(1)
    for kw in ({"M": 9}, {"V": 1}):
        args = dict(M=M, V=V)
        args.update(kw)
        with pytest.raises(ValueError):
            Kn.view_uncertainty_samples(a["raw"], blk, M * blk, args["M"], args["V"], N, K, a["back"], thr)
    with pytest.raises(ValueError, match="raw holds"):
        Kn.view_uncertainty_samples(a["raw"][:V * M * blk - 1], blk, M * blk, M, V, N, K, a["back"][:V * N * 6], thr)
    with pytest.raises(ValueError, match="dist_thr"):
        Kn.view_uncertainty_samples(a["raw"], blk, M * blk, M, V, N, K, a["back"][:V * N * 6], None)
    torch.cuda.synchronize()
