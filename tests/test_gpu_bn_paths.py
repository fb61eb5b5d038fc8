"""BatchNorm paths (bn_fwd.hip, bn_bwd.hip) that the other GPU tests do not reach: the scalar
kernels (HW % 4 != 0, or an operand that is not 16-byte aligned), the per-plane backward
apply at every unroll with both addends and in place, the three apply kernels against each
other, and the bounded statistics (the 2xfp16 scale of dx) with a short last slice.

Inputs and tolerances are test_gpu_kernels.py::test_bn_forward_backward_vs_torch's: x =
3 randn + 5, gamma in [0.5, 1.5), the reference F.relu(F.batch_norm(...)) with autograd on the
CPU in f32, dx to rtol 1e-4 / atol 1e-5, dgamma and dbeta to 1e-4 / 1e-4, the running
statistics to 1e-6 / 1e-6 (mean) and 1e-5 / 1e-6 (variance).  Everything that has a second
kernel computing the same expression is compared bit for bit.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS, MOM = 1e-5, 0.1


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ubpl_amd import _lib
    _lib.load()


def _close(a, b, rtol, atol):
    np.testing.assert_allclose(a.detach().cpu().double().numpy(), b.detach().cpu().double().numpy(), rtol=rtol,
                               atol=atol)


def _same(a, b, what):
    ia, ib = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    assert a.shape == b.shape and torch.equal(ia, ib), \
        "%s differs in %d of %d elements" % (what, int((ia != ib).sum()), a.numel())


_CASES = {}


def _case(shape):
    """One shape's inputs, its CPU reference (made once, never written again) and the device
    BatchNorm's forward statistics, which every backward call below starts from."""
    if shape in _CASES:
        return _CASES[shape]
    from ubpl_amd import kernels as Kn
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(31 + 7 * H + W)
    d = dict(x=torch.randn(B, C, H, W, generator=gen) * 3 + 5, gam=torch.rand(C, generator=gen) + 0.5,
             bet=torch.randn(C, generator=gen), rm=torch.randn(C, generator=gen),
             rv=torch.rand(C, generator=gen) + 0.5)
    for k in ("dz", "add1", "add2"):
        d[k] = torch.randn(B, C, H, W, generator=gen)
    xr = d["x"].clone().requires_grad_(True)
    gr, br = d["gam"].clone().requires_grad_(True), d["bet"].clone().requires_grad_(True)
    rmr, rvr = d["rm"].clone(), d["rv"].clone()
    y = F.relu(F.batch_norm(xr, rmr, rvr, gr, br, True, MOM, EPS))
    y.backward(d["dz"])
    d.update(y=y.detach(), dx=xr.grad, dg=gr.grad, db=br.grad, rm_ref=rmr, rv_ref=rvr)
    g = {k: d[k].to(DEV) for k in ("x", "gam", "bet", "dz", "add1", "add2")}
    g["part"] = Kn.bn_part(B, C, DEV)
    g["mean"], g["istd"], g["sc"], g["sh"] = [torch.empty(C, device=DEV) for _ in range(4)]
    g["rm"], g["rv"] = d["rm"].to(DEV), d["rv"].to(DEV)
    Kn.bn_forward_stats(g["x"], g["gam"], g["bet"], EPS, MOM, g["rm"], g["rv"], g["part"], g["mean"], g["istd"],
                        g["sc"], g["sh"])
    d["gpu"] = g
    _CASES[shape] = d
    return d


def _backward(g, dz, x, add1=None, add2=None, out=None, part=None, coef_extra=0):
    """Kn.bn_backward from the case's forward statistics into fresh dgamma / dbeta -> (dx, dg, db, coef)."""
    from ubpl_amd import kernels as Kn
    C = g["gam"].numel()
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    coef = torch.empty(3 * C + coef_extra, device=DEV)
    dx = Kn.bn_backward(dz, x, g["gam"], g["mean"], g["istd"], g["sc"], g["sh"], 1, g["part"], coef, dg, db,
                        add1=add1, add2=add2, out=out, part=part)
    return dx, dg, db, coef


@pytest.mark.parametrize("shape", [(3, 5, 3, 3), (2, 3, 5, 5)])
def test_scalar_kernels_vs_torch(shape):
    """HW % 4 != 0: stats_kernel<false>, bwd_stats_kernel<false> and bwd_apply_kernel."""
    d = _case(shape)
    g = d["gpu"]
    _close(g["rm"], d["rm_ref"], rtol=1e-6, atol=1e-6)
    _close(g["rv"], d["rv_ref"], rtol=1e-5, atol=1e-6)
    yd = torch.relu(g["x"] * g["sc"][None, :, None, None] + g["sh"][None, :, None, None])   # (bn_apply: HW % 4 == 0)
    _close(yd, d["y"], rtol=1e-5, atol=1e-5)
    dx, dg, db, _ = _backward(g, g["dz"].clone(), g["x"])
    _close(dx, d["dx"], rtol=1e-4, atol=1e-5)
    _close(dg, d["dg"], rtol=1e-4, atol=1e-4)
    _close(db, d["db"], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("shape", [(2, 3, 32, 32), (2, 3, 32, 64), (2, 2, 64, 64)])
def test_plane_apply_with_addends_every_unroll(shape):
    """bwd_apply_plane_kernel<false, U>: 256, 512 and 1024 float4s per plane are U = 1, 2 and 4."""
    d = _case(shape)
    g = d["gpu"]
    dx, dg, db, _ = _backward(g, g["dz"], g["x"], g["add1"], g["add2"], out=torch.empty_like(g["x"]))
    _close(dx, d["dx"] + d["add1"] + d["add2"], rtol=1e-4, atol=1e-5)
    _close(dg, d["dg"], rtol=1e-4, atol=1e-4)
    _close(db, d["db"], rtol=1e-4, atol=1e-4)
    dz = g["dz"].clone()
    dx2, dg2, db2, _ = _backward(g, dz, g["x"], g["add1"], g["add2"])      # in place: dx is dz
    assert dx2.data_ptr() == dz.data_ptr()
    _same(dx2, dx, "dx in place")
    _same(dg2, dg, "dgamma")
    _same(db2, db, "dbeta")


def _off_by_one_float(t):
    """The same values in a view one float into a larger buffer: 4-byte aligned only."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.mark.parametrize("shape", [(2, 3, 32, 32), (2, 3, 8, 8)])
def test_apply_kernels_agree_bit_for_bit(shape):
    """The plane (32x32) and the grid-stride float4 (8x8) apply against the scalar one on the
    same values.  The coefficients come from one set of backward partials both times (only the
    f64 finalize runs: identical coefficients), so dx must be bit-equal."""
    from ubpl_amd import kernels as Kn
    g = _case(shape)["gpu"]
    assert all(g[k].data_ptr() % 16 == 0 for k in ("dz", "x", "add1", "add2"))
    part = Kn.bn_bwd_partials(g["dz"], g["x"], g["sc"], g["sh"], g["mean"], 1)
    dx, dg, db, coef = _backward(g, g["dz"], g["x"], g["add1"], g["add2"], out=torch.empty_like(g["x"]), part=part)
    m = {k: _off_by_one_float(g[k]) for k in ("dz", "x", "add1", "add2")}
    dxm, dgm, dbm, coefm = _backward(g, m["dz"], m["x"], m["add1"], m["add2"],
                                     out=_off_by_one_float(torch.zeros_like(g["x"])), part=part)
    _same(coefm, coef, "coefficients")
    _same(dgm, dg, "dgamma")
    _same(dbm, db, "dbeta")
    _same(dxm, dx, "dx")


def test_bounded_statistics_with_a_short_last_slice():
    """bwd_stats_kernel<true, true> (bn_backward_split, npieces 2) at B=5, C=16, 64x64: two batch
    slices per channel, of three and of two images.  Its sums, slices and order are
    bwd_stats_kernel<true, false>'s, so dgamma / dbeta are bit-equal to bn_backward's; the
    scale it leaves at coef[3C] is a power of two that keeps every |dx * scale| <= 2^14."""
    from ubpl_amd import kernels as Kn
    d = _case((5, 16, 64, 64))
    g = d["gpu"]
    C = 16
    dx, dg, db, coef = _backward(g, g["dz"], g["x"], out=torch.empty_like(g["x"]))
    _close(dx, d["dx"], rtol=1e-4, atol=1e-5)
    dg2, db2 = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    coef2 = torch.empty(3 * C + 1, device=DEV)
    Kn.bn_backward_split(g["dz"], g["x"], g["gam"], g["mean"], g["istd"], g["sc"], g["sh"], 1, g["part"], coef2, dg2,
                         db2, npieces=2, pad=1)
    _same(dg2, dg, "dgamma")
    _same(db2, db, "dbeta")
    _same(coef2[:3 * C], coef, "coefficients")
    s = float(coef2[3 * C])
    assert s > 0 and math.isfinite(s) and math.frexp(s)[0] == 0.5, s
    top = float(dx.abs().max()) * s
    print("scale 2^%d, max |dx * scale| = %.1f" % (math.frexp(s)[1] - 1, top))
    assert top <= 2.0 ** 14, (s, top)
