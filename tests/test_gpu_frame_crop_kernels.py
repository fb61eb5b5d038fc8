"""ubpl_crop_frames on the device against the float64 restatement of the reference's evaluation
crop (tests/frame_crop_ref.py): R = 32, five frames of mixed sizes in one bank, the cases of
frame_crop_ref.CASES — up-scale, Gaussian radius 0 / 1 / 2, pre-resize at non-integer factors,
a box over each frame edge and one wholly outside, a frame narrower than the Gaussian radius,
several boxes on one frame — and n = 1.

Accuracy: max |device - restatement| < 2e-5 over EVERY pixel (the bar tests/test_gpu_augment.py
sets for this kernel's radius-0 special case).  It holds by derivation: each pass is a convex
float32 sum of at most 62 terms on values <= 1 (<= 63 * 2^-24 = 3.8e-6 per pass), the
coordinates are float64, and u8 * (1/255.f) is within one float32 ulp of u8 / 255."""
import numpy as np
import pytest
import torch

import frame_crop_ref as FR

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 2e-5


@pytest.fixture(scope="module")
def bank():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ubpl_amd import _lib
    from ubpl_amd.frames import FrameBank
    _lib.load()
    return FrameBank(FR.case_frames(), FR.CASE_MEANS, DEV)


@pytest.fixture(scope="module")
def ref():
    frames = FR.case_frames()
    return np.stack([FR.ref_crop(frames[f], c, s, FR.CASE_RES, FR.CASE_MEANS) for _, f, c, s in FR.CASES])


def _args(idx=None):
    cases = FR.CASES if idx is None else [FR.CASES[i] for i in idx]
    return [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases]


def test_every_case_matches_the_restatement(bank, ref):
    frame, center, scale = _args()
    assert len({f for f in frame}) == len(FR.CASE_SIZES) and max(frame.count(f) for f in frame) > 3
    out = bank.crop(frame, center, scale, FR.CASE_RES)
    assert out.shape == (len(FR.CASES), 3, FR.CASE_RES, FR.CASE_RES) and out.dtype == torch.float32
    got = out.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    worst = 0.0
    for i, c in enumerate(FR.CASES):
        err = float(np.abs(got[i] - ref[i]).max())
        worst = max(worst, err)
        print("%-62s max |device - restatement| = %.2e" % (c[0], err))
    for i, c in enumerate(FR.CASES):
        assert float(np.abs(got[i] - ref[i]).max()) < TOL, c[0]
    print("worst %.2e (bar %.0e)" % (worst, TOL))
    outside = [c[0] for c in FR.CASES].index("box wholly outside the frame")
    want = -torch.tensor(FR.CASE_MEANS).view(3, 1, 1).expand(3, FR.CASE_RES, FR.CASE_RES)
    assert torch.equal(out[outside].cpu(), want)


def test_two_launches_give_equal_bits(bank):
    frame, center, scale = _args()
    a = bank.crop(frame, center, scale, FR.CASE_RES)
    b = bank.crop(frame, center, scale, FR.CASE_RES)
    assert torch.equal(a, b)


@pytest.mark.parametrize("i", [0, 5, 11, 14])
def test_one_box(bank, ref, i):
    frame, center, scale = _args([i])
    out = torch.full((1, 3, FR.CASE_RES, FR.CASE_RES), float("nan"), device=DEV)
    got = bank.crop(frame, center, scale, FR.CASE_RES, out=out)
    assert got is out
    assert float(np.abs(out[0].cpu().numpy().astype(np.float64) - ref[i]).max()) < TOL


def test_chunked_workspace_gives_the_same_bits(bank, monkeypatch):
    """The wrapper splits the boxes where the intermediate would pass its budget: with a budget
    of a few boxes the launches are several and the output is the one launch's."""
    from ubpl_amd import _lib
    from ubpl_amd.kernels import augment as KA
    frame, center, scale = _args()
    whole = bank.crop(frame, center, scale, FR.CASE_RES)
    seen = []
    call = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (seen.append((name, a[7])), call(name, *a))[1])
    monkeypatch.setattr(KA, "CROP_WORKSPACE_BYTES", 200 * 1024)
    parts = bank.crop(frame, center, scale, FR.CASE_RES)
    assert torch.equal(parts, whole)
    assert len(seen) > 2 and {n for n, _ in seen} == {"ubpl_crop_frames"} and sum(k for _, k in seen) == len(FR.CASES)


def test_wrapper_refuses_what_the_kernel_would_read_out_of_bounds(bank):
    from ubpl_amd import kernels as Kn
    from ubpl_amd.frames import crop_plan
    plan = crop_plan(bank.sizes, [2], [(100, 75)], [0.224], FR.CASE_RES)
    t = plan.table.copy()
    t[0, 0] = len(bank)
    with pytest.raises(ValueError, match="frame index"):
        Kn.crop_frames(bank.bank, bank.off, bank.hw, t, plan.gauss, bank.chan_mean, FR.CASE_RES)
    with pytest.raises(ValueError, match="past the end of the bank"):
        Kn.crop_frames(bank.bank[:-1].clone(), bank.off, bank.hw, plan.table, plan.gauss, bank.chan_mean, FR.CASE_RES)
    with pytest.raises(ValueError, match="shape"):
        Kn.crop_frames(bank.bank, bank.off, bank.hw, plan.table, plan.gauss, bank.chan_mean, FR.CASE_RES,
                       out=torch.empty(2, 3, FR.CASE_RES, FR.CASE_RES, device=DEV))
