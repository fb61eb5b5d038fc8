"""Crop from raw frames, host side (no GPU): frames.crop_plan — the one statement of the
reference's branch logic — against the branch-by-branch float64 restatement
(tests/frame_crop_ref.py), and the composite form the device kernel runs, evaluated densely in
numpy from the plan, against the same restatement."""
import itertools

import numpy as np
import pytest
import torch

import frame_crop_ref as FR
from ubpl_amd import frames as F
from ubpl_amd import kernels as Kn


def test_plan_integers_match_the_restatement_over_a_grid():
    sizes = [(37, 53), (150, 200), (301, 420), (1080, 1920), (3, 300)]
    checked = {"crop": 0, "resize": 0, "refused": 0}
    for R in (32, 64):
        # sf = scale * 200 / R: below, just below, at, just above 2, and up to the limit
        sfs = [0.63, 1.1, 1.99, 1.9999, 2.0, 2.0001, 2.7, 7.9, 16.0]
        for (fi, (ht, wd)), sf in itertools.product(enumerate(sizes), sfs):
            scale = np.float32(sf * R / 200.0)
            centers = [(wd / 2.0, ht / 2.0), (0.0, 0.0), (wd - 0.5, ht - 0.25), (-40.0, 17.3), (wd + 90.0, -12.5),
                       (wd / 3.0, ht + 400.0), (11.0, 7.0)]
            for c in centers:
                try:
                    sf32, new_ht, new_wd, ul, br = FR.ref_geometry(ht, wd, c, scale, R)
                except ValueError:
                    new_ht = new_wd = 0
                if new_ht is not None and min(new_ht, new_wd) < 1:      # (an empty pre-resize: refused as well)
                    with pytest.raises(ValueError, match="too small"):
                        F.crop_plan(sizes, [fi], [c], [scale], R)
                    checked["refused"] += 1
                    continue
                plan = F.crop_plan(sizes, [fi], [c], [scale], R)
                b = plan.boxes[0]
                assert b["sf"] == sf32 and b["branch"] == ("crop" if new_ht is None else "resize"), (R, fi, sf, c)
                assert (b["ul"], b["br"], b["new_ht"], b["new_wd"]) == (ul, br, new_ht, new_wd), (R, fi, sf, c)
                t = plan.table[0]
                if new_ht is None:
                    assert tuple(t[1:7])[:5] == (ul[0], br[0] - ul[0], R, 0, R)
                    assert tuple(t[7:13])[:5] == (ul[1], br[1] - ul[1], R, 0, R)
                    assert tuple(t[13:15]) == (0, br[1] - ul[1])
                else:
                    assert tuple(t[1:7])[:5] == (0, wd, new_wd, ul[0], br[0] - ul[0])
                    assert tuple(t[7:13])[:5] == (0, ht, new_ht, ul[1], br[1] - ul[1])
                    assert 0 <= t[13] and t[14] >= 1 and t[13] + t[14] <= ht
                checked[b["branch"]] += 1
    assert checked["crop"] >= 200 and checked["resize"] >= 200 and checked["refused"] >= 10, checked
    # the float32 sf decides the branch: 1.9999 crops, 2.0 pre-resizes
    assert F.crop_plan([(150, 200)], None, [(100, 75)], [np.float32(1.9999 * 32 / 200)], 32).boxes[0]["branch"] == "crop"
    assert F.crop_plan([(150, 200)], None, [(100, 75)], [0.32], 32).boxes[0]["branch"] == "resize"


@pytest.fixture(scope="module")
def cases():
    frames = FR.case_frames()
    fr = [c[1] for c in FR.CASES]
    center = [c[2] for c in FR.CASES]
    scale = [c[3] for c in FR.CASES]
    plan = F.crop_plan(FR.CASE_SIZES, fr, center, scale, FR.CASE_RES)
    ref = [FR.ref_crop(frames[f], c, s, FR.CASE_RES, FR.CASE_MEANS) for f, c, s in zip(fr, center, scale)]
    return frames, plan, ref


def test_cases_cover_what_they_name(cases):
    _, plan, ref = cases
    by = {c[0]: (plan.boxes[i], plan.table[i]) for i, c in enumerate(FR.CASES)}
    assert [by[n][0]["branch"] for n in ("up-scale: a 20 px box, sf 0.63", "Gaussian radius 0, sf 1.1")] == ["crop"] * 2
    assert by["up-scale: a 20 px box, sf 0.63"][1][2] == 20
    assert [int(by["Gaussian radius %d, sf %s" % (r, s)][1][6]) for r, s in ((0, "1.1"), (1, "1.4"), (2, "1.95"))] \
        == [0, 1, 2]
    for n, sf in (("pre-resize, sf 2.0", 2.0), ("pre-resize, sf 2.7", 2.7), ("pre-resize, sf 7.9", 7.9)):
        assert by[n][0]["branch"] == "resize" and abs(by[n][0]["sf"] - sf) < 1e-5
    narrow = by["frame narrower than the Gaussian radius (3 rows, radius 4)"][1]
    assert narrow[8] == 3 and narrow[12] == 4
    # a pre-resized box over the left / top edge is R - 1 wide (the reference's int truncation):
    # the last resize is then no identity, and the plan carries it
    over = by["pre-resized box over the left and top edges"][1]
    assert over[5] == FR.CASE_RES - 1 and over[11] == FR.CASE_RES - 1
    outside = ref[[c[0] for c in FR.CASES].index("box wholly outside the frame")]
    assert np.array_equal(outside, np.broadcast_to(-np.array(FR.CASE_MEANS).reshape(3, 1, 1), outside.shape))


def test_composite_form_equals_the_restatement(cases):
    frames, plan, ref = cases
    for i, c in enumerate(FR.CASES):
        got = FR.plan_dense(plan, i, frames[c[1]], FR.CASE_MEANS)
        err = float(np.abs(got - ref[i]).max())
        print("%-62s max |dense - restatement| = %.2e" % (c[0], err))
        assert err < 1e-12, (c[0], err)


def test_identity_box_is_the_frame():
    rs = np.random.RandomState(3)
    img = rs.randint(0, 256, (64, 64, 3)).astype(np.uint8)
    plan = F.crop_plan([(64, 64)], None, [(32, 32)], [64 / 200.0], 64)
    assert plan.boxes[0] == {"sf": 1.0, "branch": "crop", "ul": (0, 0), "br": (64, 64), "new_ht": None, "new_wd": None}
    assert tuple(plan.table[0]) == (0, 0, 64, 64, 0, 64, 0, 0, 64, 64, 0, 64, 0, 0, 64, 0)
    assert plan.gauss.shape == (1, 2, 2) and np.array_equal(plan.gauss[0], [[1, 0], [1, 0]])
    want = np.transpose(img / 255.0, (2, 0, 1)) - np.array(FR.CASE_MEANS).reshape(3, 1, 1)
    assert np.array_equal(FR.plan_dense(plan, 0, img, FR.CASE_MEANS), want)
    assert np.array_equal(FR.ref_crop(img, (32, 32), 64 / 200.0, 64, FR.CASE_MEANS), want)
    # the Mouse validation crop: 256 x 256 at the image centre and scale 256 / 200
    plan = F.crop_plan([(256, 256)], None, torch.tensor([[128, 128]]), torch.tensor([256 / 200.0]), 256)
    assert tuple(plan.table[0][:15]) == (0, 0, 256, 256, 0, 256, 0, 0, 256, 256, 0, 256, 0, 0, 256)


def test_refusals():
    sizes = [(37, 53), (150, 200)]
    with pytest.raises(ValueError, match="beyond the supported"):
        F.crop_plan(sizes, [1], [(100, 75)], [np.float32(16.5 * 32 / 200)], 32)
    with pytest.raises(ValueError, match="too small"):                 # 37 x 53 by sf 16: 2 x 3 is fine, ...
        F.crop_plan([(20, 25)], [0], [(10, 10)], [np.float32(14.0 * 32 / 200)], 32)   # ... 20 x 25 by 14: 1 x 1
    F.crop_plan(sizes, [0], [(10, 10)], [np.float32(16.0 * 32 / 200)], 32)
    for bad in ([2], [-1]):
        with pytest.raises(ValueError, match="frame index"):
            F.crop_plan(sizes, bad, [(10, 10)], [0.2], 32)
    with pytest.raises(ValueError, match="frame index"):
        F.crop_plan(sizes, [0.5], [(10, 10)], [0.2], 32)
    with pytest.raises(ValueError, match="do not describe one set"):
        F.crop_plan(sizes, [0, 1], [(10, 10)], [0.2, 0.2], 32)
    with pytest.raises(ValueError, match="do not describe one set"):
        F.crop_plan(sizes, [0], [(10, 10)], [0.2, 0.3], 32)
    with pytest.raises(ValueError, match="do not describe one set"):
        F.crop_plan(sizes, None, [(10, 10)], [0.2], 32)              # frame None: one box per frame
    with pytest.raises(ValueError, match="empty box"):
        F.crop_plan(sizes, [0], [(10.5, 10.5)], [1e-6], 32)


def test_wrapper_checks_the_plan_and_chunks_the_workspace():
    from ubpl_amd.kernels import _check
    plan = F.crop_plan(FR.CASE_SIZES, [2, 3], [(100, 75), (200, 140)], [0.224, 0.432], 32)
    hw = np.array(FR.CASE_SIZES, np.int32)
    off = np.concatenate([[0], np.cumsum(hw[:, 0].astype(np.int64) * hw[:, 1] * 3)[:-1]])
    nbank = int((hw[:, 0].astype(np.int64) * hw[:, 1] * 3).sum())
    _check._crop_plan(plan.table, plan.gauss, off, hw, nbank, 32)
    with pytest.raises(ValueError, match="past the end of the bank"):
        _check._crop_plan(plan.table, plan.gauss, off, hw, nbank - 1, 32)
    for col, val, msg in ((0, 5, "frame index"), (6, 7, "out of range"), (2, 0, "out of range"),
                          (14, 0, "source rows"), (13, 300, "source rows")):
        t = plan.table.copy()
        t[1, col] = val
        with pytest.raises(ValueError, match=msg):
            _check._crop_plan(t, plan.gauss, off, hw, nbank, 32)
    with pytest.raises(ValueError, match="gauss is"):
        _check._crop_plan(plan.table, plan.gauss[:1], off, hw, nbank, 32)
    # chunks: boxes x 3 x (largest row count) x R floats within the budget, every box once, in order
    rows = [300, 300, 1080, 40, 40, 40, 2000]
    for budget in (1 << 20, 4 << 20, 256 << 20):
        chunks = Kn._crop_chunks(rows, 256, budget)
        assert [a for a, _ in chunks] == [0] + [e for _, e in chunks[:-1]] and chunks[-1][1] == len(rows)
        for a, e in chunks:
            assert e - a == 1 or (e - a) * 12 * max(rows[a:e]) * 256 <= budget
    assert Kn._crop_chunks(rows, 256, 256 << 20) == [(0, len(rows))]
    assert Kn._crop_chunks(rows, 256, 1 << 20) == [(0, 1), (1, 2), (2, 3), (3, 6), (6, 7)]
    assert Kn.CROP_WORKSPACE_BYTES == 256 << 20
    # a launch holds at most 65535 boxes (the box is grid.y), however small the workspace they need
    many = Kn._crop_chunks([8] * 140000, 8)
    assert many == [(0, 65535), (65535, 131070), (131070, 140000)] and Kn.CROP_MAX_BOXES == 65535
    # a row range that misses a tap is refused (the kernel would skip the tap: wrong pixels, no
    # fault), while any range that holds every tap passes; the taps are recomputed from the axis
    for i, (a, b) in enumerate(_check._crop_taps(plan.table[k, 7:13], 32) for k in range(2)):
        first, rows = (int(v) for v in plan.table[i, 13:15])
        assert first <= a and b < first + rows
        for col, val in ((13, a + 1), (14, b - first)):
            t = plan.table.copy()
            t[i, col] = val
            with pytest.raises(ValueError, match="reads source rows|leave its virtual source"):
                _check._crop_plan(t, plan.gauss, off, hw, nbank, 32)
        t = plan.table.copy()
        t[i, 13:15] = a, b - a + 1                            # the tightest range
        _check._crop_plan(t, plan.gauss, off, hw, nbank, 32)
    assert _check._crop_taps((0, 20, 20, 500, 32, 0), 32) is None      # a box outside the zoom grid


def test_every_case_plan_holds_its_taps():
    """crop_plan's row ranges against the tap-by-tap recomputation the wrapper's check runs, on the
    kernel cases and on boxes at the sf = 2 boundary over every frame edge."""
    from ubpl_amd.kernels import _check
    plan = F.crop_plan(FR.CASE_SIZES, [c[1] for c in FR.CASES], [c[2] for c in FR.CASES], [c[3] for c in FR.CASES],
                       FR.CASE_RES)
    hw = np.array(FR.CASE_SIZES, np.int32)
    size = hw[:, 0].astype(np.int64) * hw[:, 1] * 3
    _check._crop_plan(plan.table, plan.gauss, np.concatenate([[0], np.cumsum(size)[:-1]]), hw, int(size.sum()),
                      FR.CASE_RES)
    for sf in (1.99, 2.0, 3.3, 9.0, 16.0):
        for c in ((0, 0), (420, 301), (-30, 150), (210, 330), (3.5, 7.25)):
            p = F.crop_plan([(301, 420)], None, [c], [np.float32(sf * 32 / 200)], 32)
            need = _check._crop_taps(p.table[0, 7:13], 32)
            assert need is None or (p.table[0, 13] <= need[0] and need[1] < p.table[0, 13] + p.table[0, 14]), (sf, c)
