"""The clamp-free sample5 takes its minus-side taps from the centre's quad (idx - 1, idx - cols) with the centre's
fractions (csrc/pagk_device.h; the float32 facts are swept in test_sampler_minus_cpu.py).  Here the device sampler is held
against the oracle's, bit for bit, where that could go wrong: at the binade tops 2 .. 1024, where X - 1 changes binade and
X + 1 rounds, on images just wide (high) enough to have them inside the clamp-free domain; the clamped form outside that
domain; and a tracking launch of the pipelined 4-wave body whose patches straddle 512 and 1024."""
import numpy as np
import pytest

from oracle import pagk_oracle as orc
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, synth

import sampler_cases as sc

pytestmark = pytest.mark.gpu
F = np.float32
LONG, SHORT = 1032, 6   # [1, LONG - 2) holds 1024 + ulp; [1, SHORT - 2) = [1, 4)


def _image(rows, cols):
    return np.random.default_rng(0x51DE + cols).integers(1, 256, (rows, cols), dtype=np.uint8)


def _binade_axis():
    """2^k - 2 ulp, 2^k - ulp, 2^k, 2^k + ulp for k = 1..10, and 1.0 with its float neighbours."""
    vals = [np.nextafter(F(1), F(0)), F(1), np.nextafter(F(1), F(2))]
    for k in range(1, 11):
        t = F(2 ** k)
        below = np.nextafter(t, F(0))
        vals += [np.nextafter(below, F(0)), below, t, np.nextafter(t, F(np.inf))]
    return np.array(vals, F)


def _cross(xs, ys):
    xy = np.empty((len(xs) * len(ys), 2), F)
    xy[:, 0] = np.repeat(xs, len(ys))
    xy[:, 1] = np.tile(ys, len(xs))
    return xy


def _check5(ctx, img, xy, what, free_must_cover=None):
    """sample5<true> at every row of xy, sample5<false> at those inside its domain, against the oracle."""
    rows, cols = img.shape
    want = orc.sample(img, sc.five(xy).reshape(-1, 2)).reshape(-1, 5)
    got = ctx.selftest_sample(0, 0, 2, xy)
    bad = np.flatnonzero((sc.bits(got) != sc.bits(want)).any(axis=1))
    assert bad.size == 0, f"{what}: sample5<true> differs from the oracle at {bad.size} coordinates, the first {xy[bad[0]]}: " \
                          f"{got[bad[0]]} vs {want[bad[0]]}"
    sel = sc.inside(xy, cols, rows, 1)
    if free_must_cover is not None:
        assert sel.sum() == free_must_cover, f"{what}: {sel.sum()} coordinates in the clamp-free domain, expected {free_must_cover}"
        free = ctx.selftest_sample(0, 0, 3, xy[sel])
        bad = np.flatnonzero((sc.bits(free) != sc.bits(want[sel])).any(axis=1))
        assert bad.size == 0, f"{what}: sample5<false> differs from the oracle at {bad.size} coordinates, the first " \
                              f"{xy[sel][bad[0]]}: {free[bad[0]]} vs {want[sel][bad[0]]}"
    else:
        assert sel.sum() == 0, f"{what}: meant to lie outside the clamp-free domain"


@pytest.mark.parametrize("long_axis", ["x", "y"])
def test_binade_tops(ctx, long_axis):
    img = _image(SHORT, LONG) if long_axis == "x" else _image(LONG, SHORT)
    ctx.frame_upload(0, img, 1)
    a, other = _binade_axis(), np.array([1.0, 2.25, 3.75], F)
    xy = _cross(a, other) if long_axis == "x" else _cross(other, a)
    # everything but 1 - ulp is inside [1, 1030) x [1, 4)
    _check5(ctx, img, xy, f"binade tops on {long_axis}", free_must_cover=(len(a) - 1) * len(other))


@pytest.mark.parametrize("long_axis", ["x", "y"])
def test_clamped_form_outside_the_clamp_free_domain(ctx, long_axis):
    img = _image(SHORT, LONG) if long_axis == "x" else _image(LONG, SHORT)
    ctx.frame_upload(0, img, 1)
    eighth = F(0.125)
    low = np.arange(-16, 8, dtype=F) * eighth                        # [-2, 1)
    high = F(LONG - 2) + np.arange(0, 16, dtype=F) * eighth          # the last two columns (rows)
    a = np.concatenate([low, [np.nextafter(F(1), F(0))], high, [np.nextafter(F(LONG), F(0))]]).astype(F)
    other = np.array([-0.5, 0.0, 1.0, 2.25, 3.75, 4.5, 5.0, 5.5], F)
    xy = _cross(a, other) if long_axis == "x" else _cross(other, a)
    _check5(ctx, img, xy, f"clamped form, {long_axis} outside")


# ---- a tracking launch through the pipelined body -------------------------------------------------------------------
W, H_IMG, HALF = 1032, 600, 10


def _tracking_case():
    w = synth.make_workload("minus", W, H_IMG, 8, seed=0x51DE5, half_patch=HALF, iterations=30, pyramids=1,
                            motion="translation", has_gyro=False)
    shift = np.array([1.37, -0.83], F)   # make_workload's translation
    pt_ref = np.array([[508.3, 300.6],     # patch columns 498 .. 518: across 512
                       [1015.7, 200.2],    # 1005 .. 1026 (+1: 1027 < cols - 1): across 1024, clamp-free
                       [300.4, 509.1],     # patch rows across 512
                       [513.9, 514.2],     # both axes just above 512: the minus taps reach below it
                       [1022.6, 505.5],    # reaches past the last column: the clamped form
                       [11.8, 40.3],       # reaches the first columns: the clamped form
                       [640.2, 77.7],      # switched off on input
                       [255.5, 127.5]], F)
    err = np.array([[0.6, -0.4], [-0.5, 0.3], [0.2, 0.7], [-0.7, -0.2], [0.4, 0.4], [-0.3, 0.5], [0.0, 0.0], [0.5, -0.6]], F)
    pt_init = (pt_ref + shift + err).astype(F)
    affine = np.tile(np.array([1.0, 0.0, 0.0, 1.0], F), (8, 1))
    affine[1] = (1.01, 0.02, -0.015, 0.99)
    affine[3] = (0.98, -0.03, 0.025, 1.02)
    status = np.ones(8, np.uint8)
    status[6] = 0
    return w, pt_ref, pt_init, np.ascontiguousarray(affine), status


@pytest.mark.parametrize("illum", [True, False], ids=["illum", "no-illum"])
def test_tracking_across_512_and_1024(illum):
    w, pt_ref, pt_init, affine, status = _tracking_case()
    p = capi.make_params(half_patch=HALF, iterations=30, pyramids=1, has_gyro=True, illumination=illum, camera=w.camera)
    ref = orc.track(p, w.img_ref, w.img_cur, pt_ref, pt_init, affine, status, nthreads=4)
    c = capi.Context(0)
    try:
        got = c.track(p, w.img_ref, w.img_cur, pt_ref, pt_init, affine, status)
        assert c.last_variant() == 0, f"ran variant {c.last_variant()}, not the 4-wave kernel"
        c.check_launch()
    finally:
        c.close()
    for k in ("pt_un", "status", "pix_err", "iters"):
        assert np.array_equal(got[k][:8], ref[k][:8], equal_nan=True), f"{k}: device {got[k][:8]} vs oracle {ref[k][:8]}"
    assert ref["iters"][status != 0].min() >= 2, "a feature left the loop in its first iteration: the update path is not exercised"
    assert ref["status"][6] == 0
