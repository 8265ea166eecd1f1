"""The device sampler by itself: pagk_selftest_sample (sample<CLAMP> / sample5<CLAMP> of csrc/pagk_device.h on a built slot's
own tap plane) against the oracle's sampler (pagk_oracle_sample, itself held against a numpy model of the reference's
GetPixelValue in test_sampler_cpu.py), bit for bit, at every boundary coordinate of sampler_cases.coordinates.

The quarter-pixel grid weighs each of a quad's four bytes on its own (fractions 0, 0.25, 0.5, 0.75 in both axes), so this
is also the direct check of every packed tap plane: the last column and row, the wrap column of a padded level 0, the quad
of a 1-pixel level, and the planes both pyramid builders write (the single launch for even parents and at most four levels,
level by level otherwise).  The clamp-free forms are held against the clamped ones on every coordinate of the domain in
which the kernels' `interior` test selects them."""
import numpy as np
import pytest

from oracle import pagk_oracle as orc
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi

import sampler_cases as sc

pytestmark = pytest.mark.gpu
F = np.float32


def _levels(img, L):
    out = [img]
    for _ in range(1, L):
        out.append(orc.pyr_down(out[-1]))
    return out


def _check_level(ctx, slot, level, img, what, expect_interior=False):
    """Every mode of the self-test on one level whose pixels are `img`."""
    rows, cols = img.shape
    xy = sc.coordinates(cols, rows)
    want = orc.sample(img, xy)
    got = ctx.selftest_sample(slot, level, 0, xy)
    bad = np.flatnonzero(sc.bits(got) != sc.bits(want))
    assert bad.size == 0, f"{what}: {bad.size} of {len(xy)} clamped samples differ, the first at {xy[bad[0]]}: " \
                          f"device {got[bad[0]]!r}, oracle {want[bad[0]]!r}"
    # the five samples of a Gauss-Newton pixel = five single samples at the +-1 coordinates formed in float32
    xy5 = sc.five(xy)
    want5 = orc.sample(img, xy5.reshape(-1, 2)).reshape(-1, 5)
    single5 = ctx.selftest_sample(slot, level, 0, xy5.reshape(-1, 2)).reshape(-1, 5)
    got5 = ctx.selftest_sample(slot, level, 2, xy)
    for name, other in (("the oracle", want5), ("five single device samples", single5)):
        bad = np.flatnonzero((sc.bits(got5) != sc.bits(other)).any(axis=1))
        assert bad.size == 0, f"{what}: sample5 differs from {name} at {bad.size} coordinates, the first {xy[bad[0]]}: " \
                              f"{got5[bad[0]]} vs {other[bad[0]]}"
    # the clamp-free forms, wherever the call admits them
    for mode, margin, clamped in ((1, 0, got), (3, 1, got5)):
        sel = sc.inside(xy, cols, rows, margin)
        if expect_interior:
            assert sel.sum() > 100, f"{what}: mode {mode} has only {sel.sum()} coordinates in its domain"
        free = ctx.selftest_sample(slot, level, mode, xy[sel])
        assert np.array_equal(sc.bits(free), sc.bits(clamped[sel])), \
            f"{what}: the clamp-free mode {mode} differs from the clamped one inside its domain"


@pytest.mark.parametrize("name", list(sc.images()))
def test_level0_images(ctx, name):
    img = sc.images()[name]
    ctx.frame_upload(0, img, 1)
    _check_level(ctx, 0, 0, img, name, expect_interior=name.startswith("13x7"))


@pytest.mark.parametrize("width,height,L,top", sc.PYRAMIDS, ids=[f"{w}x{h}-L{L}" for w, h, L, _ in sc.PYRAMIDS])
def test_pyramid_levels(ctx, width, height, L, top):
    img = sc.frame(width, height)
    ctx.frame_upload(0, img, L)
    levels = _levels(img, L)
    assert levels[-1].shape == top
    for l, lvl in enumerate(levels):
        assert np.array_equal(ctx.frame_download_level(0, l, width, height), lvl), f"level {l}"
        _check_level(ctx, 0, l, lvl, f"{width}x{height} level {l} ({lvl.shape[1]}x{lvl.shape[0]})")


def test_clamp_free_calls_outside_their_domain_are_refused(ctx):
    img = sc.images()["13x7"]   # cols 13, rows 7
    ctx.frame_upload(0, img, 1)
    inside1, inside3 = np.array([[5.25, 3.5]], F), np.array([[5.25, 3.5]], F)
    out = np.zeros(16, F)

    def rc(mode, pts):
        pts = np.ascontiguousarray(pts, F)
        return ctx.lib.pagk_selftest_sample(ctx.h, 0, 0, mode, len(pts), pts.ctypes.data, out.ctypes.data)
    below_one = np.nextafter(F(1), F(0))
    for mode, ok, outside in (
            (1, inside1, [(12.0, 3.0), (3.0, 6.0), (np.nextafter(F(0), F(-1)), 3.0), (3.0, -0.25), (np.nan, 3.0), (3.0, np.nan),
                          (np.inf, 3.0), (-1e30, 3.0)]),
            (3, inside3, [(11.0, 3.0), (3.0, 5.0), (below_one, 3.0), (3.0, below_one), (np.nan, 3.0), (3.0, np.inf)])):
        assert rc(mode, ok) == capi.PAGK_OK
        for bad in outside:
            # one bad coordinate behind good ones: nothing is launched
            assert rc(mode, np.concatenate([ok, ok, np.array([bad], F)])) == capi.PAGK_E_ARG, (mode, bad)
    # the largest admitted coordinates
    assert rc(1, [(np.nextafter(F(12), F(0)), np.nextafter(F(6), F(0))), (-0.0, -0.0)]) == capi.PAGK_OK
    assert rc(3, [(np.nextafter(F(11), F(0)), np.nextafter(F(5), F(0))), (1.0, 1.0)]) == capi.PAGK_OK
    # other argument errors, and the context is usable afterwards
    assert rc(4, inside1) == capi.PAGK_E_ARG and rc(-1, inside1) == capi.PAGK_E_ARG
    assert ctx.lib.pagk_selftest_sample(ctx.h, 0, 1, 0, 1, inside1.ctypes.data, out.ctypes.data) == capi.PAGK_E_ARG   # no level 1
    assert ctx.lib.pagk_selftest_sample(ctx.h, 0, 0, 0, 1, None, out.ctypes.data) == capi.PAGK_E_ARG
    assert ctx.lib.pagk_selftest_sample(None, 0, 0, 0, 1, inside1.ctypes.data, out.ctypes.data) == capi.PAGK_E_ARG
    xy = sc.coordinates(13, 7)
    assert np.array_equal(sc.bits(ctx.selftest_sample(0, 0, 0, xy)), sc.bits(orc.sample(img, xy)))
    ctx.check_launch()
