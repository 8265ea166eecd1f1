"""The oracle's sampler by itself: pagk_oracle_sample (the static get_pixel_value that every oracle function calls) held bit
for bit against a numpy float32 model of PatchMatch::GetPixelValue (reference src/patch_match.cpp:391-406) written line by
line on the flat buffer, at every boundary coordinate of sampler_cases.coordinates: on 13 x 7, 2 x 1 and 1 x 1 images and on
a 13 x 7 view of a buffer with 16 bytes per row and non-zero padding.  test_sampler_gpu.py holds the device sampler against
the same oracle function on the same coordinates."""
import os
import subprocess

import numpy as np
import pytest

from oracle import pagk_oracle as orc

import sampler_cases as sc

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(sc.images()))
def test_oracle_sampler_equals_the_numpy_model(built, name):
    img = sc.images()[name]
    rows, cols = img.shape
    xy = sc.coordinates(cols, rows)
    # the set is what it claims to be: the quarter-pixel grid over [-2, size + 2], and the edges' float neighbours
    grid = (4 * (cols + 4) + 1) * (4 * (rows + 4) + 1)
    assert xy.shape[0] > grid and np.isnan(xy).any() and np.isinf(xy).any()
    for v in (np.nextafter(F(cols), F(0)), np.nextafter(F(cols - 1), F(cols)), F(cols) - F(0.25), F(-2), F(cols + 2)):
        assert (xy[:, 0] == v).any(), v
    got, want = orc.sample(img, xy), sc.model(img, xy)
    assert np.isfinite(want).all()
    bad = np.flatnonzero(sc.bits(got) != sc.bits(want))
    assert bad.size == 0, f"{name}: {bad.size} of {len(xy)} samples differ, the first at {xy[bad[0]]}: " \
                          f"oracle {got[bad[0]]!r}, model {want[bad[0]]!r}"


def test_padding_reads_zero_and_only_a_continuous_image_wraps(built):
    """At x = 12.5 the right-hand taps are data[13]: the next row's first pixel of a continuous 13-column image, a padding
    byte (0xEE in the buffer, 0 by definition) behind a 16-byte row.  At y = 6.5 the lower taps are past the buffer: 0."""
    cont, view = sc.images()["13x7"], sc.images()["13x7-stride16"]
    assert np.array_equal(cont, view) and view.strides[0] == 16 and cont.strides[0] == 13
    assert (view.base[:, 13:] == 0xEE).all()
    rows = np.arange(6, dtype=F)
    xy = np.stack([np.full(6, 12.5, F), rows], 1)
    half = F(0.5)
    wrapped = half * cont[:6, 12].astype(F) + half * cont[1:, 0].astype(F)
    padded = half * cont[:6, 12].astype(F)
    assert (cont[1:, 0] > 0).all()   # (so that the two differ in every row)
    for sample in (orc.sample, sc.model):
        assert np.array_equal(sample(cont, xy), wrapped), sample
        assert np.array_equal(sample(view, xy), padded), sample
    # past the last row, and the corner: data[1] of the last pixel is past the end as well
    below = np.array([[3.0, 6.5], [12.5, 6.0], [12.5, 6.5]], F)
    want = np.array([half * F(cont[6, 3]), half * F(cont[6, 12]), F(0.25) * F(cont[6, 12])], F)
    for img in (cont, view):
        for sample in (orc.sample, sc.model):
            assert np.array_equal(sample(img, below), want), sample


def test_sampler_argument_checks(built):
    img = sc.images()["2x1"]
    assert orc.sample(img, np.zeros((0, 2), F)).shape == (0,)
    lib = orc.load()
    assert lib.pagk_oracle_sample(None, 1, None, None) != 0
    one = np.zeros(2, F)
    from pixel_aware_gyro_aided_klt_feature_tracker_amd.capi import image_view
    import ctypes as C
    iv = image_view(img)
    assert lib.pagk_oracle_sample(C.byref(iv), 1, one.ctypes.data, None) != 0
    assert lib.pagk_oracle_sample(C.byref(iv), -1, one.ctypes.data, one.ctypes.data) != 0


def test_header_declares_and_capi_binds_the_self_test(built):
    from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi
    hdr = open(os.path.join(ROOT, "include", "pagk.h")).read()
    assert "int pagk_selftest_sample(pagk_ctx *ctx, int32_t slot, int32_t level, int32_t mode, int32_t n, const float *xy, float *out);" in hdr
    assert "#define PAGK_VERSION 303" in hdr   # a new symbol, not a new number: ask for the symbol
    assert "int pagk_oracle_sample(const pagk_image *image, int32_t n, const float *xy, float *out);" in \
        open(os.path.join(ROOT, "oracle", "pagk_oracle.h")).read()
    lib = capi.load()
    assert "pagk_selftest_sample" in capi.EXPORTED_SYMBOLS and len(lib.pagk_selftest_sample.argtypes) == 7
    assert callable(getattr(capi.Context, "selftest_sample"))
    # argument checks that need no device
    xy, out = np.zeros(2, F), np.zeros(5, F)
    assert lib.pagk_selftest_sample(None, 0, 0, 0, 1, xy.ctypes.data, out.ctypes.data) == capi.PAGK_E_ARG


def test_oracle_sampler_runs_clean_under_the_sanitizers(tmp_path):
    """A stand-alone program (tests/sampler_sanitize.c: its own main, compiled together with the oracle's source) drives
    pagk_oracle_sample over the coordinate set on the 1 x 1, 2 x 1 and padded 13 x 7 images under AddressSanitizer and
    UBSan; each image sits in a heap block of exactly its size, so that a tap outside it is an error."""
    exe = str(tmp_path / "sampler_sanitize")
    subprocess.run(["gcc", "-std=c11", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "sampler_sanitize.c"),
                    os.path.join(ROOT, "oracle", "pagk_oracle.c"), "-o", exe, "-lm", "-lpthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "3 images" in r.stdout, r.stdout
