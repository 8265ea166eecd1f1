"""csrc/pagk_select.h: select_variant gives what launch_track's chain of booleans gave before the header existed, the
batch's question and the block5 choice are the conditions the launches spelled out, and the patch-shape helpers give the
template arguments that track_routes.py lists by hand."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import track_routes as tr

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pixel_aware_gyro_aided_klt_feature_tracker_amd", "csrc")

COLUMNS = ("kernel", "half", "calc_ncc", "pyramids", "iterations", "n", "concurrency", "lv_error", "levels_shared",
           "mfma_min", "wave_min", "quad_min", "levels_min", "all_variants")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("select") / "select_probe.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-o", so,
                    os.path.join(HERE, "select_probe.cpp")], check=True)
    lib = C.CDLL(so)
    for name in ("select_probe", "batched_probe"):
        getattr(lib, name).restype = None
        getattr(lib, name).argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    lib.block5_probe.restype = C.c_int32
    lib.block5_probe.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32]
    lib.shape_probe.restype = None
    lib.shape_probe.argtypes = [C.c_int32, C.c_void_p]
    lib.common_probe.restype = C.c_int32
    lib.common_probe.argtypes = [C.c_int32]
    return lib


def chain_of_booleans(kernel, half, calc_ncc, pyramids, iterations, n, concurrency, lv_error, levels_shared,
                      mfma_min, wave_min, quad_min, levels_min, all_variants):
    """launch_track's selection as it stood before the header, line by line (on arrays: & | ~ for && || !): the five
    booleans, the two of them that existed only under PAGK_ALL_VARIANTS, and the nested ternary of last_variant."""
    mfma_ok = (half == 5) | (half == 7) | (half == 10)
    n_sel = n * concurrency
    use_rows = all_variants & (mfma_ok & ~calc_ncc & (iterations >= 1) & (kernel == 6))
    use_levels = mfma_ok & ~calc_ncc & (pyramids >= 2) & lv_error & (
        (kernel == 7) | ((kernel == 0) & ((concurrency == 1) | levels_shared) & (n_sel >= levels_min)))
    quad_like = (kernel == 5) | (kernel == 6) | (kernel == 7)
    use_quad = ~use_rows & ~use_levels & mfma_ok & ~calc_ncc & (quad_like | ((kernel == 0) & (n_sel >= quad_min)))
    use_wave = ~use_quad & ~use_rows & ~use_levels & mfma_ok & (
        (kernel == 3) | quad_like | ((kernel == 0) & (n_sel >= wave_min)))
    use_mfma = all_variants & (~use_wave & mfma_ok & ((kernel == 2) | ((kernel == 0) & (n_sel >= mfma_min))))
    w = np.where
    return w(kernel == 1, 1, w(use_levels, 7, w(use_rows, 6, w(use_quad, 5, w(use_wave, 3, w(
        (kernel == 4) & mfma_ok, 4, w(use_mfma, 2, 0)))))))


def batch_condition(kernel, half, calc_ncc, pyramids, lv_error, levels_min, total_n, total_q):
    """pagk_track_device_batch's `batched` as it stood before the header."""
    mfma_ok = (half == 5) | (half == 7) | (half == 10)
    return mfma_ok & ~calc_ncc & (pyramids >= 2) & lv_error & (total_q > 0) & (
        (kernel == 7) | ((kernel == 0) & (total_n >= levels_min)))


def product(*axes):
    grids = np.meshgrid(*[np.asarray(a, np.int64) for a in axes], indexing="ij")
    return np.stack([g.ravel() for g in grids], axis=1)


def columns(rows, names=COLUMNS):
    flags = ("calc_ncc", "lv_error", "levels_shared", "all_variants")
    return {name: rows[:, k].astype(bool) if name in flags else rows[:, k] for k, name in enumerate(names)}


# (mfma_min, wave_min, quad_min, levels_min): distinct and even, in the product's order and in another one
THRESHOLDS = ((50, 20, 30, 40), (10, 40, 30, 20))


def launch_sizes(thresholds):
    # each threshold - 1, exactly, + 1 -- for n itself and, under concurrency 2, for 2 n -- plus 0 and 1
    return sorted({0, 1} | {t // c + d for t in thresholds for c in (1, 2) for d in (-1, 0, 1)})


@pytest.mark.parametrize("thresholds", THRESHOLDS)
def test_select_variant_equals_the_chain_of_booleans_it_replaces(probe, thresholds):
    rows = product(range(8), range(1, 16), (0, 1), (1, 2, 3), (0, 1), launch_sizes(thresholds), (1, 2), (0, 1), (0, 1),
                   *[(t,) for t in thresholds], (0, 1))
    got = np.full(len(rows), -1, np.int32)
    probe.select_probe(rows.ctypes.data, len(rows), got.ctypes.data)
    want = chain_of_booleans(**columns(rows))
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} of {len(rows)} inputs differ, the first: {dict(zip(COLUMNS, rows[bad[0]]))} -> " \
                          f"{got[bad[0]]}, the chain gave {want[bad[0]]}"
    # the product build never answers 2 or 6, and every variant is reached by some input
    assert not np.isin(got[rows[:, 13] == 0], (2, 6)).any()
    assert set(got.tolist()) == set(range(8))


def test_corners_that_fell_out_of_the_chain(probe):
    def variant(**kw):
        base = dict(kernel=0, half=10, calc_ncc=0, pyramids=3, iterations=10, n=100, concurrency=1, lv_error=1,
                    levels_shared=0, mfma_min=0x7fffffff, wave_min=6000, quad_min=7000, levels_min=6000, all_variants=1)
        base.update(kw)
        row = np.array([base[name] for name in COLUMNS], np.int64)
        got = np.zeros(1, np.int32)
        probe.select_probe(row.ctypes.data, 1, got.ctypes.data)
        return int(got[0])
    assert [variant(kernel=1, half=h) for h in (3, 10, 15)] == [1, 1, 1]            # selector 1 wins whatever h
    assert [variant(kernel=k, calc_ncc=1) for k in (5, 6, 7)] == [3, 3, 3]
    assert [variant(kernel=k, half=6) for k in range(2, 8)] == [0] * 6              # a non-common h
    assert variant(kernel=7, pyramids=1) == 5
    assert variant(kernel=7, lv_error=0) == 5
    assert (variant(kernel=6, iterations=0), variant(kernel=6, iterations=1), variant(kernel=6, all_variants=0)) == (5, 6, 5)
    assert (variant(kernel=2), variant(kernel=2, all_variants=0)) == (2, 0)
    # selector 0: thresholds on n * concurrency; 7 only for a context alone on the device (or PAGK_LEVELS_SHARED)
    assert (variant(n=5999), variant(n=6000), variant(n=3000, concurrency=2), variant(n=3500, concurrency=2)) == (0, 7, 3, 5)
    assert variant(n=3500, concurrency=2, levels_shared=1) == 7
    assert (variant(n=6000, calc_ncc=1), variant(n=7000, pyramids=1)) == (3, 5)


def test_the_batch_asks_select_variant(probe):
    thresholds = THRESHOLDS[0]
    # (kernel .. all_variants as above, the lead context's own n and concurrency being anything), total_n, total_q
    rows = product(range(8), range(1, 16), (0, 1), (1, 2, 3), (0, 1), (0, 1000), (1, 2), (0, 1), (0, 1),
                   *[(t,) for t in thresholds], (0, 1), launch_sizes(thresholds), (0, 5))
    got = np.full(len(rows), -1, np.int32)
    probe.batched_probe(rows.ctypes.data, len(rows), got.ctypes.data)
    c = columns(rows, COLUMNS + ("total_n", "total_q"))
    want = batch_condition(c["kernel"], c["half"], c["calc_ncc"], c["pyramids"], c["lv_error"], c["levels_min"],
                           c["total_n"], c["total_q"])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} of {len(rows)} inputs differ, the first: {rows[bad[0]].tolist()}"
    assert want.any() and not want.all()


def test_block5_choice(probe):
    cus = 256
    for window in (0, 1):
        for n, inside in ((4 * cus, False), (4 * cus + 1, True), (5 * cus, True), (5 * cus + 1, False)):
            assert probe.block5_probe(n, 2500, window, cus) == int(bool(window) and inside), (n, window)
        assert [probe.block5_probe(n, 2500, window, cus) for n in (2499, 2500, 2501)] == [0, 1, 1]
    # PAGK_BLOCK5_MIN=1 (the block5 route of the instantiation matrix): every launch
    assert [probe.block5_probe(n, 1, 0, cus) for n in (1, 67)] == [1, 1]
    # the expression launch_track spelled out before the header, over a range that covers both ends of both rules
    for n, block5_min, window in itertools.product(range(0, 1500, 7), (1, 1100, 2500), (0, 1)):
        want = n >= block5_min or (bool(window) and n > 4 * cus and n <= 5 * cus)
        assert probe.block5_probe(n, block5_min, window, cus) == int(want), (n, block5_min, window)


def test_patch_shapes_are_the_template_arguments_of_the_routes(probe):
    for h in range(1, 16):
        out = np.zeros(5, np.int32)
        probe.shape_probe(h, out.ctypes.data)
        P, nr, tail, nch, mfma_nr = out.tolist()
        assert P == (2 * h + 1) ** 2
        assert (nr, tail) == tr.BLOCK_ARGS[h], h
        assert bool(probe.common_probe(h)) == (h in tr.COMMON), h
        if h in tr.COMMON:
            assert nch == tr.NCH[h] and (mfma_nr, tail) == tr.MFMA_ARGS[h], h
