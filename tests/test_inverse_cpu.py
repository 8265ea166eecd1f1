"""CPU tests of the template-Jacobian mode (include/pagk.h, pagk_params::inverse == PAGK_INVERSE_TEMPLATE): the parameter
check at the boundary, and the plain-C restatement (tests/inverse_ref.c) that the GPU tests compare with bit for bit -- its
summation order, determinism, exits, accuracy against the ground truth and the forward oracle, and the conditions under which
the GPU matrix says something.  No device."""
import os
import subprocess

import numpy as np
import pytest

import inverse_ref_util as iu
import shape_cases as sc
from oracle import pagk_oracle as orc
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi
from util import params_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE2 = (96, 64, 2)


# ---- the boundary --------------------------------------------------------------------------------------------------------
def test_check_params_admits_0_and_2_only(built):
    assert capi.PAGK_INVERSE_TEMPLATE == 2
    assert "pagk_params_check" in capi.EXPORTED_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "pagk.h")).read()
    assert "#define PAGK_INVERSE_TEMPLATE 2" in hdr and "int pagk_params_check(const pagk_params *params);" in hdr
    for inverse, want in ((0, capi.PAGK_OK), (2, capi.PAGK_OK), (1, capi.PAGK_E_UNSUPPORTED), (3, capi.PAGK_E_UNSUPPORTED),
                          (True, capi.PAGK_E_UNSUPPORTED), (255, capi.PAGK_E_UNSUPPORTED)):
        for h in (1, 5, 15):
            p = capi.make_params(half_patch=h, iterations=20, pyramids=3, inverse=inverse)
            assert p.inverse == int(inverse)
            assert capi.params_check(p) == want, (inverse, h)
    # the other checks are the ones they were, in either mode
    for inverse in (0, 2):
        assert capi.params_check(capi.make_params(half_patch=16, inverse=inverse)) == capi.PAGK_E_ARG
        assert capi.params_check(capi.make_params(pyramids=9, inverse=inverse)) == capi.PAGK_E_ARG
        assert capi.params_check(capi.make_params(solver_variant=16, inverse=inverse)) == capi.PAGK_E_ARG
    assert capi.load().pagk_params_check(None) == capi.PAGK_E_ARG
    assert capi.has_variant(8) and not capi.has_variant(9)


# ---- the sums --------------------------------------------------------------------------------------------------------------
def _model_sum(terms, dtype):
    """The order of include/pagk.h in numpy scalars of `dtype`."""
    v = [dtype(0)] * 64
    for k, t in enumerate(terms):
        v[k % 64] = dtype(v[k % 64] + dtype(t))
    for m in (1, 2, 4, 8, 16, 32):
        v = [dtype(v[s] + v[s ^ m]) for s in range(64)]
    return v[0]


def test_summation_order_of_the_restatement():
    lib = iu.lib()
    rng = np.random.default_rng(11)
    for count in (0, 1, 9, 63, 64, 65, 121, 441, 961):
        # magnitudes spread over thirty binades: any other order gives other bits
        t64 = (rng.standard_normal(count) * np.exp2(rng.integers(-15, 15, count))).astype(np.float64)
        t32 = t64.astype(np.float32)
        with np.errstate(over="ignore"):
            assert lib.inverse_ref_sum_f64(t64.ctypes.data, count) == _model_sum(t64, np.float64), count
            got32 = np.float32(lib.inverse_ref_sum_f32(t32.ctypes.data, count))
            assert got32 == _model_sum(t32, np.float32), count
    ones = np.ones(961, np.float64)
    assert lib.inverse_ref_sum_f64(ones.ctypes.data, 961) == 961.0


# ---- determinism -----------------------------------------------------------------------------------------------------------
def test_restatement_is_deterministic_and_independent_of_the_feature_order():
    w = sc.workload(SHAPE2, 5)
    for mode in sc.MODES:
        p = iu.shape_params(w, mode)
        first = iu.restated(SHAPE2, 5, mode)
        again = iu.track_workload(w, p)
        iu.assert_same(again, first, w.n, f"second run, {mode}")
        perm = np.random.default_rng(3).permutation(w.n)
        c = np.ascontiguousarray
        shuffled = iu.track(p, w.img_ref, w.img_cur, c(w.pt_ref[perm]), c(w.pt_init[perm]), c(w.affine[perm]), c(w.status_in[perm]))
        back = {k: c(first[k][perm]) for k in iu.KEYS}
        iu.assert_same(shuffled, back, w.n, f"permuted features, {mode}")
    # the image pair and the caller-built pyramids give the same bits
    lv_r, lv_c = [w.img_ref], [w.img_cur]
    for _ in range(w.pyramids - 1):
        lv_r.append(orc.pyr_down(lv_r[-1]))
        lv_c.append(orc.pyr_down(lv_c[-1]))
    pyr = iu.track_pyr(iu.shape_params(w, "lean"), lv_r, lv_c, w.pt_ref, w.pt_init, w.affine, w.status_in)
    iu.assert_same(pyr, iu.restated(SHAPE2, 5, "lean"), w.n, "caller-built pyramids")


# ---- exits -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", (5, 10))
def test_flat_patches_and_the_iteration_limits(h):
    w = sc.workload(SHAPE2, h)
    a, b, pt_ref, pt_init, status, idx = iu.flat_pair(w, h, w.pyramids)
    live = status[:w.n] > 0
    others = live.copy()
    others[idx] = False
    runs = {}
    for iterations in (0, 1, 2, 20):
        p = iu.shape_params(w, "lean")
        p.iterations = iterations
        runs[iterations] = r = iu.track(p, a, b, pt_ref, pt_init, w.affine, status)
        assert (r["iters"][:w.n][~live] == 0).all() and (r["status"][:w.n][~live] == 0).all()
        if iterations == 0:
            # no iteration runs: bSuccess keeps its initial value (:194), the point is the prediction carried down the levels
            assert (r["status"][:w.n][live] == 1).all() and (r["iters"][:w.n] == 0).all() and (r["pix_err"][:w.n] == 0).all()
            continue
        # a flat patch: H is zero, the solve returns NaN at iteration 0 of every level (:322): status 0, one iteration a level
        assert (r["status"][idx] == 0).all(), (iterations, r["status"][idx])
        assert (r["iters"][idx] == w.pyramids).all(), (iterations, r["iters"][idx])
        assert (r["pix_err"][idx] == 0).all()
        per_level = r["iters"][:w.n][others]
        assert (per_level >= w.pyramids).all() and (per_level <= iterations * w.pyramids).all()
    assert (runs[1]["iters"][:w.n][others] == w.pyramids).all()            # the limit ends every level
    assert (runs[2]["iters"][:w.n][others] > w.pyramids).any()             # a second iteration runs somewhere ...
    assert (runs[20]["iters"][:w.n][others] > 2 * w.pyramids).any()        # ... and 2 is a limit that binds
    assert int(runs[20]["status"][:w.n][others].sum()) >= 10               # (the rectangles leave texture for the others)


# ---- accuracy ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [name for name, _ in iu.ACCURACY])
def test_accuracy_against_the_truth_and_the_forward_oracle(name):
    """Per workload: every live feature ends with status 1 and within 0.5 px of the truth (the forward oracle satisfies both; its
    largest error on these workloads is 0.243 px), and the median error is at most 1.25 times the forward oracle's.  Measured
    (median / max error in px, iterations per live feature; forward | this mode):
        320x240 h10              0.0267 / 0.106, 10.5 | 0.0301 / 0.165, 11.7
        320x240 h5               0.0379 / 0.243, 11.1 | 0.0372 / 0.251, 12.2
        752x480 EUROC h10        0.0262 / 0.145, 10.7 | 0.0272 / 0.159, 11.6
        320x240 h7 omega         0.0330 / 0.146, 11.0 | 0.0340 / 0.164, 12.2
        640x480 h10 translation  0.0223 / 0.178, 10.9 | 0.0226 / 0.195, 11.5"""
    w = iu.accuracy_workload(name)
    p = params_for(w)
    fwd = orc.track(p, w.img_ref, w.img_cur, w.pt_ref, w.pt_init, w.affine, w.status_in, nthreads=8)
    inv = iu.track_workload(w, iu.inverse_params(p))
    live = w.status_in[:w.n] > 0
    assert int(live.sum()) >= 90

    def err(o):
        return np.linalg.norm(o["pt_un"][:w.n][live].astype(np.float64) - w.pt_true[:w.n][live], axis=1)
    ef, ei = err(fwd), err(inv)
    print(f"{name}: forward {np.median(ef):.4f} / {ef.max():.3f}, {fwd['iters'][:w.n][live].mean():.1f} | "
          f"inverse {np.median(ei):.4f} / {ei.max():.3f}, {inv['iters'][:w.n][live].mean():.1f}")
    assert (fwd["status"][:w.n][live] == 1).all() and ef.max() <= 0.5
    assert (inv["status"][:w.n][live] == 1).all()
    assert ei.max() <= 0.5, ei.max()
    assert np.median(ei) <= 1.25 * np.median(ef), (np.median(ei), np.median(ef))


# ---- the GPU matrix says something ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sc.SHAPES, ids=sc.shape_id)
def test_shape_matrix_is_not_vacuous(shape):
    for h in iu.HALVES:
        w = sc.workload(shape, h)
        what = f"{sc.shape_id(shape)} h={h}"
        lean = iu.restated(shape, h, "lean")
        fwd = sc.oracle(shape, h, "lean")
        live = w.status_in[:w.n] > 0
        tracked = lean["status"][:w.n] > 0
        assert int(live.sum()) >= 60, f"{what}: {int(live.sum())} live"
        assert int(tracked.sum()) >= 60, f"{what}: {int(tracked.sum())} tracked"
        differs = (lean["pt_un"][:w.n].view(np.uint32) != fwd["pt_un"][:w.n].view(np.uint32)).any(axis=1)
        assert differs[tracked].all(), f"{what}: {int((tracked & ~differs).sum())} tracked points equal the forward oracle's"
        # the generic kernel cannot ignore the penalty and the solver switches unnoticed
        both = iu.restated(shape, h, "both")
        moved = (both["pt_un"][:w.n].view(np.uint32) != lean["pt_un"][:w.n].view(np.uint32)).any(axis=1)
        assert int((moved & tracked).sum()) >= 1, what


# ---- sanitizers ------------------------------------------------------------------------------------------------------------------
def test_restatement_runs_clean_under_the_sanitizers(tmp_path):
    """A stand-alone program (tests/inverse_sanitize.c: its own main, compiled together with tests/inverse_ref.c and the oracle's
    source) tracks features on and beyond every border, NaN, infinite and huge coordinates included, under AddressSanitizer
    and UBSan; each image and each pyramid level sits in a heap block of exactly its size."""
    exe = str(tmp_path / "inverse_sanitize")
    subprocess.run(["gcc", "-std=gnu99", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "inverse_sanitize.c"),
                    os.path.join(ROOT, "tests", "inverse_ref.c"), os.path.join(ROOT, "oracle", "pagk_oracle.c"), "-o", exe,
                    "-lm", "-lpthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "4 images" in r.stdout, r.stdout
