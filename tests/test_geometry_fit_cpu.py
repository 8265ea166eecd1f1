"""The RANSAC fits of GeometryValidation (include/pagk.h pagk_geometry_fit): the plain-C restatement the device is held
to (tests/geometry_fit_ref.c) against the ground truth of seeded two-view scenes, its sampling recipe, its masks and
its degenerate inputs.  No GPU needed."""
import numpy as np
import pytest

from fit_ref_util import (build_ref, collinear_case, epipolar_error, normalised, params, ref_fit, ref_samples,
                          transfer_error)
from util import make_geometry_case

WIDE = (0.6, -0.3, 0.2)   # a baseline at which F is well conditioned (the default case is close to a pure rotation)
MASK = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return build_ref(tmp_path_factory.mktemp("fitref"))


def _scene(seed, n, planar, noise, outliers):
    return make_geometry_case(seed, n, outlier_fraction=outliers, noise_px=noise, planar=planar,
                              translation=(0.05, -0.02, 0.01) if planar else WIDE)


def _truth(g, planar):
    e = transfer_error(g["H21"], g["pts1"], g["pts2"]) if planar else epipolar_error(g["F21"], g["pts1"], g["pts2"])
    return e <= 3.0, np.abs(e - 3.0) < 0.05


@pytest.mark.parametrize("planar", [True, False])
@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("noise,outliers", [(0.0, 0.0), (0.0, 0.2), (0.0, 0.4), (0.2, 0.2), (0.4, 0.4)])
def test_restatement_recovers_ground_truth(ref, planar, seed, noise, outliers):
    g = _scene(seed, 1000, planar, noise, outliers)
    r = ref_fit(ref, params(seed=seed), g["pts1"], g["pts2"])
    key, mk, info = ("H21", "mask_H", r["H"]) if planar else ("F21", "mask_F", r["F"])
    assert info["status"] == 1 and info["best"] >= 0 and info["valid"] > 0
    assert info["refit_count"] == int(r[mk].sum())
    d = np.abs(normalised(r[key]) - normalised(g[key])).max()
    # exact data: the true model to 1e-6; outliers that happen to fall inside the threshold, or pixel noise, enter the
    # (unweighted, unrefined) least-squares refit
    assert d <= (1e-6 if noise == 0 and outliers == 0 else 1e-2), d
    truth, ambiguous = _truth(g, planar)
    wrong = (r[mk].astype(bool) != truth) & ~ambiguous
    if noise == 0 and outliers == 0:
        assert not wrong.any(), np.flatnonzero(wrong)
    else:   # the refit model is off by a fraction of a pixel: a few points near the threshold may move
        assert wrong.sum() <= 0.005 * len(truth), np.flatnonzero(wrong)
    assert abs(r["H21"][2, 2] - 1.0) == 0.0 and (planar or r["F21"][2, 2] == 1.0)
    assert np.allclose(r["H12"] @ r["H21"], np.eye(3), atol=1e-9)


def test_planar_scene_gives_no_fundamental_matrix(ref):
    # 8 points of one plane leave the 8-point system degenerate: every F hypothesis is invalid
    g = _scene(4, 500, True, 0.0, 0.0)
    r = ref_fit(ref, params(seed=4), g["pts1"], g["pts2"])
    assert r["H"]["status"] == 1 and r["F"] == dict(status=0, best=-1, best_count=0, refit_count=0, valid=0, adaptive=0)
    assert (r["hyp_counts"][2000:] == -1).all() and not r["mask_F"].any() and not r["F21"].any()


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def _draws(seed, model, hyp, m, s):
    out, d = [], 0
    while len(out) < s and d < 64:
        z = _splitmix64(seed ^ _splitmix64((model << 56) | (hyp << 8) | d))
        d += 1
        c = ((z >> 32) * m) >> 32
        if c not in out:
            out.append(c)
    return out if len(out) == s else [-1] * s


def test_sampling_recipe_known_answers(ref):
    # SplitMix64 reference values (Vigna's splitmix64.c, state 0 then 0x9E3779B97F4A7C15 ...)
    assert _splitmix64(0) == 0xE220A8397B1DCDAF
    assert ref.gfr_splitmix64(0) == 0xE220A8397B1DCDAF and ref.gfr_splitmix64(1) == _splitmix64(1)
    # the index recipe, restated a third time here
    for seed, model, m in ((0, 0, 9), (1234, 1, 1000), (0xDEADBEEFCAFEF00D, 0, 20000), (7, 1, 9)):
        got = ref_samples(ref, seed, model, m, 0, 50)
        want = np.array([_draws(seed, model, h, m, 8 if model else 4) for h in range(50)])
        assert np.array_equal(got, want)
        assert ((got >= 0) & (got < m)).all()
        assert all(len(set(r)) == len(r) for r in got.tolist())
    # fixed values: a change of the recipe shows here
    assert ref_samples(ref, 1, 0, 1000, 0, 1).tolist() == [_draws(1, 0, 0, 1000, 4)]
    assert _draws(1, 0, 0, 1000, 4) == [ref.gfr_draw(1, 0, 0, d, 1000) for d in range(4)]


def test_adaptive_count_and_log(ref):
    for x in (0.005, 0.01, 0.3, 0.5, 0.7071, 0.9, 0.999999):
        assert abs(ref.gfr_log(x) - np.log(x)) <= 4e-16 * abs(np.log(x)) + 1e-300
    # ceil(log(1 - conf) / log(1 - w^s)) as OpenCV's RANSACUpdateNumIters
    assert ref.gfr_adaptive(500, 1000, 4, 0.995) == int(np.ceil(np.log(0.005) / np.log(1 - 0.5 ** 4)))
    assert ref.gfr_adaptive(1000, 1000, 8, 0.99) == 1
    assert ref.gfr_adaptive(0, 1000, 8, 0.99) == 0


def test_status_false_points_take_no_part(ref):
    g = _scene(5, 600, True, 0.2, 0.2)
    st = (np.random.default_rng(5).random(600) < 0.7).astype(np.uint8)
    r = ref_fit(ref, params(seed=5), g["pts1"], g["pts2"], st)
    assert r["m"] == int(st.sum())
    assert not r["mask_H"][st == 0].any() and not r["mask_F"][st == 0].any()
    keep = st.astype(bool)
    c = ref_fit(ref, params(seed=5), g["pts1"][keep], g["pts2"][keep])
    assert c["models"].tobytes() == r["models"].tobytes() and np.array_equal(c["info"], r["info"])
    assert np.array_equal(c["mask_H"], r["mask_H"][keep]) and np.array_equal(c["mask_F"], r["mask_F"][keep])


@pytest.mark.parametrize("n", [0, 1, 8])
def test_eight_or_fewer_points_fit_nothing(ref, n):
    g = _scene(6, 20, False, 0.0, 0.0)
    r = ref_fit(ref, params(), g["pts1"][:n], g["pts2"][:n])
    for k in ("H", "F"):
        assert r[k] == dict(status=0, best=-1, best_count=0, refit_count=0, valid=0, adaptive=0)
    assert not r["models"].any() and (r["hyp_counts"] == -1).all()
    # status-true points count, not the array length
    st = np.zeros(20, np.uint8)
    st[:8] = 1
    assert ref_fit(ref, params(), g["pts1"], g["pts2"], st)["info"][0] == 0


def test_collinear_or_identical_input_gives_no_model(ref):
    p1, p2 = collinear_case()
    r = ref_fit(ref, params(), p1, p2)
    assert r["H"]["status"] == 0 and r["F"]["status"] == 0 and not r["models"].any()
    assert r["H"]["valid"] == 0   # every 4-point sample is collinear
    same = np.tile(np.float32([[100.0, 200.0]]), (50, 1))
    r = ref_fit(ref, params(), same, same + np.float32(1))
    assert r["info"][0] == 0 and r["info"][6] == 0 and r["H"]["valid"] == 0 and r["F"]["valid"] == 0


def test_fit_params_default_and_layout(built):
    import ctypes as C

    from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi
    p = capi.fit_params_default()
    assert (p.seed, p.iters_H, p.iters_F, p.thresh_H, p.thresh_F, p.conf_H, p.conf_F) == (0, 2000, 1000, 3.0, 3.0,
                                                                                           0.995, 0.99)
    assert C.sizeof(capi.FitParams) == 48 and capi.fit_params_default(seed=7, iters_F=10).iters_F == 10
    with pytest.raises(TypeError):
        capi.fit_params_default(iters=5)
