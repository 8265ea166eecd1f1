"""GPU tests of the two-view pose (include/pagk.h "Two-view pose"): pagk_pose_2d2d bit for bit against the plain-C
restatement (tests/pose_ref.c) over sizes, budgets, status masks and scene kinds; the sampler's model id 2; the H and F
halves against pagk_geometry_fit; degenerate inputs; determinism; pagk_pose_from_matches_device behind the detector, the
descriptors and the matcher, captured once and replayed on a second pair; the ground-truth bounds of the CPU file."""
import numpy as np
import pytest
import torch

import pose_ref_util as pu
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, host_api, synth
from util import make_geometry_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL_FIT = dict(iters_H=32, iters_F=32)   # the H and F of these calls are not what is under test: a small budget


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return pu.build_ref(tmp_path_factory.mktemp("poseref"))


def _scene(seed, n, planar=False, noise=0.3, outliers=0.25):
    return make_geometry_case(seed, max(n, 1), outlier_fraction=outliers, noise_px=noise, planar=planar, translation=pu.WIDE)


def _pp(seed, fit=None, **kw):
    return capi.pose_params_default(seed=seed, fit=capi.fit_params_default(seed=seed, **(fit or {})), **kw)


def _same(got, want):
    assert got["pose"].tobytes() == want["pose"].tobytes()
    assert np.array_equal(got["pose_info"], want["pose_info"])
    assert np.array_equal(got["mask_E"], want["mask_E"]) and np.array_equal(got["mask_pose"], want["mask_pose"])
    if want.get("cand_counts") is not None:
        assert np.array_equal(got["cand_counts"], want["cand_counts"])


def _run(ctx, pts1, pts2, st, p, **kw):
    return ctx.pose_2d2d(pts1, pts2, pu.F, pu.CX, pu.CY, st, p, cand_counts=True, **kw)


@pytest.mark.parametrize("n", [0, 4, 5, 6, 9, 63, 64, 65, 257, 1000])
@pytest.mark.parametrize("planar", [False, True])
def test_bit_identical_to_restatement(built, ctx, ref, n, planar):
    g = _scene(700 + n, n, planar)
    p1, p2 = g["pts1"][:n], g["pts2"][:n]
    for iters_E in (1, 17, 64):    # a lone hypothesis, a partial workgroup, full ones
        for seed, with_status in ((11, False), (0xC0FFEE, True)):
            st = None
            if with_status:
                st = (np.random.default_rng(seed + n).random(n) < 0.85).astype(np.uint8)
                st[:5] = 1
            want = pu.ref_pose(ref, pu.params(seed=seed, iters_E=iters_E), p1, p2, st, cand_counts=True)
            got = _run(ctx, p1, p2, st, _pp(seed, SMALL_FIT, iters_E=iters_E))
            _same(got, want)
            if n >= 63 and iters_E == 64 and not with_status:
                assert got["info"]["status"] == 1
    ctx.check_launch()


def test_defaults_and_the_h_and_f_halves(built, ctx, ref):
    # once at the defaults with n = 1000; the H and F of the call are pagk_geometry_fit's on the same input, byte for byte
    for seed, planar in ((41, False), (42, True)):
        g = _scene(seed, 1000, planar)
        st = (np.random.default_rng(seed).random(1000) < 0.95).astype(np.uint8)
        p = _pp(seed)
        got = _run(ctx, g["pts1"], g["pts2"], st, p)
        _same(got, pu.ref_pose(ref, pu.params(seed=seed), g["pts1"], g["pts2"], st, cand_counts=True))
        fit = ctx.geometry_fit(g["pts1"], g["pts2"], st, p.fit)
        assert got["models"].tobytes() == fit["models"].tobytes() and np.array_equal(got["fit_info"], fit["info"])
        assert np.array_equal(got["mask_H"], fit["mask_H"]) and np.array_equal(got["mask_F"], fit["mask_F"])
        assert got["info"]["status"] == 1 and fit["info"][0] == 1
    # the "more than 8 points" rule is the fit's, the five of E are its own: six points have an E and neither H nor F
    g = _scene(43, 6, False, 0.0, 0.0)
    got = _run(ctx, g["pts1"], g["pts2"], None, _pp(1, iters_E=32))
    fit = ctx.geometry_fit(g["pts1"], g["pts2"], None, capi.fit_params_default(seed=1))
    assert got["info"]["status"] == 1 and got["fit_info"].tolist() == fit["info"].tolist() == [0, -1, 0, 0, 0, 0] * 2
    assert not got["models"].any()


def test_fit_samples_of_model_2(built, ctx, ref):
    for seed, m in ((1, 1000), (0xC0FFEE, 7), (9, 5), (9, 4)):
        assert np.array_equal(ctx.selftest_fit_samples(seed, 2, m, 0, 64), pu.ref_samples(ref, seed, m, 0, 64))
        assert np.array_equal(ctx.selftest_fit_samples(seed, 2, m, 900, 17), pu.ref_samples(ref, seed, m, 900, 17))
    assert capi.load().pagk_selftest_fit_samples(ctx.h, 1, 3, 10, 0, 1, np.zeros(8, np.int32).ctypes.data) == capi.PAGK_E_ARG


@pytest.mark.parametrize("name", ["all_equal", "collinear", "pure_rotation", "nan_coordinate"])
def test_degenerate_inputs(built, ctx, ref, name):
    p1, p2 = pu.degenerate_cases()[name]
    got = _run(ctx, p1, p2, None, _pp(3, SMALL_FIT, iters_E=64))
    _same(got, pu.ref_pose(ref, pu.params(seed=3, iters_E=64), p1, p2, cand_counts=True))
    assert np.isfinite(got["pose"]).all()
    if got["info"]["status"] == 0:
        assert not got["pose"].any() and not got["mask_E"].any() and not got["mask_pose"].any()
    # a tie between the four poses goes to the first: no depth is below 1e-9
    got = _run(ctx, p1, p2, None, _pp(3, SMALL_FIT, iters_E=64, max_depth=1e-9))
    _same(got, pu.ref_pose(ref, pu.params(seed=3, iters_E=64, max_depth=1e-9), p1, p2, cand_counts=True))
    assert got["pose_info"][8:13].tolist() == [0] * 5
    ctx.check_launch()


def test_bad_arguments(built, ctx):
    g = _scene(51, 40)
    for kw in (dict(iters_E=0), dict(thresh_E=0.0), dict(conf_E=1.0), dict(max_depth=float("nan")),
               dict(fit=capi.fit_params_default(iters_F=0))):
        with pytest.raises(capi.PagkError):
            ctx.pose_2d2d(g["pts1"], g["pts2"], pu.F, pu.CX, pu.CY, None, capi.pose_params_default(**kw))
    for f, cx in ((0.0, 1.0), (-1.0, 1.0), (float("nan"), 1.0), (1.0, float("inf"))):
        with pytest.raises(capi.PagkError):
            ctx.pose_2d2d(g["pts1"], g["pts2"], f, cx, 0.0)
    lib, p, z = capi.load(), capi.pose_params_default(), None
    assert lib.pagk_pose_2d2d(ctx.h, p, 1.0, 0.0, 0.0, -1, z, z, z, z, z, z, z, z, z, z, z, z) == capi.PAGK_E_ARG
    assert lib.pagk_pose_2d2d_device(ctx.h, p, 1.0, 0.0, 0.0, 10, z, z, z, z, z, z, z, z, z, z, z, z) == capi.PAGK_E_ARG
    assert lib.pagk_pose_from_matches_device(ctx.h, p, 1.0, 0.0, 0.0, 0, z, z, 1, z, z, z, z, z, z, z, z, z, z, z,
                                             z) == capi.PAGK_E_ARG
    ctx.check_launch()


def test_determinism(built, ctx):
    g = _scene(31, 1000)
    p = _pp(5, SMALL_FIT, iters_E=256)
    a = _run(ctx, g["pts1"], g["pts2"], None, p)
    b = _run(ctx, g["pts1"], g["pts2"], None, p)
    c2 = capi.Context(0)
    try:
        c = _run(c2, g["pts1"], g["pts2"], None, p)
    finally:
        c2.close()
    _same(a, b)
    _same(a, c)


def test_ground_truth_on_the_device(built, ctx):
    # implied by bit-identity; asserted once so that this file stands alone
    for seed in (21, 23):
        g = _scene(seed, 1000, False, 0.0, 0.0)
        r = ctx.pose_2d2d(g["pts1"], g["pts2"], pu.F, pu.CX, pu.CY, None, _pp(seed, SMALL_FIT))
        assert r["info"]["status"] == 1 and r["info"]["best_count"] == 1000
        assert pu.rotation_angle_deg(r["R"]) <= pu.R_BOUND_DEG and pu.direction_angle_deg(r["t"]) <= pu.T_BOUND_DEG
        assert float(r["t"] @ np.asarray(pu.WIDE)) > 0
    g = _scene(22, 1000)
    r = ctx.pose_2d2d(g["pts1"], g["pts2"], pu.F, pu.CX, pu.CY, None, _pp(22, SMALL_FIT))
    true_in = pu.sampson_px(pu.true_essential(), g["pts1"], g["pts2"]) <= 1.0
    assert int((r["mask_E"].astype(bool) & true_in).sum()) >= 0.9 * int(true_in.sum())
    g = _scene(24, 1000, True, 0.0, 0.0)
    r = ctx.pose_2d2d(g["pts1"], g["pts2"], pu.F, pu.CX, pu.CY, None, _pp(24, SMALL_FIT))
    assert r["info"]["status"] == 1 and r["info"]["best_count"] == 1000
    assert r["pose_info"][9 + r["info"]["pose"]] == r["pose_info"][9:13].max()


def test_host_api_pose_estimation(built, ctx):
    g = _scene(61, 500)
    K = np.array([[pu.CAM.fx, 0, pu.CAM.cx], [0, pu.CAM.fy, pu.CAM.cy], [0, 0, 1]])
    p = _pp(7, SMALL_FIT, iters_E=128)
    got = host_api.pose_estimation_2d2d(g["pts1"], g["pts2"], K, None, p, ctx=ctx)
    want = ctx.pose_2d2d(g["pts1"], g["pts2"], pu.F, pu.CX, pu.CY, None, p)
    assert got["pose"].tobytes() == want["pose"].tobytes() and got["models"].tobytes() == want["models"].tobytes()
    assert got["info"]["status"] == 1


def test_from_matches_behind_detect_describe_match_captured_and_replayed(built, ref):
    import detect_ref_util as du
    import orb_ref_util as ou
    w, h, n_features = 160, 120, 80
    base = [du.texture_image(synth, w + 8, h + 6, s) for s in (12, 13)]
    # two pairs of 160 x 120 crops of one textured image each, a few pixels apart: the matcher finds real matches
    pairs = [(np.ascontiguousarray(b[0:h, 0:w]), np.ascontiguousarray(b[3:h + 3, 5:w + 5])) for b in base]
    cap = capi.detect_fast_bounds(w, h, n_features)[1]
    pat = ou.seeded_pattern()
    fast, orb = capi.fast_params_default(n_features=n_features), capi.orb_params_default()
    f, cx, cy = 120.0, 80.0, 60.0
    K = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]])
    p = _pp(19, SMALL_FIT, iters_E=64)
    c = capi.Context(0)
    try:
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            c.set_stream(stream.cuda_stream)
            c.orb_set_pattern(pat)
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)    # noqa: E731
            d_img = [z((h, w), torch.uint8) for _ in range(2)]
            d_k = [z((cap, 2), torch.float32) for _ in range(2)]
            d_di, d_oi = [z(8, torch.int32) for _ in range(2)], [z(8, torch.int32) for _ in range(2)]
            d_d = [z((cap, 32), torch.uint8) for _ in range(2)]
            d_idx, d_dist, d_keep, d_mi = z(cap, torch.int32), z(cap, torch.int32), z(cap, torch.uint8), z(8, torch.int32)
            d_models, d_pose = z(27, torch.float64), z(21, torch.float64)
            d_masks = [z(cap, torch.uint8) for _ in range(4)]
            d_fi, d_pi = z(capi.FIT_INFO_WORDS, torch.int32), z(capi.POSE_INFO_WORDS, torch.int32)

            def work():
                for s in range(2):
                    c.frame_set_device(s, d_img[s].data_ptr(), w, h, w, 1)
                    c.detect_fast_device(fast, s, None, cap, d_k[s], None, d_di[s])
                    c.orb_describe_device(orb, s, cap, d_k[s], d_di[s], None, d_d[s], d_oi[s])
                c.orb_match_device(orb, cap, d_d[0], d_di[0], cap, d_d[1], d_di[1], d_idx, d_dist, d_keep, d_mi)
                c.pose_from_matches_device(p, f, cx, cy, cap, d_k[0], d_di[0], cap, d_k[1], d_di[1], d_idx, d_keep, d_models,
                                           d_pose, *d_masks, d_fi, d_pi)

            def feed(pair):
                for s in range(2):
                    d_img[s].copy_(torch.from_numpy(pair[s]).to(DEV))

            def snapshot():
                stream.synchronize()
                return [t.cpu().numpy().copy() for t in [d_models, d_pose, *d_masks, d_fi, d_pi, d_idx, d_keep, *d_k, *d_di]]

            def check(snap, how):
                models, pose, mH, mF, mE, mP, fi, pi, idx, keep, k0, k1, n0, n1 = snap
                nq, nt = int(n0[0]), int(n1[0])
                st = np.zeros(cap, np.uint8)
                st[:nq] = (keep[:nq] != 0) & (idx[:nq] >= 0) & (idx[:nq] < nt)
                pts1, pts2 = np.zeros((cap, 2), np.float32), np.zeros((cap, 2), np.float32)
                pts1[:nq] = k0[:nq]
                pts2[st != 0] = k1[idx[st != 0]]
                print(f"{how}: {nq} x {nt} keypoints, {int(st.sum())} matches, pose info {pi[:13].tolist()}")
                assert int(st.sum()) >= 9, "the pair has too few matches to say anything"
                want = pu.ref_pose(ref, pu.params(seed=19, iters_E=64), pts1, pts2, st, f, cx, cy)
                assert pose.tobytes() == want["pose"].tobytes() and np.array_equal(pi, want["pose_info"])
                assert np.array_equal(mE, want["mask_E"]) and np.array_equal(mP, want["mask_pose"])
                # the host route fed with the same matches
                host = host_api.pose_estimation_2d2d(pts1, pts2, K, st, p, ctx=c)
                assert host["pose"].tobytes() == pose.tobytes() and host["models"].tobytes() == models.tobytes()
                assert np.array_equal(host["mask_H"], mH) and np.array_equal(host["mask_F"], mF)
                assert np.array_equal(host["fit_info"], fi) and np.array_equal(host["pose_info"], pi)
                assert pi[0] == 1

            direct = []
            for pair in pairs:                     # the direct calls (the first one sizes every workspace)
                feed(pair)
                work()
                direct.append(snapshot())
                check(direct[-1], "direct")
            c.graph_begin()
            try:
                with pytest.raises(capi.PagkError):   # the host-buffer form is not capturable
                    c.pose_2d2d(np.zeros((9, 2), np.float32), np.zeros((9, 2), np.float32), f, cx, cy)
                work()
            finally:
                gid = c.graph_end()
            for k in (1, 0):                       # replays on the other pair first: each equals the direct calls
                feed(pairs[k])
                c.graph_launch(gid)
                snap = snapshot()
                assert all(a.tobytes() == b.tobytes() for a, b in zip(snap, direct[k])), k
            c.graph_destroy(gid)
            c.check_launch()
            # host_api.orb_pose_pair is the same two calls on host arrays
            hp = host_api.orb_pose_pair(pairs[0][0], pairs[0][1], n_features, pat, K, fast, orb, p, ctx=c)
            assert hp["pose"]["pose"].tobytes() == direct[0][1].tobytes()
            assert hp["pose"]["models"].tobytes() == direct[0][0].tobytes()
    finally:
        c.set_stream(None)
        c.close()
