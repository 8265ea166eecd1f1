"""GPU tests of the synchronous host-buffer entry points as the C ABI states them, called through ctypes without the
capi.Context wrappers (which pass every optional output and arrays longer than needed).  Every output is an array of
exactly the documented length followed by guard bytes: the guards stay intact, the payload is what the wrapper returns
for the same inputs, an optional array may be NULL without a change to the others, n = 0 touches no per-feature byte, and
a call the device form refuses after its inputs were queued leaves the context usable."""
import ctypes as C

import numpy as np
import pytest

import detect_ref_util as du
import lk_ref_util as lu
import orb_ref_util as ou
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, synth

pytestmark = pytest.mark.gpu
GUARD, FILL = 64, 0x5A
COUNTS = (0, 1, 65)
F32, I32, U8, F64 = np.float32, np.int32, np.uint8, np.float64


class Buf:
    """An array of exactly `shape` elements followed by GUARD bytes of FILL; `init`: the payload (an in/out array), FILL
    otherwise."""

    def __init__(self, dtype, shape, init=None):
        self.dtype, self.shape = np.dtype(dtype), tuple(int(s) for s in np.atleast_1d(shape))
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.raw = np.full(self.nbytes + GUARD, FILL, U8)
        if init is not None:
            self.raw[:self.nbytes] = np.ascontiguousarray(init, self.dtype).reshape(-1).view(U8)
        self.first = self.raw.copy()

    @property
    def ptr(self):
        return self.raw.ctypes.data

    def payload(self):
        return self.raw[:self.nbytes].view(self.dtype).reshape(self.shape)

    def guard_ok(self):
        return bool((self.raw[self.nbytes:] == FILL).all())

    def untouched(self):
        return self.raw.tobytes() == self.first.tobytes()


def _run(call, spec, null=()):
    """spec: name -> (dtype, shape[, initial payload]).  -> (return code, name -> Buf); the names in `null` are passed as NULL."""
    bufs = {k: Buf(*v) for k, v in spec.items()}
    rc = call({k: (None if k in null else b.ptr) for k, b in bufs.items()})
    return rc, bufs


def _check(call, spec, want, optional=(), rc_want=0, untouched=()):
    """The exact-size call against `want` (name -> the wrapper's array), then every optional output NULL in turn and all
    at once.  `untouched`: outputs the call must not write at all."""
    rc, bufs = _run(call, spec)
    assert rc == rc_want
    for k, b in bufs.items():
        assert b.guard_ok(), f"{k}: written beyond its documented length"
        if k in untouched:
            assert b.untouched(), f"{k}: written"
        else:
            assert b.payload().tobytes() == np.ascontiguousarray(want[k], b.dtype).tobytes(), k
    for null in [(k,) for k in optional] + ([tuple(optional)] if len(optional) > 1 else []):
        rc2, bufs2 = _run(call, spec, null)
        assert rc2 == rc_want, null
        for k, b in bufs2.items():
            if k in null:
                assert b.untouched()
            else:
                assert b.raw.tobytes() == bufs[k].raw.tobytes(), (null, k)
    return bufs


def _fptr(addr):
    return None if addr is None else C.cast(addr, C.POINTER(C.c_float))


def _rc_of(fn):
    """The wrapper's result and the code it ended with (a PagkError's code, else 0)."""
    try:
        return fn(), 0
    except capi.PagkError as e:
        return None, e.code


@pytest.fixture(scope="module")
def tex():
    return ou.images(synth)["97x80 texture"]


@pytest.fixture(scope="module")
def pattern():
    return ou.seeded_pattern()


# ---- detectors -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_corners", COUNTS)
@pytest.mark.parametrize("masked", [False, True])
def test_detect_corners(ctx, tex, max_corners, masked):
    mask = du.holes_mask(97, 80, 12) if masked else None
    det = capi.detect_params_default(min_distance=5.0)
    want = ctx.detect_corners(tex, mask, max_corners, det)
    iv = capi.image_view(tex)
    call = lambda p: ctx.lib.pagk_detect_corners(ctx.h, C.byref(det), C.byref(iv), capi._ptr(mask), max_corners, p["corners"],
                                                 p["info"])
    spec = dict(corners=(F32, (max_corners, 2)), info=(I32, capi.DETECT_INFO_WORDS))
    want = dict(corners=want["buffer"][:max_corners], info=want["info"])
    _check(call, spec, want, optional=("info",), untouched=("corners",) if max_corners == 0 else ())
    if max_corners:
        assert want["info"][0] >= 1


@pytest.mark.parametrize("n_features", COUNTS[1:])
@pytest.mark.parametrize("masked", [False, True])
def test_detect_fast(ctx, n_features, masked):
    img = du.noise_image(62, 62, 3)   # the "62x62 noise" case of fast_ref_util.cases
    mask = du.holes_mask(62, 62, 6) if masked else None
    want = ctx.detect_fast(img, mask, n_features)
    cap = capi.detect_fast_bounds(62, 62, n_features)[1]
    fp, iv = capi.fast_params_default(n_features=n_features), capi.image_view(img)
    call = lambda p: ctx.lib.pagk_detect_fast(ctx.h, C.byref(fp), C.byref(iv), capi._ptr(mask), cap, p["keypoints"], p["response"],
                                              p["info"])
    spec = dict(keypoints=(F32, (cap, 2)), response=(F32, cap), info=(I32, capi.DETECT_INFO_WORDS))
    _check(call, spec, dict(keypoints=want["buffer"], response=want["response_buffer"], info=want["info"]),
           optional=("response", "info"))
    assert want["info"][0] >= 1


# ---- hand-overs ------------------------------------------------------------------------------------------------------------
HANDOVER_SIZES = [(1, 0), (1, 1), (65, 65), (65, 40)]   # (cap, target_n)


def _handover_inputs(cap, w, h):
    """status / pt_predict / pt_predict_un of cap features (two thirds alive), a state with reach_flag set."""
    rng = np.random.default_rng(17 + cap)
    st = (rng.random(cap) < 0.66).astype(U8)
    un = np.column_stack([rng.uniform(0, w, cap), rng.uniform(0, h, cap)]).astype(F32)
    pp = (un + F32([0.25, -0.5])).astype(F32)
    state = np.zeros(capi.HANDOVER_STATE_WORDS, I32)
    state[1] = 1
    return st, pp, un, state


def _handover_spec(cap, w, h, state, info):
    spec = dict(keys=(F32, (cap, 2)), keys_un=(F32, (cap, 2)), keys_normal=(F32, (cap, 2)), index_in_last=(I32, cap),
                live=(U8, cap), mask=(U8, (h, w)), state=(I32, capi.HANDOVER_STATE_WORDS, state))
    if info:
        spec["info"] = (I32, capi.DETECT_INFO_WORDS)
    return spec


@pytest.mark.parametrize("cap,target_n", HANDOVER_SIZES)
@pytest.mark.parametrize("n_cand", COUNTS)
def test_frame_handover(ctx, cap, target_n, n_cand):
    w, h = 97, 80
    p = capi.make_params(camera=synth.generic_camera(w, h))
    st, pp, un, state = _handover_inputs(cap, w, h)
    cand = lu.interior_points(w, h, n_cand, 2, 5)
    want = ctx.frame_handover(p, w, h, cap, target_n, 60.0, st, pp, un, cand, state=state)
    ncand, cbuf = np.array([n_cand], I32), np.ascontiguousarray(cand)
    call = lambda q: ctx.lib.pagk_frame_handover(ctx.h, C.byref(p), w, h, cap, target_n, 60.0, st.ctypes.data, pp.ctypes.data,
                                                 un.ctypes.data, n_cand, ncand.ctypes.data, cbuf.ctypes.data if n_cand else None,
                                                 q["keys"], q["keys_un"], q["keys_normal"], q["index_in_last"], q["live"],
                                                 q["mask"], q["state"])
    _check(call, _handover_spec(cap, w, h, state, False), want, optional=("keys_normal", "mask"))


@pytest.mark.parametrize("cap,target_n", HANDOVER_SIZES)
@pytest.mark.parametrize("detector", ["harris", "fast"])
def test_frame_handover_with_detector(ctx, tex, cap, target_n, detector):
    h, w = tex.shape
    p = capi.make_params(camera=synth.generic_camera(w, h))
    st, pp, un, state = _handover_inputs(cap, w, h)
    iv = capi.image_view(tex)
    if detector == "harris":
        dp = capi.detect_params_default(min_distance=5.0)
        want = ctx.frame_handover_detect(p, tex, cap, target_n, 60.0, st, pp, un, dp, state=state)
        fn = ctx.lib.pagk_frame_handover_detect
    else:
        dp = capi.fast_params_default()
        want, rc_want = _rc_of(lambda: ctx.frame_handover_fast(p, tex, cap, target_n, 60.0, st, pp, un, dp, state=state))
        fn = ctx.lib.pagk_frame_handover_fast
        if want is None:   # (no target and no n_features: refused before anything is queued)
            assert target_n == 0 and rc_want == capi.PAGK_E_ARG
    call = lambda q: fn(ctx.h, C.byref(p), w, h, cap, target_n, 60.0, st.ctypes.data, pp.ctypes.data, un.ctypes.data,
                        C.byref(dp), C.byref(iv), q["keys"], q["keys_un"], q["keys_normal"], q["index_in_last"], q["live"],
                        q["mask"], q["state"], q["info"])
    spec = _handover_spec(cap, w, h, state, True)
    if want is None:
        _check(call, spec, {}, rc_want=capi.PAGK_E_ARG, untouched=tuple(spec))
    else:
        _check(call, spec, want, optional=("keys_normal", "mask", "info"))
        if target_n == 65:
            assert want["state"][3] > 0   # some detected points were added


# ---- ORB -------------------------------------------------------------------------------------------------------------------
def _describe_call(c, orb, img, kp):
    iv, n = capi.image_view(img), int(kp.shape[0])
    return lambda p: c.lib.pagk_orb_describe(c.h, C.byref(orb), C.byref(iv), n, kp.ctypes.data if n else None, p["angle"], p["desc"],
                                             p["info"])


@pytest.mark.parametrize("n", COUNTS)
def test_orb_describe(ctx, tex, pattern, n):
    ctx.orb_set_pattern(pattern)
    orb, kp = capi.orb_params_default(), np.ascontiguousarray(ou.many_keypoints(97, 80, 65)[:n])
    want = ctx.orb_describe(tex, kp, orb)
    spec = dict(angle=(F32, n), desc=(U8, (n, 32)), info=(I32, capi.ORB_INFO_WORDS))
    _check(_describe_call(ctx, orb, tex, kp), spec, want, optional=("angle", "info"), untouched=("angle", "desc") if n == 0 else ())
    assert want["info"][0] + want["info"][1] == n


def test_orb_describe_refused_after_inputs_were_queued(ctx, tex, pattern):
    """Without a pattern the device form refuses when the count has already been queued for upload from the entry point's
    own frame: the call returns PAGK_E_ARG with nothing written, and the context serves the next call as usual."""
    ctx.orb_set_pattern(pattern)
    orb, kp = capi.orb_params_default(), np.ascontiguousarray(ou.many_keypoints(97, 80, 65))
    want = ctx.orb_describe(tex, kp, orb)
    fresh = capi.Context(0)
    try:
        spec = dict(angle=(F32, 65), desc=(U8, (65, 32)), info=(I32, capi.ORB_INFO_WORDS))
        call = _describe_call(fresh, orb, tex, kp)
        _check(call, spec, {}, rc_want=capi.PAGK_E_ARG, untouched=tuple(spec))
        fresh.orb_set_pattern(pattern)
        _check(call, spec, want)
    finally:
        fresh.close()


@pytest.mark.parametrize("nq,nt", [(0, 0), (0, 65), (65, 0), (1, 1), (1, 65), (65, 1), (65, 65)])
def test_orb_match(ctx, nq, nt):
    orb = capi.orb_params_default()
    dq, dt = ou.random_descriptors(65, 1)[:nq], ou.random_descriptors(65, 2)[:nt].copy()
    for k in range(0, min(nq, nt), 2):
        dt[k] = ou.flip_bits(dq[k], 3 + k % 40, k)   # near rows: matches above and below the distance filter
    dq, dt = np.ascontiguousarray(dq), np.ascontiguousarray(dt)
    want = ctx.orb_match(dq, dt, orb)
    call = lambda p: ctx.lib.pagk_orb_match(ctx.h, C.byref(orb), nq, dq.ctypes.data if nq else None, nt,
                                            dt.ctypes.data if nt else None, p["train_idx"], p["distance"], p["keep"], p["info"])
    spec = dict(train_idx=(I32, nq), distance=(I32, nq), keep=(U8, nq), info=(I32, capi.ORB_INFO_WORDS))
    _check(call, spec, want, optional=("info",), untouched=("train_idx", "distance", "keep") if nq == 0 else ())


# ---- Lucas-Kanade ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
def test_lk_track(ctx, n):
    case = lu.shapes(synth)["40x24 h10: level 0 only"]
    ref, cur = case["ref"], case["cur"]
    pts = np.ascontiguousarray(lu.interior_points(40, 24, 65, 6, 9)[:n])
    lk = capi.lk_params_default(**case["p"])
    want = ctx.lk_track(ref, cur, pts, lk)
    ir, ic = capi.image_view(ref), capi.image_view(cur)
    call = lambda p: ctx.lib.pagk_lk_track(ctx.h, C.byref(lk), C.byref(ir), C.byref(ic), n, pts.ctypes.data if n else None,
                                           p["pt_out"], p["status"], p["status_raw"], p["err"], p["flow"], p["info"])
    spec = dict(pt_out=(F32, (n, 2)), status=(U8, n), status_raw=(U8, n), err=(F32, n), flow=(F32, (n, 2)),
                info=(I32, capi.LK_INFO_WORDS))
    _check(call, spec, want, optional=("status_raw", "flow", "info"),
           untouched=("pt_out", "status", "status_raw", "err", "flow") if n == 0 else ())
    assert want["info"][0] == n


# ---- geometry --------------------------------------------------------------------------------------------------------------
def _correspondences(n):
    """n points under a homography plus noise; every fifth one an outlier."""
    rng = np.random.default_rng(41)
    p1 = np.column_stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)])
    Hm = np.array([[1.01, 0.02, 3.0], [-0.015, 0.99, -2.0], [1e-5, -2e-5, 1.0]])
    q = np.column_stack([p1, np.ones(n)]) @ Hm.T
    p2 = q[:, :2] / q[:, 2:] + rng.normal(0, 0.3, (n, 2))
    p2[::5] += rng.uniform(-40, 40, p2[::5].shape)
    return np.ascontiguousarray(p1, F32), np.ascontiguousarray(p2, F32), Hm


@pytest.mark.parametrize("n", COUNTS)
def test_geometry_scores(ctx, n):
    p1, p2, Hm = _correspondences(n)
    H21, H12 = np.ascontiguousarray(Hm), np.ascontiguousarray(np.linalg.inv(Hm))
    F21 = np.ascontiguousarray([[0, -1e-4, 0.01], [1e-4, 0, -0.02], [-0.01, 0.02, 0.3]], F64)
    inH, inF, sH, sF = ctx.geometry_scores(H21, H12, F21, p1, p2, 1.0)
    call = lambda p: ctx.lib.pagk_geometry_scores(ctx.h, H21.ctypes.data, H12.ctypes.data, F21.ctypes.data, n, capi._ptr(p1),
                                                  capi._ptr(p2), 1.0, p["inliers_H"], p["inliers_F"], _fptr(p["score_H"]),
                                                  _fptr(p["score_F"]))
    spec = dict(inliers_H=(U8, n), inliers_F=(U8, n), score_H=(F32, 1), score_F=(F32, 1))
    _check(call, spec, dict(inliers_H=inH, inliers_F=inF, score_H=[sH], score_F=[sF]),
           untouched=("inliers_H", "inliers_F") if n == 0 else ())


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("with_status", [False, True])
def test_geometry_fit(ctx, n, with_status):
    p1, p2, _ = _correspondences(n)
    st = (np.arange(n) % 7 != 3).astype(U8) if with_status else None
    fp = capi.fit_params_default(seed=7, iters_H=96, iters_F=48)
    want = ctx.geometry_fit(p1, p2, st, fp, hyp_counts=True)
    call = lambda p: ctx.lib.pagk_geometry_fit(ctx.h, C.byref(fp), n, capi._ptr(p1), capi._ptr(p2), capi._ptr(st), p["models"],
                                               p["mask_H"], p["mask_F"], p["info"], p["hyp_counts"])
    spec = dict(models=(F64, 27), mask_H=(U8, n), mask_F=(U8, n), info=(I32, capi.FIT_INFO_WORDS), hyp_counts=(I32, 96 + 48))
    _check(call, spec, want, optional=("mask_H", "mask_F", "hyp_counts"), untouched=("mask_H", "mask_F") if n == 0 else ())
    if n == 65:
        assert want["H"]["best_count"] >= 30


@pytest.mark.parametrize("n", COUNTS)
def test_geometry_validation_fit(ctx, n):
    p1, p2, _ = _correspondences(n)
    st = (np.arange(n) % 7 != 3).astype(U8)
    fp = capi.fit_params_default(seed=7, iters_H=96, iters_F=48)
    cnt, st_out, score = ctx.geometry_validation_fit(p1, p2, st, 1.0, fp)
    call = lambda p: ctx.lib.pagk_geometry_validation_fit(ctx.h, C.byref(fp), n, capi._ptr(p1), capi._ptr(p2), p["status"], 1.0,
                                                          _fptr(p["track_score"]))
    spec = dict(status=(U8, n, st), track_score=(F32, 1))
    _check(call, spec, dict(status=st_out, track_score=[score]), optional=("track_score",), rc_want=cnt,
           untouched=("status",) if n == 0 else ())
    if n == 65:
        assert 8 < cnt < int(st.sum())


# ---- neighbours ------------------------------------------------------------------------------------------------------------
def _neighbour_inputs(n, m=65):
    w, h = 97, 80
    ref, cur = lu.texture_pair(synth, w, h, 31, (0.7, -0.4))
    kr = lu.interior_points(w, h, n, 8, 3)
    pu = (kr + F32([0.7, -0.4])).astype(F32)
    kc = np.concatenate([pu[:m // 2] + F32([1.5, 0.5]), lu.interior_points(w, h, m - min(n, m // 2), 8, 4)]).astype(F32)
    st = (np.arange(n) % 5 != 2).astype(U8)
    aff = np.tile(F32([1.02, 0.01, -0.01, 0.98]), (n, 1))
    return ref, cur, np.ascontiguousarray(kr), pu, np.ascontiguousarray(kc), st, np.ascontiguousarray(aff)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("with_affine", [False, True])
def test_find_near_neighbors(ctx, n, with_affine):
    ref, cur, kr, pu, kc, st, aff = _neighbour_inputs(n)
    aff, cap, m = (aff if with_affine else None), 16, int(kc.shape[0])
    want = ctx.find_near_neighbors(ref, cur, 5, kr, pu, st, aff, kc, kc, level=1, cap=cap)
    ir, ic = capi.image_view(ref), capi.image_view(cur)
    call = lambda p: ctx.lib.pagk_find_near_neighbors(ctx.h, C.byref(ir), C.byref(ic), 5, n, capi._ptr(kr), capi._ptr(pu),
                                                      capi._ptr(st), capi._ptr(aff), m, capi._ptr(kc), capi._ptr(kc), 1, 10.0, 1,
                                                      cap, p["count"], p["idx"], p["dist"], p["ncc"])
    # in/out like the wrapper's: the lists of skipped features keep the caller's content
    spec = dict(count=(I32, n, np.zeros(n, I32)), idx=(I32, (n, cap), np.full((n, cap), -1, I32)),
                dist=(F32, (n, cap), np.zeros((n, cap), F32)), ncc=(F32, (n, cap), np.zeros((n, cap), F32)))
    _check(call, spec, want, rc_want=want["rc"], untouched=tuple(spec) if n == 0 else ())
    if n == 65:
        assert want["rc"] == 0 and want["count"].max() >= 1


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("with_affine", [False, True])
def test_ncc_free(ctx, n, with_affine):
    ref, cur, kr, pu, _, _, aff = _neighbour_inputs(n)
    aff = aff if with_affine else None
    want = ctx.ncc_free(ref, cur, 5, kr, pu, aff)
    ir, ic = capi.image_view(ref), capi.image_view(cur)
    call = lambda p: ctx.lib.pagk_ncc_free(ctx.h, C.byref(ir), C.byref(ic), 5, n, capi._ptr(kr), capi._ptr(pu), capi._ptr(aff),
                                           p["ncc"])
    _check(call, dict(ncc=(F32, n)), dict(ncc=want), untouched=("ncc",) if n == 0 else ())


# ---- selftests -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
def test_selftest_divide(ctx, n):
    rng = np.random.default_rng(2)
    num, den = rng.uniform(0.1, 1e6, n), rng.uniform(0.1, 1e3, n)
    want = dict(zip(("q_plain", "q_prepared", "root", "root_lean"), ctx.selftest_divide(num, den)))
    call = lambda p: ctx.lib.pagk_selftest_divide(ctx.h, n, capi._ptr(num), capi._ptr(den), p["q_plain"], p["q_prepared"], p["root"],
                                                  p["root_lean"])
    spec = {k: (F64, n) for k in want}
    _check(call, spec, want, untouched=tuple(spec) if n == 0 else ())


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("model", [0, 1])
def test_selftest_fit_samples(ctx, count, model):
    want = ctx.selftest_fit_samples(11, model, 40, 3, count)
    call = lambda p: ctx.lib.pagk_selftest_fit_samples(ctx.h, 11, model, 40, 3, count, p["idx"])
    _check(call, dict(idx=(I32, (count, 8 if model else 4))), dict(idx=want), untouched=("idx",) if count == 0 else ())


@pytest.mark.parametrize("n", COUNTS)
def test_selftest_repeat_sum(ctx, n):
    c = np.random.default_rng(3).uniform(-255, 255, n).astype(F32)
    closed, loop = ctx.selftest_repeat_sum(c, 441)
    call = lambda p: ctx.lib.pagk_selftest_repeat_sum(ctx.h, n, capi._ptr(c), 441, p["closed"], p["loop"])
    spec = dict(closed=(F64, n), loop=(F64, n))
    _check(call, spec, dict(closed=closed, loop=loop), untouched=tuple(spec) if n == 0 else ())


@pytest.mark.parametrize("n", COUNTS)
def test_selftest_solve(ctx, n):
    rng = np.random.default_rng(4)
    A = rng.normal(size=(n, 4, 4))
    Hs = np.ascontiguousarray(A @ A.transpose(0, 2, 1) + 4 * np.eye(4))
    b = np.ascontiguousarray(rng.normal(size=(n, 4)))
    names = ("x_serial", "norm_serial", "x_lanes", "nsq_lanes")
    want = dict(zip(names, ctx.selftest_solve(Hs, b)))
    call = lambda p: ctx.lib.pagk_selftest_solve(ctx.h, n, capi._ptr(Hs), capi._ptr(b), 0, *(p[k] for k in names))
    spec = dict(x_serial=(F64, (n, 4)), norm_serial=(F64, n), x_lanes=(F64, (n, 4)), nsq_lanes=(F64, n))
    _check(call, spec, want, untouched=names if n == 0 else ())


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_selftest_sample(ctx, tex, n, mode):
    ctx.frame_upload(0, tex, 2)
    xy = np.ascontiguousarray(lu.interior_points(48, 40, n, 3, 6))   # inside level 1 (48 x 40), clear of its border
    want = ctx.selftest_sample(0, 1, mode, xy)
    call = lambda p: ctx.lib.pagk_selftest_sample(ctx.h, 0, 1, mode, n, capi._ptr(xy), p["out"])
    _check(call, dict(out=(F32, (n, 5) if mode >= 2 else n)), dict(out=want), untouched=("out",) if n == 0 else ())
