"""No result depends on what the library's own workspaces held before the call.

test_device_bounds_gpu.py guards the CALLER's arrays.  The library's own blocks -- the buffers reserve() hands out and
Layout carves anew for every call, the frame slots, the staging blocks of the host forms -- only ever grow and are reused
by every later call: the same bytes mean different things from one call to the next, and which parts a launch needs clean
is decided by hand, part by part.  A fresh allocation is normally zero and a suite that runs its cases in ascending size
leaves leftovers that are zero or happen to be right, so a missing clear or a kernel that reads a part it never wrote
passes everywhere else.  Here every row is one scenario of tests/device_plans.py on a Context of its own and runs, for a
small problem S, a second problem S' of the same sizes (another seed or image) and larger problems D (every Layout offset
moves):
  1. fresh context: pagk_selftest_fill_workspaces(1, also_new), then S -- every first allocation arrives as 0x00000001;
  2. fill 0 (also_new off), upload again, S;
  3. fill 1 (also_new on: what D allocates arrives non-zero too), upload again, S -- the buffers no longer grow;
  4. per D: D against its own restatement, then S with no fill -- a large problem's leftovers under a small one's layout;
  5. S', then S with no fill -- legal values of the same fields, of another problem.
Every check is device_plans.run_once: guards intact, outputs byte-identical to the restatement, never to another call
into the library.  The caller arrays of a row come out of ONE arena (16 MiB, every array with a guard of at least its own
size on both sides), so that even a stale index stays inside memory the test owns and shows as a damaged guard.

Only the words 0 and 1 are used, for the reason tests/arena.py gives for its integer fills: as an index, a count or a flag
both are small legal values -- a kernel that wrongly reads one computes a wrong result, not a wild address -- and they
differ as counters, flags, keys and bytes.  A float accumulator would not notice 1.4e-45: steps 4 and 5 cover those, for
the sizes run.  The host-form rows run steps 1 to 3 (they share the device forms' launches: new there are the staging
block and also_new)."""
import functools

import numpy as np
import pytest
import torch

import arena as ar
import detect_ref_util as du
import device_plans as dp
import fast_ref_util as fu
import fit_ref_util as ftu
import handover_ref_util as hu
import instantiation_cases as cases
import inverse_ref_util as iu
import lk_ref_util as lu
import pose_ref_util as pu
import sampler_cases as smp
import shape_cases as sc
from device_plans import COUNTS, DEV, F32, F64, H, U8, W
from oracle import pagk_oracle as orc
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, synth
from util import make_geometry_case, needs_variant

pytestmark = pytest.mark.gpu
BIG = 130     # the count of the larger problems


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    return dp.Refs(tmp_path_factory)


# ---- the sequence ------------------------------------------------------------------------------------------------------------
def _sequence(refs, make, S, S2, Ds, contexts=1, host=False):
    """`make(c, refs, **size) -> Plan` (c: the row's context, or the list of its `contexts` contexts)."""
    ctxs = [capi.Context(0) for _ in range(contexts)]
    c = ctxs[0] if contexts == 1 else ctxs
    arena = ar.Arena(DEV)
    count = [0]

    def fill(word, also_new=False):
        for x in ctxs:
            x.selftest_fill_workspaces(word, also_new)

    def go(size, what):
        count[0] += 1
        dp.run_once(arena, f"call{count[0]}.", make(c, refs, **size), what)
    try:
        fill(1, True)
        go(S, "step 1: fresh context, every new block filled with 1")
        fill(0)
        go(S, "step 2: workspaces filled with 0")
        fill(1, True)
        go(S, "step 3: workspaces filled with 1")
        if host:
            return
        for k, D in enumerate(Ds):
            go(D, f"step 4: larger problem {k}")
            go(S, f"step 4: the small problem on the leftovers of larger problem {k}")
        go(S2, "step 5: second problem of the same sizes")
        go(S, "step 5: the small problem on the leftovers of the second")
    finally:
        for x in ctxs:
            x.close()


def _bare(what, fn):
    """A scenario without caller arrays: `fn()` issues the call(s) and asserts on what comes back."""
    return dp.Plan(what, [], lambda v, null: fn(), {})


# ---- frame slots: pads, packed taps, the pixel past a row -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edge_workload(width, height, n, levels, seed):
    """A tracking workload whose first features sit on the last two rows and columns of every level (x / 2^l stays within two
    pixels of the level's last column for every level when it does at level 0)."""
    w = synth.make_workload(f"content-{width}x{height}-n{n}-L{levels}-s{seed:x}", width, height, max(n, 8), seed=seed, half_patch=5,
                            iterations=20, pyramids=levels, edge_fraction=0.3)
    last = np.array([(width - 1.25, height - 1.5), (width - 2.0, height * 0.5), (width * 0.5, height - 2.0), (width - 1.0, height - 1.0),
                     (width - 1.75, 3.0), (3.0, height - 1.75), (width - 2.5, height - 2.5), (width - 1.0, height * 0.25)], F32)
    w.pt_ref[:8] = last
    w.pt_init[:8] = last + F32([0.4, -0.3])
    w.status_in[:8] = 1
    for a in (w.img_ref, w.img_cur, w.pt_ref, w.pt_init, w.affine, w.status_in):
        a.setflags(write=False)
    return w


_ORACLES = {}   # by workload name: the oracle's (or, inverse, tests/inverse_ref.c's) result with the lean parameters


def _oracle(w, inverse=False):
    key = (w.name, inverse)
    if key not in _ORACLES:
        _ORACLES[key] = iu.track_workload(w, iu.shape_params(w, "lean")) if inverse else cases.run_oracle(w, "lean")
    return _ORACLES[key]


def _track_size(w, n, variant, handover=False, selector=0, inverse=False):
    return dict(w=w, n=n, variant=variant, handover=handover, selector=selector, inverse=inverse)


def _track(c, refs, w, n, variant, handover, selector, inverse):
    p, ref = (iu.shape_params(w, "lean") if inverse else cases.params(w, "lean")), _oracle(w, inverse)
    return dp.track(c, f"track_device {w.name} n={n} kernel {selector}", w, p, ref, n, variant if n else None, handover and n > 0,
                    selector)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("selector", [0, 3])
def test_frame_upload_and_track(built, refs, selector, n):
    """frame_upload + track_device with the 4-wave kernel and the one-wave kernel on the 97 x 80 frame, features on the last
    two rows and columns of every level; D: a 128 x 96 frame with one level more in the same slots, 130 features."""
    S = _track_size(_edge_workload(W, H, 65, 3, 0xC0DE), n, selector, selector=selector)
    S2 = _track_size(_edge_workload(W, H, 65, 3, 0xC0DF), n, selector, selector=selector)
    D = _track_size(_edge_workload(128, 96, BIG, 4, 0xC0E0), BIG, selector, selector=selector)
    for size in (S, S2, D):     # (the oracle's word: the features on the border run the loop, so their patches are sampled there)
        assert (_oracle(size["w"])["iters"][:8] >= 2).all(), "a border feature does not iterate"
    _sequence(refs, _track, S, S2, [D])


def _sampled(c, slot, image, levels, pad=0):
    """pagk_selftest_sample in its clamped modes on every level of a slot that holds `image`, at the coordinates of the last
    three rows and columns (and past them) and a thinned set of the others, against the oracle's sampler.  Level 0 of a frame
    that was given with rows `pad` bytes wider than the frame is sampled as such a frame (the pixel past a row is a padding
    byte, which reads as 0: oracle/README.md)."""
    for l, lvl in enumerate(dp._levels(image, levels)):
        rows, cols = lvl.shape
        if l == 0 and pad:
            wide = np.zeros((rows, cols + pad), np.uint8)
            wide[:, :cols] = lvl
            lvl = wide[:, :cols]
        xy = smp.coordinates(cols, rows)
        with np.errstate(invalid="ignore"):
            near = (xy[:, 0] >= cols - 3) | (xy[:, 1] >= rows - 3)
        xy = np.ascontiguousarray(np.concatenate([xy[near][::7], xy[~near][::53]]))
        got = c.selftest_sample(slot, l, 0, xy)
        assert np.array_equal(smp.bits(got), smp.bits(orc.sample(lvl, xy))), f"level {l}: clamped samples"
        got5 = c.selftest_sample(slot, l, 2, xy)
        want5 = orc.sample(lvl, smp.five(xy).reshape(-1, 2)).reshape(-1, 5)
        assert np.array_equal(smp.bits(got5), smp.bits(want5)), f"level {l}: the five samples of a pixel"
    c.check_launch()


def _set_and_sample(c, refs, pad, image=None, levels=3):
    """frame_set_device, then the packed taps it made (the levels themselves are downloaded by the scenario)."""
    image = dp.texture() if image is None else image
    plan = dp.frame_set_device(c, refs, pad, image, levels)
    run = plan.run

    def both(v, null):
        run(v, null)
        _sampled(c, 2, image, levels, pad)
    plan.run = both
    return plan


@pytest.mark.parametrize("pad", [0, 13])
def test_frame_set_device(built, refs, pad):
    S2 = dict(pad=pad, image=du.texture_image(synth, W, H, 21))
    _sequence(refs, _set_and_sample, dict(pad=pad), S2, [dict(pad=pad, image=dp.larger_texture(), levels=4)])


@pytest.mark.parametrize("cn,pad", [(1, 0), (3, 5)])
def test_frame_rectify_device(built, refs, cn, pad):
    """D: a larger raw frame and one level more for the same maps' size (a slot keeps the size of its first frame: the call
    refuses maps of another size, so the block grows by the level only)."""
    S = dict(pad=pad, cn=cn)
    _sequence(refs, dp.frame_rectify_device, S, dict(alt=1, **S), [dict(pad=pad, cn=cn, src=(128, 96), levels=3)])


def _sample(c, refs, image, levels):
    def fn():
        c.frame_upload(1, image, levels)
        _sampled(c, 1, image, levels)
    return _bare(f"selftest_sample {image.shape[1]} x {image.shape[0]}, {levels} levels", fn)


def test_selftest_sample(built, refs):
    S, S2 = dict(image=dp.texture(), levels=3), dict(image=du.texture_image(synth, W, H, 21), levels=3)
    _sequence(refs, _sample, S, S2, [dict(image=dp.larger_texture(), levels=4)])


# ---- QUAD_WS, LV, SUSP and the row queue ------------------------------------------------------------------------------------------
_CONT = (("PAGK_QUAD_BUDGET", "3"), ("PAGK_SUSPEND_LONE", "0"))   # test_workspaces_gpu.py, track_routes._CONT
_WHOLE = (("PAGK_QUAD_BUDGET", "0"),)


@functools.lru_cache(maxsize=None)
def _route_workload(n, levels, seed):
    w = synth.make_workload(f"content-route-n{n}-L{levels}-s{seed:x}", cases.WIDTH, cases.HEIGHT, n, seed=seed, half_patch=5,
                            iterations=cases.ITERATIONS, pyramids=levels, camera=synth.D435I, edge_fraction=0.3)
    for a in (w.img_ref, w.img_cur, w.pt_ref, w.pt_init, w.affine, w.status_in):
        a.setflags(write=False)
    return w


def _route_sizes(variant, handover):
    S = _track_size(cases.workload(5), 65, variant, handover, variant)
    S2 = _track_size(_route_workload(cases.N, 3, 0x2B1), 65, variant, handover, variant)
    D = _track_size(_route_workload(BIG, 4, 0x2B2), BIG, variant, handover, variant)
    return S, S2, D


def _late(w, n):
    ref = _oracle(w)
    live = w.status_in[:n] > 0
    return int((ref["iters"][:n][live] > cases.BUDGET).sum())


@pytest.mark.parametrize("variant,handover", [
    (5, False), (5, True), pytest.param(6, False, marks=[needs_variant(6)]), (7, False), (7, True)],
    ids=["quad", "quad-handover", "rows", "levels", "levels-handover"])
def test_track_routes(built, refs, monkeypatch, variant, handover):
    """Four features per wave (5), the row queue (6) and one level per wave (7), with and without the hand-over to the
    finisher after three iterations: 65 of the instantiation matrix's features on three levels; D: 130 features on four."""
    for var, value in (_CONT if handover else _WHOLE):
        monkeypatch.setenv(var, value)
    S, S2, D = _route_sizes(variant, handover)
    if handover:
        for size in (S, S2, D):
            assert _late(size["w"], size["n"]) >= 1, "no feature passes the hand-over budget"
    _sequence(refs, _track, S, S2, [D])


def test_track_template_jacobian(built, refs):
    """Variant 8 (inverse == PAGK_INVERSE_TEMPLATE) on 96 x 64 with two levels; D: 128 x 96 with three, 130 features."""
    S = _track_size(sc.workload((96, 64, 2), 5), 65, 8, inverse=True)
    S2 = _track_size(sc._workload(96, 64, 2, 5, sc.N, 0x77A1), 65, 8, inverse=True)
    D = _track_size(sc._workload(128, 96, 3, 5, BIG, 0x77A2), BIG, 8, inverse=True)
    _sequence(refs, _track, S, S2, [D])


def _fused(c, refs, w, n, seed):
    return dp.fused(c, f"track_device_fused {w.name} n={n}", w, cases.params(w, "lean"), _oracle(w), 0, seed, 13, n)


def test_track_fused(built, refs):
    S, S2, D = _route_sizes(0, False)
    _sequence(refs, _fused, dict(w=S["w"], n=65, seed=81), dict(w=S2["w"], n=65, seed=82), [dict(w=D["w"], n=BIG, seed=83)])


def _batch(ctxs, refs, ws, ns):
    return dp.batch(ctxs[:len(ws)], f"track_device_batch {[w.name for w in ws]} n={ns}", ws, cases.params(ws[0], "lean"),
                    [_oracle(w) for w in ws], 7, 7, False, ns)


def test_track_batch(built, refs):
    """pagk_track_device_batch (one level per wave): streams of 1, 65 and 30 features; D: 130 and 67 features on four levels."""
    ws = cases.batch_workloads(5)
    others = (_route_workload(1, 3, 0x2C1), _route_workload(cases.N, 3, 0x2B1), _route_workload(30, 3, 0x2C2))
    D = (_route_workload(BIG, 4, 0x2B2), _route_workload(cases.N, 4, 0x2C3))
    _sequence(refs, _batch, dict(ws=ws, ns=(1, 65, 30)), dict(ws=others, ns=(1, 65, 30)), [dict(ws=D, ns=(BIG, cases.N))], contexts=3)


# ---- DET, FAST, HAND ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_corners", COUNTS)
@pytest.mark.parametrize("masked", [False, True])
def test_detect_corners_device(built, refs, max_corners, masked):
    S = dict(max_corners=max_corners, masked=masked)
    S2 = dict(image=du.texture_image(synth, W, H, 21), alt=1, **S)
    D = dict(max_corners=BIG, masked=masked, image=dp.larger_texture(), min_distance=3.0, cap=BIG + 30)
    _sequence(refs, dp.detect_corners_device, S, S2, [D])


def _noise(width, height, seed):
    return du.noise_image(width, height, seed)


@pytest.mark.parametrize("n_features", COUNTS[1:])
@pytest.mark.parametrize("masked", [False, True])
def test_detect_fast_device(built, refs, n_features, masked):
    """S: the 97 x 80 texture; D: 128 x 96 noise (a corner in nearly every cell) with n_features = 130."""
    S = dict(n_features=n_features, masked=masked, image=dp.texture())
    S2 = dict(n_features=n_features, masked=masked, image=du.texture_image(synth, W, H, 21), alt=1)
    _sequence(refs, dp.detect_fast_device, S, S2, [dict(n_features=BIG, masked=masked, image=_noise(128, 96, 7))])


def _fast_cells(c, refs, image):
    def fn():
        got, want = c.selftest_fast_cells(image), fu.ref_cells(refs.fast, image)
        assert got["n"] == want["n"] >= 1
        assert got["xy"].tobytes() == want["xy"].tobytes() and got["score"].tobytes() == want["score"].tobytes()
        c.check_launch()
    return _bare(f"selftest_fast_cells {image.shape[1]} x {image.shape[0]}", fn)


def test_selftest_fast_cells(built, refs):
    _sequence(refs, _fast_cells, dict(image=dp.texture()), dict(image=du.texture_image(synth, W, H, 21)),
              [dict(image=_noise(128, 96, 7))])


@pytest.mark.parametrize("n_cand", COUNTS)
def test_frame_handover_device(built, refs, n_cand):
    """Every call without d_mask: the mask the hand-over works on is the context's own (HAND)."""
    S = dict(n_cand=n_cand)
    _sequence(refs, _handover_own_mask, S, dict(alt=1, **S), [dict(n_cand=BIG, cand_cap=BIG + 10, cap=96, target=86)])


def _handover_own_mask(c, refs, **size):
    """frame_handover_device with d_mask NULL: the mask the call works on is the context's own."""
    plan = dp.frame_handover_device(c, refs, **size)
    plan.arrays = [a for a in plan.arrays if a[1] != "d_mask"]
    plan.want = {k: v for k, v in plan.want.items() if k != "d_mask"}
    run = plan.run
    plan.run = lambda v, null: run(dict(v, d_mask=None), null)
    return plan


@pytest.mark.parametrize("detector", ["harris", "fast"])
def test_frame_handover_with_detector_device(built, refs, detector):
    S = dict(detector=detector)
    S2 = dict(detector=detector, image=du.texture_image(synth, W, H, 21), alt=1)
    _sequence(refs, dp.frame_handover_with_detector_device, S, S2, [dict(detector=detector, image=dp.larger_texture())])


# ---- FIT, POSE ---------------------------------------------------------------------------------------------------------------------
def _fit(n, iters_H, iters_F):
    return dict(n=n, fit=dict(seed=7, iters_H=iters_H, iters_F=iters_F))


FIT_LARGER = [_fit(64, 64, 64), _fit(16, 128, 64), _fit(16, 64, 128), _fit(64, 128, 128)]   # n alone, each budget alone, together


@pytest.mark.parametrize("with_status", [False, True])
def test_geometry_fit_device(built, refs, with_status):
    S = dict(with_status=with_status, **_fit(16, 64, 64))
    _sequence(refs, dp.geometry_fit_device, S, dict(alt=1, **S), [dict(with_status=with_status, **D) for D in FIT_LARGER])


def test_geometry_validation_device(built, refs):
    S = _fit(16, 64, 64)
    _sequence(refs, dp.geometry_validation_device, S, dict(alt=1, **S), FIT_LARGER)


POSE_LARGER = [dict(n=64, iters_E=64), dict(n=16, iters_E=128), dict(n=64, iters_E=128)]


@pytest.mark.parametrize("with_status", [False, True])
def test_pose_2d2d_device(built, refs, with_status):
    S = dict(n=16, iters_E=64, with_status=with_status)
    _sequence(refs, dp.pose_2d2d_device, S, dict(alt=1, **S), [dict(with_status=with_status, **D) for D in POSE_LARGER])


@pytest.mark.parametrize("nq", COUNTS)
def test_pose_from_matches_device(built, refs, nq):
    S = dict(nq=nq, iters_E=64)
    D = [dict(nq=BIG, nt=BIG, cap_q=BIG + 10, cap_t=BIG + 6, iters_E=64), dict(nq=nq, iters_E=128)]
    _sequence(refs, dp.pose_from_matches_device, S, dict(alt=1, **S), D)


# ---- ASSOC -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
def test_match_features_device(built, refs, n):
    _sequence(refs, dp.match_features_device, dict(n=n), dict(n=n, alt=1), [dict(n=BIG, m=BIG)])


@pytest.mark.parametrize("min_matches", [0, 100])
@pytest.mark.parametrize("n", COUNTS)
def test_search_gyro_predict_device(built, refs, n, min_matches):
    S = dict(n=n, min_matches=min_matches)
    # (with 130 features more than 100 may match: the second level of the larger problem is asked for with a bound beyond n)
    _sequence(refs, dp.search_gyro_predict_device, S, dict(alt=1, **S), [dict(n=BIG, m=BIG, min_matches=1000 if min_matches else 0)])


@pytest.mark.parametrize("n", COUNTS)
def test_search_klt_device(built, refs, n):
    _sequence(refs, dp.search_klt_device, dict(n=n), dict(n=n, alt=1), [dict(n=BIG, m=BIG, cap=BIG + 10)])


# ---- ORB_BLUR, ORB_KEYS ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
def test_orb_describe_device(built, refs, n):
    """Width 97: three padded columns in the blurred image."""
    S2 = dict(n=n, image=du.texture_image(synth, W, H, 21), alt=1)
    _sequence(refs, dp.orb_describe_device, dict(n=n), S2, [dict(n=BIG, image=dp.larger_texture(), cap=BIG + 10)])


@pytest.mark.parametrize("nq,nt", [(0, 65), (65, 0), (1, 1), (1, 65), (65, 65)])
def test_orb_match_device(built, refs, nq, nt):
    """(1, 65) after (65, 65): 64 keys of the larger call lie behind the one the small call resets."""
    S = dict(nq=nq, nt=nt)
    _sequence(refs, dp.orb_match_device, S, dict(alt=1, **S), [dict(nq=65, nt=65), dict(nq=BIG, nt=BIG, cap_q=BIG + 10, cap_t=BIG + 6)])


# ---- LK_PYR ------------------------------------------------------------------------------------------------------------------------
LK_LARGER = dict(size=(192, 128), lk=dict(half_patch=10, max_level=3))


def test_lk_pyramid_device(built, refs):
    S, D = dp.lk_pyramid_device(None, refs), dp.lk_pyramid_device(None, refs, **LK_LARGER)
    assert "2 levels" in S.what and "3 levels" in D.what, (S.what, D.what)
    _sequence(refs, dp.lk_pyramid_device, {}, dict(alt=1), [LK_LARGER])


@pytest.mark.parametrize("n", COUNTS)
def test_lk_track_device(built, refs, n):
    _sequence(refs, dp.lk_track_device, dict(n=n), dict(n=n, alt=1), [dict(n=BIG, cap=BIG + 10, **LK_LARGER)])


# ---- host scratch: FEAT, SCORE, FITIO, POSEIO, HANDIO, a Staged's own block ---------------------------------------------------------
def _same(got, want, keys, n, what):
    for k in keys:
        g, w = np.asarray(got[k])[:n], np.asarray(want[k])[:n]
        assert g.tobytes() == np.ascontiguousarray(w, g.dtype).tobytes(), f"{what}: {k} differs from the restatement"


def _host_track(c, refs, n, pyr):
    w = cases.workload(5)
    p, ref = cases.params(w, "lean"), cases.oracle(5, "lean")
    args = [np.ascontiguousarray(a[:n]) for a in (w.pt_ref, w.pt_init, w.affine, w.status_in)]

    def fn():
        if pyr:
            got = c.track_pyr(p, dp._levels(w.img_ref, w.pyramids), dp._levels(w.img_cur, w.pyramids), *args)
        else:
            got = c.track(p, w.img_ref, w.img_cur, *args)
        c.check_launch()
        _same(got, ref, dp.OUT_KEYS, n, "track_pyr" if pyr else "track")
    return _bare(f"{'track_pyr' if pyr else 'track'} n={n}", fn)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("pyr", [False, True], ids=["track", "track_pyr"])
def test_host_track(built, refs, pyr, n):
    _sequence(refs, _host_track, dict(n=n, pyr=pyr), None, [], host=True)


def _host_fit(c, refs, n):
    p1, p2, _ = dp._correspondences(n)
    st = (np.arange(n) % 7 != 3).astype(U8)
    want = ftu.ref_fit(refs.fit, ftu.params(**dp.FIT), p1, p2, st)

    def fn():
        got = c.geometry_fit(p1, p2, st, capi.fit_params_default(**dp.FIT), hyp_counts=True)
        c.check_launch()
        _same(got, want, ("models", "info", "hyp_counts"), None, "geometry_fit")
        _same(got, want, ("mask_H", "mask_F"), n, "geometry_fit")
    return _bare(f"geometry_fit n={n}", fn)


def _host_pose(c, refs, n):
    g = make_geometry_case(700, 65, outlier_fraction=0.25, noise_px=0.3, planar=False, translation=pu.WIDE)
    p1, p2 = np.ascontiguousarray(g["pts1"][:n]), np.ascontiguousarray(g["pts2"][:n])
    st = (np.arange(n) % 7 != 3).astype(U8)
    pose, fit = dp._pose_want(refs, 11, p1, p2, st)
    pp = capi.pose_params_default(seed=11, fit=capi.fit_params_default(seed=11, **dp.SMALL_FIT), iters_E=dp.ITERS_E)

    def fn():
        got = c.pose_2d2d(p1, p2, pu.F, pu.CX, pu.CY, st, pp, cand_counts=True)
        c.check_launch()
        _same(got, dict(models=fit["models"], fit_info=fit["info"], pose=pose["pose"], pose_info=pose["pose_info"],
                        cand_counts=pose["cand_counts"]), ("models", "fit_info", "pose", "pose_info", "cand_counts"), None, "pose_2d2d")
        _same(got, dict(mask_H=fit["mask_H"], mask_F=fit["mask_F"], mask_E=pose["mask_E"], mask_pose=pose["mask_pose"]),
              ("mask_H", "mask_F", "mask_E", "mask_pose"), n, "pose_2d2d")
    return _bare(f"pose_2d2d n={n}", fn)


def _host_handover(c, refs, n):
    p = capi.make_params(camera=synth.generic_camera(W, H))
    st, pp, un, state = dp._handover_inputs(dp.CAP)
    cand = lu.interior_points(W, H, n, 2, 5)
    want = hu.ref_handover(refs.handover, hu.camera_of(p), W, H, dp.CAP, dp.TARGET, dp.THRESHOLD, st, pp, un, cand, state=state)

    def fn():
        got = c.frame_handover(p, W, H, dp.CAP, dp.TARGET, dp.THRESHOLD, st, pp, un, cand, state=state)
        c.check_launch()
        _same(got, want, dp.HANDOVER_OUT, None, "frame_handover")
    return _bare(f"frame_handover n_cand={n}", fn)


def _host_scores(c, refs, n):
    p1, p2, Hm = dp._correspondences(n)
    H21, H12 = np.ascontiguousarray(Hm), np.ascontiguousarray(np.linalg.inv(Hm))
    F21 = np.ascontiguousarray([[0, -1e-4, 0.01], [1e-4, 0, -0.02], [-0.01, 0.02, 0.3]], F64)
    inH, sH = orc.check_homography(H21, H12, p1, p2, 1.0)
    inF, sF = orc.check_fundamental(F21, p1, p2, 1.0)

    def fn():
        gH, gF, gsH, gsF = c.geometry_scores(H21, H12, F21, p1, p2, 1.0)
        c.check_launch()
        assert np.array_equal(gH[:n], inH[:n]) and np.array_equal(gF[:n], inF[:n]), "geometry_scores: inlier flags"
        assert F32(gsH).tobytes() == F32(sH).tobytes() and F32(gsF).tobytes() == F32(sF).tobytes(), "geometry_scores: scores"
    return _bare(f"geometry_scores n={n}", fn)


def _host_neighbours(c, refs, n):
    ref, cur, kr, pu_, kc, st, aff = dp._neighbour_inputs(n)
    want = orc.find_near_neighbors(ref, cur, 5, kr, pu_, st, aff, kc, kc, level=1, radius_unit=10.0, cap=dp.NBR_CAP)
    assert want["rc"] == 0

    def fn():
        got = c.find_near_neighbors(ref, cur, 5, kr, pu_, st, aff, kc, kc, level=1, radius_unit=10.0, cap=dp.NBR_CAP)
        c.check_launch()
        assert got["rc"] == 0 and np.array_equal(got["count"][:n], want["count"][:n]), "find_near_neighbors: counts"
        live = np.arange(dp.NBR_CAP)[None, :] < want["count"][:n, None]
        for k in ("idx", "dist", "ncc"):
            assert got[k][:n][live].tobytes() == want[k][:n][live].tobytes(), f"find_near_neighbors: {k}"
    return _bare(f"find_near_neighbors n={n}", fn)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("make", [_host_fit, _host_pose, _host_handover, _host_scores, _host_neighbours],
                         ids=["geometry_fit", "pose_2d2d", "frame_handover", "geometry_scores", "find_near_neighbors"])
def test_host_form(built, refs, make, n):
    _sequence(refs, make, dict(n=n), None, [], host=True)


# ---- the hook's refusals -----------------------------------------------------------------------------------------------------------
def test_fill_refusals(built):
    """PAGK_E_ARG for a NULL context, inside a capture and while a graph of the context is alive -- and the context serves the
    next call as usual."""
    lib = capi.load()
    assert lib.pagk_selftest_fill_workspaces(None, 1, 0) == capi.PAGK_E_ARG
    c = capi.Context(0)
    try:
        frame = torch.from_numpy(np.array(dp.texture())).to(DEV)
        torch.cuda.synchronize()
        c.frame_upload(0, dp.texture(), 2)
        c.frame_set_device(1, frame.data_ptr(), W, H, W, 2)      # (sizes slot 1 for the captured call)
        c.sync()
        c.graph_begin()
        try:
            c.frame_set_device(1, frame.data_ptr(), W, H, W, 2)
            assert lib.pagk_selftest_fill_workspaces(c.h, 1, 0) == capi.PAGK_E_ARG
            assert "inside a graph capture" in lib.pagk_last_error(c.h).decode()
        finally:
            g = c.graph_end()
        assert lib.pagk_selftest_fill_workspaces(c.h, 1, 0) == capi.PAGK_E_ARG
        assert "is alive" in lib.pagk_last_error(c.h).decode()
        assert np.array_equal(c.frame_download_level(0, 1, W, H), orc.pyr_down(dp.texture())), "a refused fill wrote"
        c.graph_destroy(g)
        c.selftest_fill_workspaces(1)
        with pytest.raises(capi.PagkError):
            c.frame_download_level(0, 1, W, H)      # no slot is valid after a fill
        c.frame_upload(0, dp.texture(), 2)
        assert np.array_equal(c.frame_download_level(0, 1, W, H), orc.pyr_down(dp.texture()))
    finally:
        c.close()
