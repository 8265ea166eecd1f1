"""Every device entry point on guarded, exact-length device arrays (tests/arena.py), one case per row of
tests/device_forms.py and shape.  The engine and the per-entry-point scenarios are in tests/device_plans.py.

The parity tests compare the bytes an array is documented to have and nothing else; their device arrays come out of one
packed buffer or out of torch's caching allocator, where a write one row past n lands in a neighbour and a read past the
end returns some other tensor's bytes.  Here every caller array is exactly its documented length with a guard band on both
sides, and every case
  1. runs the call under guard fill A: no guard damaged; every output payload byte-identical to the restatement the
     module's own GPU test uses; rows the header says are left untouched still hold the sentinel; inputs unchanged;
  2. rewrites the guards with fill B, resets the outputs and runs again: the same bytes (a read outside an array that
     steers a result shows here), no guard damaged;
  3. runs once more with each optional output NULL: the others unchanged.
The expected bytes never come from another call into the library."""
import numpy as np
import pytest
import torch

import arena as ar
import device_plans as dp
import instantiation_cases as cases
import inverse_ref_util as iu
import shape_cases as sc
import track_routes as tr
from device_plans import COUNTS, DEV, I32, check
from oracle import pagk_oracle as orc
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi
from util import needs_variant

pytestmark = pytest.mark.gpu


def test_the_arena_on_the_device(built):
    """The checks of test_arena_cpu.py once on device memory: a planted byte behind an array, one in front of it, one inside
    the payload, under both fills."""
    for which in ("A", "B"):
        a = ar.Arena(DEV, capacity=1 << 16, which=which)
        v = a.out("res", torch.float32, (3, 2), "float")
        a.inp("n", np.array([3], I32), "index")
        assert v.is_cuda and v.data_ptr() % 256 == 0 and a.damaged() == {}
        e = a.entries["res"]
        for off in (24, -1, 5):
            a.raw[a.base + e.off + off] = 0x5A
        torch.cuda.synchronize()
        assert a.damaged() == {"res": [-1, 24]} and a.inputs_unchanged() == []


# ---- trackers ----------------------------------------------------------------------------------------------------------------
def _route_cases():
    out = []
    for r in tr.ROUTES:
        if not r.test.startswith("test_instantiations_gpu.py"):
            continue
        marks = [needs_variant(r.needs_variant)] if r.needs_variant else []
        out += [pytest.param(r.name, h, marks=marks, id=f"{r.name}-h{h}") for h in r.halves]
    return out


ROUTE_MODES = ("lean", "both")


@pytest.mark.parametrize("name,h", _route_cases())
def test_track_route(built, request, monkeypatch, name, h):
    """Every row of track_routes.ROUTES that the instantiation matrix runs, on its workload (320 x 240, three levels, 67
    features: the last quad wave has spare rows), through the DEVICE forms with every array in the arena -- also the rows
    whose own test goes through pagk_track, whose staging block would hide an overrun."""
    r = tr.route(name)
    cases.check_not_vacuous(h, continuation=r.handover)
    for var, value in r.env:
        monkeypatch.setenv(var, value)
    w = cases.workload(h)
    if r.entry == "track_device_batch":
        return _batch(r, h)
    c = capi.Context(0) if (r.env or r.entry != "track") else request.getfixturevalue("ctx")
    try:
        for selector, variant in zip(r.selectors, r.variants):
            for k, mode in enumerate(ROUTE_MODES):
                what = f"{name} h={h} kernel {selector} {mode}"
                p, ref = cases.params(w, mode), cases.oracle(h, mode)
                if r.entry == "track_device_fused":
                    check(dp.fused(c, what, w, p, ref, variant, 16 * h + k, pad=13 * (1 - k)))
                else:
                    check(dp.track(c, what, w, p, ref, w.n, variant, r.handover, selector))
    finally:
        if c is not request.getfixturevalue("ctx"):
            c.close()


def _batch(r, h):
    """pagk_track_device_batch: streams of 1, 67 and 30 features as one launch, every stream's arrays in the arena."""
    ws = cases.batch_workloads(h)
    assert [w.n for w in ws] == [1, 67, 30]
    ctxs = [capi.Context(0) for _ in ws]
    try:
        for mode in ROUTE_MODES:
            check(dp.batch(ctxs, f"batch h={h} {mode}", ws, cases.params(ws[0], mode), cases.batch_oracles(h, mode), r.selectors[0],
                           r.variants[0], r.handover))
    finally:
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("h", iu.HALVES)
def test_track_template_jacobian(ctx, h):
    """Variant 8 (inverse == PAGK_INVERSE_TEMPLATE, k_inv_wave) on 96 x 64 with two levels, against tests/inverse_ref.c."""
    shape = (96, 64, 2)
    w = sc.workload(shape, h)
    for mode in sc.MODES:
        check(dp.track(ctx, f"template Jacobian h={h} {mode}", w, iu.shape_params(w, mode), iu.restated(shape, h, mode),
                       w.n, 8, False))


@pytest.mark.parametrize("selector,variant", [(0, 0), (3, 3)])
def test_track_ncc(ctx, selector, variant):
    """calculate_ncc: the ncc field holds results (not all 1) and stays inside its array."""
    w = cases.workload(5)
    p = cases.params(w, "lean")
    p.calculate_ncc = 1
    ref = orc.track(p, w.img_ref, w.img_cur, w.pt_ref, w.pt_init, w.affine, w.status_in, nthreads=8)
    assert (ref["ncc"][:w.n][ref["status"][:w.n] > 0] != 1).any()
    check(dp.track(ctx, f"ncc kernel {selector}", w, p, ref, w.n, variant, False, selector))


@pytest.mark.parametrize("selector,variant", [(0, 0), (1, 1), (3, 3), (5, 5), (7, 7)])
@pytest.mark.parametrize("n", [0, 1])
def test_track_one_and_none(built, monkeypatch, n, selector, variant):
    """n = 1: one row of every output.  n = 0: every output untouched (zero-length arrays: only guards around the pointer)."""
    monkeypatch.setenv("PAGK_QUAD_BUDGET", "0")
    w = cases.workload(5)
    c = capi.Context(0)
    try:
        for mode in ROUTE_MODES:
            ref = cases.oracle(5, mode)   # features are independent: the first row of the 67-feature run
            plan = dp.track(c, f"n={n} kernel {selector} {mode}", w, cases.params(w, mode), ref, n, variant if n else None, False,
                            selector)
            if n == 0:
                plan.want = {k: (lambda s: s) for k in plan.want}
            check(plan)
    finally:
        c.close()


# ---- everything else ---------------------------------------------------------------------------------------------------------
# The smallest inputs of each module's own GPU test; counts from test_host_forms_gpu.COUNTS; where a form has a capacity it
# is strictly larger than the count the restatement returns, so that a tail exists (asserted on the restatement's result).
@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    return dp.Refs(tmp_path_factory)


def _own():
    return capi.Context(0)


# -- frames
@pytest.mark.parametrize("pad", [0, 13])
def test_frame_set_device(built, refs, pad):
    c = _own()
    try:
        check(dp.frame_set_device(c, refs, pad))
    finally:
        c.close()


@pytest.mark.parametrize("pad", [0, 13])
def test_frame_set_device_batch(built, refs, pad):
    """Three contexts' frames as one call: an even frame, the 97 x 80 texture (odd parents) and a 160 x 120 one."""
    ctxs = [_own() for _ in range(3)]
    try:
        check(dp.frame_set_device_batch(ctxs, refs, pad))
    finally:
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("pad", [0, 5])
def test_frame_rectify_device(built, refs, pad, cn):
    c = _own()
    try:
        check(dp.frame_rectify_device(c, refs, pad, cn))
    finally:
        c.close()


# -- prediction
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("form", ["", "_rot", "_live"])
def test_gyro_predict_device(ctx, refs, form, n):
    check(dp.gyro_predict_device(ctx, refs, form, n))


# -- Step 3
@pytest.mark.parametrize("n", COUNTS)
def test_post_filter_device(ctx, refs, n):
    check(dp.post_filter_device(ctx, refs, n))


# -- hand-overs
@pytest.mark.parametrize("n_cand", COUNTS)
def test_frame_handover_device(ctx, refs, n_cand):
    check(dp.frame_handover_device(ctx, refs, n_cand))


@pytest.mark.parametrize("detector", ["harris", "fast"])
def test_frame_handover_with_detector_device(built, refs, detector):
    c = _own()
    try:
        check(dp.frame_handover_with_detector_device(c, refs, detector))
    finally:
        c.close()


# -- detectors
@pytest.mark.parametrize("max_corners", COUNTS)
@pytest.mark.parametrize("masked", [False, True])
def test_detect_corners_device(ctx, refs, max_corners, masked):
    check(dp.detect_corners_device(ctx, refs, max_corners, masked))


@pytest.mark.parametrize("n_features", COUNTS[1:])
@pytest.mark.parametrize("masked", [False, True])
def test_detect_fast_device(ctx, refs, n_features, masked):
    check(dp.detect_fast_device(ctx, refs, n_features, masked))


# -- ORB
@pytest.mark.parametrize("n", COUNTS)
def test_orb_describe_device(ctx, refs, n):
    check(dp.orb_describe_device(ctx, refs, n))


@pytest.mark.parametrize("nq,nt", [(0, 65), (65, 0), (1, 1), (1, 65), (65, 65)])
def test_orb_match_device(ctx, refs, nq, nt):
    check(dp.orb_match_device(ctx, refs, nq, nt))


# -- Lucas-Kanade
def test_lk_pyramid_device(ctx, refs):
    """The row without a caller array: the levels it builds for a slot, against the restatement."""
    dp.lk_pyramid_device(ctx, refs).run({}, ())


@pytest.mark.parametrize("n", COUNTS)
def test_lk_track_device(ctx, refs, n):
    check(dp.lk_track_device(ctx, refs, n))


# -- geometry
@pytest.mark.parametrize("n", COUNTS)
def test_geometry_scores_device(ctx, refs, n):
    check(dp.geometry_scores_device(ctx, refs, n))


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("with_status", [False, True])
def test_geometry_fit_device(ctx, refs, n, with_status):
    check(dp.geometry_fit_device(ctx, refs, n, with_status))


@pytest.mark.parametrize("n", COUNTS)
def test_geometry_validation_device(ctx, refs, n):
    check(dp.geometry_validation_device(ctx, refs, n))


# -- pose
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("with_status", [False, True])
def test_pose_2d2d_device(ctx, refs, n, with_status):
    check(dp.pose_2d2d_device(ctx, refs, n, with_status))


@pytest.mark.parametrize("nq", COUNTS)
def test_pose_from_matches_device(ctx, refs, nq):
    check(dp.pose_from_matches_device(ctx, refs, nq))


# -- neighbours and association
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("with_affine", [False, True])
def test_near_neighbors_device(ctx, refs, n, with_affine):
    check(dp.near_neighbors_device(ctx, refs, n, with_affine))


@pytest.mark.parametrize("n", COUNTS)
def test_match_features_device(ctx, refs, n):
    check(dp.match_features_device(ctx, refs, n))


@pytest.mark.parametrize("min_matches", [0, 100])
@pytest.mark.parametrize("n", COUNTS)
def test_search_gyro_predict_device(ctx, refs, n, min_matches):
    check(dp.search_gyro_predict_device(ctx, refs, n, min_matches))


@pytest.mark.parametrize("n", COUNTS)
def test_search_klt_device(ctx, refs, n):
    check(dp.search_klt_device(ctx, refs, n))
