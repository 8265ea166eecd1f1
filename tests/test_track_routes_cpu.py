"""The route table (track_routes.py) against the build: every tracking kernel the product library carries is reached
by a row of the table or exempted with a reason, and every kernel a row names exists.  Works from the kernel NAMES in
kernel_resources.json (written by build_hip) alone.  Also: the conditions under which the rows of the GPU matrix say
something, checked on the CPU oracle for every patch size -- of the instantiation matrix and of the shape matrix."""
import json

import pytest

import shape_cases as sc
import track_routes as tr


@pytest.fixture(scope="module")
def built_kernels(built):
    with open(built.RESOURCES_JSON) as f:
        names = [k for k in json.load(f) if "k_track_" in k]
    parsed = {s: tr.parse_symbol(s) for s in names}
    assert all(parsed.values()), f"tracking kernel names that do not parse: {[s for s, p in parsed.items() if not p]}"
    return {p: s for s, p in parsed.items()}


def test_symbol_parser():
    assert tr.parse_symbol("_ZN4pagk13k_track_blockILi2ELi25ELi4ELb0ELb0ELb1EEEvNS_9TrackArgsE") == ("k_track_block", (2, 25, 4, 0, 0, 1))
    assert tr.parse_symbol("_ZN4pagk14k_track_block5ILi2ELi25ELb1EEEvNS_9TrackArgsE") == ("k_track_block5", (2, 25, 1))
    assert tr.parse_symbol("_ZN4pagk17k_track_block_pyrILi1ELi1ELb0EEEvNS_9TrackArgsENS_7PyrArgsE") == ("k_track_block_pyr", (1, 1, 0))
    assert tr.parse_symbol("_ZN4pagk14k_track_threadENS_9TrackArgsE") == ("k_track_thread", ())
    assert tr.parse_symbol("_ZN4pagk12k_track_quadILi7ELb0ELb1ELb1EEEvNS_9TrackArgsE") == ("k_track_quad", (7, 0, 1, 1))
    assert tr.parse_symbol("_ZN4pagk14k_gyro_predictENS_11PredictArgsE") is None


def test_template_arguments_follow_the_patch_size():
    for h, (nr, tail) in tr.BLOCK_ARGS.items():
        P = (2 * h + 1) ** 2
        assert (nr, tail) == (-(-P // 256), P % 32), h
    for h in tr.COMMON:
        P = (2 * h + 1) ** 2
        assert tr.NCH[h] == -(-P // 64) and tr.MFMA_ARGS[h] == (-(-P // 128), P % 32), h
    assert sorted(tr.BLOCK_ARGS) == list(range(1, 16))


def test_every_built_tracking_kernel_is_claimed(built_kernels):
    claimed = tr.claimed()
    unclaimed = sorted(s for k, s in built_kernels.items() if k not in claimed and k not in tr.EXEMPT)
    assert not unclaimed, f"tracking kernels that no row of tests/track_routes.py reaches: {unclaimed}"
    assert all(reason.strip() for reason in tr.EXEMPT.values())
    assert not set(tr.EXEMPT) & set(claimed), "a kernel is both claimed and exempt"


def test_every_claimed_kernel_is_built(built_kernels):
    missing = {k: rows[0] for k, rows in tr.claimed().items() if k not in built_kernels}
    assert not missing, f"rows of tests/track_routes.py name kernels that are not in the build: {missing}"
    gone = [k for k in tr.EXEMPT if k not in built_kernels]
    assert not gone, f"exempt kernels that are not in the build: {gone}"
    # with the test above: rows + exemptions == the build's tracking kernels (69 today: 67 + 2)


def test_rows_are_well_formed():
    names = [r.name for r in tr.ROUTES]
    assert len(set(names)) == len(names)
    for r in tr.ROUTES:
        assert len(r.selectors) == len(r.variants) == len(r.kernels) and r.halves, r.name
        assert r.entry in ("track", "track_device_fused", "track_device_batch"), r.name
        # LEAN and generic parameters reach different kernels wherever the template has the switch
        for h in r.halves:
            lean, generic = r.claims(h, True), r.claims(h, False)
            assert len(lean) == len(generic) and all(a[0].startswith("k_track_") for a in lean + generic), (r.name, h)


def test_every_row_names_the_test_that_runs_it():
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    for r in tr.ROUTES:
        module, _, name = r.test.partition("::")
        with open(os.path.join(here, module)) as f:
            assert f"\ndef {name}(" in f.read(), f"{r.name}: {r.test} does not exist"


@pytest.mark.parametrize("h", range(1, 16))
def test_matrix_rows_cannot_pass_vacuously(built, h):
    """On the oracle alone: the generic modes move tracked points, the d = 0 features fail under the penalty, and (patch
    sizes of the continuation rows) most live features run past the hand-over budget."""
    import instantiation_cases as cases
    cases.check_not_vacuous(h, continuation=h in tr.COMMON)


def _shape_halves():
    return sorted({h for r in tr.ROUTES if r.test.startswith("test_instantiations_gpu.py") for h in sc.halves(r.name)})


@pytest.mark.parametrize("shape", sc.SHAPES, ids=sc.shape_id)
def test_shape_rows_cannot_pass_vacuously(built, shape):
    """The shape matrix (test_shapes_gpu.py) on the oracle alone, for every half patch a row runs: enough features are live
    and tracked, the two modes differ, most features pass the continuation routes' budget, and every level of every
    stream of the batch exists."""
    assert _shape_halves() == [1, 5, 7, 10, 15]
    for h in _shape_halves():
        sc.check_not_vacuous(sc.workload(shape, h), sc.budget(shape[2]) if h in tr.COMMON else None)
    for h in tr.COMMON:
        ws = sc.batch_workloads(shape, h)
        assert [w.n for w in ws] == [1, 67, 30] and ws[1] is sc.workload(shape, h)
        assert len({w.img_ref.shape for w in ws}) == 3 and {w.pyramids for w in ws} == {shape[2]}
        assert all(min(w.img_ref.shape) >> (shape[2] - 1) >= 1 for w in ws)
        for mode in sc.MODES:
            assert all(ref["status"][:w.n].any() or w.n == 1 for w, ref in zip(ws, sc.batch_oracles(shape, h, mode)))


def test_deep_slot_rows_cannot_pass_vacuously(built):
    for h in sorted({h for name in sc.DEEP_ROUTES for h in sc.halves(name)}):
        sc.check_not_vacuous(sc.deep_workload(h))


def test_shape_matrix_variants_follow_select_variant():
    """shape_cases.expected_variants restates the one rule of csrc/pagk_select.h that depends on the depth."""
    assert sc.expected_variants("levels", 1) == (5,) and sc.expected_variants("levels", 2) == (7,)
    assert sc.expected_variants("continuation-live", 1) == (5, 5) and sc.expected_variants("continuation-live", 8) == (5, 7)
    assert sc.expected_variants("batch", 1) == (5,) and sc.expected_variants("block", 1) == (0,)
    assert sc.budget(1) == 1 and {sc.budget(L) for L in range(2, 9)} == {3}
