"""The solve's scalar branch on a rejected 4th pivot (csrc/pagk_device.h: Pivot3Known, the form the pipelined 4-wave
kernel runs) through pagk_selftest_solve against the CPU oracle, bit for bit: systems on which the branch goes either
way, the values at which it turns, and solves that leave the lean form for the plain divisions.  Which way a system
goes is told by the restatement of tests/pivot3_cases.py (held against the oracle in tests/test_solver_pivot3_cpu.py)."""
import numpy as np
import pytest

from oracle import pagk_oracle as orc

import pivot3_cases as pc

pytestmark = pytest.mark.gpu

MASKS = (0, pc.ALL_SOLVER_BITS)


@pytest.fixture
def alternatives():
    yield orc.set_alternatives
    orc.set_alternatives(0)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _assert_solves_match(ctx, alternatives, H, b, mask, names=None):
    alternatives(mask)
    ref_x = np.zeros((len(H), 4))
    ref_n = np.zeros(len(H))
    for i in range(len(H)):
        ref_x[i], ref_n[i] = orc.llt_solve4(H[i], b[i])
    alternatives(0)
    xs, ns, xl, nl = ctx.selftest_solve(np.ascontiguousarray(H).reshape(-1, 16), np.ascontiguousarray(b), mask)

    def where(bad):
        rows = np.unique(np.nonzero(bad)[0])
        return [names[i] if names else int(i) for i in rows[:8]]
    for form, got in (("one lane per system", xs), ("four lanes per system", xl)):
        bad = np.isnan(got) != np.isnan(ref_x)
        assert not bad.any(), f"{form}, solver bits {mask}: NaN pattern differs in {where(bad)}"
        bad = ~np.isnan(ref_x) & (_bits(got) != _bits(ref_x))
        assert not bad.any(), f"{form}, solver bits {mask}: bits differ in {where(bad)}"
    okn = ~np.isnan(ref_n)
    assert np.array_equal(_bits(ns[okn]), _bits(ref_n[okn]))
    with np.errstate(invalid="ignore"):
        bad = (nl < float.fromhex("0x1.a36e2eb1c432cp-14")) != (ref_n < 1e-2)
    assert not bad.any(), f"convergence test, solver bits {mask}: differs in {where(bad[:, None])}"


@pytest.mark.parametrize("P", pc.PATCH_SIZES)
def test_structured_singular_systems(ctx, alternatives, P):
    """(a) 4096 systems per patch size of the two-round bodies, summed like the kernels': both sides of the branch"""
    H, b = pc.structured(P)
    for mask in MASKS:
        k = pc.classify(H, mask)
        assert (k == 3).sum() >= 1000 and (k == 4).sum() >= 200, np.bincount(k, minlength=5)
        _assert_solves_match(ctx, alternatives, H, b, mask)


def test_edges_of_the_branch(ctx, alternatives):
    """(b) x3 = +-0, the limits of the lean form's range, NaN, negative, comfortably accepted; rejecting and accepting
    systems follow each other within a wave's sixteen turns"""
    names, H, b, stop = pc.edges()
    assert (stop == 3).any() and (stop == 4).any()
    for mask in MASKS:
        _assert_solves_match(ctx, alternatives, H, b, mask, names)


def test_out_of_range_early_pivots_still_take_the_redo(ctx, alternatives):
    """(c) pivot 0, 1 or 2 zero, negative, NaN or out of range: the plain-division form answers"""
    names, H, b = pc.early_pivots()
    for mask in MASKS:
        _assert_solves_match(ctx, alternatives, H, b, mask, names)
