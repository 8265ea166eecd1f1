"""The restatement that classifies a system's 4th pivot (tests/pivot3_cases.py) against the CPU oracle, bit for bit, on
every system the GPU test (tests/test_solver_pivot3_gpu.py) uses -- and the share of solves in which the reference
rejects that pivot on systems summed the way the kernels sum them, which is what the device's branch is for
(csrc/pagk_device.h: Pivot3Known)."""
import numpy as np
import pytest

from oracle import pagk_oracle as orc

import pivot3_cases as pc


@pytest.fixture
def alternatives():
    orc.build()
    yield orc.set_alternatives
    orc.set_alternatives(0)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _hold(H, b, alt, what):
    """restate == pagk_oracle_llt_solve4 on every system: NaN where it has NaN, the same bits elsewhere"""
    for i in range(len(H)):
        ref_x, ref_n = orc.llt_solve4(H[i], b[i])
        x, nrm, _, _ = pc.restate(H[i], b[i], alt)
        got, ref = np.append(x, nrm), np.append(ref_x, ref_n)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what} system {i} (solver bits {alt})"
        ok = ~np.isnan(ref)
        assert np.array_equal(_bits(got[ok]), _bits(ref[ok])), f"{what} system {i} (solver bits {alt})"


@pytest.mark.parametrize("alt", [0, pc.ALL_SOLVER_BITS])
@pytest.mark.parametrize("P", pc.PATCH_SIZES)
def test_restatement_is_the_oracle_on_structured_systems(alternatives, P, alt):
    H, b = pc.structured(P)
    alternatives(alt)
    _hold(H, b, alt, f"structured P = {P}")


@pytest.mark.parametrize("alt", [0, 1, 2, 4, 8, 32, pc.ALL_SOLVER_BITS])
def test_restatement_is_the_oracle_on_the_edges(alternatives, alt):
    alternatives(alt)
    names, H, b, _ = pc.edges()
    _hold(H, b, alt, "edge")
    names, H, b = pc.early_pivots()
    _hold(H, b, alt, "early pivot")


def test_edges_stop_where_they_are_built_to_stop():
    names, H, b, stop = pc.edges()
    got = pc.classify(H)
    assert [n for n, g, s in zip(names, got, stop) if g != s] == []
    assert (stop == 3).sum() >= 10 and (stop == 4).sum() >= 10
    # and the early-pivot set holds solves that stop at 0, 1 and 2 as well as ones that run through
    got = pc.classify(pc.early_pivots()[1])
    assert all((got == k).sum() >= 8 for k in range(5)), np.bincount(got, minlength=5)


@pytest.mark.parametrize("P", pc.PATCH_SIZES)
def test_both_sides_of_the_branch_are_populated(P):
    """what the GPU test requires of its case (a): at least 1000 rejected and 200 accepted 4th pivots per patch size,
    and no earlier pivot rejected"""
    for alt in (0, pc.ALL_SOLVER_BITS):
        k = pc.classify(pc.structured(P)[0], alt)
        assert (k == 3).sum() >= 1000 and (k == 4).sum() >= 200 and (k < 3).sum() == 0, np.bincount(k, minlength=5)


def test_reference_rejects_the_4th_pivot_in_most_flagship_solves():
    """P = 441 products of float32 (Ix, Iy, c, 1) per entry, summed in order (BASELINE configs[1]: h = 10): the reference
    returns at the 4th pivot in at least half of the systems.  (Counted in the oracle itself on synth.config(1, n=1000)
    with the benchmark's parameters: 8890 of 10618 solves, 83.7 %)"""
    H, _ = pc.structured(441)
    k = pc.classify(H)
    assert (k < 3).sum() == 0
    share = (k == 3).mean()
    print(f"4th pivot rejected in {100 * share:.1f} % of {len(H)} systems")
    assert share >= 0.5
