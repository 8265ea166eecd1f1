"""The oracle against the reference's OWN text, compiled: oracle/_ref/ref_patchmatch is src/patch_match.cpp and src/utils.cpp of
the reference, unchanged, built against the project's stand-ins for OpenCV and Eigen (oracle/ref_shim; recipe `make -C oracle ref`,
run by build() where the reference's sources are).  What this pins: OpticalFlowMultiLevel, ..._onePixel, the member and the free
GetPixelValue, DistortPoints / DistortVecPoints, PatchMatch::NCC and the free NCC -- their promotions, loop orders, clamps and
branches.  What it cannot pin: the arithmetic of Eigen (llt, solve, norm), cv::resize and libm's log, which the oracle's
definitions supply on BOTH sides (oracle/README.md); tests/test_reference_pin.py still waits for a real build for those.

The tests that run the binary skip only where neither the reference's sources nor a built binary exist.  The last test needs no
binary: it holds the oracle to the binary's committed outputs (tests/golden/ref_shim/), so the pin survives on such machines."""
import functools
import os

import numpy as np
import pytest

import reference_cases as rc
from oracle import pagk_oracle as orc
from util import golden_cases, load_golden

HAVE_REFERENCE = os.access(os.path.join(rc.REFERENCE, "src", "patch_match.cpp"), os.R_OK) or os.path.exists(rc.REF_BIN)
needs_binary = pytest.mark.skipif(not HAVE_REFERENCE, reason="neither the reference's sources nor oracle/_ref/ref_patchmatch are here")
SENSITIVE_MASKS = {1: "lower-solve association", 8: "LLT reciprocal", 32: "4th-pivot sum"}   # oracle/README.md: each moves points


@pytest.fixture(scope="module")
def ref(built, tmp_path_factory):
    """Runs the compiled reference, once per case: name -> (params, inputs, outputs)."""
    # build_reference() never raises (every test of the suite builds through it); here its failure is a failure
    assert built.build_reference() or not os.access(os.path.join(rc.REFERENCE, "src", "patch_match.cpp"), os.R_OK), \
        "the reference's sources are present and `make -C oracle ref` did not build them (its output is on stderr)"
    assert os.path.exists(rc.REF_BIN)
    workdir = tmp_path_factory.mktemp("ref_shim")

    @functools.lru_cache(maxsize=None)
    def run(name):
        if name.startswith("golden:"):
            params, inp, _ = load_golden(name[7:])
        else:
            params, inp = rc.params_of(rc.case(name)), rc.make_inputs(rc.case(name))
        out, proc = rc.run_reference(params, inp, workdir, name.replace(":", "_"))
        assert out is not None, f"{name}: ref_patchmatch exited with {proc.returncode}: {proc.stderr}"
        for a in list(inp.values()) + list(out.values()):
            a.setflags(write=False)
        return params, inp, out
    return run


def oracle_track(params, inp):
    return orc.track(params, inp["img_ref"], inp["img_cur"], inp["pt_ref"], inp["pt_init"], inp["affine"], inp["status_in"])


def assert_bit_equal(got, want, n, what, skip_rows=()):
    keep = np.setdiff1d(np.arange(n), np.asarray(list(skip_rows), np.int64))
    for k in rc.OUTPUTS:
        a, b = np.asarray(got[k][:n])[keep], np.asarray(want[k][:n])[keep]
        assert a.dtype == b.dtype, f"{what}: {k} is {a.dtype}, the reference writes {b.dtype}"
        assert np.array_equal(a, b, equal_nan=True), f"{what}: {k} differs from the compiled reference in rows {keep[rc.differing_rows({k: a}, {k: b}, len(keep), (k,))][:8]}"


@needs_binary
@pytest.mark.parametrize("name", [c.name for c in rc.CASES])
def test_table_case(ref, name):
    c = rc.case(name)
    params, inp, want = ref(name)
    n = c.n
    # the conditions of the table, from the reference's outputs alone
    excluded = rc.EXCLUDED.get(name, {})
    assert len(excluded) <= rc.MAX_EXCLUDED_SHARE * n and all(isinstance(r, str) and r for r in excluded.values())
    assert want["status"].shape == (n,) and int(np.count_nonzero(inp["status_in"] == 0)) in range(max(1, n // 25), n // 10 + 1)
    if c.content == "texture":
        assert 2 * int(want["status"].sum()) >= n, f"{name}: the reference tracks only {int(want['status'].sum())} of {n} rows"
        assert int((want["status"] == 0).sum()) >= 1
    assert_bit_equal(oracle_track(params, inp), want, n, name, excluded)


@needs_binary
@pytest.mark.parametrize("name", golden_cases())
def test_golden_case(ref, name):
    params, inp, want = ref("golden:" + name)
    assert_bit_equal(oracle_track(params, inp), want, inp["pt_ref"].shape[0], name)


@needs_binary
@pytest.mark.parametrize("name", [c.name for c in rc.NCC_CASES])
def test_free_ncc_overloads(ref, tmp_path, name):
    c = rc.ncc_case(name)
    inp = rc.make_ncc_inputs(c)
    by_images, by_values, proc = rc.run_reference_ncc(c, inp, tmp_path)
    assert by_images is not None, f"{name}: ref_patchmatch --ncc exited with {proc.returncode}: {proc.stderr}"
    n = inp["pt_ref"].shape[0]
    got = np.array([orc.ncc_free(inp["img_ref"], inp["img_cur"], c.half_patch, inp["pt_ref"][i], inp["pt_cur"][i],
                                 inp["affine"][i] if c.use_affine else None) for i in range(n)], np.float32)
    excluded = rc.EXCLUDED.get(name, {})
    assert len(excluded) <= rc.MAX_EXCLUDED_SHARE * n
    keep = np.setdiff1d(np.arange(n), np.asarray(list(excluded), np.int64))
    assert np.isfinite(by_images).all()
    for label, want in (("NCC(ref, cur, ...)", by_images), ("NCC(values, mean, cur, ...)", by_values)):
        assert np.array_equal(got[keep], want[keep]), f"{name}: {label} differs from pagk_oracle_ncc_free in rows {keep[got[keep] != want[keep]][:8]}"


@needs_binary
@pytest.mark.parametrize("mask", sorted(SENSITIVE_MASKS))
def test_comparison_sees_an_alternative(ref, mask):
    """The comparison is not vacuous: the oracle with ONE Eigen association switched no longer reproduces the binary (which
    carries the mask-0 definitions) on the 1000-point workload."""
    name = "cfg1_752x480"
    params, inp, want = ref(name)
    try:
        orc.set_alternatives(mask)
        got = oracle_track(params, inp)
    finally:
        orc.set_alternatives(0)
    rows = rc.differing_rows(got, want, rc.case(name).n)
    assert len(rows) >= 1, f"switching the {SENSITIVE_MASKS[mask]} changes no row: the comparison cannot see it"
    assert len(rc.differing_rows(oracle_track(params, inp), want, rc.case(name).n)) == 0   # ... and mask 0 is restored


@needs_binary
def test_sanitizer_build_is_clean(ref, tmp_path):
    """The same program under AddressSanitizer and UBSan (a stand-alone CPU program), over the whole table and the NCC cases:
    exit status 0 and nothing reported.  A report says where the reference reads: widen the stand-in's slack or name an
    exclusion in reference_cases.EXCLUDED; never suppress it."""
    assert os.path.exists(rc.REF_BIN_SAN)
    for c in rc.CASES:
        out, proc = rc.run_reference(rc.params_of(c), rc.make_inputs(c), tmp_path, c.name, binary=rc.REF_BIN_SAN)
        assert proc.returncode == 0 and proc.stderr == "" and out is not None, f"{c.name}: exit {proc.returncode}\n{proc.stderr[-4000:]}"
    for c in rc.NCC_CASES:
        by_images, _, proc = rc.run_reference_ncc(c, rc.make_ncc_inputs(c), tmp_path, binary=rc.REF_BIN_SAN)
        assert proc.returncode == 0 and proc.stderr == "" and by_images is not None, f"{c.name}: exit {proc.returncode}\n{proc.stderr[-4000:]}"


@needs_binary
@pytest.mark.parametrize("name", rc.committed_cases())
def test_committed_fixture_is_what_the_binary_writes(ref, name):
    params, inp, want = ref(name)
    fparams, finp, fout, built_with = rc.load_fixture(name)
    assert bytes(fparams) == bytes(params)
    for k in inp:
        assert np.array_equal(finp[k], inp[k]) and finp[k].strides == inp[k].strides, f"{name}: input {k} of the fixture is not the table's"
    assert_bit_equal(fout, want, rc.case(name).n, name + " (fixture)")
    for word in ("src/patch_match.cpp:33-469", "src/utils.cpp:25-202", "stand-ins", "pagk_oracle_llt_solve4", "pagk_oracle_pyr_down", "pagk_oracle_log"):
        assert word in built_with


@needs_binary
@pytest.mark.parametrize("name", [c.name for c in rc.NCC_CASES])
def test_committed_ncc_fixture_is_what_the_binary_writes(ref, tmp_path, name):
    c = rc.ncc_case(name)
    inp = rc.make_ncc_inputs(c)
    by_images, by_values, _ = rc.run_reference_ncc(c, inp, tmp_path)
    finp, f_images, f_values, built_with = rc.load_ncc_fixture(name)
    for k in inp:
        assert np.array_equal(finp[k], inp[k]) and finp[k].strides == inp[k].strides
    assert np.array_equal(f_images, by_images) and np.array_equal(f_values, by_values) and "src/utils.cpp:110-148" in built_with


# ---- no binary needed -------------------------------------------------------------------------------------------------------
def test_every_committed_case_has_its_fixture():
    have = sorted(os.path.splitext(f)[0] for f in os.listdir(rc.FIXTURE_DIR) if f.endswith(".npz"))
    assert have == sorted(rc.committed_cases() + [c.name for c in rc.NCC_CASES])
    largest = os.path.getsize(os.path.join(os.path.dirname(rc.FIXTURE_DIR), "h10_it30_L4.npz"))
    assert all(os.path.getsize(os.path.join(rc.FIXTURE_DIR, f + ".npz")) <= largest for f in have)


@pytest.mark.parametrize("name", rc.committed_cases())
def test_oracle_reproduces_the_committed_reference_outputs(built, name):
    params, inp, want, _ = rc.load_fixture(name)
    assert_bit_equal(oracle_track(params, inp), want, inp["pt_ref"].shape[0], name)


@pytest.mark.parametrize("name", [c.name for c in rc.NCC_CASES])
def test_oracle_reproduces_the_committed_reference_ncc(built, name):
    inp, by_images, by_values, _ = rc.load_ncc_fixture(name)
    c = rc.ncc_case(name)
    got = np.array([orc.ncc_free(inp["img_ref"], inp["img_cur"], c.half_patch, inp["pt_ref"][i], inp["pt_cur"][i],
                                 inp["affine"][i] if c.use_affine else None) for i in range(inp["pt_ref"].shape[0])], np.float32)
    assert np.array_equal(got, by_images) and np.array_equal(got, by_values)
