"""The project's CPU side against the reference's OWN ORB extractor, compiled: oracle/_ref/ref_orb is src/ORBextractor.cc of the
reference, unchanged, under the reference's own include/ORBextractor.h, built against a stand-in OpenCV of its own
(oracle/ref_shim/orb; recipe `make -C oracle ref`).  What this pins: the constructor's level and quota table, ComputePyramid's
sizes, the cell arithmetic, skip rules and fall-back pass of ComputeKeyPointsOctTree, DistributeOctTree and DivideNode -- the
bucket of a key, push-front order, the inner loop's sort, walk and break, the best of a node -- the scaling and the mask test of
DetectFeatures, IC_Angle and computeOrbDescriptor, against tests/fast_detect_ref.c (fdr_*), tests/orb_ref.c (orb_ref_*),
tests/orb_levels_ref.c (olr_*) and the numpy models, bit for bit.  What it cannot pin: cv::FAST, resize, copyMakeBorder,
GaussianBlur, fastAtan2, cvRound, the sine and cosine of a float and pow, which the project's definitions supply on BOTH sides
(oracle/pagk_oracle_cv.h; the tests at the end hold the restatements' own copies byte-equal to them), and the order of nodes of
equal size in the sort of :708, which in the reference is the order of their addresses: the program's allocator makes that the
creation order (or, on a switch, its reverse).

The reference outside what the library accepts, and therefore not compared: a frame with (W - 32) / (H - 32) < 0.5 (62 x 903,
say) makes nIni 0 at :567, and :593 then indexes an empty vector (the sanitizer build reports it); include/pagk.h refuses such
a size.

The tests that run the binary skip only where neither the reference's sources nor a built binary exist.  The tests at the end
need no binary: they hold the CPU side to the binary's committed outputs (tests/golden/ref_shim/orb/)."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import fast_ref_util as fu
import orb_levels_ref_util as lu
import orb_ref_util as ou
import reference_cases as rc
import reference_orb_util as pu
from oracle import pagk_oracle as orc

HAVE_REFERENCE = os.access(os.path.join(rc.REFERENCE, "src", "ORBextractor.cc"), os.R_OK) or os.path.exists(rc.ORB_BIN)
needs_binary = pytest.mark.skipif(not HAVE_REFERENCE, reason="neither the reference's sources nor oracle/_ref/ref_orb are here")
NAMES = [c.name for c in rc.ORB_CASES]
COMMITTED = [c.name for c in rc.ORB_CASES if c.committed]
F = np.float32


@pytest.fixture(scope="module")
def libs(built, tmp_path_factory):
    return pu.build_libs(tmp_path_factory)


@pytest.fixture(scope="module")
def orb(built, tmp_path_factory):
    """Runs the compiled reference extractor, once per (case, switches): -> (inputs, outputs)."""
    assert built.build_reference() or not os.access(os.path.join(rc.REFERENCE, "src", "ORBextractor.cc"), os.R_OK), \
        "the reference's sources are present and `make -C oracle ref` did not build them (its output is on stderr)"
    assert os.path.exists(rc.ORB_BIN)
    workdir = tmp_path_factory.mktemp("ref_orb")

    def run_inputs(inp, name, binary=rc.ORB_BIN):
        out, proc = rc.run_orb(inp, workdir, name, binary=binary)
        assert out is not None and proc.stderr == "", f"{name}: ref_orb exited with {proc.returncode}: {proc.stderr[-4000:]}"
        return out

    @functools.lru_cache(maxsize=None)
    def run(name, descending=False, border_a5=False):
        inp = rc.make_orb_inputs(rc.orb_case(name), descending=descending, border_a5=border_a5)
        out = run_inputs(inp, f"{name}_{int(descending)}{int(border_a5)}")
        for a in list(inp.values()) + list(out.values()):
            a.setflags(write=False)
        return inp, out
    run.inputs = run_inputs
    return run


def keys_of(inp, out=None):
    ex = pu.extractor_of(inp)
    keys = ["scale", "inv_scale", "quota", "umax", "kp", "octave", "response", "size"] + [f"level_{l}" for l in range(ex.n_levels)]
    return keys + (["angle", "desc"] if ex.extract else [])


def assert_same(got, want, keys, what):
    for k in keys:
        assert k in want, f"{what}: the compiled reference wrote no {k}"
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {k} is {a.dtype}{a.shape}, the reference writes {b.dtype}{b.shape}"
        assert pu.same_bits(a, b), f"{what}: {k} differs from the compiled reference:\n{a}\n{b}"


def check_cpu_side(libs, inp, want, what, reverse_tie=False):
    """Every output group of the binary against the restatements and the models."""
    ex = pu.extractor_of(inp)
    h, w = inp["img"].shape
    # olr_levels / olr_resize / olr_extract
    got, table, r = pu.restated(libs, inp, reverse_tie=True if reverse_tie else None)
    assert_same(got, want, keys_of(inp), what + " (olr_extract)")
    assert [lv.shape for lv in r["levels"]] == list(zip(table["height"].tolist(), table["width"].tolist()))
    # model_levels / model_pyramid
    m, mtable = pu.modelled(inp)
    assert_same(m, want, ["scale", "inv_scale", "quota"] + [f"level_{l}" for l in range(ex.n_levels)], what + " (numpy models)")
    assert np.array_equal(mtable["size"], table["size"]) and np.array_equal(want["size"], mtable["size"][want["octave"]].astype(F))
    # per level: the cells and the raw list against the FAST log, fdr_detect and orb_ref_describe through compose()
    levels = pu.level_images(want)
    for l, img in enumerate(levels):
        log, cells, grid = pu.cells_of_log(want, l), fu.ref_cells(libs.fast, img, ex.ini_threshold, ex.min_threshold), fu.model_grid(*img.shape[::-1])
        assert log["cells"] == [(x0, y0, x1 - x0, y1 - y0) for (_, _, x0, y0, x1, y1) in grid["cells"]], f"{what}: the cells of level {l}"
        assert log["thresholds"] <= {(1, ex.ini_threshold), (2, ex.min_threshold)}
        assert pu.same_bits(log["xy"], cells["xy"]) and pu.same_bits(log["score"], cells["score"]), f"{what}: the raw list of level {l}"
        assert (log["first_empty"], log["empty"], len(log["cells"])) == (cells["first_empty"], cells["empty"], cells["cells"])
    comp = pu.compose(libs, levels, table, ex, inp.get("mask"), inp.get("pattern") if ex.extract else None, reverse_tie)
    assert_same(comp, want, ["kp", "octave", "response", "size", "angle"] + (["desc"] if ex.extract else []), what + " (fdr_detect + orb_ref_describe)")
    # one level: the numpy model of the detector, its mask included
    if ex.n_levels == 1 and max(h, w) <= 480:
        d = fu.model_detect(inp["img"], inp.get("mask"), ex.n_features, ini=ex.ini_threshold, mn=ex.min_threshold, reverse_tie=reverse_tie)
        assert pu.same_bits(d["keypoints"][:d["n"]], want["kp"]) and pu.same_bits(d["response"][:d["n"]], want["response"]), what + " (model_detect)"
    return comp


@needs_binary
@pytest.mark.parametrize("name", NAMES)
def test_table_case(orb, libs, name):
    """The ascending allocator: every output of the binary, bit for bit."""
    inp, want = orb(name)
    assert pu.same_bits(want["level_0"], inp["img"]) and pu.same_bits(want["umax"], np.array(ou.UMAX, np.int32))
    check_cpu_side(libs, inp, want, name)


@needs_binary
@pytest.mark.parametrize("name", COMMITTED)
def test_descending_allocator_is_the_reversed_tie_rule(orb, libs, name):
    inp, want = orb(name, descending=True)
    check_cpu_side(libs, inp, want, name + " (descending)", reverse_tie=True)


def tie_free(orb, name):
    return not pu.differing(orb(name)[1], orb(name, descending=True)[1], keys_of(orb(name)[0]))


@needs_binary
def test_rule_and_reverse_differ_somewhere(orb):
    differ = [n for n in COMMITTED if not tie_free(orb, n)]
    assert {"nini2_ties_91x62", "inner_320x240", "levels8_240x224"} <= set(differ), differ
    assert sum(tie_free(orb, n) for n in COMMITTED) >= 3


def level_stats(libs, inp, out):
    """Per level: the restatement's stats with the model's branch counters and the log's counts."""
    ex, res = pu.extractor_of(inp), []
    for l, img in enumerate(pu.level_images(out)):
        n_l = max(int(out["quota"][l]), 1)
        m = fu.model_detect(img, None, n_l, ini=ex.ini_threshold, mn=ex.min_threshold)
        log = pu.cells_of_log(out, l)
        res.append(dict(m["stats"], **m["branches"], nodes=int(m["info"][4]), raw=int(m["info"][1]), n=n_l, first_empty=log["first_empty"],
                        empty=log["empty"], cells=len(log["cells"]), grid=fu.model_grid(*img.shape[::-1]), log=log))
    return res


@needs_binary
def test_the_table_reaches_every_branch_it_names(orb, libs):
    """From the FAST log, the numpy model's counters and the outputs of the compiled reference."""
    st = {n: level_stats(libs, *orb(n)) for n in COMMITTED}
    one = lambda n: st[n][0]
    # ---- cells
    s = one("one_cell_62x62")
    assert s["cells"] == 1 and s["inner"] >= 1 and s["broke"] >= 1 and s["nodes"] == 22 > s["n"]
    s = one("nini2_boundary_key")
    inp, out = orb("nini2_boundary_key")
    assert s["n_ini"] == 2 and float(s["grid"]["hx"]) == 29.5 and [29.0, 14.0] in s["log"]["xy"].tolist()
    assert [45.0, 30.0] in out["kp"].tolist() and s["inner"] == 0 and s["nodes"] < s["n"]                # size == prevSize
    M = fu.model_m(inp["img"])
    assert M[25, 60] == M[25, 61] > 20 and not {(60.0, 25.0), (61.0, 25.0)} & {tuple(p) for p in out["kp"].tolist()}
    k = out["kp"].tolist().index([30.0, 40.0])
    assert ou.model_moments(inp["img"], 30, 40) == (0, 0) and out["angle"][k] == 0                       # the flat disc
    assert one("nini2_ties_91x62")["n_ini"] == 2 and one("nini2_ties_91x62")["ties"] >= 1 and one("nini2_ties_91x62")["best_ties"] >= 1
    assert one("round_2p5_107x62")["n_ini"] == 3 and (107 - 32) / (62 - 32) == 2.5
    assert one("round_0p5_62x92")["n_ini"] == 1 and (62 - 32) / (92 - 32) == 0.5
    s = one("column_skip_813x62")
    assert s["grid"]["n_cols"] == 26 and s["cells"] == 25 and max(x0 for x0, _, _, _ in s["log"]["cells"]) == 16 + 24 * 31
    assert fu.model_grid(812, 62)["n_cols"] * fu.model_grid(812, 62)["n_rows"] == len(fu.model_grid(812, 62)["cells"])   # 813 is the first
    s = one("row_skip_468x903")
    assert s["grid"]["n_rows"] == 29 and s["cells"] == 28 * s["grid"]["n_cols"] and max(y0 for _, y0, _, _ in s["log"]["cells"]) == 16 + 27 * 31
    assert fu.model_grid(468, 902)["n_rows"] * fu.model_grid(468, 902)["n_cols"] == len(fu.model_grid(468, 902)["cells"])
    for n in COMMITTED:   # maxX / maxY clamped to the border: the last cell of every level ends on it
        for lv in st[n]:
            x0, y0, w, h = lv["log"]["cells"][-1]
            assert (x0 + w, y0 + h) == (lv["grid"]["max_bx"], lv["grid"]["max_by"])
    s = one("fallback_152x92")
    assert s["first_empty"] >= 3 and 1 <= s["empty"] < s["first_empty"]
    assert {t for _, t in s["log"]["thresholds"]} == {20, 7}
    # ---- tree
    s = one("prev_size_planted")
    assert s["inner"] == 0 and s["nodes"] == s["raw"] < s["n"]
    s = one("inner_320x240")
    assert s["inner"] >= 1 and s["broke"] >= 1 and s["ties"] >= 50 and s["best_ties"] >= 10 and s["nodes"] >= s["n"]
    s = one("n1_160x120")
    assert s["n"] == 1 and s["inner"] == 0 and s["nodes"] == 4
    s = one("flat_255")
    assert s["raw"] == 0 and s["nodes"] == 0 and s["empty"] == s["cells"] and len(orb("flat_255")[1]["kp"]) == 0
    # ---- levels
    inp, out = orb("levels8_240x224")
    assert [out[f"level_{l}"].shape for l in (0, 7)] == [(224, 240), (63, 67)] and (np.bincount(out["octave"], minlength=8) >= 1).all()
    assert any(out[f"level_{l}"].shape[0] % 2 for l in range(7)) and any(out[f"level_{l}"].shape[1] % 2 for l in range(7))   # odd parents
    inp, out = orb("levels2_1p5_corner")
    assert out["scale"].tolist() == [1.0, 1.5] and out["level_1"].shape == (80, 107) and (np.bincount(out["octave"]) >= 1).all()
    assert np.abs(inp["pattern"]).min() == 13
    inp, out = orb("quota_tie_1p4")
    factor = F(F(1) / F(1.4))
    nd = F(F(F(162) * F(F(1) - factor)) / F(F(1) - F(float(factor) * float(factor))))
    assert float(nd) == 94.5 and out["quota"].tolist() == [94, 68]
    inp, out = orb("quota_zero_last")
    assert out["quota"].tolist() == [1, 1, 0] and st["quota_zero_last"][2]["inner"] == 0 and st["quota_zero_last"][2]["nodes"] >= 1
    assert (out["octave"] == 2).sum() == st["quota_zero_last"][2]["nodes"]      # N = 0 and N = 1: done after the first round, the same nodes
    inp, out = orb("size_tie_75x75")
    assert float(F(F(75) * out["inv_scale"][1])) == 62.5 and out["level_1"].shape == (62, 62)
    lv1 = out["kp"][out["octave"] == 1] / out["scale"][1]
    assert np.rint(lv1).min() == 19 and np.rint(lv1).max() == 62 - 20
    assert {19, 42} <= set(np.rint(lv1[:, 0]).tolist()) and {19, 42} <= set(np.rint(lv1[:, 1]).tolist())
    assert (np.bincount((out["angle"] // 45).astype(int), minlength=8) >= 1).all()       # both polynomial branches, x < 0, y < 0
    inp, out = orb("masked_levels4")
    ex = pu.extractor_of(inp)
    table = lu.ref_levels(libs.levels, ex.n_features, ex.scale_factor, ex.n_levels, 240, 224)
    unmasked = pu.compose(libs, pu.level_images(out), table, ex)
    dropped = np.bincount(unmasked["octave"], minlength=4) - np.bincount(out["octave"], minlength=4)
    assert dropped[0] >= 1 and dropped[1:].sum() >= 1, dropped


@needs_binary
@pytest.mark.parametrize("name", ["levels8_240x224", "levels2_1p5_corner", "size_tie_75x75", "one_cell_62x62"])
def test_nothing_reads_the_border(orb, name):
    """copyMakeBorder's border filled with 0xA5 instead of the reflection: no output changes, on every level -- FAST's cells
    start 16 inside a level, the disc of IC_Angle and the rotated pattern stay 19 - 18 inside, and the blur works on a clone
    of the level without its border."""
    plain, a5 = orb(name)[1], orb(name, border_a5=True)[1]
    assert set(plain) == set(a5) and not pu.differing(a5, plain, list(plain))


def _changed(inp, **kw):
    c = {k: np.array(v, copy=True) for k, v in inp.items()}
    for k, f in kw.items():
        f(c[k])
    return c


CHANGES = [   # (case, the output group, what changes, the change): each provably changes the compiled reference's output
    ("one_cell_62x62", ["kp", "response"], "one pixel", dict(img=lambda a: a.__setitem__((30, 30), 255 - a[30, 30]))),
    ("fallback_152x92", ["kp", "response"], "the second threshold", dict(cfg=lambda a: a.__setitem__(3, 12))),
    ("inner_320x240", ["kp", "response"], "N", dict(cfg=lambda a: a.__setitem__(0, 90))),
    ("quota_tie_1p4", ["quota"], "N across the tie", dict(cfg=lambda a: a.__setitem__(0, 163))),
    ("levels2_1p5_corner", ["level_1"], "one pixel", dict(img=lambda a: a.__setitem__((60, 80), 255 - a[60, 80]))),
    ("levels2_1p5_corner", ["desc"], "one pattern point", dict(pattern=lambda a: a.__setitem__(slice(0, 2), (-13, 13)))),
    ("size_tie_75x75", ["angle"], "one pixel", dict(img=lambda a: a.__setitem__((40, 40), 255 - a[40, 40]))),
    ("masked_levels4", ["kp", "octave"], "one mask byte", None),
]


@needs_binary
@pytest.mark.parametrize("k", range(len(CHANGES)))
def test_comparison_sees_a_changed_input(orb, libs, k):
    """The comparison is not vacuous: after an input change that changes the compiled reference's output, the CPU side run on
    the unchanged input no longer compares equal -- and run on the changed input it does again."""
    name, group, what, change = CHANGES[k]
    inp, want = orb(name)
    if change is None:   # the mask byte under the first keypoint of a level above 0
        j = int(np.flatnonzero(want["octave"] >= 1)[0])
        x, y = int(want["kp"][j, 0]), int(want["kp"][j, 1])
        change = dict(mask=lambda a: a.__setitem__((y, x), 0))
    changed = _changed(inp, **change)
    want2 = orb.inputs(changed, f"{name}_changed_{k}")
    got = pu.restated(libs, inp)[0]
    assert not pu.differing(got, want, group)
    assert pu.differing(want2, want, group), f"{what} does not change the compiled reference's {group}: the row proves nothing"
    assert pu.differing(got, want2, group), f"{what}: the comparison cannot see it"
    check_cpu_side(libs, changed, want2, f"{name} after {what}")


@needs_binary
def test_descriptors_under_the_references_own_table(orb, libs):
    """The table the reference's constructor copies is read from the program's pipe and handed to orb_ref_describe in memory;
    nothing of it is written to a file, here or in the repository."""
    text = subprocess.run([rc.ORB_BIN, "--table"], capture_output=True, text=True, check=True).stdout
    table = np.array(text.split(), np.int32)
    assert table.shape == (1024,) and np.abs(table).max() <= 13 and len(np.unique(table.reshape(512, 2), axis=0)) > 200
    for name in ("levels8_240x224", "size_tie_75x75"):
        inp = rc.make_orb_inputs(rc.orb_case(name), own_table=True)
        assert "pattern" not in inp
        want = orb.inputs(inp, name + "_own_table")
        assert pu.differing(want, orb(name)[1], ["desc"]) and not pu.differing(want, orb(name)[1], ["kp", "angle"])
        check_cpu_side(libs, dict(inp, pattern=table), want, name + " (the reference's own table)")


@needs_binary
@pytest.mark.parametrize("binary", [rc.ORB_BIN, rc.ORB_BIN_SAN])
def test_no_sine_cosine_or_pow_comes_from_libm(orb, binary):
    syms = subprocess.run(["nm", binary], capture_output=True, text=True, check=True).stdout.splitlines()
    names = {line.split()[-1].split("@")[0]: line.split()[-2] for line in syms if len(line.split()) >= 2}
    family = ("sin", "cos", "sincos", "sinf", "cosf", "sincosf", "pow", "powf", "atan2", "atan2f")
    assert not [f for f in family if names.get(f) == "U"], "a libm function decides a result"
    assert all(names.get(f) == "T" for f in ("sinf", "cosf", "sincosf", "pow"))


@needs_binary
def test_sanitizer_build_is_clean(orb):
    """The same program under AddressSanitizer and UBSan (a stand-alone CPU program with its own main, the default allocator),
    over the whole table: exit status 0, nothing reported.  Its outputs are compared on the rows where the tie rule and its
    reverse agree: there the order of addresses cannot matter."""
    assert os.path.exists(rc.ORB_BIN_SAN)
    compared = 0
    for c in rc.ORB_CASES:
        out = orb.inputs(rc.make_orb_inputs(c), c.name + "_san", binary=rc.ORB_BIN_SAN)
        want = orb(c.name)[1]
        assert set(out) == set(want)
        if c.committed and tie_free(orb, c.name):
            assert not pu.differing(out, want, list(want)), c.name
            compared += 1
    assert compared >= 3


@needs_binary
@pytest.mark.parametrize("name", COMMITTED)
def test_committed_fixture_is_what_the_binary_writes(orb, name, tmp_path):
    import sys
    sys.path.insert(0, os.path.join(rc.ROOT, "tests", "golden"))
    import make_ref_shim
    inp, want = orb(name)
    finp, fout = rc.load_orb_fixture(name)
    assert set(finp) == set(inp) and not pu.differing(finp, inp, list(inp)), f"{name}: the fixture's inputs are not the table's"
    assert set(fout) == set(want) and not pu.differing(fout, want, list(want)), f"{name}: the fixture is not what the binary writes today"
    again = os.path.join(str(tmp_path), name + ".npz")
    make_ref_shim.save_npz(again, **make_ref_shim.orb_arrays(rc.orb_case(name), str(tmp_path)))
    assert open(again, "rb").read() == open(os.path.join(rc.ORB_FIXTURE_DIR, name + ".npz"), "rb").read(), "the fixture does not regenerate byte for byte"


# ---- no binary needed -------------------------------------------------------------------------------------------------------
def test_every_case_has_its_fixture_and_every_fixture_is_small():
    have = sorted(os.path.splitext(f)[0] for f in os.listdir(rc.ORB_FIXTURE_DIR))
    assert have == sorted(COMMITTED)
    largest = max(os.path.getsize(os.path.join(rc.FIXTURE_DIR, f)) for f in os.listdir(rc.FIXTURE_DIR) if f.endswith(".npz"))
    assert all(os.path.getsize(os.path.join(rc.ORB_FIXTURE_DIR, f + ".npz")) <= largest for f in have)
    for f in have:   # arrays only: numeric dtypes, nothing pickled, no text
        z = np.load(os.path.join(rc.ORB_FIXTURE_DIR, f + ".npz"), allow_pickle=False)
        assert all(z[k].dtype in (np.uint8, np.int32, np.float32) for k in z.files)


def test_no_file_of_the_repository_holds_the_references_table():
    """the repository does not contain bit_pattern_31_.  The patterns the fixtures carry are the tests' own."""
    for name in COMMITTED:
        inp, _ = rc.load_orb_fixture(name)
        if "pattern" in inp:
            c = rc.orb_case(name)
            assert pu.same_bits(inp["pattern"], np.ascontiguousarray(rc.orb_pattern(c.pattern), np.int32))


@pytest.mark.parametrize("name", COMMITTED)
def test_cpu_side_reproduces_the_committed_reference_outputs(libs, name):
    inp, want = rc.load_orb_fixture(name)
    check_cpu_side(libs, inp, want, name)


# ---- the definitions: one each (oracle/pagk_oracle_cv.h); the restatements' own copies are held byte-equal to them ---------
def _level_set():
    """Every level image of every committed row, from the fixtures."""
    out = []
    for name in COMMITTED:
        inp, want = rc.load_orb_fixture(name)
        out += [(name, l, img) for l, img in enumerate(pu.level_images(want))]
    return out


def test_fast_definition_equals_the_restatements_copy(libs):
    """pagk_oracle_fast9 over the cells of the grid, with the fall-back pass, against fdr_cells (tests/fast_detect_ref.c)."""
    for name, l, img in _level_set():
        g, xy, score = fu.model_grid(*img.shape[::-1]), [], []
        for (i, j, x0, y0, x1, y1) in g["cells"]:
            k = orc.fast9(img[y0:y1, x0:x1], fu.INI_TH)
            if not len(k):
                k = orc.fast9(img[y0:y1, x0:x1], fu.MIN_TH)
            xy += [(x + x0 - 16, y + y0 - 16) for x, y, _ in k.tolist()]
            score += k[:, 2].tolist()
        want = fu.ref_cells(libs.fast, img)
        assert pu.same_bits(np.array(xy, F).reshape(-1, 2), want["xy"]) and pu.same_bits(np.array(score, np.int32), want["score"]), (name, l)


def test_resize_blur_and_border_definitions_equal_the_restatements_copies(libs):
    for name, l, img in _level_set():
        assert pu.same_bits(orc.blur7(img), ou.ref_blur(libs.orb, img)) and pu.same_bits(orc.blur7(img), ou.model_blur(img)), (name, l)
        assert pu.same_bits(orc.border_reflect101(img, 19), np.pad(img, 19, mode="reflect")), (name, l)
        assert (orc.border_reflect101(img, 19, 0xA5)[:19] == 0xA5).all()
    for name in COMMITTED:
        _, want = rc.load_orb_fixture(name)
        lv = pu.level_images(want)
        for a, b in zip(lv, lv[1:]):
            assert pu.same_bits(orc.resize_linear(a, b.shape[1], b.shape[0]), lu.ref_resize(libs.levels, a, b.shape[1], b.shape[0])), name
            assert pu.same_bits(orc.resize_linear(a, b.shape[1], b.shape[0]), b), name
    odd = rc.orb_image("97x80 noise3")
    assert pu.same_bits(orc.resize_linear(odd[:, :95], 1, 1), lu.ref_resize(libs.levels, odd[:, :95], 1, 1))
    assert pu.same_bits(orc.resize_linear(odd, 200, 150), lu.ref_resize(libs.levels, odd, 200, 150))     # upscaling: the single-tap columns


def test_fast_atan2_definition_equals_the_restatements_copy(libs):
    rng = np.random.default_rng(5)
    pairs = [(y, x) for y in (-3.0, -1.0, 0.0, 1.0, 2.0) for x in (-2.0, -1.0, 0.0, 1.0, 3.0)] + rng.integers(-400000, 400000, (4000, 2)).astype(F).tolist()
    for y, x in pairs:
        a = orc.fast_atan2(y, x)
        assert a.tobytes() == F(libs.orb.orb_ref_fast_atan2(y, x)).tobytes() == ou.model_fast_atan2(y, x).tobytes(), (y, x)


def test_sine_and_cosine_definition_equals_the_restatements_copy(libs):
    """36001 angles over [0, 360] degrees, as computeOrbDescriptor forms them (:136)."""
    import ctypes as C
    a, b = C.c_float(0), C.c_float(0)
    for k in range(36001):
        r = F(F(k / 100.0) * ou.FACTOR_PI)
        libs.orb.orb_ref_cos_sin(r, C.addressof(a), C.addressof(b))
        sn, cs = orc.sin_cos(float(r))
        assert F(cs).tobytes() == F(a.value).tobytes() and F(sn).tobytes() == F(b.value).tobytes(), k


def test_pow_definition_narrows_like_the_hosts_pow():
    """pow((double)factor, (double)nlevels) of :461 is narrowed to float at once: for 1 to 8 levels and every scale factor of the
    table -- and a sweep of others -- the repeated product and the host's pow give the same float."""
    factors = sorted({float(c.scale) for c in rc.ORB_CASES} | {1.0 + k / 64.0 for k in range(1, 33)})
    for sf in factors:
        factor = F(F(1) / F(sf))
        for n in range(1, 9):
            assert F(orc.pow_int(float(factor), n)).tobytes() == F(math.pow(float(factor), n)).tobytes(), (sf, n)
    assert orc.pow_int(0.5, 2.5) is None and orc.pow_int(0.5, -1) is None and orc.pow_int(0.5, 0) == 1.0
