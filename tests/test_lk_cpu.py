"""CPU tests of pyramidal Lucas-Kanade (tracker type 0): the plain-C restatement (tests/lk_ref.c) against an independent
numpy model of the definition in include/pagk.h ("Pyramidal Lucas-Kanade"), byte for byte, on every shape the GPU tests use
(both tables); which exits of the level loop those shapes take; what every parameter case changes; hand-checkable cases of
the pyramid, the derivatives and the tracker; ground truth on a shifted texture; the boundary (header, bindings, argument
checks that need no device)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lk_ref_util as lu
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pagk_lk_params_default", "pagk_lk_params_check", "pagk_lk_levels", "pagk_lk_pyramid_device",
                "pagk_lk_track_device", "pagk_lk_track", "pagk_selftest_lk_level")
F = np.float32


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return lu.build_ref(tmp_path_factory.mktemp("lk_ref"))


@pytest.fixture(scope="module")
def shapes():
    return lu.shapes(synth)


@pytest.fixture(scope="module")
def edges():
    return lu.edge_shapes(synth)


@pytest.fixture(scope="module")
def restated(ref, shapes, edges):
    """name (of either table) -> the restatement of that case, computed once and left unchanged."""
    memo = {}

    def get(name):
        if name not in memo:
            c = shapes[name] if name in shapes else edges[name]
            memo[name] = lu.ref_track(ref, c["ref"], c["cur"], c["pts"], c["p"], c["cap"], c["n"])
        return memo[name]
    return get


# ---- the boundary --------------------------------------------------------------------------------------------------------
def test_header_declares_and_capi_binds_the_entry_points(built):
    hdr = open(os.path.join(ROOT, "include", "pagk.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = capi.load()
    for name in ENTRY_POINTS:
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name) and getattr(lib, name).argtypes, name
        assert re.search(r"\b(?:int|void) " + name + r"\s*\(", code), name
        # every declaration cites the reference lines it stands for, directly above it
        decl = re.search(r"\b(?:int|void) " + name + r"\(", hdr).start()
        comment = hdr[:decl].rsplit("/*", 1)[1]
        assert "src/gyro_aided_tracker.cpp:353-380" in comment and comment.rstrip().endswith("*/"), name
    begin = hdr[hdr.index("hipGraph capture of the per-frame work"):hdr.index("int pagk_graph_begin")]
    assert "pagk_lk_pyramid_device" in begin and "pagk_lk_track_device" in begin
    for word in ("NOT claimed", "tests/lk_ref.c", "EXACT integers", "0x1p-20f", "FLT_EPSILON"):     # the definition stands here
        assert word in hdr, word
    assert [f[0] for f in capi.LkParams._fields_] == ["half_patch", "max_level", "max_count", "epsilon", "min_eig_threshold",
                                                      "err_threshold"]
    assert C.sizeof(capi.LkParams) == 40
    d = capi.lk_params_default()
    assert (d.half_patch, d.max_level, d.max_count, d.epsilon, d.min_eig_threshold, d.err_threshold) == (10, 2, 30, 0.01, 1e-4, 12.0)
    for meth in ("lk_pyramid_device", "lk_track_device", "lk_track", "selftest_lk_level"):
        assert callable(getattr(capi.Context, meth))


def test_lk_levels(built, ref):
    h = lambda hp, **kw: capi.lk_params_default(half_patch=hp, **kw)     # noqa: E731
    assert capi.lk_levels(96, 64, h(10)) == 1            # level 2 would be 24 x 16: not larger than 21
    assert capi.lk_levels(40, 24, h(10)) == 0
    assert capi.lk_levels(48, 36, h(2)) == 2
    assert capi.lk_levels(21, 40, h(10)) == capi.PAGK_E_ARG
    assert capi.lk_levels(40, 21, h(10)) == capi.PAGK_E_ARG
    assert capi.lk_levels(752, 480, h(10, max_level=0)) == 0
    assert capi.lk_levels(752, 480, h(10)) == 2
    assert capi.lk_levels(752, 480, h(10, max_level=7)) == 4          # 47 x 30 at level 4, 24 x 15 at level 5
    assert capi.lk_levels(752, 480, h(0)) == capi.PAGK_E_ARG
    for w, hh, hp, ml in ((96, 64, 10, 2), (40, 24, 10, 2), (48, 36, 2, 2), (21, 40, 10, 2), (33, 31, 1, 7), (160, 120, 15, 2)):
        got = capi.lk_levels(w, hh, h(hp, max_level=ml))
        assert (got if got >= 0 else -1) == ref.lk_ref_levels(w, hh, hp, ml) == lu.model_levels(w, hh, hp, ml)


def test_lk_params_check_refuses_each_bad_field(built):
    assert capi.lk_params_check(capi.lk_params_default()) == capi.PAGK_OK
    assert capi.lk_params_check(capi.lk_params_default(half_patch=1, max_level=0, max_count=1, epsilon=0.0, min_eig_threshold=0.0,
                                                       err_threshold=0.0)) == capi.PAGK_OK
    assert capi.lk_params_check(capi.lk_params_default(half_patch=15, max_level=7)) == capi.PAGK_OK
    bad = [dict(half_patch=0), dict(half_patch=16), dict(max_level=-1), dict(max_level=8), dict(max_count=0),
           dict(epsilon=-1e-9), dict(epsilon=float("nan")), dict(epsilon=float("inf")), dict(min_eig_threshold=-1.0),
           dict(min_eig_threshold=float("nan")), dict(err_threshold=-1.0), dict(err_threshold=float("nan")),
           dict(err_threshold=float("inf"))]
    for kw in bad:
        assert capi.lk_params_check(capi.lk_params_default(**kw)) == capi.PAGK_E_ARG, kw
    assert capi.load().pagk_lk_params_check(None) == capi.PAGK_E_ARG
    with pytest.raises(TypeError):
        capi.lk_params_default(window=3)


def test_every_entry_point_refuses_without_a_context(built):
    lib = capi.load()
    p = capi.lk_params_default()
    one = np.zeros(16, np.float32)
    img = capi.image_view(np.zeros((64, 64), np.uint8))
    a = one.ctypes.data
    assert lib.pagk_lk_pyramid_device(None, C.byref(p), 0) == capi.PAGK_E_ARG
    assert lib.pagk_lk_track_device(None, C.byref(p), 0, 1, 4, a, None, a, a, None, a, None, a) == capi.PAGK_E_ARG
    assert lib.pagk_lk_track(None, C.byref(p), C.byref(img), C.byref(img), 1, a, a, a, None, a, None, None) == capi.PAGK_E_ARG
    assert lib.pagk_selftest_lk_level(None, 0, 1, a, 64) == capi.PAGK_E_ARG
    assert lib.pagk_lk_levels(64, 64, None) == capi.PAGK_E_ARG


# ---- restatement against model ---------------------------------------------------------------------------------------------
def test_restatement_and_model_agree_on_every_shape(ref, shapes):
    seen = np.zeros(lu.INFO_WORDS, np.int64)
    for name, c in shapes.items():
        r = lu.ref_track(ref, c["ref"], c["cur"], c["pts"], c["p"], c["cap"], c["n"])
        m = lu.model_track(c["ref"], c["cur"], c["pts"], c["p"], c["cap"], c["n"])
        assert lu.differing(r, m, lu.KEYS + ("iters", "why")) == [], name
        la, lb = lu.ref_levels(ref, c["ref"], c["p"]), [c["ref"]]
        for _ in range(len(la) - 1):
            lb.append(lu.model_pyrdown(lb[-1]))
        assert all(np.array_equal(x, y) for x, y in zip(la, lb)), name
        assert r["info"][0] == (len(c["pts"]) if c["n"] is None else c["n"]) and np.all(r["info"][6:] == 0)
        assert r["info"][1] == r["status_raw"].sum() and r["info"][2] == r["status"].sum()
        seen += r["info"]
        seen[6] += int(r["iters"].max() == c["p"]["max_count"])
    # the shapes reach every rule: lost to either test, dropped by the error filter, stopped by the iteration count
    assert seen[4] > 0 and seen[5] > 0 and seen[1] > seen[2] > 0 and seen[6] > 0


def test_shapes_are_what_the_table_says(ref, shapes):
    tops = {name: lu.ref_track(ref, c["ref"], c["cur"], c["pts"][:1], c["p"])["info"][3] for name, c in shapes.items()}
    assert list(tops.values()) == [2, 1, 0, 2, 1, 2]
    c = shapes["48x36 h2: three levels, borders, non-finite"]
    r = lu.ref_track(ref, c["ref"], c["cur"], c["pts"], c["p"])
    pts = c["pts"]
    nonfinite = ~np.isfinite(pts).all(axis=1) | (np.abs(pts) > 1e8).any(axis=1)
    assert nonfinite.sum() == 3 and not r["status_raw"][nonfinite].any() and not r["err"][nonfinite].any()
    assert r["status_raw"][8] == 0 and r["status_raw"][10] == 0 and r["status_raw"][12] == 0 and r["status_raw"][14] == 0
    c = shapes["160x120 h5: cap 300, count 257"]
    r = lu.ref_track(ref, c["ref"], c["cur"], c["pts"], c["p"], c["cap"], c["n"])
    for k in ("pt_out", "status", "status_raw", "err", "flow"):
        assert not r[k][257:].any(), k
    z = lu.ref_track(ref, c["ref"], c["cur"], c["pts"], c["p"], c["cap"], 0)
    assert z["info"].tolist() == [0, 0, 0, 2, 0, 0, 0, 0] and not z["pt_out"].any() and not z["status"].any()


# ---- the edge table ------------------------------------------------------------------------------------------------------
def _npix(win: int) -> int:
    """lk_npix of csrc/pagk_lk_kernel.h."""
    return 1 if win <= 7 else 2 if win <= 11 else 4 if win <= 15 else 8 if win <= 21 else 16


def _chain(src: str, name: str):
    """`constexpr int name(int v) { return v OP n ? a : v OP m ? b : ... : z; }` of the kernel header as a Python function."""
    var, expr = re.search(r"constexpr int " + name + r"\(int (\w+)\) \{ return ([^;]*); \}", src).groups()
    *tests, last = [part.strip() for part in expr.split(":")]
    steps = [re.fullmatch(r"(\w+) (<=|==) (\d+) \? (\d+)", t).groups() for t in tests]
    assert all(v == var for v, _, _, _ in steps)

    def f(x: int) -> int:
        for _, op, bound, val in steps:
            if (x <= int(bound)) if op == "<=" else (x == int(bound)):
                return int(val)
        return int(last)
    return f


def test_the_chooser_gives_every_window_its_instantiation():
    """lk_npix, lk_max_win and the switch of lk_kernel, read from the source: every instantiation with 64 NPIX >= win^2 computes
    the same exact sums, so which of them a window launches cannot be seen in any output.  It is pinned here: the smallest
    power of two that holds the window, a tile sized for the largest window of that instantiation, one case per NPIX; and
    the edge table runs both ends of every range."""
    csrc = os.path.join(ROOT, "pixel_aware_gyro_aided_klt_feature_tracker_amd", "csrc")
    hdr = open(os.path.join(csrc, "pagk_lk_kernel.h")).read()
    npix, max_win = _chain(hdr, "lk_npix"), _chain(hdr, "lk_max_win")
    wins = range(3, 32, 2)                                              # half patches 1 .. PAGK_MAX_HALF_PATCH
    for win in wins:
        want = next(n for n in (1, 2, 4, 8, 16) if 64 * n >= win * win)
        assert npix(win) == want == _npix(win), win
    for n in (1, 2, 4, 8, 16):
        served = [win for win in wins if npix(win) == n]
        assert max_win(n) == max(served), n                              # (the tile of k_lk_track<n>: (max_win + 3)^2 bytes)
        assert lu.NPIX_OF_WIN[min(served)] == lu.NPIX_OF_WIN[max(served)] == n
    assert len(lu.NPIX_OF_WIN) == 10 and re.search(r"constexpr int kLkMaxWin = 31;", hdr)
    host = open(os.path.join(csrc, "pagk_hip.hip")).read()
    switch = host[host.index("LkKernel lk_kernel(int win)"):host.index("int lk_track_slots(")]
    assert "switch (lk_npix(win))" in switch
    assert re.findall(r"case (\d+): return k_lk_track<(\d+)>;", switch) == [(str(n), str(n)) for n in (1, 2, 4, 8)]
    assert re.findall(r"default: return k_lk_track<(\d+)>;", switch) == ["16"]
    assert "hipLaunchKernelGGL(lk_kernel(a.win)," in host


def test_restatement_and_model_agree_on_every_edge_case(ref, edges, restated):
    for name, c in edges.items():
        r = restated(name)
        m = lu.model_track(c["ref"], c["cur"], c["pts"], c["p"], c["cap"], c["n"])
        assert lu.differing(r, m, lu.KEYS + ("iters", "why")) == [], name
        assert r["info"][0] == len(c["pts"]) and np.all(r["info"][6:] == 0), name
        assert r["info"][1] == r["status_raw"].sum() and r["info"][2] == r["status"].sum(), name
        top = r["info"][3]
        assert not r["why"][:, top + 1:].any(), name                       # nothing above the top level
        assert np.all(r["why"][:, :top + 1] > 0), name                     # every feature passes through every level
        assert np.all((r["why"][:, 0] >= lu.RANGE) | (r["status_raw"] == 0)), name
        assert np.all(r["why"][r["iters"] > 0, 0] >= lu.RANGE) and np.all(r["iters"][r["why"][:, 0] > lu.RANGE] > 0), name


def test_edge_table_is_what_it_says(ref, edges, restated):
    wins = {}
    for name, c in edges.items():
        h, w = c["ref"].shape
        win = 2 * c["p"]["half_patch"] + 1
        assert w <= 160 and h <= 128 and len(c["pts"]) <= 64 and c["cur"].shape == (h, w), name
        assert c["npix"] == _npix(win) and (not name.startswith("win") or f"win{win} npix{c['npix']} " in name), name
        top = restated(name)["info"][3]
        if "minimal" in name:
            assert (w, h) == (win + 1, win + 1) and c["p"]["max_level"] == 0 and top == 0 and c["host"], name
            wins.setdefault(win, set()).add("minimal")
        if "three levels" in name:
            assert top == 2 and c["host"] == (c["npix"] == 4), name
            wins.setdefault(win, set()).add("three levels")
        for word, want in (("top 3", 3), ("top 4", 4), ("max_level=0", 0), ("max_level=1", 1), ("96x80 defaults", 2)):
            if word in name:
                assert top == want, name
        ints = (c["pts"] == np.rint(c["pts"])).all(axis=1)
        assert ints.sum() >= 4 and (~ints).sum() >= 4, name               # integer and fractional coordinates in every case
    # both ends of every instantiation's window range, each on both frames
    assert wins == {win: {"minimal", "three levels"} for win in (3, 7, 9, 11, 13, 15, 17, 21, 23, 31)}
    assert sorted(wins) == sorted(lu.NPIX_OF_WIN) and all(_npix(w) == n for w, n in lu.NPIX_OF_WIN.items())
    assert sum(~np.isfinite(c["pts"]).all(axis=1).any() for c in edges.values()) < len(edges)     # some cases without NaN ...
    assert sum(np.isnan(c["pts"]).any() for c in edges.values()) >= 8                             # ... and some with
    c = edges["p7 160x128 max_level=1 over pyramids of 3"]
    assert ref.lk_ref_levels(160, 128, 7, c["pyr"]["max_level"]) == 3 and c["p"]["max_level"] == 1
    for name in ("p7 96x80 pitches 29 and 3", "p7 96x80 pitches 3 and 29"):
        assert sorted(edges[name]["pitch"]) == [96 + 3, 96 + 29]
    assert edges["p7 96x80 pitches 29 and 3"]["pitch"] == edges["p7 96x80 pitches 3 and 29"]["pitch"][::-1]


def test_every_exit_of_the_level_loop_is_taken(shapes, edges, restated):
    """Coverage conditions over the two tables, on the restatement alone: every code 1 .. 6 of `why` in at least 3 features at
    level 0 and in at least 3 features at some level above 0 (no code had to be excused: template out of range, step 5, out
    of range inside the iteration, epsilon, oscillation and count are all reached above level 0 as well); in every NPIX group
    at least 8 features end with raw status 1 and at least one with 0."""
    level0, above = np.zeros(7, np.int64), np.zeros(7, np.int64)
    ended = {n: [0, 0] for n in (1, 2, 4, 8, 16)}
    for name, c in list(shapes.items()) + list(edges.items()):
        r = restated(name)
        n = int(r["info"][0])
        why = r["why"][:n]
        for code in range(1, 7):
            level0[code] += int((why[:, 0] == code).sum())
            above[code] += int((why[:, 1:] == code).any(axis=1).sum())
        g = ended[_npix(2 * c["p"]["half_patch"] + 1)]
        g[1] += int(r["status_raw"][:n].sum())
        g[0] += n - int(r["status_raw"][:n].sum())
    print("why at level 0:", level0[1:].tolist(), "above level 0:", above[1:].tolist(), "ended with 0 / 1 per NPIX:", ended)
    for code in range(1, 7):
        assert level0[code] >= 3, code
        assert above[code] >= 3, code
    for npix, (lost, tracked) in ended.items():
        assert tracked >= 8 and lost >= 1, npix


def test_every_parameter_case_changes_what_it_is_meant_to(edges, restated):
    base = restated("p7 96x80 defaults")
    get = lambda tail: restated("p7 96x80 " + tail)     # noqa: E731
    for name, c in edges.items():
        if c["base"]:                                     # the same frame and features as the default run
            b = edges[c["base"]]
            assert c["ref"] is b["ref"] and c["cur"] is b["cur"] and c["pts"] is b["pts"], name
    iterated = lambda r: r["why"] >= lu.RANGE             # noqa: E731
    assert base["iters"].max() > 2 and (base["why"] == lu.EPSILON).any() and (base["why"] == lu.OSCILLATION).any()
    r = get("max_count=1")
    assert r["iters"].max() == 1 and np.all(np.isin(r["why"][iterated(r)], (lu.RANGE, lu.EPSILON, lu.COUNT)))
    assert (r["why"] == lu.COUNT).any() and not (r["why"] == lu.OSCILLATION).any()
    r = get("max_count=2")
    assert r["iters"].max() == 2 and (r["why"] == lu.COUNT).any() and lu.differing(r, get("max_count=1")) != []
    r = get("epsilon=0")
    assert not (r["why"] == lu.EPSILON).any() and (r["why"] == lu.OSCILLATION).sum() > (base["why"] == lu.OSCILLATION).sum()
    r = get("epsilon=1")
    assert iterated(r).any() and np.all(np.isin(r["why"][iterated(r)], (lu.RANGE, lu.EPSILON)))
    assert (r["why"] == lu.EPSILON).sum() > (base["why"] == lu.EPSILON).sum()
    lo, hi = get("min_eig_threshold=0"), get(f"min_eig_threshold={lu.MIN_EIG_HALF:g}")
    assert lo["info"][4] < base["info"][4] < hi["info"][4]
    reach = int((base["why"][:, 0] >= lu.MIN_EIG).sum())                      # features that come to step 5 at level 0
    assert 0.4 * reach <= hi["info"][4] <= 0.6 * reach                         # "roughly half"
    r = get("err_threshold=0")
    assert r["info"][2] == 0 and r["info"][1] == base["info"][1] > 0 and not r["status"].any()
    assert lu.differing(r, base, ("pt_out", "status_raw", "err", "flow")) == []
    r = get(f"err_threshold={lu.ERR_NEVER:g}")
    assert r["info"][2] == r["info"][1] == base["info"][1] > base["info"][2] and r["err"].max() < lu.ERR_NEVER
    assert [get(f"max_level={l}")["info"][3] for l in (0, 1)] == [0, 1] and base["info"][3] == 2
    assert lu.differing(get("max_level=0"), base) != [] and lu.differing(get("max_level=1"), base) != []
    for name in ("p7 96x80 pitches 29 and 3", "p7 96x80 pitches 3 and 29"):   # a pitch changes nothing
        assert lu.differing(restated(name), base, lu.KEYS + ("iters", "why")) == []
    deep, cut = restated("p7 160x128 max_level=7: top 3"), restated("p7 160x128 max_level=1 over pyramids of 3")
    assert deep["info"][3] == 3 and cut["info"][3] == 1 and lu.differing(deep, cut) != []
    assert restated("p2 136x120 max_level=7: top 4")["info"][3] == 4


def test_extreme_contrast_reaches_the_integer_bounds(ref, edges, restated):
    """The 0 / 255 squares reach the largest derivative of the definition, 4080, in both directions, and the largest
    difference, 8160, at a tracked feature with a = b = 0."""
    for hp in (7, 15):
        c = edges[f"checker h{hp} inverse"]
        assert set(np.unique(c["ref"])) == {0, 255} and np.array_equal(c["cur"], 255 - c["ref"])
        one = edges[f"checker h{hp} one pixel"]
        assert np.array_equal(one["ref"], c["ref"])
        assert np.array_equal(one["cur"][:, 1:], one["ref"][:, :-1]) and c["p"]["max_level"] == one["p"]["max_level"] == 1
        for img in (c["ref"], c["cur"], one["cur"]):
            dx, dy = lu.ref_scharr(ref, img)
            assert np.abs(dx).max() == 4080 and np.abs(dy).max() == 4080
        # level 0 alone: at its first iteration a feature on integer coordinates reads J exactly where its template read I,
        # with a = b = 0, iw = (16384, 0, 0, 0): Ival = 32 I, the sample of J = 32 J, diff = 32 (J - I) = +-8160 everywhere
        c = edges[f"checker h{hp} inverse level 0"]
        r = restated(f"checker h{hp} inverse level 0")
        win = 2 * hp + 1
        weights = lu._weights(lu.F(0), lu.F(0))
        assert weights == (16384, 0, 0, 0)
        I, J = lu._Level(c["ref"], win), lu._Level(c["cur"], win)
        ints = (c["pts"] == np.rint(c["pts"])).all(axis=1)
        tracked = np.flatnonzero(ints & (r["why"][:, 0] > lu.RANGE))          # came through the first iteration
        assert len(tracked) >= 3
        for k in tracked:
            x0, y0 = int(c["pts"][k, 0]) - hp, int(c["pts"][k, 1]) - hp
            diff = ((J.window(J.gray, x0, y0, win, weights) + 256) >> 9) - ((I.window(I.gray, x0, y0, win, weights) + 256) >> 9)
            assert np.abs(diff).max() == 8160 and np.abs(diff).min() == 8160, k
        assert r["status_raw"][tracked].any()                                 # and some of them end with raw status 1


def test_pyramid_shapes_cover_the_grid_of_the_kernel(ref):
    """Level widths 63, 64, 65, 128, 129; level heights of every residue modulo 4 from an even and from an odd parent; the
    restatement and the model agree on every level."""
    p = lu.params(half_patch=1, max_level=7)
    widths, heights, wparents = set(), set(), set()
    for name, img in lu.pyramid_shapes().items():
        levels = lu.ref_levels(ref, img, p)
        assert len(levels) >= 2, name
        for l in range(1, len(levels)):
            ph, pw = levels[l - 1].shape
            h, w = levels[l].shape
            widths.add(w), heights.add((h % 4, ph % 2)), wparents.add(pw % 2)
            assert np.array_equal(levels[l], lu.model_pyrdown(levels[l - 1])), (name, l)
    assert {63, 64, 65, 128, 129} <= widths and wparents == {0, 1}
    assert heights == {(r, par) for r in range(4) for par in range(2)}


# ---- hand-checkable cases ------------------------------------------------------------------------------------------------
def test_pyrdown_by_hand(ref):
    for img in (np.full((9, 12), 77, np.uint8), np.full((7, 5), 255, np.uint8), np.zeros((4, 4), np.uint8)):
        out = lu.ref_pyrdown(ref, img)
        assert out.shape == ((img.shape[0] + 1) // 2, (img.shape[1] + 1) // 2) and np.all(out == img[0, 0])
        assert np.array_equal(out, lu.model_pyrdown(img))
    # an impulse at an even position (2, 2) of a 5 x 5 image meets the kernel's centre for output (1, 1) and its outer taps
    # for the neighbours: the outputs are the 2-D kernel at offsets 2 (x - 1), 2 (y - 1), the border taps folded back in
    imp = np.zeros((5, 5), np.uint8)
    imp[2, 2] = 255
    w = np.array([1, 4, 6, 4, 1])
    fold = np.array([w[0] + w[4], w[2], w[0] + w[4]])         # outputs 0 and 2 see it through tap 4 or 0 and once more through r()
    expect = (255 * np.outer(fold, fold) + 128) >> 8
    assert np.array_equal(lu.ref_pyrdown(ref, imp), expect)
    full = np.zeros((5, 5), np.int64)                         # and the whole kernel, read off impulses at all 25 positions
    for y in range(5):
        for x in range(5):
            big = np.zeros((13, 13), np.uint8)
            big[4 + y, 4 + x] = 255
            full[y, x] = lu.ref_pyrdown(ref, big)[3, 3]       # output (3, 3) reads rows / columns 4 .. 8
    assert np.array_equal(full, (255 * np.outer(w, w) + 128) >> 8)
    # odd width and height: the last output column reads r(W + 1) = W - 3
    odd = np.arange(7 * 9, dtype=np.uint8).reshape(7, 9) * 3
    got = lu.ref_pyrdown(ref, odd)
    cols = [6, 7, 8, 7, 6]                                     # columns 6 .. 10 through r()
    rows = [4, 5, 6, 5, 4]
    s = sum(int(w[i]) * int(w[j]) * int(odd[rows[j], cols[i]]) for i in range(5) for j in range(5))
    assert got.shape == (4, 5) and got[3, 4] == (s + 128) >> 8
    assert np.array_equal(got, lu.model_pyrdown(odd))


def test_scharr_of_a_ramp_by_hand(ref):
    slope = 3
    ramp = np.tile((10 + slope * np.arange(20)).astype(np.uint8), (11, 1))
    dx, dy = lu.ref_scharr(ref, ramp)
    assert np.all(dy == 0)
    assert np.all(dx[:, 1:-1] == 32 * slope)                  # (3 + 10 + 3) * 2 * slope
    assert np.all(dx[:, 0] == 0) and np.all(dx[:, -1] == 0)   # r(-1) = 1 and r(W) = W - 2: both neighbours are the same pixel
    mx, my = lu.model_scharr(ramp)
    assert np.array_equal(dx, mx) and np.array_equal(dy, my)
    dx, dy = lu.ref_scharr(ref, ramp.T.copy())
    assert np.all(dx == 0) and np.all(dy[1:-1, :] == 32 * slope) and np.all(dy[0] == 0) and np.all(dy[-1] == 0)
    noise = np.random.default_rng(3).integers(0, 256, (13, 17), dtype=np.uint8)
    dx, dy = lu.ref_scharr(ref, noise)
    mx, my = lu.model_scharr(noise)
    assert np.array_equal(dx, mx) and np.array_equal(dy, my) and max(np.abs(mx).max(), np.abs(my).max()) <= 4080


def test_flat_patch_fails_the_min_eigenvalue_test(ref):
    a, b = lu.texture_pair(synth, 64, 48, 5)
    a[10:40, 10:50] = 90
    p = lu.params(half_patch=5, max_level=0)
    r = lu.ref_track(ref, a, b, np.array([[30, 25], [50.5, 8.25]], np.float32), p)
    assert r["status_raw"].tolist() == [0, 1] and r["err"][0] == 0 and r["info"][4] == 1 and r["info"][5] == 0
    assert np.array_equal(r["pt_out"][0], [30, 25]) and r["iters"][0] == 0


def test_identical_pair_stays_put_after_one_iteration(ref):
    a, _ = lu.texture_pair(synth, 96, 64, 6)
    pts = lu.interior_points(96, 64, 24, 12, 7)
    for hp in (2, 10):
        r = lu.ref_track(ref, a, a, pts, lu.params(half_patch=hp))
        assert np.all(r["status_raw"] == 1) and np.all(r["iters"] == 1)
        assert lu.same_array(r["pt_out"], pts) and not r["err"].any() and not r["flow"].any()


def test_range_rule_at_its_edges(ref):
    # a template whose corner floors to -win or to W - 1 exactly is in range, half a pixel further it is not.  In range there
    # means: at most one column or row of the window has derivatives (they are zero outside the level), so the feature goes on
    # to the conditioning test and is lost there -- the two counters tell the cases apart
    a, _ = lu.texture_pair(synth, 48, 36, 8)
    win, half = 5, 2.0
    pts = np.array([(-win + half, 18), (-win + half - 0.5, 18), (47 + half, 18), (48 + half, 18), (24, -win + half),
                    (24, -win + half - 0.5), (24, 35 + half), (24, 36 + half)], np.float32)
    r = lu.ref_track(ref, a, a, pts, lu.params(half_patch=2, max_level=0))
    assert not r["status_raw"].any() and r["info"][4] == 4 and r["info"][5] == 4
    assert lu.same_array(r["pt_out"], pts) and not r["err"].any()
    for k in range(8):
        one = lu.ref_track(ref, a, a, pts[k:k + 1], lu.params(half_patch=2, max_level=0))["info"]
        assert (one[4], one[5]) == ((1, 0) if k % 2 == 0 else (0, 1)), k


# ---- ground truth --------------------------------------------------------------------------------------------------------
SHIFT = (1.37, -0.62)
REACHED_MEDIAN = 0.0133        # px, the restatement on this scene (0.01334)
BOUND_MEDIAN = 2 * REACHED_MEDIAN


def test_restatement_tracks_a_known_translation(ref):
    a, b = lu.texture_pair(synth, 160, 120, 31, SHIFT)
    pts = lu.interior_points(160, 120, 64, 16, 32)
    r = lu.ref_track(ref, a, b, pts, lu.params(half_patch=5))
    kept = r["status"] > 0
    d = np.hypot(*(r["pt_out"].astype(np.float64) - (pts.astype(np.float64) + np.array(SHIFT))).T)
    print(f"kept {kept.sum()} of 64, median distance {np.median(d[kept]):.4f} px, largest {d[kept].max():.4f} px")
    assert kept.sum() >= 0.9 * 64
    assert np.median(d[kept]) < BOUND_MEDIAN
    assert lu.differing(r, lu.model_track(a, b, pts, lu.params(half_patch=5))) == []


# ---- sanitizers ----------------------------------------------------------------------------------------------------------
def test_restatement_runs_clean_under_the_sanitizers(tmp_path):
    """A stand-alone program (tests/lk_sanitize.c: its own main, compiled together with tests/lk_ref.c) tracks features on and
    beyond every border, NaN, infinite and huge coordinates included, under AddressSanitizer and UBSan; each image sits in a
    heap block of exactly its size, so that a read outside it is an error."""
    exe = str(tmp_path / "lk_sanitize")
    subprocess.run(["gcc", "-std=c99", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "lk_sanitize.c"),
                    os.path.join(ROOT, "tests", "lk_ref.c"), "-o", exe, "-lm"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "4 images" in r.stdout, r.stdout
