"""CPU tests of the FAST-cells-and-quadtree detector's ground truth: the plain-C restatement (tests/fast_detect_ref.c)
against an independent numpy model of the definition in include/pagk.h, byte for byte, on every test image; the figures
the images were chosen by; planted truth; the properties of the result; the tie rule; the boundary (header, bindings,
argument checks that need no device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fast_ref_util as fu
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("pagk_fast_params_check", "pagk_detect_fast_bounds", "pagk_detect_fast_device", "pagk_detect_fast",
                    "pagk_frame_handover_fast_device", "pagk_frame_handover_fast", "pagk_selftest_fast_cells")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return fu.build_ref(tmp_path_factory.mktemp("fast_ref"))


@pytest.fixture(scope="module")
def cases():
    return fu.cases(synth)


@pytest.fixture(scope="module")
def results(ref, cases):
    """name -> (restated, model), computed once and left unchanged."""
    memo = {}

    def get(name):
        if name not in memo:
            img, mask, n, _ = cases[name]
            memo[name] = (fu.ref_detect(ref, img, mask, n), fu.model_detect(img, mask, n))
        return memo[name]
    return get


def test_header_declares_and_capi_binds_the_new_entry_points(built):
    hdr = open(os.path.join(ROOT, "include", "pagk.h")).read()
    assert re.search(r"#define PAGK_VERSION (\d+)", hdr).group(1) == "303"
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = capi.load()
    assert re.search(r"\bvoid pagk_fast_params_default\s*\(", code) and hasattr(lib, "pagk_fast_params_default")
    assert code.index("pagk_selftest_corner_response") < code.index("pagk_fast_params") < code.index("pagk_rectify_params")
    for name in NEW_ENTRY_POINTS + ("pagk_fast_params_default",):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name) and getattr(lib, name).argtypes, name
        # every new declaration cites the reference function it stands for, directly above it
        decl = re.search(r"\b(?:int|void) " + name + r"\(", hdr).start()
        comment = hdr[:decl].rsplit("/*", 1)[1]
        assert "src/ORBextractor.cc:1148-1205" in comment and comment.rstrip().endswith("*/"), name
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
    for meth in ("detect_fast_device", "detect_fast", "frame_handover_fast_device", "frame_handover_fast", "selftest_fast_cells"):
        assert callable(getattr(capi.Context, meth))
    begin = hdr[hdr.index("hipGraph capture of the per-frame work"):hdr.index("int pagk_graph_begin")]
    for name in ("pagk_detect_fast_device", "pagk_frame_handover_fast_device", "pagk_detect_corners_device"):
        assert name in begin
    assert "ORBextractor are not provided" not in hdr
    assert [f[0] for f in capi.FastParams._fields_] == ["ini_threshold", "min_threshold", "n_features", "n_levels"]
    assert C.sizeof(capi.FastParams) == 16
    d = capi.fast_params_default()
    assert (d.ini_threshold, d.min_threshold, d.n_features, d.n_levels) == (20, 7, 0, 1)


def test_argument_checks_that_need_no_device(built, ref):
    lib = capi.load()
    ok = capi.fast_params_default(n_features=400)
    assert capi.fast_params_check(ok) == capi.PAGK_OK and capi.fast_params_check(capi.fast_params_default()) == capi.PAGK_OK
    for bad in (dict(ini_threshold=-1), dict(ini_threshold=256), dict(min_threshold=-1), dict(min_threshold=256),
                dict(n_features=-1)):
        assert capi.fast_params_check(capi.fast_params_default(**bad)) == capi.PAGK_E_ARG, bad
    assert capi.fast_params_check(capi.fast_params_default(n_levels=8)) == capi.PAGK_E_UNSUPPORTED
    assert capi.fast_params_check(capi.fast_params_default(n_levels=0)) == capi.PAGK_E_UNSUPPORTED
    assert lib.pagk_fast_params_check(None) == capi.PAGK_E_ARG
    for w, h in ((61, 200), (200, 61), (62, 200)):       # fewer than one cell; nIni = round(30 / 168) = 0
        with pytest.raises(capi.PagkError):
            capi.detect_fast_bounds(w, h, 100)
        assert fu.ref_bounds(ref, w, h, 100) is None and fu.model_bounds(w, h, 100) is None
    with pytest.raises(capi.PagkError):
        capi.detect_fast_bounds(640, 480, 0)
    # without a context every entry point refuses; n_levels = 8 is refused as unsupported wherever the parameters are read
    img = np.zeros((480, 640), np.uint8)
    iv = capi.image_view(img)
    p = capi.make_params(camera=synth.D435I)
    assert lib.pagk_detect_fast_device(None, C.byref(ok), 0, None, 1000, None, None, None) == capi.PAGK_E_ARG
    assert lib.pagk_detect_fast(None, C.byref(ok), C.byref(iv), None, 1000, None, None, None) == capi.PAGK_E_ARG
    assert lib.pagk_selftest_fast_cells(None, C.byref(ok), C.byref(iv), None, None, None) == capi.PAGK_E_ARG
    assert lib.pagk_frame_handover_fast_device(None, C.byref(p), 640, 480, 448, 400, 320.0, None, None, None, C.byref(ok), 0,
                                               None, None, None, None, None, None, None, None) == capi.PAGK_E_ARG
    assert lib.pagk_frame_handover_fast(None, C.byref(p), 640, 480, 448, 400, 320.0, None, None, None, C.byref(ok),
                                        C.byref(iv), None, None, None, None, None, None, None, None) == capi.PAGK_E_ARG


def test_bounds_against_the_models(built, ref):
    for w, h, n in ((62, 62, 20), (97, 80, 50), (91, 62, 5), (320, 240, 100), (640, 480, 400), (640, 480, 1), (752, 480, 1000),
                    (641, 479, 700), (1920, 1080, 20000), (400, 62, 3), (62, 80, 10)):
        got = capi.detect_fast_bounds(w, h, n)
        assert got == fu.ref_bounds(ref, w, h, n) == fu.model_bounds(w, h, n), (w, h, n, got)
    assert capi.detect_fast_bounds(640, 480, 400) == (280 * 16 * 16, 402)
    assert capi.detect_fast_bounds(640, 480, 1) == (280 * 16 * 16, 4)          # the first round's overshoot: 4 * nIni
    assert capi.detect_fast_bounds(400, 62, 3)[1] == 4 * 12                    # nIni = round(368 / 30) = 12
    g = fu.model_grid(91, 62)
    assert (g["w_cell"], g["n_cols"]) == (59, 1)                               # the widest cell
    g = fu.model_grid(1920, 1080)
    assert g["n_cols"] * g["n_rows"] - len(g["cells"]) == g["n_rows"] > 0      # the skip rule drops the last column


@pytest.mark.parametrize("name", fu.CASE_NAMES)
def test_restatement_equals_the_numpy_model(ref, cases, results, name):
    img, mask, n, exp = cases[name]
    r, m = results(name)
    print(f"{name}: info {r['info'][:6].tolist()} (model {m['info'][:6].tolist()}) stats {r['stats']}")
    rc, mc = fu.ref_cells(ref, img), m["cells"]
    assert rc["n"] == mc["n"] and rc["xy"].tobytes() == mc["xy"].tobytes() and rc["score"].tobytes() == mc["score"].tobytes()
    assert (rc["first_empty"], rc["empty"], rc["cells"]) == (mc["first_empty"], mc["empty"], mc["cells"])
    assert fu.same_fast(r, m) == []
    assert r["stats"] == m["stats"]
    h, w = img.shape
    fu.check_expected(name, exp, r["info"], r["stats"], cells=rc["cells"], w_cell=fu.model_grid(w, h)["w_cell"])
    # the properties of every result
    raw_bound, out_bound = fu.ref_bounds(ref, w, h, n)
    cnt, nodes = r["n"], int(r["info"][4])
    assert cnt <= nodes <= out_bound and r["stats"]["longest"] <= out_bound and rc["n"] <= raw_bound
    assert not r["keypoints"][cnt:].any() and not r["response"][cnt:].any() and not r["info"][6:].any()
    kp = r["keypoints"][:cnt]
    assert ((kp[:, 0] >= 19) & (kp[:, 0] < w - 19) & (kp[:, 1] >= 19) & (kp[:, 1] < h - 19)).all()
    assert (r["response"][:cnt] >= 1).all()
    if mask is not None and cnt:
        assert (mask[kp[:, 1].astype(int), kp[:, 0].astype(int)] != 0).all()
    # no two raw keypoints of one cell are 8-adjacent (the raw lists are equal: the model's counts per cell cut both)
    xy = rc["xy"].astype(np.int64)
    start = 0
    for (i, j, x0, y0, x1, y1), k in zip(mc["grid"]["cells"], mc["per_cell"]):
        pts = xy[start:start + k]
        start += k
        assert ((pts[:, 0] >= x0 - fu.BORDER + 3) & (pts[:, 0] < x1 - fu.BORDER - 3)).all(), (name, i, j)
        assert ((pts[:, 1] >= y0 - fu.BORDER + 3) & (pts[:, 1] < y1 - fu.BORDER - 3)).all(), (name, i, j)
        if k > 1:
            assert (np.diff(pts[:, 1] * 100000 + pts[:, 0]) > 0).all(), (name, i, j)       # raster order
            d = np.abs(pts[:, None, :] - pts[None, :, :]).max(-1) + np.eye(k, dtype=np.int64) * 9
            assert d.min() >= 2, (name, i, j)
    assert start == len(xy)
    # every returned keypoint is a raw keypoint with its score, so the returned ones of a cell are not 8-adjacent either
    raw_of = {(int(x) + fu.BORDER, int(y) + fu.BORDER): int(sc) for (x, y), sc in zip(rc["xy"], rc["score"])}
    assert len(raw_of) == rc["n"]
    for (x, y), sc in zip(kp, r["response"][:cnt]):
        assert raw_of.get((int(x), int(y))) == int(sc), (name, x, y)
    assert len({(int(x), int(y)) for x, y in kp}) == cnt


def test_mask_and_large_target_properties(ref, cases, results):
    img, mask, n, _ = cases["texture with holes"]
    masked, _ = results("texture with holes")
    plain, _ = results("texture N=400")
    kp, nn = plain["keypoints"][:plain["n"]], plain["n"]
    keep = mask[kp[:, 1].astype(int), kp[:, 0].astype(int)] != 0
    assert 0 < keep.sum() < nn
    assert masked["keypoints"][:masked["n"]].tobytes() == kp[keep].tobytes()       # the masked points removed, the order kept
    assert masked["response"][:masked["n"]].tobytes() == plain["response"][:nn][keep].tobytes()
    assert masked["info"][1:].tolist() == plain["info"][1:].tolist()               # the tree does not see the mask
    # N >= the raw count: every raw keypoint is its own node
    for name in ("62x62 noise", "320x240 texture"):
        im = cases[name][0]
        raw = fu.ref_cells(ref, im)
        r = fu.ref_detect(ref, im, None, raw["n"] + 10)
        assert r["n"] == raw["n"] == int(r["info"][4])
        got = set(map(tuple, np.column_stack([r["keypoints"][:r["n"]], r["response"][:r["n"]]]).tolist()))
        want = set(map(tuple, np.column_stack([raw["xy"] + fu.BORDER, raw["score"].astype(np.float32)]).tolist()))
        assert got == want


def test_planted_pixels_are_found_exactly(ref, cases, results):
    img, pts = fu.planted_pixels()
    h, w = img.shape
    inside = {p: v for p, v in pts.items() if 19 <= p[0] < w - 19 and 19 <= p[1] < h - 19}
    assert len(inside) == 272
    for r in results("planted pixels"):
        assert r["n"] == 272 == int(r["info"][4])
        got = {(int(x), int(y)): float(s) for (x, y), s in zip(r["keypoints"][:272], r["response"][:272])}
        assert got == {p: float(v - 41) for p, v in inside.items()}
    # a flat square is no use here: its corner ties with its diagonal neighbour and strict suppression removes both
    sq = np.full((100, 100), 40, np.uint8)
    sq[40:60, 40:60] = 200
    assert fu.ref_detect(ref, sq, None, 50)["n"] == fu.model_detect(sq, None, 50)["n"]


def test_flat_and_all_zero_mask(results):
    for r in results("flat 255"):
        assert r["info"].tolist() == [0, 0, 54, 54, 0, 1, 0, 0] and not r["keypoints"].any()
    for r in results("all-zero mask"):
        assert r["n"] == 0 and r["info"][4] > 0 and not r["keypoints"].any() and not r["response"].any()


def test_the_tie_rule_is_exercised_and_restated(ref, cases):
    img, _, n, _ = cases["texture N=400"]
    a, b = fu.model_detect(img, None, n), fu.model_detect(img, None, n, reverse_tie=True)
    assert a["stats"]["ties"] > 200
    assert fu.same_fast(a, b) != [], "equal sizes never decide anything on this image"
    ra, rb = fu.ref_detect(ref, img, None, n), fu.ref_detect(ref, img, None, n, reverse_tie=True)
    assert fu.same_fast(ra, a) == [] and fu.same_fast(rb, b) == []       # the C restatement follows the stated rule, both ways


def test_the_large_image(ref):
    name, n, exp = fu.BIG
    img = fu.big_image(synth)
    r = fu.ref_detect(ref, img, None, n)
    rc = fu.ref_cells(ref, img)
    print(f"{name}: info {r['info'][:6].tolist()} stats {r['stats']}")
    fu.check_expected(name, exp, r["info"], r["stats"], cells=rc["cells"])
    assert r["n"] == rc["n"] < n            # fewer raw keypoints than N: every one is returned
    m = fu.model_cells(img)
    assert m["xy"].tobytes() == rc["xy"].tobytes() and m["score"].tobytes() == rc["score"].tobytes()
