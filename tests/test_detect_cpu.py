"""CPU tests of the corner detector's ground truth: the plain-C restatement (tests/corner_detect_ref.c) against an
independent numpy model of the definition in include/pagk.h, planted corners, the properties of the result, the tie
rule, and the boundary (header, bindings)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import detect_ref_util as du
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 640, 480
NEW_ENTRY_POINTS = ("pagk_detect_corners_device", "pagk_detect_corners", "pagk_frame_handover_detect_device",
                    "pagk_frame_handover_detect", "pagk_selftest_corner_response")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return du.build_ref(tmp_path_factory.mktemp("detect_ref"))


@pytest.fixture(scope="module")
def texture():
    return du.texture_image(synth, W, H, 7)


def test_header_declares_and_capi_binds_the_new_entry_points(built):
    hdr = open(os.path.join(ROOT, "include", "pagk.h")).read()
    assert "#define PAGK_DETECT_INFO_WORDS 8" in hdr and capi.DETECT_INFO_WORDS == 8
    assert re.search(r"#define PAGK_VERSION (\d+)", hdr).group(1) == "303"
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = capi.load()
    assert re.search(r"\bvoid pagk_detect_params_default\s*\(", code)
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes, name
        # every entry point cites the reference function it stands for
        comment = hdr[:hdr.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "src/frame.cpp:156-218" in comment, name
    for meth in ("detect_corners_device", "detect_corners", "frame_handover_detect_device", "frame_handover_detect",
                 "selftest_corner_response"):
        assert callable(getattr(capi.Context, meth))
    begin = hdr[hdr.index("hipGraph capture of the per-frame work"):hdr.index("int pagk_graph_begin")]
    for name in ("pagk_detect_corners_device", "pagk_frame_handover_detect_device", "pagk_frame_handover_device",
                 "pagk_post_filter_device"):
        assert name in begin
    # the parameter block: three doubles and an int32, in the header's order
    assert [f[0] for f in capi.DetectParams._fields_] == ["quality_level", "min_distance", "harris_k", "raw_cap"]
    assert capi.DetectParams.raw_cap.offset == 24 and C.sizeof(capi.DetectParams) == 32
    d = capi.detect_params_default()
    assert (d.quality_level, d.min_distance, d.harris_k, d.raw_cap) == (0.005, 20.0, 0.04, 0)


def test_new_entry_points_check_their_arguments_without_a_device(built):
    lib = capi.load()
    p = capi.make_params(camera=synth.D435I)
    d = capi.detect_params_default()
    img = np.zeros((H, W), np.uint8)
    iv = capi.image_view(img)
    assert lib.pagk_detect_corners_device(None, C.byref(d), 0, None, 100, None, None, None) == capi.PAGK_E_ARG
    assert lib.pagk_detect_corners(None, C.byref(d), C.byref(iv), None, 100, None, None) == capi.PAGK_E_ARG
    assert lib.pagk_frame_handover_detect_device(None, C.byref(p), W, H, 400, 400, 320.0, None, None, None, C.byref(d), 0,
                                                 None, None, None, None, None, None, None, None) == capi.PAGK_E_ARG
    assert lib.pagk_frame_handover_detect(None, C.byref(p), W, H, 400, 400, 320.0, None, None, None, C.byref(d),
                                          C.byref(iv), None, None, None, None, None, None, None, None) == capi.PAGK_E_ARG
    assert lib.pagk_selftest_corner_response(None, C.byref(iv), None) == capi.PAGK_E_ARG


def _inputs(texture):
    """name -> (image, mask): the cases the restatement and the model are compared on."""
    return {
        "texture": (texture, None),
        "noise": (du.noise_image(W, H), None),
        "all 255": (np.full((H, W), 255, np.uint8), None),
        "mask all zero": (texture, np.zeros((H, W), np.uint8)),
        "mask with holes": (texture, du.holes_mask(W, H)),
    }


@pytest.mark.parametrize("name", ["texture", "noise", "all 255", "mask all zero", "mask with holes"])
def test_restatement_equals_the_numpy_model(ref, texture, name):
    img, mask = _inputs(texture)[name]
    r = du.ref_detect(ref, img, mask, 1000, with_response=True)
    m = du.model_detect(img, mask, 1000)
    print(f"{name}: info {r['info'][:5].tolist()} (model {m['info'][:5].tolist()})")
    assert np.array_equal(r["R"].view(np.uint32), m["R"].view(np.uint32)), "response map"
    assert np.array_equal(du.ref_response(ref, img).view(np.uint32), m["R"].view(np.uint32))
    assert r["info"][1] == m["info"][1], "raw count"
    assert du.same_detect(r, m) == []
    if name in ("all 255", "mask all zero"):
        assert r["info"].tolist() == [0] * 8 and not r["corners"].any()
    else:
        assert r["n"] > 100


def test_the_sizes_the_plan_was_made_with(ref, texture):
    # the numpy model's figures for the three 640 / 752-wide images: raw candidates and corners at distance 20
    for img, raw, n in ((du.texture_image(synth, 752, 480, 1), 9638, 581), (texture, 9616, 494), (du.noise_image(W, H), 17703, 508)):
        r = du.ref_detect(ref, img, None, 5000)
        assert (int(r["info"][1]), r["n"]) == (raw, n)
        assert r["info"][4] == raw   # the limit was not reached: the walk visited every candidate


def test_planted_corners_are_found_exactly(ref):
    img, pts = du.planted_squares(W, H)
    assert len(pts) == 252 and len(set(pts)) == 252
    xy = np.array(pts)
    d = np.sqrt(((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1)) + np.eye(252) * 1e9
    assert d.min() >= 23
    for cap in (252, 300):
        r = du.ref_detect(ref, img, None, cap)
        assert r["n"] == 252 and int(r["info"][1]) == 252
        assert set(map(tuple, r["corners"][:252].astype(int).tolist())) == set(pts)
    m = du.model_detect(img, None, 300, min_distance=0.0)   # the model needs no distance test to find the same
    assert m["n"] == 252 and set(map(tuple, m["corners"][:252].astype(int).tolist())) == set(pts)
    assert du.same_detect(du.ref_detect(ref, img, None, 300), du.model_detect(img, None, 300)) == []


def test_properties_on_the_texture(ref, texture):
    mask = du.holes_mask(W, H)
    r = du.ref_detect(ref, texture, mask, 1000, with_response=True)
    n, pts = r["n"], r["corners"][:r["n"]].astype(np.int64)
    assert n > 100 and not r["corners"][n:].any()
    resp = r["R"][pts[:, 1], pts[:, 0]]
    assert (np.diff(resp) <= 0).all() and (resp > 0).all()                          # responses descend along the list
    dd = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1) + np.eye(n, dtype=np.int64) * 10 ** 9
    assert dd.min() >= 400                                                          # nobody closer than min_distance
    assert (mask[pts[:, 1], pts[:, 0]] != 0).all()                                  # nobody on a masked pixel
    assert (pts[:, 0] >= 1).all() and (pts[:, 0] <= W - 2).all() and (pts[:, 1] >= 1).all() and (pts[:, 1] <= H - 2).all()
    for k in (0, 1, 50, n - 1):                                                     # a smaller limit gives a prefix
        s = du.ref_detect(ref, texture, mask, k, cap=1000)
        assert s["n"] == k and s["corners"][:k].tobytes() == r["corners"][:k].tobytes() and not s["corners"][k:].any()
        assert s["info"][4] <= r["info"][4] and (k > 0 or s["info"][4] == 0)
    assert du.ref_detect(ref, texture, mask, -3, cap=10)["n"] == 0                  # a negative limit is 0
    assert du.ref_detect(ref, texture, mask, 5000, cap=40)["n"] == 40               # the limit never exceeds cap
    raw = int(r["info"][1])
    o = du.ref_detect(ref, texture, mask, 1000, raw_cap=raw - 1)                    # one too few: nothing, and said so
    assert o["n"] == 0 and o["info"][:5].tolist() == [0, raw, 1, int(r["info"][3]), 0] and not o["corners"].any()
    assert du.same_detect(o, du.model_detect(texture, mask, 1000, raw_cap=raw - 1)) == []
    assert du.same_detect(du.ref_detect(ref, texture, mask, 1000, raw_cap=raw), r) == []


def test_the_raw_bound_holds_on_noise(ref):
    for w, h in ((W, H), (641, 479), (14, 14)):
        assert ref.cdr_raw_bound(w, h) == du.raw_bound(w, h) == ((w - 1) // 2) * ((h - 1) // 2)
    assert du.raw_bound(752, 480) == 89625 and du.raw_bound(W, H) == 76241 and du.raw_bound(1920, 1080) == 516901
    r = du.ref_detect(ref, du.noise_image(W, H), None, 10, quality_level=0.0)       # every positive local maximum
    assert 17703 <= int(r["info"][1]) <= du.raw_bound(W, H)


def test_the_tie_rule(ref):
    img = du.tie_bar()
    assert np.array_equal(img, img[:, ::-1])
    R = du.ref_response(ref, img)
    assert np.array_equal(R.view(np.uint32), R[:, ::-1].view(np.uint32))            # mirror-symmetric, bit for bit
    assert R[10, 31] == R[10, 32] == R[39, 31] == R[39, 32] == R.max()
    for det in (du.ref_detect(ref, img, None, 10, min_distance=0.5), du.model_detect(img, None, 10, min_distance=0.5)):
        assert det["info"][:2].tolist() == [2, 2]
        assert det["corners"][:2].tolist() == [[32.0, 39.0], [32.0, 10.0]]          # the later pixel, the higher index first
