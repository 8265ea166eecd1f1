"""CPU tests of ORB over a scale pyramid (include/pagk.h "ORB over a scale pyramid"): the boundary (header, bindings, struct
size, citations, checks that need no device); the level table of the library, of the plain-C restatement
(tests/orb_levels_ref.c) and of an independent float32 model; the resize of the restatement against a numpy model, byte for
byte; the composition of an extract out of the one-level restatements; the restatement under the sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import detect_ref_util as du
import fast_ref_util as fu
import orb_levels_ref_util as lu
import orb_ref_util as ou
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, host_api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("pagk_orb_extractor_check", "pagk_orb_extractor_levels", "pagk_orb_extract_slot", "pagk_orb_slot_read",
                    "pagk_orb_match_slots", "pagk_orb_match_slots_read", "pagk_orb_extract_levels", "pagk_orb_detect_levels",
                    "pagk_selftest_orb_level")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return lu.build_ref(tmp_path_factory.mktemp("orb_levels_ref"))


@pytest.fixture(scope="module")
def one_level(tmp_path_factory):
    d = tmp_path_factory.mktemp("orb_levels_one")
    return fu.build_ref(d), ou.build_ref(d)


def _ex(**kw):
    return capi.orb_extractor_default(**kw)


# ---- the boundary --------------------------------------------------------------------------------------------------------
def test_header_declares_and_capi_binds_the_new_entry_points(built):
    hdr = open(os.path.join(ROOT, "include", "pagk.h")).read()
    assert re.search(r"#define PAGK_VERSION (\d+)", hdr).group(1) == "303"
    assert re.search(r"#define PAGK_ORB_MAX_LEVELS 8\b", hdr) and re.search(r"#define PAGK_ORB_LEVELS_INFO_WORDS 32\b", hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = capi.load()
    # the section sits behind "ORB descriptors and matching" and in front of Lucas-Kanade
    assert hdr.index("ORB descriptors and matching:") < hdr.index("---- ORB over a scale pyramid") < hdr.index("---- Pyramidal Lucas-Kanade")
    assert code.index("pagk_orb_match(") < code.index("pagk_orb_extractor") < code.index("pagk_lk_params")
    for name in NEW_ENTRY_POINTS + ("pagk_orb_extractor_default",):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name) and getattr(lib, name).argtypes, name
        # every declaration cites the reference lines it stands for, directly above it
        decl = re.search(r"\b(?:int|void) " + name + r"\(", hdr).start()
        comment = hdr[:decl].rsplit("/*", 1)[1]
        assert re.search(r"src/ORB(extractor\.cc|DetectAndDespMatcher\.cpp):\d+", comment), name
        assert comment.rstrip().endswith("*/"), name
        # no entry point of this section takes a caller's array in device memory
        args = code[code.index(name + "("):].split(";", 1)[0]
        assert not re.search(r"\bd_\w+", args) and "device pointer" not in comment.lower(), name
    for meth in ("orb_extract_slot", "orb_slot_read", "orb_match_slots", "orb_match_slots_read", "orb_extract_levels",
                 "orb_detect_levels", "selftest_orb_level"):
        assert callable(getattr(capi.Context, meth)), meth
    for fn in ("orb_extract_levels", "orb_detect_levels", "orb_match_pair_levels"):
        assert callable(getattr(host_api, fn)), fn
    begin = hdr[hdr.index("hipGraph capture of the per-frame work"):hdr.index("int pagk_graph_begin")]
    assert "pagk_orb_extract_slot" in begin and "pagk_orb_match_slots" in begin
    assert "is not provided; computeOrientation" not in hdr and "cv::resize at 1 / 1.2) is not" not in hdr
    for word in ("tests/orb_levels_ref.c", "NOT claimed", "identical to the reference's N = 0", "never read", "2 2 2 1 1 1 1 0"):
        assert word in hdr, word
    assert [f[0] for f in capi.OrbExtractor._fields_] == ["n_features", "scale_factor", "n_levels", "ini_threshold",
                                                          "min_threshold"]
    assert C.sizeof(capi.OrbExtractor) == 20
    d = _ex()
    assert (d.n_features, d.scale_factor, d.n_levels, d.ini_threshold, d.min_threshold) == (1000, np.float32(1.2), 8, 20, 7)
    # the two one-level structs keep refusing more levels
    assert capi.orb_params_check(capi.orb_params_default(n_levels=8)) == capi.PAGK_E_UNSUPPORTED
    assert capi.fast_params_check(capi.fast_params_default(n_levels=8)) == capi.PAGK_E_UNSUPPORTED


def test_argument_checks_that_need_no_device(built):
    lib = capi.load()
    assert capi.orb_extractor_check(_ex()) == capi.PAGK_OK
    for ok in (dict(n_levels=1), dict(n_levels=8), dict(scale_factor=1.5), dict(scale_factor=float(np.nextafter(np.float32(1), np.float32(2)))),
               dict(ini_threshold=0, min_threshold=255), dict(n_features=1), dict(n_features=1 << 24)):
        assert capi.orb_extractor_check(_ex(**ok)) == capi.PAGK_OK, ok
    for bad in (dict(n_levels=0), dict(n_levels=9), dict(scale_factor=1.0), dict(scale_factor=1.6), dict(scale_factor=float("nan")),
                dict(scale_factor=0.8), dict(ini_threshold=-1), dict(ini_threshold=256), dict(min_threshold=-1),
                dict(min_threshold=256), dict(n_features=0), dict(n_features=(1 << 24) + 1)):
        assert capi.orb_extractor_check(_ex(**bad)) == capi.PAGK_E_ARG, bad
        assert capi.orb_extractor_levels(_ex(**bad), 640, 480)["rc"] == capi.PAGK_E_ARG, bad
    assert lib.pagk_orb_extractor_check(None) == capi.PAGK_E_ARG
    lib.pagk_orb_extractor_default(None)
    assert lib.pagk_orb_extractor_levels(None, 640, 480, None, None, None, None, None, None) == capi.PAGK_E_ARG
    e = _ex()
    assert lib.pagk_orb_extractor_levels(C.byref(e), 640, 480, None, None, None, None, None, None) == capi.PAGK_OK
    # without a context every entry point refuses
    orb, iv = capi.orb_params_default(), capi.image_view(np.zeros((240, 320), np.uint8))
    assert lib.pagk_orb_extract_slot(None, C.byref(e), C.byref(orb), 0) == capi.PAGK_E_ARG
    assert lib.pagk_orb_slot_read(None, 0, 10, None, None, None, None, None, None) == capi.PAGK_E_ARG
    assert lib.pagk_orb_match_slots(None, C.byref(orb), 0, 1) == capi.PAGK_E_ARG
    assert lib.pagk_orb_match_slots_read(None, 0, 10, None, None, None, None) == capi.PAGK_E_ARG
    assert lib.pagk_orb_extract_levels(None, C.byref(e), C.byref(orb), C.byref(iv), 10, None, None, None, None, None, None) == capi.PAGK_E_ARG
    assert lib.pagk_orb_detect_levels(None, C.byref(e), C.byref(iv), None, 10, None, None, None, None) == capi.PAGK_E_ARG
    assert lib.pagk_selftest_orb_level(None, 0, 0, None, 0) == capi.PAGK_E_ARG


# ---- the level table -----------------------------------------------------------------------------------------------------
def _same_table(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("width", "height", "scale", "quota", "size")) \
        and a["out_bound"] == b["out_bound"]


def test_level_table_of_library_restatement_and_model_agree(built, ref):
    seen = refused = 0
    for w, h in ((97, 80), (160, 120), (120, 160), (320, 240), (321, 243), (640, 480), (752, 480), (1241, 376), (1920, 1080),
                 (62, 62), (75, 75), (91, 62), (3000, 70), (32767, 200)):
        for sf in (1.2, 1.1, 1.5, 1.25, 1.01, 1.3333334):
            for nl in (1, 2, 3, 4, 5, 8):
                for nf in (1, 3, 10, 400, 1000, 5000):
                    lib_t = capi.orb_extractor_levels(_ex(n_features=nf, scale_factor=sf, n_levels=nl), w, h)
                    ref_t = lu.ref_levels(ref, nf, sf, nl, w, h)
                    mod_t = lu.model_levels(nf, sf, nl, w, h)
                    assert (lib_t["rc"] != 0) == (ref_t is None) == (mod_t is None), (w, h, sf, nl, nf)
                    if mod_t is None:
                        refused += 1
                        continue
                    seen += 1
                    assert _same_table(lib_t, mod_t) and _same_table(ref_t, mod_t), (w, h, sf, nl, nf, lib_t, ref_t, mod_t)
                    assert int(mod_t["quota"].sum()) >= nf or mod_t["quota"][-1] == 0
                    assert (mod_t["quota"] >= 0).all() and mod_t["width"][0] == w and mod_t["height"][0] == h
    print(f"{seen} tables compared, {refused} refused by all three")
    assert seen > 1000 and refused > 100


def test_known_quotas_and_sizes(built, ref):
    def quota(nf, nl, sf=1.2, w=640, h=480):
        t = capi.orb_extractor_levels(_ex(n_features=nf, scale_factor=sf, n_levels=nl), w, h)
        assert t["rc"] == 0 and _same_table(t, lu.ref_levels(ref, nf, sf, nl, w, h)) and _same_table(t, lu.model_levels(nf, sf, nl, w, h))
        return list(t["quota"])
    assert quota(1000, 8) == [217, 181, 151, 126, 105, 87, 73, 60]
    assert quota(10, 8) == [2, 2, 2, 1, 1, 1, 1, 0]
    assert quota(1, 3) == [0, 0, 1]
    assert quota(400, 4) == [129, 107, 89, 75]
    assert quota(1000, 1) == [1000]
    t = capi.orb_extractor_levels(_ex(n_levels=8), 320, 240)
    assert (t["width"][-1], t["height"][-1]) == (89, 67) and (t["width"][0], t["height"][0]) == (320, 240)
    assert list(t["size"]) == [int(np.float32(31) * s) for s in t["scale"]] and t["size"][0] == 31
    t = capi.orb_extractor_levels(_ex(n_levels=4), 160, 120)
    assert list(zip(t["width"], t["height"])) == [(160, 120), (133, 100), (111, 83), (93, 69)]
    # out_bound is the sum of the one-level bounds with N = max(quota, 1)
    t = capi.orb_extractor_levels(_ex(n_features=10, n_levels=8), 320, 240)
    want = sum(fu.model_bounds(int(a), int(b), max(int(q), 1))[1] for a, b, q in zip(t["width"], t["height"], t["quota"]))
    assert t["out_bound"] == want
    # scales: one float32 rounding per level
    s = np.float32(1)
    for l in range(8):
        assert capi.orb_extractor_levels(_ex(n_levels=8), 640, 480)["scale"][l] == s
        s = np.float32(s * np.float32(1.2))


def test_sizes_the_table_refuses(built, ref):
    for w, h, nl, why in ((97, 80, 3, "third level 67 x 56"), (160, 120, 5, "fifth level 77 x 58"), (91, 62, 2, "second level 76 x 52"),
                          (61, 200, 1, "level 0 too narrow"), (200, 32768, 1, "level 0 too tall"), (70, 400, 1, "nIni 0")):
        assert capi.orb_extractor_levels(_ex(n_levels=nl), w, h)["rc"] == capi.PAGK_E_ARG, why
        assert lu.ref_levels(ref, 1000, 1.2, nl, w, h) is None and lu.model_levels(1000, 1.2, nl, w, h) is None, why
    t = lu.model_levels(1000, 1.2, 3, 97, 80)
    assert t is None and (int(np.rint(np.float32(97) / np.float32(1.44))), int(np.rint(np.float32(80) / np.float32(1.44)))) == (67, 56)
    assert capi.orb_extractor_levels(_ex(n_levels=2), 97, 80)["rc"] == 0      # the smallest legal two-level image of this shape
    assert capi.orb_extractor_levels(_ex(n_levels=4), 160, 120)["rc"] == 0
    for bad in (1.0, 1.6):
        assert capi.orb_extractor_levels(_ex(scale_factor=bad), 640, 480)["rc"] == capi.PAGK_E_ARG
    for bad in (0, 9):
        assert capi.orb_extractor_levels(_ex(n_levels=bad), 640, 480)["rc"] == capi.PAGK_E_ARG


# ---- the resize ----------------------------------------------------------------------------------------------------------
def _resize_both(ref, src, dw, dh, **kw):
    r, m = lu.ref_resize(ref, src, dw, dh, **kw), lu.model_resize(src, dw, dh)
    assert r.tobytes() == m.tobytes(), (src.shape, dw, dh)
    return r


def test_resize_restatement_equals_the_numpy_model(ref):
    noise = du.noise_image(161, 123, 9)
    # a same-size resize is a copy; a constant image stays constant
    assert _resize_both(ref, noise, 161, 123).tobytes() == noise.tobytes()
    for v in (0, 1, 130, 255):
        assert (_resize_both(ref, np.full((80, 97), v, np.uint8), 81, 67) == v).all()
    # ramps: monotone in, monotone out up to one grey level (each of the two `>> 16` of the vertical pass drops less than one
    # unit of a value in quarters of a grey level, so two pixels of the same exact value can land on neighbouring bytes, never
    # further apart), the ends reached within the step of one source pixel
    yy, xx = np.mgrid[0:120, 0:160]
    for ramp in ((xx * 255 // 159).astype(np.uint8), (yy * 255 // 119).astype(np.uint8), ((xx + yy) * 255 // 278).astype(np.uint8)):
        out = _resize_both(ref, ramp, 133, 100).astype(np.int64)
        assert (np.diff(out, axis=1) >= -1).all() and (np.diff(out, axis=0) >= -1).all()
        assert out[0, 0] <= out[50, 66] <= out[-1, -1] and out[-1, -1] - out[0, 0] > 250
        assert abs(int(out[0, 0]) - int(ramp[0, 0])) <= 2 and abs(int(out[-1, -1]) - int(ramp[-1, -1])) <= 2
    # noise at odd and even sizes, every ratio the definition allows and a pitch above the width on both sides
    for (sw, sh), (dw, dh) in (((161, 123), (134, 103)), ((160, 120), (133, 100)), ((133, 100), (111, 83)), ((111, 83), (93, 69)),
                               ((97, 80), (81, 67)), ((150, 150), (100, 100)), ((101, 99), (100, 98)), ((64, 64), (63, 43)),
                               ((320, 240), (267, 200))):
        src = du.noise_image(sw, sh, sw + dh)
        out = _resize_both(ref, src, dw, dh)
        assert lu.ref_resize(ref, lu.padded(src, 7), dw, dh, dpitch=dw + 3).tobytes() == out.tobytes()
        # a bilinear value lies between the extremes of its four taps: the whole image stays inside the source's range
        assert out.min() >= src.min() and out.max() <= src.max()


def test_pyramid_of_an_extract_is_the_chain_of_resizes(ref):
    img = lu.texture(synth, 160, 120)
    ex = _ex(n_levels=4, n_features=400)
    r = lu.ref_extract(ref, img, ex, ou.seeded_pattern())
    want = lu.model_pyramid(img, lu.model_levels(400, 1.2, 4, 160, 120))
    assert [a.shape for a in r["levels"]] == [(120, 160), (100, 133), (83, 111), (69, 93)]
    for a, b in zip(r["levels"], want):
        assert a.tobytes() == b.tobytes()


# ---- composition -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, nl, nf", [((160, 120), 4, 400), ((120, 160), 4, 1000), ((97, 80), 2, 300), ((320, 240), 8, 1000),
                                           ((320, 240), 8, 10), ((160, 120), 3, 1)])
def test_an_extract_is_the_one_level_restatements_per_level(ref, one_level, shape, nl, nf):
    """Level l's segment of an extract equals fdr_detect(level image l, N_l) plus orb_ref_describe, scaled; octaves ascend;
    the per-level counts add up."""
    w, h = shape
    img = lu.texture(synth, w, h, 23)
    ex, pat = _ex(n_levels=nl, n_features=nf), ou.seeded_pattern()
    r = lu.ref_extract(ref, img, ex, pat)
    t = r["table"]
    c = lu.compose(one_level[0], one_level[1], lu.model_pyramid(img, t), t, ex, pat)
    n = r["n"]
    print(f"{w} x {h}, {nl} levels, {nf} features: quotas {list(t['quota'])}, counts {c['counts']}")
    assert n == sum(c["counts"]) == len(c["keypoints"]) and n <= r["cap"]
    for k in ("keypoints", "octave", "response", "angle", "desc"):
        assert r[k][:n].tobytes() == c[k].tobytes(), k
        assert not r[k][n:].any(), k
    info = r["info"]
    assert info[0] == n and info[2] == nl and list(info[8:8 + nl]) == c["counts"] and list(info[24:24 + nl]) == list(t["quota"])
    assert info[1] == int((r["angle"][:n] == -1).sum()) and not info[3:8].any() and not info[8 + nl:16].any()
    assert (np.diff(r["octave"][:n]) >= 0).all() and n > 0
    assert (info[16:16 + nl] >= info[8:8 + nl]).all()
    # a level with quota 0 runs with N = 1 and still returns the keypoints of its first round
    for l in range(nl):
        if t["quota"][l] == 0:
            assert c["counts"][l] >= 1
    # scaled coordinates stay inside the original image
    assert (r["keypoints"][:n, 0] < w).all() and (r["keypoints"][:n, 1] < h).all() and (r["keypoints"][:n] >= 16).all()


def test_masked_detect_drops_keypoints_at_their_scaled_positions(ref):
    img = lu.texture(synth, 160, 120, 23)
    ex = _ex(n_levels=4, n_features=400)
    full = lu.ref_extract(ref, img, ex)
    ext = lu.ref_extract(ref, img, ex, ou.seeded_pattern())
    n = full["n"]
    assert n == ext["n"] and full["keypoints"].tobytes() == ext["keypoints"].tobytes() and "angle" not in full
    assert lu.ref_extract(ref, img, ex, mask=np.ones((120, 160), np.uint8))["keypoints"].tobytes() == full["keypoints"].tobytes()
    mask = np.ones((120, 160), np.uint8)
    mask[30:90, 40:110] = 0
    m = lu.ref_extract(ref, img, ex, mask=mask)
    kp = full["keypoints"][:n]
    keep = mask[kp[:, 1].astype(np.int64), kp[:, 0].astype(np.int64)] != 0
    assert m["n"] == int(keep.sum()) and 0 < m["n"] < n
    assert m["keypoints"][:m["n"]].tobytes() == kp[keep].tobytes() and m["octave"][:m["n"]].tobytes() == full["octave"][:n][keep].tobytes()
    assert not m["keypoints"][m["n"]:].any()
    dropped_upper = int((~keep & (full["octave"][:n] > 0)).sum())
    assert dropped_upper > 0                                    # the zero block removes upper-level keypoints too
    assert list(m["info"][8:12]) == [int((keep & (full["octave"][:n] == l)).sum()) for l in range(4)]


def test_a_flat_image_gives_no_keypoints_at_any_level(ref):
    r = lu.ref_extract(ref, np.full((240, 320), 99, np.uint8), _ex(n_levels=8), ou.seeded_pattern())
    assert r["n"] == 0 and not r["info"][:2].any() and r["info"][2] == 8 and not r["info"][8:24].any()
    assert not r["keypoints"].any() and not r["desc"].any()


# ---- sanitizers ------------------------------------------------------------------------------------------------------------
def test_restatement_runs_clean_under_the_sanitizers(tmp_path):
    """A stand-alone program (tests/orb_levels_sanitize.c: its own main, compiled together with the three restatements) runs
    an extract and a masked detect at 97 x 80 with 2 levels and 160 x 120 with 4 under AddressSanitizer and UBSan."""
    exe = str(tmp_path / "orb_levels_sanitize")
    srcs = [os.path.join(ROOT, "tests", f) for f in ("orb_levels_sanitize.c", "orb_levels_ref.c", "fast_detect_ref.c", "orb_ref.c")]
    subprocess.run(["gcc", "-std=c99", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", *srcs, "-o", exe, "-lm"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "3 runs clean" in r.stdout, r.stdout
