"""CPU tests of the ORB descriptors and the matcher's ground truth: the plain-C restatement (tests/orb_ref.c) against an
independent numpy model of the definition in include/pagk.h ("ORB descriptors and matching"), byte for byte; the blur's
closed forms; the steering pair against the correctly rounded cosine and sine; planted truth; the matcher's rules; the
boundary (header, bindings, argument checks that need no device)."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import orb_ref_util as ou
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("pagk_orb_params_check", "pagk_orb_pattern_check", "pagk_orb_set_pattern", "pagk_orb_describe_device",
                    "pagk_orb_describe", "pagk_orb_match_device", "pagk_orb_match")
F = np.float32


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return ou.build_ref(tmp_path_factory.mktemp("orb_ref"))


@pytest.fixture(scope="module")
def images():
    return ou.images(synth)


# ---- the boundary --------------------------------------------------------------------------------------------------------
def test_header_declares_and_capi_binds_the_new_entry_points(built):
    hdr = open(os.path.join(ROOT, "include", "pagk.h")).read()
    assert re.search(r"#define PAGK_VERSION (\d+)", hdr).group(1) == "303"
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = capi.load()
    assert re.search(r"\bvoid pagk_orb_params_default\s*\(", code)
    assert code.index("pagk_undistort_maps") < code.index("pagk_orb_params") < code.index("pagk_selftest_divide")
    for name in NEW_ENTRY_POINTS + ("pagk_orb_params_default",):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name) and getattr(lib, name).argtypes, name
        # every new declaration cites the reference lines it stands for, directly above it
        decl = re.search(r"\b(?:int|void) " + name + r"\(", hdr).start()
        comment = hdr[:decl].rsplit("/*", 1)[1]
        assert re.search(r"src/ORB(extractor\.cc|DetectAndDespMatcher\.cpp):\d+", comment), name
        assert comment.rstrip().endswith("*/"), name
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
    for meth in ("orb_set_pattern", "orb_describe_device", "orb_describe", "orb_match_device", "orb_match"):
        assert callable(getattr(capi.Context, meth))
    begin = hdr[hdr.index("hipGraph capture of the per-frame work"):hdr.index("int pagk_graph_begin")]
    assert "pagk_orb_describe_device" in begin and "pagk_orb_match_device" in begin
    assert "descriptors are not\n * provided" not in hdr and "descriptors are not provided" not in hdr
    for word in ("0x1.ca44dep+5f", "0x1.921fb544p+0", "NOT claimed", "tests/orb_ref.c"):       # the definition stands here
        assert word in hdr, word
    assert [f[0] for f in capi.OrbParams._fields_] == ["blur_weights", "match_floor", "n_levels"]
    assert C.sizeof(capi.OrbParams) == 24
    d = capi.orb_params_default()
    assert (list(d.blur_weights), d.match_floor, d.n_levels) == ([54, 49, 34, 18], 30, 1)
    # the stated derivation of the default taps: exp(-k^2 / 8) normalised, times 256, the centre absorbing the remainder
    g = [math.exp(-k * k / 8.0) for k in range(4)]
    q = [256.0 * v / (g[0] + 2 * sum(g[1:])) for v in g]
    assert [round(v) for v in q[1:]] == [49, 34, 18] and 256 - 2 * (49 + 34 + 18) == 54 and abs(q[0] - 54) < 1.5


def test_argument_checks_that_need_no_device(built):
    lib = capi.load()
    assert capi.orb_params_check(capi.orb_params_default()) == capi.PAGK_OK
    assert capi.orb_params_check(capi.orb_params_default(blur_weights=(256, 0, 0, 0), match_floor=0)) == capi.PAGK_OK
    assert capi.orb_params_check(capi.orb_params_default(blur_weights=(70, 42, 33, 18))) == capi.PAGK_OK
    for bad in (dict(blur_weights=(55, 49, 34, 18)), dict(blur_weights=(54, 49, 34, 17)), dict(blur_weights=(56, 49, 34, 16)),
                dict(blur_weights=(258, -1, 0, 0)),
                dict(blur_weights=(-2, 129, 0, 0)), dict(match_floor=-1), dict(match_floor=257)):
        assert capi.orb_params_check(capi.orb_params_default(**bad)) == capi.PAGK_E_ARG, bad
    assert capi.orb_params_check(capi.orb_params_default(n_levels=8)) == capi.PAGK_E_UNSUPPORTED
    assert capi.orb_params_check(capi.orb_params_default(n_levels=0)) == capi.PAGK_E_UNSUPPORTED
    assert lib.pagk_orb_params_check(None) == capi.PAGK_E_ARG
    lib.pagk_orb_params_default(None)
    # the pattern's range
    assert lib.pagk_orb_pattern_check(None) == capi.PAGK_E_ARG
    for pat in (ou.seeded_pattern(), ou.corner_pattern(), np.zeros(1024, np.int32)):
        assert capi.orb_pattern_check(pat) == capi.PAGK_OK
        assert pat.min() >= -13 and pat.max() <= 13
    for pos, v in ((0, 14), (1023, 14), (511, -14), (7, -14), (300, 1 << 20)):
        pat = ou.seeded_pattern()
        pat[pos] = v
        assert capi.orb_pattern_check(pat) == capi.PAGK_E_ARG, (pos, v)
    with pytest.raises(ValueError):
        capi.orb_pattern_check(np.zeros(1023, np.int32))
    # without a context every entry point refuses; n_levels = 8 is refused as unsupported wherever the parameters are read
    ok, pat = capi.orb_params_default(), ou.seeded_pattern()
    iv = capi.image_view(np.zeros((80, 97), np.uint8))
    assert lib.pagk_orb_set_pattern(None, pat.ctypes.data) == capi.PAGK_E_ARG
    assert lib.pagk_orb_describe_device(None, C.byref(ok), 0, 10, None, None, None, None, None) == capi.PAGK_E_ARG
    assert lib.pagk_orb_describe(None, C.byref(ok), C.byref(iv), 0, None, None, None, None) == capi.PAGK_E_ARG
    assert lib.pagk_orb_match_device(None, C.byref(ok), 10, None, None, 10, None, None, None, None, None, None) == capi.PAGK_E_ARG
    assert lib.pagk_orb_match(None, C.byref(ok), 0, None, 0, None, None, None, None, None) == capi.PAGK_E_ARG


# ---- the restatement against the model ---------------------------------------------------------------------------------
def _describe_both(ref, img, pattern, kp, **kw):
    r, m = ou.ref_describe(ref, img, pattern, kp, **kw), ou.model_describe(img, pattern, kp, **kw)
    assert r["blurred"].tobytes() == m["blurred"].tobytes()
    assert ou.same(r, m, ou.DESC_KEYS) == []
    return r


@pytest.mark.parametrize("name", ["97x80 texture", "160x120 texture"])
@pytest.mark.parametrize("pattern", ["seeded", "corners"])
def test_restatement_equals_the_numpy_model_on_textures(ref, images, name, pattern):
    img = images[name]
    h, w = img.shape
    pat = ou.seeded_pattern() if pattern == "seeded" else ou.corner_pattern()
    kp = ou.grid_keypoints(w, h)
    r = _describe_both(ref, img, pat, kp)
    n = len(kp)
    inside = int(r["info"][0])
    print(f"{name}, {pattern}: {n} keypoints, {inside} described, {int(r['info'][1])} outside")
    assert inside + int(r["info"][1]) == n and 0 < inside < n and not r["info"][2:].any()
    out = r["angle"][:n] == -1
    assert out.sum() == r["info"][1] and not r["desc"][:n][out].any()
    assert ((r["angle"][:n][~out] >= 0) & (r["angle"][:n][~out] <= 360)).all()
    distinct = len({bytes(d) for d in r["desc"][:n][~out]})
    assert distinct > inside // 2 if pattern == "seeded" else 1 < distinct <= 4        # (the corner pattern has two pairs)
    # other weights, a count below the list, a capacity above it: the tail is zero
    r2 = _describe_both(ref, img, pat, kp, weights=(70, 42, 33, 18), n=n - 5, cap=n + 9)
    assert not r2["desc"][n - 5:].any() and not r2["angle"][n - 5:].any()
    assert r2["blurred"].tobytes() != r["blurred"].tobytes()


def test_the_corner_pattern_reaches_eighteen():
    """Taps of (+-13, +-13) rotated by 45 degrees land 18 pixels from the centre: a centre at 19 reads column 1."""
    reach = 0
    for k in range(36001):
        a, b = ou.model_cos_sin(F(k / 100.0) * ou.FACTOR_PI)
        reach = max(reach, abs(int(np.rint(F(13) * b + F(13) * a))), abs(int(np.rint(F(13) * a - F(13) * b))))
    assert reach == 18 < ou.EDGE


def test_flat_edges_and_octants(ref, images):
    pat = ou.seeded_pattern()
    kp = np.array([[48, 40], [30, 40], [48, 25], [60.5, 40.5]], np.float32)
    r = _describe_both(ref, images["flat"], pat, kp)
    assert not r["desc"].any() and not r["angle"].any() and r["info"][0] == 4          # fastAtan2(0, 0) = 0, no tap is smaller
    # a horizontal edge through the centre row: m10 = 0 exactly, the angle folds to 90 or 270; a vertical one: 0 or 180
    m = np.zeros(2, np.int32)
    for name, centre, want in (("horizontal step", (48, 40), 90.0), ("horizontal step", (48, 39), 90.0),
                               ("vertical step", (48, 40), 0.0), ("vertical step", (47, 40), 0.0)):
        img = images[name]
        for flip in (False, True):
            im = np.ascontiguousarray(255 - img) if flip else img
            ref.orb_ref_moments(im.ctypes.data, im.strides[0], centre[0], centre[1], m.ctypes.data)
            assert tuple(m) == ou.model_moments(im, *centre)
            assert (m[0] == 0) == name.startswith("horizontal") and (m[1] == 0) == name.startswith("vertical")
            r = _describe_both(ref, im, pat, np.array([centre], np.float32))
            assert float(r["angle"][0]) == (want + 180.0 if flip else want), (name, centre, flip)
    octants = []
    for k in range(8):
        r = _describe_both(ref, images[f"gradient octant {k}"], pat, np.array([[48, 40], [40, 33]], np.float32))
        octants.append(int(r["angle"][0] // 45))
        assert abs(float(r["angle"][0]) - (22.5 + 45 * k)) < 1.0
    assert octants == list(range(8))


def test_fast_atan2_restatement_equals_the_model(ref):
    rng = np.random.default_rng(3)
    ys = np.concatenate([[0, 0, 1, -1, 5, -5, 0, 1300000, -1300000], rng.integers(-1300000, 1300001, 3000)])
    xs = np.concatenate([[0, 7, 0, 0, 5, 5, -3, 1300000, 1], rng.integers(-1300000, 1300001, 3000)])
    for y, x in zip(ys, xs):
        got, want = F(ref.orb_ref_fast_atan2(float(y), float(x))), ou.model_fast_atan2(y, x)
        assert got.tobytes() == want.tobytes(), (y, x)
        true = math.degrees(math.atan2(y, x)) % 360.0
        assert abs(float(got) - true) < 0.02 or abs(float(got) - true - 360) < 0.02, (y, x)        # OpenCV documents 0.3 degrees
    assert ref.orb_ref_fast_atan2(0.0, 0.0) == 0.0 and ref.orb_ref_fast_atan2(0.0, -4.0) == 180.0
    assert ref.orb_ref_fast_atan2(3.0, 0.0) == 90.0 and ref.orb_ref_fast_atan2(-3.0, 0.0) == 270.0


# ---- the blur ----------------------------------------------------------------------------------------------------------
def test_blur_closed_forms(ref):
    for wts in (ou.DEFAULT_WEIGHTS, (70, 42, 33, 18), (256, 0, 0, 0)):
        w7 = np.array([wts[abs(k)] for k in range(-3, 4)], np.int64)
        delta = np.zeros((41, 37), np.uint8)
        delta[20, 18] = 255
        want = np.zeros((41, 37), np.int64)
        want[17:24, 15:22] = (np.outer(w7, w7) * 255 + 32768) >> 16
        for got in (ou.ref_blur(ref, delta, wts), ou.model_blur(delta, wts)):
            assert np.array_equal(got, want)
        full = np.full((9, 4), 255, np.uint8)                      # the smallest width: every column is a border column
        for got in (ou.ref_blur(ref, full, wts), ou.model_blur(full, wts)):
            assert (got == 255).all()
    # a delta one pixel from the corner: the reflection folds a second tap onto it (r(-1) = 1)
    corner = np.zeros((12, 12), np.uint8)
    corner[1, 1] = 200
    got = ou.ref_blur(ref, corner)
    assert got.tobytes() == ou.model_blur(corner).tobytes()
    assert got[0, 0] == ((2 * 49) ** 2 * 200 + 32768) >> 16 and got[1, 1] == ((54 + 34) ** 2 * 200 + 32768) >> 16
    assert got[0, 1] == (2 * 49 * (54 + 34) * 200 + 32768) >> 16 and not got[5:, :].any() and not got[:, 5:].any()
    noise = np.random.default_rng(1).integers(0, 256, (33, 29), dtype=np.uint8)
    wide = np.zeros((33, 64), np.uint8)
    wide[:, :29] = noise
    assert ou.ref_blur(ref, wide[:, :29]).tobytes() == ou.model_blur(noise).tobytes()             # a pitch above the width


# ---- the steering pair ---------------------------------------------------------------------------------------------------
def _exact_cos_sin(x: Fraction, terms: int = 40):
    """cos and sin of a rational by their series: |x| < 7, 40 terms of each leave less than 7^80 / 80! < 1e-50."""
    c = s = Fraction(0)
    t = Fraction(1)
    for k in range(terms):
        c += t
        t = t * x / (2 * k + 1)
        s += t
        t = -t * x / (2 * k + 2)
    return c, s


def _round_f32(v: Fraction) -> np.float32:
    """The float32 nearest to a rational (ties cannot occur for the values used here: asserted)."""
    if v == 0:
        return F(0)
    a = abs(v)
    e = math.floor(math.log2(float(a)))
    while Fraction(2) ** e > a:
        e -= 1
    while Fraction(2) ** (e + 1) <= a:
        e += 1
    ulp = Fraction(2) ** (e - 23)
    q = a / ulp
    lo = q.numerator // q.denominator
    assert q - lo != Fraction(1, 2)
    m = lo + (1 if q - lo > Fraction(1, 2) else 0)
    return F(float(m * ulp) * (1 if v > 0 else -1))


def test_steering_pair_over_every_hundredth_degree(ref):
    a, b = C.c_float(0), C.c_float(0)
    disagree = []
    worst = 0.0
    for k in range(36001):
        r = F(k / 100.0) * ou.FACTOR_PI
        ref.orb_ref_cos_sin(float(r), C.addressof(a), C.addressof(b))
        ma, mb = ou.model_cos_sin(r)
        assert (F(a.value).tobytes(), F(b.value).tobytes()) == (ma.tobytes(), mb.tobytes()), k
        la, lb = F(np.cos(np.float64(r))), F(np.sin(np.float64(r)))
        if la.tobytes() != ma.tobytes() or lb.tobytes() != mb.tobytes():
            disagree.append(k)
    print(f"steering: {len(disagree)} of 36001 angles differ from the platform's cos / sin: {disagree[:10]}")
    # wherever the platform's library and the definition differ, exact arithmetic decides: the definition must be the
    # correctly rounded one
    for k in disagree:
        r = F(k / 100.0) * ou.FACTOR_PI
        ec, es = _exact_cos_sin(Fraction(float(r)))
        ma, mb = ou.model_cos_sin(r)
        assert (ma.tobytes(), mb.tobytes()) == (_round_f32(ec).tobytes(), _round_f32(es).tobytes()), k
    # the stated error bound of the f64 pair, on a sample (exact arithmetic is slow)
    for k in list(range(0, 36001, 257)) + [4500, 9000, 13500, 18000, 27000, 36000]:
        r = F(k / 100.0) * ou.FACTOR_PI
        x = float(r)
        kk = int(x * float.fromhex("0x1.45f306dc9c883p-1") + 0.5)
        t = (x - kk * float.fromhex("0x1.921fb544p+0")) - kk * float.fromhex("0x1.0b4611a626331p-34")
        assert abs(t) <= math.pi / 4 + 1e-9 and 0 <= kk <= 4
        ec, es = _exact_cos_sin(Fraction(x))
        z = t * t
        s = t + t * (z * (ou._S[0] + z * (ou._S[1] + z * (ou._S[2] + z * (ou._S[3] + z * (ou._S[4] + z * ou._S[5]))))))
        c = 1.0 - z * (0.5 - z * (ou._C[0] + z * (ou._C[1] + z * (ou._C[2] + z * (ou._C[3] + z * (ou._C[4] + z * ou._C[5]))))))
        co, si = ((c, s), (-s, c), (-c, -s), (s, -c))[kk & 3]
        worst = max(worst, abs(float(Fraction(co) - ec)), abs(float(Fraction(si) - es)))
    print(f"steering: largest error of the f64 pair on the sample {worst:.3g} (bound 2^-45 = {2.0 ** -45:.3g})")
    assert worst <= 2.0 ** -45


# ---- planted truth -----------------------------------------------------------------------------------------------------
def test_translated_image_gives_identical_descriptors_and_the_identity_match(ref):
    import detect_ref_util as du
    base = du.texture_image(synth, 200, 160, 21)
    img_a, img_b = np.ascontiguousarray(base[10:130, 10:170]), np.ascontiguousarray(base[8:128, 7:167])    # B(x + 3, y + 2) = A(x, y)
    h, w = img_a.shape
    assert np.array_equal(img_a[30:60, 40:80], img_b[32:62, 43:83])
    kp = np.array([(x, y) for y in range(22, h - 22 - 2, 6) for x in range(22, w - 22 - 3, 6)], np.float32)
    kp_b = kp + np.array([3, 2], np.float32)
    assert (kp_b[:, 0] < w - 22).all() and (kp_b[:, 1] < h - 22).all() and kp.min() >= 22
    pat = ou.seeded_pattern()
    da, db = _describe_both(ref, img_a, pat, kp), _describe_both(ref, img_b, pat, kp_b)
    n = len(kp)
    assert da["info"][0] == n == db["info"][0]
    assert da["desc"].tobytes() == db["desc"].tobytes() and da["angle"].tobytes() == db["angle"].tobytes()
    assert len({bytes(d) for d in da["desc"]}) == n                                    # no two keypoints look alike
    for m in (ou.ref_match(ref, da["desc"], db["desc"]), ou.model_match(da["desc"], db["desc"])):
        assert np.array_equal(m["train_idx"], np.arange(n)) and not m["distance"].any() and m["keep"].all()
        assert m["info"].tolist() == [n, n, n, 0, int(m["info"][4]), 30, 0, 0] and m["info"][4] == 0


# ---- the matcher -------------------------------------------------------------------------------------------------------
def _match_both(ref, dq, dt, **kw):
    r, m = ou.ref_match(ref, dq, dt, **kw), ou.model_match(dq, dt, **kw)
    assert ou.same(r, m, ou.MATCH_KEYS) == []
    return r


def test_matcher_rules(ref):
    dt = ou.random_descriptors(40, 1)
    # duplicates of one row at 3, 17 and 39: the lowest index wins; distance 0
    dt[17] = dt[3]
    dt[39] = dt[3]
    dq = np.stack([dt[3], dt[39], ou.flip_bits(dt[20], 5, 1), np.bitwise_not(dt[8])])
    r = _match_both(ref, dq, dt)
    assert r["train_idx"][:3].tolist() == [3, 3, 20] and r["distance"][:3].tolist() == [0, 0, 5]
    assert r["info"][:6].tolist() == [4, 4, 3, 0, int(r["distance"][3]), 30] and r["keep"].tolist() == [1, 1, 1, 0]
    # distance 256: one train row, the query its complement
    r = _match_both(ref, np.bitwise_not(dt[:1]), dt[:1])
    assert (r["train_idx"][0], r["distance"][0], r["keep"][0]) == (0, 256, 1) and r["info"][:6].tolist() == [1, 1, 1, 256, 256, 512]
    # both branches of the threshold, and a query exactly at it.  Train rows far from each other; queries 20, 40 and 41
    # bits from theirs: min_dist 20 -> threshold 40: 40 is kept, 41 is not
    base = ou.random_descriptors(3, 5)
    dq = np.stack([ou.flip_bits(base[0], 20, 2), ou.flip_bits(base[1], 40, 3), ou.flip_bits(base[2], 41, 4)])
    r = _match_both(ref, dq, base)
    assert r["distance"].tolist() == [20, 40, 41] and r["keep"].tolist() == [1, 1, 0] and r["info"][:6].tolist() == [3, 3, 2, 20, 41, 40]
    # min_dist 0 -> threshold = the floor: 30 is kept, 31 is not; another floor moves it
    dq = np.stack([base[0], ou.flip_bits(base[1], 30, 3), ou.flip_bits(base[2], 31, 4)])
    r = _match_both(ref, dq, base)
    assert r["keep"].tolist() == [1, 1, 0] and r["info"][:6].tolist() == [3, 3, 2, 0, 31, 30]
    r = _match_both(ref, dq, base, match_floor=31)
    assert r["keep"].tolist() == [1, 1, 1] and r["info"][5] == 31
    # no queries, no train rows, and a capacity beyond the count
    r = _match_both(ref, dq[:0], base)
    assert r["info"].tolist() == [0, 0, 0, 0, 0, 30, 0, 0] and (r["train_idx"][0], r["distance"][0], r["keep"][0]) == (-1, 257, 0)
    r = _match_both(ref, dq, base[:0])
    assert r["info"].tolist() == [3, 0, 0, 0, 0, 30, 0, 0]
    assert r["train_idx"].tolist() == [-1] * 3 and r["distance"].tolist() == [257] * 3 and not r["keep"].any()
    r = _match_both(ref, dq, base, cap_q=7, nq=2)
    assert r["train_idx"].tolist() == [0, 1, -1, -1, -1, -1, -1] and r["distance"][2:].tolist() == [257] * 5 and r["info"][0] == 2
    # a larger random case
    _match_both(ref, ou.random_descriptors(70, 8), ou.random_descriptors(130, 9))
