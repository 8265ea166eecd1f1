"""GPU tests of ORB over a scale pyramid (include/pagk.h "ORB over a scale pyramid"): every pyramid level, the extract and
the masked detect host forms, the slot form, the match between two slots' sets, capture and replay, independence from what
the workspaces held, and the refusals -- every comparison bit for bit with the plain-C restatement
(tests/orb_levels_ref.c on top of tests/fast_detect_ref.c and tests/orb_ref.c).  The shapes are the smallest at which the
code can still go wrong: 97 x 80 with 2 levels (the smallest legal two-level image), 160 x 120 with 4 (odd level sizes 133,
111, 93, 69 and nIni 1 and 2), 120 x 160 with 4 (portrait), 320 x 240 with 8 (the smallest 4:3 image that holds the full
pyramid)."""
import numpy as np
import pytest
import torch

import orb_levels_ref_util as lu
import orb_ref_util as ou
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, host_api, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATTERNS = {"seeded": ou.seeded_pattern, "corners": ou.corner_pattern}
SHAPES = [((97, 80), 2), ((160, 120), 4), ((120, 160), 4), ((320, 240), 8)]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return lu.build_ref(tmp_path_factory.mktemp("orb_levels_ref"))


@pytest.fixture(scope="module")
def oref(tmp_path_factory):
    return ou.build_ref(tmp_path_factory.mktemp("orb_ref"))


def _ex(**kw):
    return capi.orb_extractor_default(**kw)


def _image(w, h, seed=23):
    return lu.texture(synth, w, h, seed)


@pytest.fixture(scope="module")
def restated(ref):
    """(w, h, seed, n_levels, n_features, pattern name or None, mask key) -> the restatement, computed once and left unchanged."""
    memo = {}

    def get(w, h, nl, nf, pattern="seeded", seed=23, mask=None):
        key = (w, h, nl, nf, pattern, seed, None if mask is None else mask.tobytes())
        if key not in memo:
            pat = None if pattern is None else PATTERNS[pattern]()
            memo[key] = lu.ref_extract(ref, _image(w, h, seed), _ex(n_levels=nl, n_features=nf), pat, mask)
        return memo[key]
    return get


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _set_slot(ctx, slot, img, pitch=None):
    """The image into a frame slot: uploaded, or read in place from the left columns of a wider device buffer (returned: the
    caller keeps it alive while the slot is used)."""
    h, w = img.shape
    if pitch is None:
        ctx.frame_upload(slot, img, 1)
        return None
    keep = torch.full((h, pitch), 255, dtype=torch.uint8, device=DEV)
    keep[:, :w] = _dev(img)
    torch.cuda.synchronize()
    ctx.frame_set_device(slot, keep.data_ptr(), w, h, pitch, 1)
    return keep


# ---- the pyramid -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, nl", SHAPES)
def test_every_pyramid_level_with_a_slot_pitch_above_the_width(ctx, restated, shape, nl):
    w, h = shape
    want = restated(w, h, nl, 1000)
    ctx.orb_set_pattern(ou.seeded_pattern())
    keep = _set_slot(ctx, 2, _image(w, h), pitch=w + 5)
    ctx.orb_extract_slot(_ex(n_levels=nl), 2)
    for l, lv in enumerate(want["levels"]):
        lh, lw = lv.shape
        got = ctx.selftest_orb_level(2, l, lw, lh, pitch=lw + 3)
        assert got.tobytes() == lv.tobytes(), (shape, l)
    with pytest.raises(capi.PagkError):
        ctx.selftest_orb_level(2, nl, 62, 62)
    with pytest.raises(capi.PagkError):
        ctx.selftest_orb_level(2, 1, int(want["table"]["width"][1]), int(want["table"]["height"][1]), pitch=int(want["table"]["width"][1]) - 1)
    got = ctx.orb_slot_read(2, want["cap"])
    assert lu.same_set(got, want) == []
    del keep


# ---- the extract host form -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["seeded", "corners"])
@pytest.mark.parametrize("shape, nl, nf", [((160, 120), 4, 1000), ((320, 240), 8, 1000), ((320, 240), 8, 10), ((160, 120), 3, 1)])
def test_extract_host_form(ctx, restated, shape, nl, nf, pattern):
    w, h = shape
    want = restated(w, h, nl, nf, pattern)
    got = host_api.orb_extract_levels(_image(w, h), _ex(n_levels=nl, n_features=nf), PATTERNS[pattern](), ctx=ctx)
    print(f"{w} x {h}, {nl} levels, {nf} features, {pattern}: quotas {want['table']['quota'].tolist()}, "
          f"counts {want['info'][8:8 + nl].tolist()}, outside {int(want['info'][1])}")
    assert lu.same_set(got, want) == []
    assert got["n"] == want["n"] > 0 and got["n_levels"] == nl
    if nf == 10:
        assert want["table"]["quota"][-1] == 0 and want["info"][8 + nl - 1] >= 1      # quota 0 runs with N = 1
    if nf == 1:
        assert want["table"]["quota"].tolist() == [0, 0, 1]
    # a capacity above out_bound: the rows beyond it are zeroed
    big = ctx.orb_extract_levels(_image(w, h), _ex(n_levels=nl, n_features=nf), cap=want["cap"] + 9)
    for k in ("keypoints", "octave", "response", "angle", "desc"):
        assert big["full_" + k][:want["cap"]].tobytes() == want[k].tobytes() and not big["full_" + k][want["cap"]:].any(), k


def test_flat_image_gives_no_keypoints(ctx):
    ctx.orb_set_pattern(ou.seeded_pattern())
    got = ctx.orb_extract_levels(np.full((240, 320), 99, np.uint8), _ex(n_levels=8))
    assert got["n"] == 0 and not got["info"][:2].any() and got["info"][2] == 8 and not got["info"][8:24].any()
    assert not got["full_keypoints"].any() and not got["full_desc"].any() and not got["full_angle"].any()


# ---- the masked detect -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, nl", [((160, 120), 4), ((320, 240), 8)])
def test_masked_detect(ctx, restated, shape, nl):
    w, h = shape
    mask = np.ones((h, w), np.uint8)
    mask[h // 4:3 * h // 4, w // 4:11 * w // 16] = 0
    full, want = restated(w, h, nl, 1000, None), restated(w, h, nl, 1000, None, mask=mask)
    n = full["n"]
    gone = mask[full["keypoints"][:n, 1].astype(np.int64), full["keypoints"][:n, 0].astype(np.int64)] == 0
    assert (gone & (full["octave"][:n] > 0)).any() and 0 < want["n"] == n - int(gone.sum())      # upper-level keypoints go too
    ex = _ex(n_levels=nl)
    got = host_api.orb_detect_levels(_image(w, h), ex, mask, ctx=ctx)
    assert lu.same_set(got, want, lu.DETECT_KEYS) == []
    assert lu.same_set(host_api.orb_detect_levels(_image(w, h), ex, None, ctx=ctx), full, lu.DETECT_KEYS) == []
    assert lu.same_set(host_api.orb_detect_levels(_image(w, h), ex, np.ones((h, w), np.uint8), ctx=ctx), full, lu.DETECT_KEYS) == []
    none = host_api.orb_detect_levels(_image(w, h), ex, np.zeros((h, w), np.uint8), ctx=ctx)
    assert none["n"] == 0 and not none["full_keypoints"].any() and none["info"][16:16 + nl].tobytes() == full["info"][16:16 + nl].tobytes()


# ---- the slot form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, nl", SHAPES)
def test_slot_form_equals_host_form(ctx, restated, shape, nl):
    w, h = shape
    want = restated(w, h, nl, 1000)
    ctx.orb_set_pattern(ou.seeded_pattern())
    ex = _ex(n_levels=nl)
    host = ctx.orb_extract_levels(_image(w, h), ex)
    for slot, pitch in ((0, None), (3, w + 1)):
        keep = _set_slot(ctx, slot, _image(w, h), pitch)
        ctx.orb_extract_slot(ex, slot)
        got = ctx.orb_slot_read(slot, want["cap"])
        assert lu.same_set(got, want) == [] and lu.same_set(got, {k: host["info"] if k == "info" else host["full_" + k] for k in lu.SET_KEYS}) == []
        only_kp = np.zeros((want["cap"], 2), np.float32)        # any array but keypoints may be NULL
        ctx._check(ctx.lib.pagk_orb_slot_read(ctx.h, slot, want["cap"], only_kp.ctypes.data, None, None, None, None, None), "read")
        assert only_kp.tobytes() == want["keypoints"].tobytes()
        del keep


def test_one_level_equals_the_existing_one_level_path(ctx):
    for (w, h), nf in (((160, 120), 80), ((320, 240), 1000), ((97, 80), 5)):
        img, pat = _image(w, h), ou.seeded_pattern()
        one = host_api.orb_extract(img, nf, pat, ctx=ctx)
        got = host_api.orb_extract_levels(img, _ex(n_levels=1, n_features=nf), pat, ctx=ctx)
        n = got["n"]
        assert n == len(one["keypoints"]) > 0 and got["cap"] == capi.detect_fast_bounds(w, h, nf)[1]
        for k in ("keypoints", "response", "angle", "desc"):
            assert got[k].tobytes() == np.asarray(one[k]).tobytes(), (w, h, k)
        assert not got["octave"].any() and got["info"][1] == one["describe_info"][1] and got["info"][16] == one["detect_info"][1]
        assert got["info"][24] == nf and got["info"][8] == n


# ---- matching --------------------------------------------------------------------------------------------------------------
def test_match_slots_equals_match_on_the_read_back_descriptors(ctx, oref, restated):
    w, h, nl = 160, 120, 4
    a, b = restated(w, h, nl, 400, seed=23), restated(w, h, nl, 400, seed=24)
    out = host_api.orb_match_pair_levels(_image(w, h, 23), _image(w, h, 24), _ex(n_levels=nl, n_features=400), ou.seeded_pattern(), ctx=ctx)
    assert lu.same_set(out["ref"], a) == [] and lu.same_set(out["cur"], b) == []
    nq, nt = a["n"], b["n"]
    direct = ctx.orb_match(out["ref"]["desc"], out["cur"]["desc"])
    want = ou.ref_match(oref, a["desc"][:nq], b["desc"][:nt], cap_q=a["cap"], nq=nq, nt=nt)
    got = ctx.orb_match_slots_read(0, a["cap"])
    print(f"match info {got['info'][:6].tolist()}")
    assert ou.same(got, want, ou.MATCH_KEYS) == []
    assert ou.same(out, direct, ou.MATCH_KEYS) == [] and got["nq"] == nq and 0 < got["kept"] <= nq
    # the other direction keeps its own result; a capacity above the set's: the rows beyond are -1 / 257 / 0
    ctx.orb_match_slots(1, 0)
    back = ctx.orb_match_slots_read(1, b["cap"] + 4)
    want_b = ou.ref_match(oref, b["desc"][:nt], a["desc"][:nq], cap_q=b["cap"] + 4, nq=nt, nt=nq)
    assert ou.same(back, want_b, ou.MATCH_KEYS) == []
    assert ou.same(ctx.orb_match_slots_read(0, a["cap"]), want, ou.MATCH_KEYS) == []


# ---- capture ---------------------------------------------------------------------------------------------------------------
def test_capture_two_extracts_and_the_match_and_replay(oref, restated):
    w, h, nl, nf = 160, 120, 4, 400
    seeds = (23, 24, 25, 26)
    pairs = [(0, 1), (2, 3), (1, 2)]
    ex, big = _ex(n_levels=nl, n_features=nf), _ex(n_levels=nl, n_features=4000)
    cap = restated(w, h, nl, nf)["cap"]
    c = capi.Context(0)
    try:
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            c.set_stream(stream.cuda_stream)
            c.orb_set_pattern(ou.seeded_pattern())
            d_img = [torch.zeros((h, w), dtype=torch.uint8, device=DEV) for _ in range(2)]

            def work():
                for s in range(2):
                    c.frame_set_device(s, d_img[s].data_ptr(), w, h, w, 1)
                    c.orb_extract_slot(ex, s)
                c.orb_match_slots(0, 1)

            def feed(pair):
                for s in range(2):
                    d_img[s].copy_(_dev(_image(w, h, seeds[pair[s]])))

            def snapshot():
                sets = [c.orb_slot_read(s, cap) for s in range(2)]
                m = c.orb_match_slots_read(0, cap)
                return sets, m

            def check(pair, how):
                sets, m = snapshot()
                want = [restated(w, h, nl, nf, seed=seeds[pair[s]]) for s in range(2)]
                for s in range(2):
                    assert lu.same_set(sets[s], want[s]) == [], (how, pair, s)
                wm = ou.ref_match(oref, want[0]["desc"][:want[0]["n"]], want[1]["desc"][:want[1]["n"]], cap_q=cap,
                                  nq=want[0]["n"], nt=want[1]["n"])
                print(f"{how} {pair}: match info {m['info'][:6].tolist()}")
                assert ou.same(m, wm, ou.MATCH_KEYS) == [], (how, pair)

            for pair in pairs:                        # the direct calls (the first one sizes every buffer)
                feed(pair)
                work()
                check(pair, "direct")
            c.graph_begin()
            try:
                with pytest.raises(capi.PagkError):   # the host-buffer and reading forms are not capturable
                    c.orb_extract_levels(_image(w, h), ex)
                with pytest.raises(capi.PagkError):
                    c.orb_detect_levels(_image(w, h), ex)
                with pytest.raises(capi.PagkError):
                    c.orb_slot_read(0, cap)
                with pytest.raises(capi.PagkError):
                    c.orb_match_slots_read(0, cap)
                with pytest.raises(capi.PagkError):
                    c.selftest_orb_level(0, 1, 133, 100)
                work()
                with pytest.raises(capi.PagkError) as e:   # growth under a capture
                    c.orb_extract_slot(big, 0)
                assert e.value.code == capi.PAGK_E_ARG
            finally:
                gid = c.graph_end()
            with pytest.raises(capi.PagkError) as e:       # growth under a live graph
                c.orb_extract_slot(big, 0)
            assert e.value.code == capi.PAGK_E_ARG
            for _ in range(2):
                for pair in (pairs[1], pairs[2], pairs[0]):   # replays with other images: each equals the direct calls
                    feed(pair)
                    c.graph_launch(gid)
                    check(pair, "replay")
            c.graph_destroy(gid)
            c.orb_extract_slot(big, 0)                        # ... and free to grow once the graph is gone
            assert c.orb_slot_read(0, restated(w, h, nl, 4000)["cap"])["n"] > 0
    finally:
        c.set_stream(None)
        c.close()


# ---- what the workspaces held ----------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_what_the_workspaces_held(oref, restated):
    w, h, nl, nf = 160, 120, 4, 400
    mask = np.ones((h, w), np.uint8)
    mask[30:90, 40:110] = 0
    want = [restated(w, h, nl, nf, seed=s) for s in (23, 24)]
    want_det = restated(w, h, nl, nf, None, mask=mask)
    ex = _ex(n_levels=nl, n_features=nf)
    c = capi.Context(0)
    try:
        c.orb_set_pattern(ou.seeded_pattern())
        for word, also_new in ((0xFFFFFFFF, True), (0x00000000, True), (0x7FC00001, False)):
            c.selftest_fill_workspaces(word, also_new)
            with pytest.raises(capi.PagkError):       # no slot is valid and no slot has a set after the fill
                c.orb_extract_slot(ex, 0)
            with pytest.raises(capi.PagkError):
                c.orb_slot_read(0, want[0]["cap"])
            assert lu.same_set(c.orb_extract_levels(_image(w, h, 23), ex), want[0]) == [], hex(word)
            assert lu.same_set(c.orb_detect_levels(_image(w, h, 23), ex, mask), want_det, lu.DETECT_KEYS) == [], hex(word)
            for s in range(2):
                c.frame_upload(s, _image(w, h, 23 + s), 1)
                c.orb_extract_slot(ex, s)
            c.orb_match_slots(0, 1)
            for s in range(2):
                assert lu.same_set(c.orb_slot_read(s, want[s]["cap"]), want[s]) == [], (hex(word), s)
            wm = ou.ref_match(oref, want[0]["desc"][:want[0]["n"]], want[1]["desc"][:want[1]["n"]], cap_q=want[0]["cap"],
                              nq=want[0]["n"], nt=want[1]["n"])
            assert ou.same(c.orb_match_slots_read(0, want[0]["cap"]), wm, ou.MATCH_KEYS) == [], hex(word)
            lv = want[1]["levels"][3]
            assert c.selftest_orb_level(1, 3, lv.shape[1], lv.shape[0]).tobytes() == lv.tobytes(), hex(word)
    finally:
        c.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_arguments_are_checked_on_a_live_context(restated):
    w, h = 160, 120
    img, ex = _image(w, h), _ex(n_levels=4)
    cap = restated(w, h, 4, 1000)["cap"]
    c = capi.Context(0)
    try:
        c.frame_upload(0, img, 1)
        with pytest.raises(capi.PagkError) as e:                     # no pattern yet
            c.orb_extract_slot(ex, 0)
        assert e.value.code == capi.PAGK_E_ARG and "pattern" in str(e.value)
        with pytest.raises(capi.PagkError) as e:
            c.orb_extract_levels(img, ex)
        assert e.value.code == capi.PAGK_E_ARG and "pattern" in str(e.value)
        assert c.orb_detect_levels(img, ex)["n"] > 0                 # DetectFeatures needs none
        c.orb_set_pattern(ou.seeded_pattern())
        with pytest.raises(capi.PagkError) as e:                     # an empty slot
            c.orb_extract_slot(ex, 1)
        assert e.value.code == capi.PAGK_E_ARG
        for slot in (-1, 4, 5):                                      # the scratch slots are not the caller's
            with pytest.raises(capi.PagkError):
                c.orb_extract_slot(ex, slot)
        with pytest.raises(capi.PagkError):                          # nothing extracted yet: no set, no match, no level
            c.orb_slot_read(0, cap)
        with pytest.raises(capi.PagkError):
            c.orb_match_slots(0, 0)
        with pytest.raises(capi.PagkError):
            c.selftest_orb_level(0, 0, w, h)
        c.orb_extract_slot(ex, 0)
        assert c.orb_slot_read(0, cap)["n"] == restated(w, h, 4, 1000)["n"]
        with pytest.raises(capi.PagkError) as e:                     # cap below out_bound
            c.orb_slot_read(0, cap - 1)
        assert e.value.code == capi.PAGK_E_ARG
        with pytest.raises(capi.PagkError):
            c.orb_extract_levels(img, ex, cap=cap - 1)
        with pytest.raises(capi.PagkError):
            c.orb_detect_levels(img, ex, cap=cap - 1)
        with pytest.raises(capi.PagkError):                          # slot 1 has no set: no match, and nothing to read
            c.orb_match_slots(0, 1)
        with pytest.raises(capi.PagkError):
            c.orb_match_slots_read(0, cap)
        c.orb_match_slots(0, 0)
        assert c.orb_match_slots_read(0, cap)["min_dist"] == 0
        with pytest.raises(capi.PagkError):
            c.orb_match_slots_read(0, cap - 1)
        for bad in (dict(n_levels=5), dict(n_levels=0), dict(n_levels=9), dict(scale_factor=1.0), dict(scale_factor=1.6),
                    dict(n_features=0), dict(ini_threshold=256)):    # 160 x 120 with 5 levels: the last level is too small
            with pytest.raises(capi.PagkError) as e:
                c.orb_extract_slot(_ex(**bad), 0)
            assert e.value.code == capi.PAGK_E_ARG, bad
            with pytest.raises(capi.PagkError):
                c.orb_extract_levels(img, _ex(**bad), cap=100000)
            with pytest.raises(capi.PagkError):
                c.orb_detect_levels(img, _ex(**bad), cap=100000)
        with pytest.raises(capi.PagkError):
            c.orb_extract_levels(_image(97, 80), _ex(n_levels=3), cap=100000)      # third level 67 x 56
        for bad in (dict(n_levels=2), dict(blur_weights=(55, 49, 34, 18))):          # orb->n_levels stays 1
            with pytest.raises(capi.PagkError) as e:
                c.orb_extract_slot(ex, 0, capi.orb_params_default(**bad))
            assert e.value.code == (capi.PAGK_E_UNSUPPORTED if "n_levels" in bad else capi.PAGK_E_ARG), bad
        # a detect form's set has no descriptors to match; the slot keeps working afterwards
        assert lu.same_set(c.orb_extract_levels(img, ex), restated(w, h, 4, 1000)) == []
    finally:
        c.close()
