"""The device entry points against the reference's OWN ORB extractor, compiled: the committed outputs of oracle/_ref/ref_orb
(src/ORBextractor.cc of the reference, unchanged, on the project's stand-in OpenCV; tests/golden/ref_shim/orb/<case>.npz, written
by tests/golden/make_ref_shim.py over reference_cases.ORB_CASES).  Only the fixtures are read: neither the reference nor the
binary is needed here.  Every comparison is bit for bit, no row is left out, and pagk_check_launch is clean after every test.

The shapes are the table's: the smallest that reach each branch of the reference's text (62 x 62 up to 813 x 62 and 468 x 903,
most under 320 x 240).  What each row exists for, and the proof that it gets there, is tests/test_reference_orb_cpu.py's."""
import numpy as np
import pytest
import torch

import reference_cases as rc
import reference_orb_util as pu
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
NAMES = [c.name for c in rc.ORB_CASES if c.committed]
ONE_LEVEL = [c.name for c in rc.ORB_CASES if c.committed and c.n_levels == 1]
EXTRACT = [c.name for c in rc.ORB_CASES if c.committed and c.mode == "extract"]


@pytest.fixture(scope="module")
def fixtures():
    """name -> (inputs, the compiled reference's outputs), loaded once and left unchanged."""
    out = {}
    for name in NAMES:
        inp, want = rc.load_orb_fixture(name)
        for a in list(inp.values()) + list(want.values()):
            a.setflags(write=False)
        out[name] = (inp, want)
    return out


@pytest.fixture(autouse=True)
def launch_state_is_clean(ctx):
    yield
    ctx.check_launch()


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)   # (the fixtures are read-only)


def _ex(inp):
    e = pu.extractor_of(inp)
    return capi.orb_extractor_default(n_features=e.n_features, scale_factor=e.scale_factor, n_levels=e.n_levels,
                                      ini_threshold=e.ini_threshold, min_threshold=e.min_threshold)


def _fast(inp, n_features):
    e = pu.extractor_of(inp)
    return capi.fast_params_default(ini_threshold=e.ini_threshold, min_threshold=e.min_threshold, n_features=int(n_features))


def _level_want(want, l):
    """The reference's keypoints of level l (in the frame's coordinates, as it returns them), responses, angles, descriptors."""
    sel = want["octave"] == l
    return {k: want[k][sel] for k in ("kp", "response", "angle", "desc") if k in want}


def _device_detect(ctx, img, mask, fast, slot=2):
    h, w = img.shape
    cap = capi.detect_fast_bounds(w, h, fast.n_features)[1]
    ctx.frame_upload(slot, np.ascontiguousarray(img), 1)
    d_mask = None if mask is None else _dev(mask)
    d_k = torch.full((cap, 2), -7.0, dtype=torch.float32, device=DEV)
    d_r = torch.full((cap,), -7.0, dtype=torch.float32, device=DEV)
    d_i = torch.full((capi.DETECT_INFO_WORDS,), -7, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    ctx.detect_fast_device(fast, slot, d_mask, cap, d_k, d_r, d_i)
    ctx.sync()
    return d_k, d_i, dict(keypoints=d_k.cpu().numpy(), response=d_r.cpu().numpy(), info=d_i.cpu().numpy(), cap=cap)


# ---- pagk_detect_fast_device and pagk_detect_fast ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ONE_LEVEL)
def test_one_level_detector(ctx, fixtures, name):
    """A one-level row IS the detector's result: keypoints, responses, the count, the raw count (from the FAST log) and the
    number of nodes."""
    inp, want = fixtures[name]
    n, raw = len(want["kp"]), len(pu.cells_of_log(want, 0)["xy"])
    fast = _fast(inp, inp["cfg"][0])
    _, _, dev = _device_detect(ctx, inp["img"], inp.get("mask"), fast)
    host = ctx.detect_fast(inp["img"], inp.get("mask"), fast.n_features, fast)
    print(f"{name}: {n} keypoints of {raw} raw for N = {fast.n_features}")
    for got, kp, resp in ((dev, dev["keypoints"], dev["response"]), (host, host["buffer"], host["response_buffer"])):
        assert got["info"][[0, 1, 4]].tolist() == [n, raw, n], name
        assert kp[:n].tobytes() == want["kp"].tobytes() and resp[:n].tobytes() == want["response"].tobytes(), name
        assert not kp[n:].any() and not resp[n:].any()
    if name in ("one_cell_62x62", "nini2_ties_91x62"):
        assert n > fast.n_features                  # a result longer than N
    if name in ("prev_size_planted", "nini2_boundary_key"):
        assert 0 < n == raw < fast.n_features       # every node ended with one key
    if name == "flat_255":
        assert n == raw == 0


@pytest.mark.parametrize("name", [n for n in NAMES if n not in ONE_LEVEL and n != "masked_levels4"])
def test_detector_on_every_level_image(ctx, fixtures, name):
    """Above level 0 the reference returns a keypoint scaled by the level's factor: the detector on the reference's level
    image with N = max(quota, 1), scaled in float32, is the reference's list of that octave."""
    inp, want = fixtures[name]
    counts = np.bincount(want["octave"], minlength=len(want["scale"]))
    assert (counts >= 1).all()
    for l, img in enumerate(pu.level_images(want)):
        lw = _level_want(want, l)
        got = ctx.detect_fast(img, None, max(int(want["quota"][l]), 1), _fast(inp, 1))
        kp = got["keypoints"] if l == 0 else (got["keypoints"] * want["scale"][l]).astype(F)
        assert kp.tobytes() == lw["kp"].tobytes() and got["response"].tobytes() == lw["response"].tobytes(), (name, l)


# ---- pagk_selftest_fast_cells -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_raw_list_against_the_fast_log(ctx, fixtures, name):
    inp, want = fixtures[name]
    total = 0
    for l, img in enumerate(pu.level_images(want)):
        log = pu.cells_of_log(want, l)
        got = ctx.selftest_fast_cells(np.ascontiguousarray(img), _fast(inp, 1))
        assert got["n"] == len(log["xy"]) and got["xy"].tobytes() == log["xy"].tobytes() and got["score"].tobytes() == log["score"].tobytes(), (name, l)
        total += got["n"]
    if name == "fallback_152x92":
        assert pu.cells_of_log(want, 0)["first_empty"] >= 3 and pu.cells_of_log(want, 0)["empty"] >= 1
    if name == "column_skip_813x62":
        assert len(pu.cells_of_log(want, 0)["cells"]) == 25
    if name == "row_skip_468x903":
        assert len(pu.cells_of_log(want, 0)["cells"]) == 28 * 14
    assert total > 0 or name == "flat_255"


# ---- pagk_orb_describe_device and pagk_orb_describe ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", EXTRACT)
def test_describe_on_the_references_keypoints(ctx, fixtures, name):
    """Angle and descriptors of every level's keypoints on the reference's level image.  Level 0's keypoints are the
    fixture's; above, the level's own coordinates are the detector's (which, scaled, are the fixture's: asserted)."""
    inp, want = fixtures[name]
    ctx.orb_set_pattern(inp["pattern"])
    for l, img in enumerate(pu.level_images(want)):
        lw = _level_want(want, l)
        n = len(lw["kp"])
        assert n >= 1
        d_k, d_i, det = _device_detect(ctx, img, None, _fast(inp, max(int(want["quota"][l]), 1)))
        kp = det["keypoints"][:n]
        assert det["info"][0] == n and (kp if l == 0 else (kp * want["scale"][l]).astype(F)).tobytes() == lw["kp"].tobytes()
        cap = det["cap"]
        d_a = torch.full((cap,), -7.0, dtype=torch.float32, device=DEV)
        d_d = torch.full((cap, 32), 0x5a, dtype=torch.uint8, device=DEV)
        d_oi = torch.full((capi.ORB_INFO_WORDS,), -7, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        ctx.orb_describe_device(capi.orb_params_default(), 2, cap, d_k, d_i, d_a, d_d, d_oi)
        ctx.sync()
        assert d_oi.cpu().numpy()[:2].tolist() == [n, 0]
        assert d_a.cpu().numpy()[:n].tobytes() == lw["angle"].tobytes() and d_d.cpu().numpy()[:n].tobytes() == lw["desc"].tobytes(), (name, l)
        host = ctx.orb_describe(np.ascontiguousarray(img), lw["kp"] if l == 0 else kp)
        assert host["angle"].tobytes() == lw["angle"].tobytes() and host["desc"].tobytes() == lw["desc"].tobytes(), (name, l)
    if name == "size_tie_75x75":
        assert (np.bincount((want["angle"] // 45).astype(int), minlength=8) >= 1).all()      # every octant
    if name == "nini2_boundary_key":
        assert (want["angle"] == 0).sum() >= 1                                               # the flat disc
    if name == "levels2_1p5_corner":
        assert np.abs(inp["pattern"]).min() == 13


# ---- pagk_orb_extractor_levels (needs no device) ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_level_table(fixtures, name):
    inp, want = fixtures[name]
    h, w = inp["img"].shape
    t = capi.orb_extractor_levels(_ex(inp), w, h)
    assert t["rc"] == 0 and t["n_levels"] == len(want["scale"])
    assert np.asarray(t["scale"], F).tobytes() == want["scale"].tobytes() and np.asarray(t["quota"], np.int32).tobytes() == want["quota"].tobytes()
    assert list(zip(np.asarray(t["height"]).tolist(), np.asarray(t["width"]).tolist())) == [lv.shape for lv in pu.level_images(want)]
    assert np.array_equal(np.asarray(t["size"])[want["octave"]].astype(F), want["size"])
    if name == "quota_tie_1p4":
        assert want["quota"].tolist() == [94, 68]
    if name == "quota_zero_last":
        assert want["quota"].tolist() == [1, 1, 0]
    if name == "size_tie_75x75":
        assert want["level_1"].shape == (62, 62)


# ---- the slot form, the host forms, every level image -------------------------------------------------------------------------
def _assert_set(got, want, keys, what):
    n = len(want["kp"])
    L = len(want["scale"])
    assert got["n"] == n == got["info"][0] and got["info"][2] == L, what
    assert got["info"][8:8 + L].tolist() == np.bincount(want["octave"], minlength=L).tolist(), what
    assert got["info"][24:24 + L].tolist() == want["quota"].tolist(), what
    names = dict(kp="keypoints")
    for k in keys:
        full = got["full_" + names.get(k, k)]
        assert full[:n].tobytes() == want[k].tobytes(), (what, k)
        assert not full[n:].any(), (what, k)


@pytest.mark.parametrize("name", EXTRACT)
def test_extract_slot_and_host_form(ctx, fixtures, name):
    inp, want = fixtures[name]
    h, w = inp["img"].shape
    ex = _ex(inp)
    cap = capi.orb_extractor_levels(ex, w, h)["out_bound"]
    ctx.orb_set_pattern(inp["pattern"])
    ctx.frame_upload(1, np.ascontiguousarray(inp["img"]), 1)
    ctx.orb_extract_slot(ex, 1)
    got = ctx.orb_slot_read(1, cap)
    keys = ("kp", "octave", "response", "angle", "desc")
    _assert_set(got, want, keys, name + " (slot)")
    for l, lv in enumerate(pu.level_images(want)):
        assert ctx.selftest_orb_level(1, l, lv.shape[1], lv.shape[0]).tobytes() == lv.tobytes(), (name, l)
    _assert_set(ctx.orb_extract_levels(np.ascontiguousarray(inp["img"]), ex), want, keys, name + " (host)")
    _assert_set(ctx.orb_detect_levels(np.ascontiguousarray(inp["img"]), ex), want, ("kp", "octave", "response"), name + " (detect)")
    assert (np.bincount(want["octave"], minlength=len(want["scale"])) >= 1).all()


@pytest.mark.parametrize("name", [n for n in NAMES if n not in EXTRACT])
def test_detect_levels(ctx, fixtures, name):
    """DetectFeatures: with the row's mask, or with none and with all ones (the reference ran with all ones)."""
    inp, want = fixtures[name]
    ex, img = _ex(inp), np.ascontiguousarray(inp["img"])
    keys = ("kp", "octave", "response")
    if "mask" in inp:
        _assert_set(ctx.orb_detect_levels(img, ex, inp["mask"]), want, keys, name)
        free = ctx.orb_detect_levels(img, ex, None)
        gone = np.bincount(free["octave"], minlength=4) - np.bincount(want["octave"], minlength=4)
        assert gone[0] >= 1 and gone[1:].sum() >= 1 and (gone >= 0).all()      # the mask drops keypoints of levels above 0
    else:
        _assert_set(ctx.orb_detect_levels(img, ex, None), want, keys, name)
        _assert_set(ctx.orb_detect_levels(img, ex, np.ones_like(img)), want, keys, name)
    if name == "quota_zero_last":
        assert (want["octave"] == 2).sum() >= 1          # the level with quota 0 ran with N = 1
