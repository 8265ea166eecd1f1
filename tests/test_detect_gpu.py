"""GPU tests of the device-side corner detector: pagk_selftest_corner_response, pagk_detect_corners[_device] and
pagk_frame_handover_detect[_device] against the plain-C restatements (tests/corner_detect_ref.c, frame_handover_ref.c),
byte for byte; capture and replay; runtime.SequenceTracker(detector=...) against a host loop."""
import numpy as np
import pytest
import torch

import detect_ref_util as du
import handover_ref_util as hu
from sequence_model import restated_handover_detect as _restated_handover_detect
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, distributed, host_api, runtime, synth

pytestmark = pytest.mark.gpu
W, H = 640, 480


@pytest.fixture(scope="module")
def dref(tmp_path_factory):
    return du.build_ref(tmp_path_factory.mktemp("detect_ref"))


@pytest.fixture(scope="module")
def href(tmp_path_factory):
    return hu.build_ref(tmp_path_factory.mktemp("handover_ref"))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _images():
    """name -> (image, mask, max_corners)"""
    tex = du.texture_image(synth, W, H, 7)
    return {
        "texture": (tex, None, 1000),
        "noise": (du.noise_image(W, H), None, 1000),
        "all 255": (np.full((H, W), 255, np.uint8), None, 100),
        "mask all zero": (tex, np.zeros((H, W), np.uint8), 100),
        "mask with holes": (tex, du.holes_mask(W, H), 1000),
        "planted squares": (du.planted_squares(W, H)[0], None, 300),
        "tie bar": (du.tie_bar(), None, 10),
        "752x480": (du.texture_image(synth, 752, 480, 1), None, 1000),          # 9 638 raw candidates
        "1920x1080": (du.texture_image(synth, 1920, 1080, 3), None, 20000),     # the sort past one workgroup's block
        "641x479": (du.texture_image(synth, 641, 479, 9), du.holes_mask(641, 479, 120), 700),
        "14x14": (du.noise_image(14, 14, 3), None, 20),
    }


IMAGE_NAMES = ["texture", "noise", "all 255", "mask all zero", "mask with holes", "planted squares", "tie bar", "752x480",
               "1920x1080", "641x479", "14x14"]


@pytest.fixture(scope="module")
def images():
    return _images()


@pytest.mark.parametrize("name", IMAGE_NAMES)
def test_response_map(ctx, dref, images, name):
    img = images[name][0]
    got = ctx.selftest_corner_response(img)
    want = du.ref_response(dref, img)
    bad = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
    print(f"{name}: {img.shape[1]} x {img.shape[0]}, {bad.size} responses differ" +
          (f", first at pixel {int(bad[0])}: {got.ravel()[bad[0]]!r} vs {want.ravel()[bad[0]]!r}" if bad.size else ""))
    assert bad.size == 0


@pytest.mark.parametrize("name", IMAGE_NAMES)
def test_detect_corners_host_form(ctx, dref, images, name):
    img, mask, mc = images[name]
    kw = dict(min_distance=0.5) if name == "tie bar" else {}
    got = ctx.detect_corners(img, mask, mc, capi.detect_params_default(**kw))
    want = du.ref_detect(dref, img, mask, mc, **kw)
    print(f"{name}: info {got['info'][:5].tolist()} (restated {want['info'][:5].tolist()})")
    assert got["info"].tobytes() == want["info"].tobytes()
    assert got["buffer"].tobytes() == want["corners"].tobytes()
    if name == "1920x1080":
        assert got["raw"] > 16384
    if name == "planted squares":
        assert set(map(tuple, got["corners"].astype(int).tolist())) == set(du.planted_squares(W, H)[1])
    if name == "tie bar":
        assert got["corners"].tolist() == [[32.0, 39.0], [32.0, 10.0]]


def _device_detect(ctx, img, mask, cap, max_corners, det, slot=2):
    ctx.frame_upload(slot, img, 1)
    d_mask = None if mask is None else _dev(mask)
    d_max = None if max_corners is None else _dev(np.array([max_corners], np.int32))
    d_c = torch.full((cap, 2), -7.0, dtype=torch.float32, device="cuda:0")
    d_i = torch.full((capi.DETECT_INFO_WORDS,), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.detect_corners_device(det, slot, d_mask, cap, d_max, d_c, d_i)
    ctx.sync()
    return dict(corners=d_c.cpu().numpy(), info=d_i.cpu().numpy())


@pytest.mark.parametrize("name", IMAGE_NAMES)
def test_detect_corners_device_form(ctx, dref, images, name):
    img, mask, mc = images[name]
    kw = dict(min_distance=0.5) if name == "tie bar" else {}
    got = _device_detect(ctx, img, mask, mc, None, capi.detect_params_default(**kw))
    want = du.ref_detect(dref, img, mask, mc, **kw)
    print(f"{name}: info {got['info'][:5].tolist()} (restated {want['info'][:5].tolist()})")
    assert du.same_detect(got, want) == []


def test_device_limit_word_determinism_and_overflow(ctx, dref, images):
    img, mask, _ = images["mask with holes"]
    det = capi.detect_params_default()
    cap = 300
    for mc in (0, 1, -4, 57, cap, cap + 1000):          # the device word: 0, 1, negative, above cap
        got = _device_detect(ctx, img, mask, cap, mc, det)
        want = du.ref_detect(dref, img, mask, mc, cap=cap)
        print(f"*d_max_corners = {mc}: info {got['info'][:5].tolist()}")
        assert du.same_detect(got, want) == [], mc
        assert got["info"][0] == min(cap, max(0, mc))
    a, b = _device_detect(ctx, img, mask, 1000, None, det), _device_detect(ctx, img, mask, 1000, None, det)
    assert du.same_detect(a, b) == []                    # the same bytes twice, whatever order the atomics took
    raw = int(a["info"][1])
    for rc, over in ((raw - 1, 1), (raw, 0), (100, 1)):
        d = capi.detect_params_default(raw_cap=rc)
        got = _device_detect(ctx, img, mask, 1000, None, d)
        want = du.ref_detect(dref, img, mask, 1000, raw_cap=rc)
        print(f"raw_cap = {rc}: info {got['info'][:5].tolist()}")
        assert du.same_detect(got, want) == [] and got["info"][2] == over and got["info"][1] == raw
        assert (got["info"][0] == 0) == bool(over)
    # other arguments of the definition: the distance switched off, a small distance (a grid of one-pixel cells in
    # global memory), a large one, another quality level and k
    for kw in (dict(min_distance=0.0), dict(min_distance=1.5), dict(min_distance=3.0), dict(min_distance=75.5),
               dict(quality_level=0.05, harris_k=0.06), dict(quality_level=0.0)):
        got = _device_detect(ctx, img, mask, 4000, None, capi.detect_params_default(**kw))
        want = du.ref_detect(dref, img, mask, 4000, **kw)
        print(f"{kw}: info {got['info'][:5].tolist()}")
        assert du.same_detect(got, want) == [], kw


def test_arguments_are_checked():
    img = du.noise_image(64, 64)
    c = capi.Context(0)
    try:
        c.frame_upload(2, img, 1)
        d_c, d_i = torch.zeros((10, 2), device="cuda:0"), torch.zeros(8, dtype=torch.int32, device="cuda:0")
        for bad in (dict(quality_level=-1.0), dict(min_distance=-2.0), dict(min_distance=float("nan")), dict(raw_cap=-1),
                    dict(harris_k=float("inf"))):
            with pytest.raises(capi.PagkError):
                c.detect_corners_device(capi.detect_params_default(**bad), 2, None, 10, None, d_c, d_i)
        with pytest.raises(capi.PagkError):
            c.detect_corners_device(capi.detect_params_default(), 3, None, 10, None, d_c, d_i)   # nothing in that slot
        with pytest.raises(capi.PagkError):
            c.detect_corners_device(capi.detect_params_default(), 2, None, 0, None, d_c, d_i)    # cap < 1
        with pytest.raises(capi.PagkError):
            c.detect_corners(np.zeros((13, 40), np.uint8), None, 10)                              # smaller than 14
        assert c.detect_corners(img, None, 0)["corners"].shape == (0, 2)
    finally:
        c.close()


# ---- the fused hand-over -----------------------------------------------------------------------------------------------
def _handover_cases(img):
    """(what, status, points, state in): survivors with the top-up running; the top-up not running; the first frame."""
    rng = np.random.default_rng(17)
    h, w = img.shape
    pts = np.stack([rng.uniform(-3, w + 3, 448), rng.uniform(-3, h + 3, 448)], 1).astype(np.float32)
    some = np.zeros(448, np.uint8)
    some[rng.permutation(448)[:250]] = 1
    many = np.zeros(448, np.uint8)
    many[rng.permutation(448)[:350]] = 1
    flag = np.zeros(8, np.int32)
    flag[1] = 1
    return [("250 survivors, flag clear", some, pts, None), ("250 survivors, flag set: below the threshold", some, pts, flag),
            ("350 survivors, flag set: no top-up", many, pts, flag), ("350 survivors, flag clear", many, pts, None),
            ("first frame", np.zeros(448, np.uint8), pts, None)]


def test_handover_detect_equals_its_definition(ctx, href, dref, images):
    img = images["texture"][0]
    p = capi.make_params(camera=synth.D435I)
    for what, st, pts, state in _handover_cases(img):
        dist = (pts + np.float32([0.25, -0.5])).astype(np.float32)
        got = ctx.frame_handover_detect(p, img, 448, 400, 320.0, st, dist, pts, state=state)
        want = _restated_handover_detect(href, dref, p, img, 448, 400, 320.0, st, dist, pts, state)
        print(f"{what}: state {got['state'][:5].tolist()} info {got['info'][:5].tolist()}")
        assert hu.same_handover(got, want) == [], what
        assert got["info"].tobytes() == want["info"].tobytes(), what
        assert got["state"][4] == 0
        if "no top-up" in what:
            assert got["info"].tolist() == [0] * 8 and got["state"][:4].tolist() == [350, 1, 350, 0]
        else:
            assert got["state"][3] == got["info"][0] > 0 and got["state"][0] == 400
    # the array-in, array-out form is the same call
    what, st, pts, state = _handover_cases(img)[0]
    a = host_api.frame_handover_detect(p, img, 448, 400, 320.0, st, pts, pts, ctx=ctx)
    b = ctx.frame_handover_detect(p, img, 448, 400, 320.0, st, pts, pts)
    assert hu.same_handover(a, b) == [] and a["info"].tobytes() == b["info"].tobytes()
    assert host_api.detect_corners(img, None, 50, ctx=ctx)["corners"].tobytes() == du.ref_detect(dref, img, None, 50)["corners"].tobytes()
    assert host_api.corner_response(img, ctx=ctx).tobytes() == du.ref_response(dref, img).tobytes()


def test_handover_detect_device_direct_and_captured(href, dref, images):
    p = capi.make_params(camera=synth.D435I)
    det = capi.detect_params_default()
    frames = [images["texture"][0], images["noise"][0], du.texture_image(synth, W, H, 21)]
    cases = _handover_cases(frames[0])
    c = capi.Context(0)
    stream = torch.cuda.Stream()
    cap = 448
    try:
        with torch.cuda.stream(stream):
            c.set_stream(stream.cuda_stream)
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda:0")  # noqa: E731
            d_img = z((H, W), torch.uint8)
            d_st, d_pp, d_ppu = z(cap, torch.uint8), z((cap, 2), torch.float32), z((cap, 2), torch.float32)
            outs = [z((cap, 2), torch.float32) for _ in range(3)]
            d_idx, d_live, d_state, d_info = z(cap, torch.int32), z(cap, torch.uint8), z(8, torch.int32), z(8, torch.int32)

            def work():
                c.frame_set_device(1, d_img.data_ptr(), W, H, W, p.pyramids)
                c.frame_handover_detect_device(p, W, H, cap, 400, 320.0, d_st, d_pp, d_ppu, det, 1, outs[0], outs[1], outs[2],
                                               d_idx, d_live, None, d_state, d_info)

            def check(k, state_in, how):
                what, st, pts, _ = cases[k]
                want = _restated_handover_detect(href, dref, p, frames[k % 3], cap, 400, 320.0, st, pts, pts, state_in)
                print(f"{how} {k} ({what}): state {d_state.cpu().numpy()[:5].tolist()} info {d_info.cpu().numpy()[:5].tolist()}")
                assert np.array_equal(d_state.cpu().numpy(), want["state"]), (how, k)
                assert np.array_equal(d_info.cpu().numpy(), want["info"]), (how, k)
                for t, name in zip(outs, ("keys", "keys_un", "keys_normal")):
                    assert t.cpu().numpy().tobytes() == want[name].tobytes(), (how, k, name)
                assert np.array_equal(d_idx.cpu().numpy(), want["index_in_last"]) and np.array_equal(d_live.cpu().numpy(), want["live"])
                return want["state"]

            def feed(k):
                what, st, pts, _ = cases[k]
                d_img.copy_(_dev(frames[k % 3])), d_st.copy_(_dev(st)), d_pp.copy_(_dev(pts)), d_ppu.copy_(_dev(pts))

            with pytest.raises(capi.PagkError):   # the slot holds no frame yet
                c.frame_handover_detect_device(p, W, H, cap, 400, 320.0, d_st, d_pp, d_ppu, det, 1, outs[0], outs[1], outs[2],
                                               d_idx, d_live, None, d_state, d_info)
            feed(0)
            work()                                   # sizes the mask and the detector's workspace
            stream.synchronize()
            state = check(0, np.zeros(8, np.int32), "direct")
            c.graph_begin()
            try:
                with pytest.raises(capi.PagkError):  # the host-buffer forms are not capturable
                    c.detect_corners(frames[0], None, 10)
                work()
            finally:
                gid = c.graph_end()
            for k in (1, 2, 4):                      # the persisting flag: set by frame 0, so 2 does not top up
                feed(k)
                c.graph_launch(gid)
                stream.synchronize()
                state = check(k, state, "replay")
            c.graph_destroy(gid)
    finally:
        c.set_stream(None)
        c.close()


# ---- a sequence ----------------------------------------------------------------------------------------------------
NF, CAP, TARGET, RATIO = 9, 448, 400, 0.8
SEQ = (0x5EED0A10, (0.035, -0.045, 0.03))


def _host_loop(ctx, p, fitp, imgs, Rs, KRKs, handover):
    """The frames through entry points that existed before the hand-over (pagk_gyro_predict_device, pagk_track_device,
    the host pagk_post_filter, pagk_geometry_validation_fit) plus handover(k, status, pt_predict, pt_predict_un, state)."""
    none = np.zeros(0, np.uint8), np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32)
    frames = [handover(0, *none, np.zeros(8, np.int32))]
    ctx.frame_upload(0, imgs[0], p.pyramids)
    for k in range(1, len(imgs)):
        prev = frames[-1]
        n = int(prev["state"][0])
        ctx.frame_upload(k & 1, imgs[k], p.pyramids)
        keys_un = np.ascontiguousarray(prev["keys_un"][:n])
        d_keys = _dev(keys_un)
        d_pu, d_pd = torch.zeros((n, 2), device="cuda:0"), torch.zeros((n, 2), device="cuda:0")
        d_st, d_A = torch.zeros(n, dtype=torch.uint8, device="cuda:0"), torch.zeros((n, 4), device="cuda:0")
        out = distributed.alloc_device_outputs(n, torch.device("cuda", 0))
        torch.cuda.synchronize()
        ctx.gyro_predict_device(p, W, H, KRKs[k - 1], Rs[k - 1][2], n, d_keys, d_pu, d_pd, d_st, d_A)
        ctx.track_device(p, (k - 1) & 1, k & 1, n, d_keys, d_pu, d_A, d_st, out)
        ctx.sync()
        o = {name: out[name].cpu().numpy()[:n] for name, _, _ in distributed.FIELDS}
        kept, st, pp, ppu = capi.post_filter(p.half_patch, o["status"], o["pix_err"], o["dist_pred"], o["pt_dist"], o["pt_un"])
        cnt, st2, _ = ctx.geometry_validation_fit(keys_un, ppu, st, 1.0, fitp)
        frames.append(handover(k, st2, pp, ppu, prev["state"]))
    return frames


def _host_loop_with_detection(ctx, p, fitp, det, imgs, Rs, KRKs):
    """... plus the host form pagk_frame_handover_detect on the current image."""
    def handover(k, st, pp, ppu, state):
        return ctx.frame_handover_detect(p, imgs[k], CAP, TARGET, TARGET * RATIO, st, pp, ppu, det=det, state=state)
    return _host_loop(ctx, p, fitp, imgs, Rs, KRKs, handover)


def test_sequence_tracker_with_a_detector_against_a_host_loop(ctx, href, dref):
    cam, imgs, Rs, KRKs, rot9, _ = hu.rotating_sequence(synth, NF, W, H, *SEQ)
    first = du.ref_detect(dref, imgs[0], None, 1000)
    print(f"first frame: {first['n']} corners at distance 20 (restated)")
    assert first["n"] >= TARGET            # the sequence can start at target_n on its own
    p = capi.make_params(half_patch=5, iterations=10, pyramids=3, has_gyro=True, camera=cam)
    fitp = capi.fit_params_default(seed=0x5EED0F17, iters_H=512, iters_F=256)
    det = capi.detect_params_default()
    want = _host_loop_with_detection(ctx, p, fitp, det, imgs, Rs, KRKs)
    states = np.array([f["state"] for f in want])
    for k, f in enumerate(want):
        print(f"  host loop frame {k}: state {f['state'][:5].tolist()} info {f['info'][:5].tolist()}")
    # the first frame of the host loop is the restated composition
    none = np.zeros(0, np.uint8), np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32)
    r0 = _restated_handover_detect(href, dref, p, imgs[0], CAP, TARGET, TARGET * RATIO, *none, None)
    assert hu.same_handover(want[0], r0) == [] and want[0]["info"].tobytes() == r0["info"].tobytes()
    assert states[0, 0] == TARGET and states[0, 3] == TARGET
    assert any(states[k, 2] < states[k - 1, 0] for k in range(1, NF)), "no frame loses features"
    assert (states[1:, 3] > 0).any(), "no frame triggers the top-up"
    assert (states[:, 4] == 0).all()

    sq = runtime.SequenceTracker(p, W, H, CAP, TARGET, RATIO, fitp, detector=det)
    try:
        with pytest.raises(ValueError):
            sq.start(imgs[0], np.zeros((3, 2), np.float32))     # a tracker with a detector takes no list
        res = [sq.start(imgs[0])]
        start = res[0].to_numpy()
        assert start["state"][0] == TARGET
        used = ["direct"]
        for k in range(1, NF):                   # nothing is synchronised or read back inside this loop
            res.append(sq.step(imgs[k], rot9[k - 1], mode="graph"))
            used.append(sq.mode_used)
        got = [r.to_numpy() for r in res]
        sq.synchronize()
    finally:
        sq.close()
    assert used[1:3] == ["direct", "direct"] and all(u == "graph" for u in used[3:]), used
    for k in range(NF):
        g, wnt = got[k], want[k]
        print(f"graph frame {k}: state {g['state'][:5].tolist()} info {g['info'][:5].tolist()}")
        assert np.array_equal(g["state"], wnt["state"]), (k, g["state"], wnt["state"])
        assert np.array_equal(g["info"], wnt["info"]), (k, g["info"], wnt["info"])
        for name in ("keys", "keys_un", "keys_normal", "index_in_last", "live"):
            assert g[name].tobytes() == np.asarray(wnt[name]).tobytes(), (k, name)
        assert int(g["live"].sum()) == g["total"] == int(wnt["state"][0])


def test_sequence_tracker_without_a_detector_is_unchanged(ctx, href):
    """detector=None: the loop fed with the application's candidate lists, against the host loop made of the older entry
    points and the restated hand-over (the truth the loop was merged against)."""
    cam, imgs, Rs, KRKs, rot9, _ = hu.rotating_sequence(synth, NF, W, H, *SEQ)
    lists = hu.seq_candidates()
    cands = [lists[k % 4] for k in range(NF)]
    p = capi.make_params(half_patch=5, iterations=10, pyramids=3, has_gyro=True, camera=cam)
    fitp = capi.fit_params_default(seed=0x5EED0F17, iters_H=512, iters_F=256)
    rcam = hu.camera_of(p)

    def handover(k, st, pp, ppu, state):   # the restated hand-over on the application's list
        return hu.ref_handover(href, rcam, W, H, CAP, TARGET, TARGET * RATIO, st, pp, ppu, cands[k], state=state)
    want = _host_loop(ctx, p, fitp, imgs, Rs, KRKs, handover)
    sq = runtime.SequenceTracker(p, W, H, CAP, TARGET, RATIO, fitp, detector=None)
    try:
        with pytest.raises(TypeError):
            sq.start(imgs[0])                                   # without a detector the list is not optional
        res = [sq.start(imgs[0], cands[0])]
        for k in range(1, NF):
            res.append(sq.step(imgs[k], rot9[k - 1], cands[k], mode="graph"))
        got = [r.to_numpy() for r in res]
        sq.synchronize()
    finally:
        sq.close()
    for k in range(NF):
        assert "info" not in got[k]
        assert np.array_equal(got[k]["state"], want[k]["state"]), k
        for name in ("keys", "keys_un", "keys_normal", "index_in_last", "live"):
            assert got[k][name].tobytes() == np.asarray(want[k][name]).tobytes(), (k, name)


# ---- the example ---------------------------------------------------------------------------------------------------
def test_stream_graph_loop_detects_its_own_keypoints(built, tmp_path):
    """examples/stream_graph_loop.cpp --detect: the first frame's keypoints and every top-up come from the device
    detector; the line of the first frame is the restated composition's count."""
    import os
    import struct
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = capi.PKG_DIR
    exe = str(tmp_path / "stream_graph_loop")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I",
                    os.path.join(root, "include"), os.path.join(root, "examples", "stream_graph_loop.cpp"), "-o", exe,
                    "-L", pkg, "-l:libpagk_hip.so", "-L", "/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{pkg}",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    Wd, Hd, NFd, NK = 320, 240, 5, 100
    cam, imgs, Rs, KRKs, _, rng = hu.rotating_sequence(synth, NFd, Wd, Hd, 0x5EED0900, (0.02, -0.015, 0.04))
    u = rng.uniform(2 * NK)
    kp = np.stack([40 + u[0::2] * (Wd - 80), 40 + u[1::2] * (Hd - 80)], axis=1).astype(np.float32)
    path = str(tmp_path / "seq.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<4i", NFd, Wd, Hd, NK))
        f.write(cam.K.astype(np.float32).tobytes())
        f.write(np.asarray(cam.dist[:4], np.float32).tobytes())
        for im in imgs:
            f.write(im.tobytes())
        f.write(kp.tobytes())
        for R in Rs:
            f.write(R.tobytes())
        for M in KRKs:
            f.write(M.tobytes())
    r = subprocess.run([exe, "--detect", path, "5", "10", "3"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    lines = r.stdout.strip().splitlines()
    print("\n".join(lines))
    ref = du.build_ref(tmp_path)
    first = du.ref_detect(ref, imgs[0], None, NK)["n"]
    assert first > NK // 2 and lines[0] == f"first frame detected {first} of {NK}"
    assert len(lines) == NFd + 1 and lines[-1].startswith("survivors") and all(", added " in ln for ln in lines[1:-1])
    assert int(lines[-1].split()[1]) > NK // 2
