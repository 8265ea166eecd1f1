"""GPU tests of the FAST-cells-and-quadtree detector: pagk_selftest_fast_cells, pagk_detect_fast[_device] and
pagk_frame_handover_fast[_device] against the plain-C restatements (tests/fast_detect_ref.c, frame_handover_ref.c), byte
for byte; capture and replay; runtime.SequenceTracker(detector=FastParams) against a host loop; the example."""
import numpy as np
import pytest
import torch

import fast_ref_util as fu
import handover_ref_util as hu
from sequence_model import restated_handover_fast as _restated_handover_fast
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, distributed, host_api, runtime, synth

pytestmark = pytest.mark.gpu
W, H = 640, 480


@pytest.fixture(scope="module")
def fref(tmp_path_factory):
    return fu.build_ref(tmp_path_factory.mktemp("fast_ref"))


@pytest.fixture(scope="module")
def href(tmp_path_factory):
    return hu.build_ref(tmp_path_factory.mktemp("handover_ref"))


@pytest.fixture(scope="module")
def cases():
    return fu.cases(synth)


@pytest.fixture(scope="module")
def restated(fref, cases):
    """name -> the restatement's result, computed once and left unchanged."""
    memo = {}

    def get(name):
        if name not in memo:
            img, mask, n, _ = cases[name]
            memo[name] = fu.ref_detect(fref, img, mask, n)
        return memo[name]
    return get


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.mark.parametrize("name", fu.CASE_NAMES)
def test_raw_list(ctx, fref, cases, name):
    img = cases[name][0]
    got, want = ctx.selftest_fast_cells(img), fu.ref_cells(fref, img)
    print(f"{name}: {got['n']} raw keypoints (restated {want['n']})")
    assert got["n"] == want["n"]
    assert got["xy"].tobytes() == want["xy"].tobytes() and got["score"].tobytes() == want["score"].tobytes()


@pytest.mark.parametrize("name", fu.CASE_NAMES)
def test_detect_fast_host_form(ctx, cases, restated, name):
    img, mask, n, exp = cases[name]
    got, want = ctx.detect_fast(img, mask, n), restated(name)
    print(f"{name}: info {got['info'][:6].tolist()} (restated {want['info'][:6].tolist()})")
    assert got["info"].tobytes() == want["info"].tobytes()
    assert got["buffer"].tobytes() == want["keypoints"].tobytes()
    assert got["response_buffer"].tobytes() == want["response"].tobytes()
    fu.check_expected(name, exp, got["info"], None)


def _device_detect(ctx, img, mask, n, slot=2, pitch=None, with_response=True):
    h, w = img.shape
    cap = capi.detect_fast_bounds(w, h, n)[1]
    if pitch is None:
        ctx.frame_upload(slot, img, 1)
        keep = None
    else:   # a pitched slot: the image in the left columns of a wider device buffer, read in place
        keep = torch.full((h, pitch), 255, dtype=torch.uint8, device="cuda:0")
        keep[:, :w] = _dev(img)
        torch.cuda.synchronize()
        ctx.frame_set_device(slot, keep.data_ptr(), w, h, pitch, 1)
    d_mask = None if mask is None else _dev(mask)
    d_k = torch.full((cap, 2), -7.0, dtype=torch.float32, device="cuda:0")
    d_r = torch.full((cap,), -7.0, dtype=torch.float32, device="cuda:0") if with_response else None
    d_i = torch.full((capi.DETECT_INFO_WORDS,), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.detect_fast_device(capi.fast_params_default(n_features=n), slot, d_mask, cap, d_k, d_r, d_i)
    ctx.sync()
    out = dict(keypoints=d_k.cpu().numpy(), info=d_i.cpu().numpy())
    out["response"] = d_r.cpu().numpy() if with_response else None
    del keep
    return out


@pytest.mark.parametrize("name", fu.CASE_NAMES)
def test_detect_fast_device_form(ctx, cases, restated, name):
    img, mask, n, _ = cases[name]
    got, want = _device_detect(ctx, img, mask, n), restated(name)     # every output pre-filled with a sentinel
    print(f"{name}: info {got['info'][:6].tolist()} (restated {want['info'][:6].tolist()})")
    assert fu.same_fast(got, want) == []


@pytest.mark.parametrize("name", ["97x80 noise", "texture with holes", "641x479 texture"])
def test_detect_fast_on_a_pitched_slot(ctx, cases, restated, name):
    img, mask, n, _ = cases[name]
    got, want = _device_detect(ctx, img, mask, n, pitch=img.shape[1] + 37), restated(name)
    assert fu.same_fast(got, want) == []


def test_determinism_and_no_response(ctx, fref, cases, restated):
    img, mask, n, _ = cases["640x480 noise"]
    a, b = _device_detect(ctx, img, mask, n), _device_detect(ctx, img, mask, n)
    assert fu.same_fast(a, b) == []                      # the same bytes twice, whatever order the atomics took
    c = _device_detect(ctx, img, mask, n, with_response=False)
    assert c["keypoints"].tobytes() == a["keypoints"].tobytes() and c["info"].tobytes() == a["info"].tobytes()
    # other thresholds are other results, and the restatement follows
    img = cases["mixed N=400"][0]
    for ini, mn in ((40, 7), (20, 20), (5, 30), (0, 0), (255, 255)):
        got = ctx.detect_fast(img, None, 300, capi.fast_params_default(ini_threshold=ini, min_threshold=mn))
        want = fu.ref_detect(fref, img, None, 300, ini=ini, mn=mn)
        print(f"thresholds {ini}, {mn}: info {got['info'][:6].tolist()}")
        assert got["info"].tobytes() == want["info"].tobytes() and got["buffer"].tobytes() == want["keypoints"].tobytes(), (ini, mn)


def test_the_large_image_host_form(ctx, fref):
    name, n, exp = fu.BIG
    img = fu.big_image(synth)
    got, want = ctx.detect_fast(img, None, n), fu.ref_detect(fref, img, None, n)
    print(f"{name}: info {got['info'][:6].tolist()}")
    assert got["info"].tobytes() == want["info"].tobytes() and got["buffer"].tobytes() == want["keypoints"].tobytes()
    assert got["response_buffer"].tobytes() == want["response"].tobytes()
    fu.check_expected(name, exp, got["info"], None)


def test_arguments_are_checked():
    img = fu.du.noise_image(97, 80, 3)
    c = capi.Context(0)
    try:
        c.frame_upload(2, img, 1)
        ob = capi.detect_fast_bounds(97, 80, 50)[1]
        d_k, d_i = torch.zeros((ob, 2), device="cuda:0"), torch.zeros(8, dtype=torch.int32, device="cuda:0")
        ok = capi.fast_params_default(n_features=50)
        c.detect_fast_device(ok, 2, None, ob, d_k, None, d_i)
        c.sync()
        for bad in (dict(ini_threshold=256), dict(min_threshold=-1), dict(n_features=0), dict(n_levels=8)):
            with pytest.raises(capi.PagkError) as e:
                c.detect_fast_device(capi.fast_params_default(**{**dict(n_features=50), **bad}), 2, None, ob, d_k, None, d_i)
            assert e.value.code == (capi.PAGK_E_UNSUPPORTED if "n_levels" in bad else capi.PAGK_E_ARG), bad
        with pytest.raises(capi.PagkError):
            c.detect_fast_device(ok, 3, None, ob, d_k, None, d_i)          # an empty slot
        with pytest.raises(capi.PagkError):
            c.detect_fast_device(ok, 2, None, ob - 1, d_k, None, d_i)      # cap < out_bound
        with pytest.raises(capi.PagkError):
            c.detect_fast(np.zeros((61, 200), np.uint8), None, 50, cap=100)
        with pytest.raises(capi.PagkError):
            c.detect_fast(np.zeros((200, 62), np.uint8), None, 50, cap=100)     # nIni = 0
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            c.set_stream(stream.cuda_stream)
            c.graph_begin()
            try:
                with pytest.raises(capi.PagkError):   # the host-buffer forms are not capturable
                    c.detect_fast(img, None, 50)
                with pytest.raises(capi.PagkError):
                    c.selftest_fast_cells(img)
                c.detect_fast_device(ok, 2, None, ob, d_k, None, d_i)   # the device form is
            finally:
                gid = c.graph_end()
            c.graph_launch(gid)
            stream.synchronize()
            c.graph_destroy(gid)
        c.set_stream(None)
    finally:
        c.close()


# ---- the fused hand-over -----------------------------------------------------------------------------------------------
def _handover_cases(img):
    """(what, status, points, state in): the cases of test_detect_gpu.py's _handover_cases."""
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


def test_handover_fast_equals_its_definition(ctx, href, fref, cases):
    img = cases["texture N=400"][0]
    p = capi.make_params(camera=synth.D435I)
    for what, st, pts, state in _handover_cases(img):
        dist = (pts + np.float32([0.25, -0.5])).astype(np.float32)
        got = ctx.frame_handover_fast(p, img, 448, 400, 320.0, st, dist, pts, state=state)
        want = _restated_handover_fast(href, fref, p, img, 448, 400, 320.0, st, dist, pts, state)
        print(f"{what}: state {got['state'][:5].tolist()} info {got['info'][:6].tolist()}")
        assert hu.same_handover(got, want) == [], what
        assert got["info"].tobytes() == want["info"].tobytes(), what
        if "no top-up" in what:
            assert got["info"].tolist() == [0] * 8 and got["state"][:5].tolist() == [350, 1, 350, 0, 0]
        else:
            assert got["state"][3] > 0 and got["info"][0] == got["info"][4] == 402
            assert got["state"][3] + got["state"][4] <= got["info"][0]
            if st.any():   # the survivors' holes reject candidates
                masked = got["mask"][got_keypoints(fref, img)[:, 1], got_keypoints(fref, img)[:, 0]] == 0
                assert got["state"][4] == int(masked.sum()) > 0
            else:
                assert got["state"][4] == 0 and got["state"][0] == 400
    # another N than the target, and the array-in, array-out forms
    what, st, pts, state = _handover_cases(img)[0]
    f = capi.fast_params_default(n_features=1000)
    a = ctx.frame_handover_fast(p, img, 448, 400, 320.0, st, pts, pts, fast=f)
    want = _restated_handover_fast(href, fref, p, img, 448, 400, 320.0, st, pts, pts, None, n_features=1000)
    assert hu.same_handover(a, want) == [] and a["info"].tobytes() == want["info"].tobytes() and a["info"][4] == 1001
    b = host_api.frame_handover_fast(p, img, 448, 400, 320.0, st, pts, pts, fast=f, ctx=ctx)
    assert hu.same_handover(a, b) == [] and a["info"].tobytes() == b["info"].tobytes()
    d = host_api.detect_fast(img, None, 400, ctx=ctx)
    assert d["keypoints"].tobytes() == fu.ref_detect(fref, img, None, 400)["keypoints"][:d["n_keypoints"]].tobytes()


def got_keypoints(fref, img, n=400):
    """The restated detector's integer keypoints on img without a mask."""
    d = fu.ref_detect(fref, img, None, n)
    return d["keypoints"][:d["n"]].astype(np.int64)


def test_handover_fast_device_direct_and_captured(href, fref, cases):
    p = capi.make_params(camera=synth.D435I)
    fast = capi.fast_params_default()
    frames = [cases["texture N=400"][0], cases["640x480 noise"][0], fu.du.texture_image(synth, W, H, 21)]
    hcases = _handover_cases(frames[0])
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
                c.frame_handover_fast_device(p, W, H, cap, 400, 320.0, d_st, d_pp, d_ppu, fast, 1, outs[0], outs[1], outs[2],
                                             d_idx, d_live, None, d_state, d_info)

            def check(k, state_in, how):
                what, st, pts, _ = hcases[k]
                want = _restated_handover_fast(href, fref, p, frames[k % 3], cap, 400, 320.0, st, pts, pts, state_in)
                print(f"{how} {k} ({what}): state {d_state.cpu().numpy()[:5].tolist()} info {d_info.cpu().numpy()[:6].tolist()}")
                assert np.array_equal(d_state.cpu().numpy(), want["state"]), (how, k)
                assert np.array_equal(d_info.cpu().numpy(), want["info"]), (how, k)
                for t, name in zip(outs, ("keys", "keys_un", "keys_normal")):
                    assert t.cpu().numpy().tobytes() == want[name].tobytes(), (how, k, name)
                assert np.array_equal(d_idx.cpu().numpy(), want["index_in_last"]) and np.array_equal(d_live.cpu().numpy(), want["live"])
                return want["state"]

            def feed(k):
                what, st, pts, _ = hcases[k]
                d_img.copy_(_dev(frames[k % 3])), d_st.copy_(_dev(st)), d_pp.copy_(_dev(pts)), d_ppu.copy_(_dev(pts))

            with pytest.raises(capi.PagkError):   # the slot holds no frame yet
                c.frame_handover_fast_device(p, W, H, cap, 400, 320.0, d_st, d_pp, d_ppu, fast, 1, outs[0], outs[1], outs[2],
                                             d_idx, d_live, None, d_state, d_info)
            feed(0)
            work()                                   # sizes the mask and the detector's workspace
            stream.synchronize()
            state = check(0, np.zeros(8, np.int32), "direct")
            c.graph_begin()
            try:
                with pytest.raises(capi.PagkError):  # the host-buffer forms are not capturable
                    c.frame_handover_fast(p, frames[0], cap, 400, 320.0, hcases[0][1], hcases[0][2], hcases[0][2])
                work()
            finally:
                gid = c.graph_end()
            for k in (1, 2, 4):                      # the persisting flag: set by frame 0, so 2 does not top up
                feed(k)
                c.graph_launch(gid)
                stream.synchronize()
                state = check(k, state, "replay")
                if k == 2:
                    assert d_info.cpu().numpy().tolist() == [0] * 8
            c.graph_destroy(gid)
    finally:
        c.set_stream(None)
        c.close()


# ---- a sequence ----------------------------------------------------------------------------------------------------
NF, CAP, TARGET, RATIO = 9, 448, 400, 0.8               # those of test_detect_gpu.py
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


def test_sequence_tracker_with_the_fast_detector_against_a_host_loop(ctx, href, fref):
    cam, imgs, Rs, KRKs, rot9, _ = hu.rotating_sequence(synth, NF, W, H, *SEQ)
    for k, (raw, nodes) in ((0, (1486, 400)), (4, (2521, 401)), (8, (4588, 400))):     # checked on the CPU model
        d = fu.ref_detect(fref, imgs[k], None, TARGET)
        assert (int(d["info"][1]), int(d["info"][4])) == (raw, nodes), (k, d["info"].tolist())
    p = capi.make_params(half_patch=5, iterations=10, pyramids=3, has_gyro=True, camera=cam)
    fitp = capi.fit_params_default(seed=0x5EED0F17, iters_H=512, iters_F=256)
    fast = capi.fast_params_default()

    def handover(k, st, pp, ppu, state):
        return ctx.frame_handover_fast(p, imgs[k], CAP, TARGET, TARGET * RATIO, st, pp, ppu, fast=fast, state=state)
    want = _host_loop(ctx, p, fitp, imgs, Rs, KRKs, handover)
    states = np.array([f["state"] for f in want])
    for k, f in enumerate(want):
        print(f"  host loop frame {k}: state {f['state'][:5].tolist()} info {f['info'][:6].tolist()}")
    none = np.zeros(0, np.uint8), np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32)
    r0 = _restated_handover_fast(href, fref, p, imgs[0], CAP, TARGET, TARGET * RATIO, *none, None)
    assert hu.same_handover(want[0], r0) == [] and want[0]["info"].tobytes() == r0["info"].tobytes()
    assert states[0, 0] == TARGET and states[0, 3] == TARGET      # the first frame reaches target_n on its own
    assert any(states[k, 2] < states[k - 1, 0] for k in range(1, NF)), "no frame loses features"
    assert (states[1:, 3] > 0).any(), "no frame triggers the top-up"

    sq = runtime.SequenceTracker(p, W, H, CAP, TARGET, RATIO, fitp, detector=fast)
    try:
        with pytest.raises(ValueError):
            sq.start(imgs[0], np.zeros((3, 2), np.float32))     # a tracker with a detector takes no list
        res = [sq.start(imgs[0])]
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
        print(f"graph frame {k}: state {g['state'][:5].tolist()} info {g['info'][:6].tolist()}")
        assert np.array_equal(g["state"], wnt["state"]), (k, g["state"], wnt["state"])
        assert np.array_equal(g["info"], wnt["info"]), (k, g["info"], wnt["info"])
        for name in ("keys", "keys_un", "keys_normal", "index_in_last", "live"):
            assert g[name].tobytes() == np.asarray(wnt[name]).tobytes(), (k, name)
        assert int(g["live"].sum()) == g["total"] == int(wnt["state"][0])


# ---- the example ---------------------------------------------------------------------------------------------------
def test_stream_graph_loop_detect_fast(built, href, fref, tmp_path):
    """examples/stream_graph_loop.cpp --detect-fast on the sequence of the existing example test: the line of the first
    frame is the restated composition's count."""
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
    r = subprocess.run([exe, "--detect-fast", path, "5", "10", "3"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    lines = r.stdout.strip().splitlines()
    print("\n".join(lines))
    p = capi.make_params(half_patch=5, iterations=10, pyramids=3, has_gyro=True, camera=cam)
    none = np.zeros(0, np.uint8), np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32)
    first = int(_restated_handover_fast(href, fref, p, imgs[0], NK, NK, 0.8 * NK, *none, None)["state"][0])
    assert first > NK // 2 and lines[0] == f"first frame detected {first} of {NK}"
    assert len(lines) == NFd + 1 and lines[-1].startswith("survivors") and all(", added " in ln for ln in lines[1:-1])
    assert int(lines[-1].split()[1]) > NK // 2
