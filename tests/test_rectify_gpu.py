"""GPU tests of the rectification (include/pagk.h "rectification"): pagk_frame_rectify_device / _pinned and pagk_rectify
against the plain-C restatement (tests/rectify_ref.c), byte for byte: level 0 and the pyramid behind it, tracking on
rectified slots, capture and replay, runtime.SequenceTracker(rectify=...), the argument errors, the example."""
import ctypes as C

import numpy as np
import pytest
import torch

import handover_ref_util as hu
import rectify_ref_util as ru
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, distributed, runtime, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rref(tmp_path_factory):
    return ru.build_ref(tmp_path_factory.mktemp("rectify_ref"))


@pytest.fixture()
def own():
    """A context of the test's own: a rectified frame goes into a slot of the maps' size only."""
    c = capi.Context(0)
    yield c
    c.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _rows(raw):
    """The raw frame's rows with their step, as one dense Hs x step array (what goes to the device)."""
    ws, hs, cn, step = ru.raw_dims(raw)
    buf = np.full((hs, step), 0xA5, np.uint8)
    buf[:, :ws * cn] = np.asarray(raw).reshape(hs, ws * cn)
    return buf, ws, hs, cn, step


def _rectify_device(c, slot, mx, my, raw, pyramids):
    buf, ws, hs, cn, step = _rows(raw)
    c.rectify_set_maps(mx, my)
    d = _dev(buf)
    c.frame_rectify_device(slot, capi.rectify_params_default(channels=cn), d.data_ptr(), ws, hs, step, pyramids)
    c.sync()
    return d


def _lens_case(cam, w, h, ws, hs, pad):
    def make(cn):
        mx, my = ru.lens_maps(cam, w, h)
        return mx, my, ru.noise_raw(ws, hs, cn, 31 * w + h + cn, pad=pad)
    return make


def _grid_case(w, h, ws=64, hs=40):
    def make(cn):
        mx, my, _, _ = ru.grid_maps(w, h, ws, hs, 13 * w + h)
        return mx, my, ru.noise_raw(ws, hs, cn, 9 + cn, pad=3)
    return make


# name -> (channels, cn -> (map_x, map_y, raw)); the small cases are those of the CPU test
CASES = {name: (ru.CHANNELS, (lambda cn, name=name: ru.small_cases(cn)[name]))
         for name in ("grid 70x37", "identity", "last column", "last row", "four borders", "non-finite")}
CASES.update({
    "640x480 mild": (ru.CHANNELS, _lens_case(ru.MILD, 640, 480, 640, 480, 0)),
    "640x480 strong": (ru.CHANNELS, _lens_case(ru.STRONG, 640, 480, 640, 480, 7)),
    "752x480 mild": (ru.CHANNELS, _lens_case(ru.MILD, 752, 480, 752, 480, 0)),
    "752x480 strong": (ru.CHANNELS, _lens_case(ru.STRONG, 752, 480, 752, 480, 2)),
    "1x1": (ru.CHANNELS, _grid_case(1, 1)),
    "3x2": (ru.CHANNELS, _grid_case(3, 2)),
    "source 1x5": (ru.CHANNELS, _grid_case(33, 9, 1, 5)),      # one pixel per row: the kernel without paired tap loads
    "source 2x1": (ru.CHANNELS, _grid_case(33, 9, 2, 1)),      # the smallest source with them
    "641x479": (ru.CHANNELS, _lens_case(ru.STRONG, 641, 479, 640, 480, 1)),       # no dimension a multiple of four
    "1921x1081 gray": ((1,), _lens_case(ru.STRONG, 1921, 1081, 1920, 1080, 0)),  # several workgroups both ways, and tails
})


@pytest.mark.parametrize("name", list(CASES))
def test_level0_equals_the_restatement(rref, name):
    channels, make = CASES[name]
    for cn in channels:
        mx, my, raw = make(cn)
        h, w = mx.shape
        want = ru.ref_rectify(rref, mx, my, raw)
        c = capi.Context(0)
        try:
            _rectify_device(c, 0, mx, my, raw, 1)
            got = c.frame_download_level(0, 0, w, h)
        finally:
            c.close()
        bad = np.flatnonzero(got.ravel() != want.ravel())
        print(f"{name}, cn {cn}: {w} x {h} from {raw.shape[1]} x {raw.shape[0]}, {int((want == 0).sum())} black, "
              f"{bad.size} bytes differ" + (f", first at {divmod(int(bad[0]), w)}" if bad.size else ""))
        assert bad.size == 0, (name, cn)
        if "strong" in name:
            assert not want[0, :8].any() and want[h // 2, w // 2] != 0          # the black border, and a picture inside it


@pytest.mark.parametrize("name", ["640x480 strong", "641x479", "grid 70x37"])
def test_pyramid_equals_that_of_the_uploaded_restated_image(rref, own, name):
    """Levels 1 and 2: the even sizes go through the single-launch pyramid, the odd ones level by level."""
    _, make = CASES[name]
    mx, my, raw = make(3)
    h, w = mx.shape
    _rectify_device(own, 0, mx, my, raw, 3)
    own.frame_upload(1, ru.ref_rectify(rref, mx, my, raw), 3)
    for lvl in (0, 1, 2):
        assert np.array_equal(own.frame_download_level(0, lvl, w, h), own.frame_download_level(1, lvl, w, h)), (name, lvl)


def test_device_pinned_and_host_forms_agree(rref, own):
    mx, my = ru.lens_maps(ru.MILD, 752, 480)
    raw = ru.noise_raw(752, 480, 3, 77, pad=9)
    want = ru.ref_rectify(rref, mx, my, raw)
    buf, ws, hs, cn, step = _rows(raw)
    rp = capi.rectify_params_default(channels=3)
    _rectify_device(own, 0, mx, my, raw, 3)
    pinned = torch.from_numpy(buf).pin_memory()
    own.frame_rectify_pinned(1, rp, pinned.data_ptr(), ws, hs, step, 3)
    own.sync()
    host = own.rectify(rp, raw)
    assert np.array_equal(own.frame_download_level(0, 0, 752, 480), want)
    assert np.array_equal(host, want)
    for lvl in (0, 1, 2):
        assert np.array_equal(own.frame_download_level(1, lvl, 752, 480), own.frame_download_level(0, lvl, 752, 480)), lvl
    # other weights reach the kernel: B, G, R order
    bgr = capi.rectify_params_default(channels=3, gray_weight=(1868, 9617, 4899))
    assert np.array_equal(own.rectify(bgr, raw), ru.ref_rectify(rref, mx, my, raw, (1868, 9617, 4899), 14))


# ---- tracking on rectified slots ---------------------------------------------------------------------------------------
TW, TH, TN = 320, 240, 67


def _colour(img):
    """A three-channel raw frame with the picture in every channel (shifted, inverted): the gray step has work to do."""
    return np.ascontiguousarray(np.stack([img, np.roll(img, 1, axis=1), 255 - np.roll(img, 2, axis=0)], axis=2))


def _track_inputs(w):
    return _dev(w.pt_ref), _dev(w.pt_init), _dev(w.affine), _dev(w.status_in)


def _outputs(out, n):
    return {name: out[name].cpu().numpy()[:n].copy() for name, _, _ in distributed.FIELDS}


def test_track_device_on_rectified_slots(rref, own):
    w = synth.make_workload("rectified", TW, TH, TN, seed=0x5EED0C01, half_patch=5, iterations=10, pyramids=3)
    p = capi.make_params(half_patch=5, iterations=10, pyramids=3, has_gyro=w.has_gyro, camera=w.camera)
    mx, my = ru.lens_maps(ru.MILD, TW, TH)
    raws = [_colour(w.img_ref), _colour(w.img_cur)]
    restated = [ru.ref_rectify(rref, mx, my, r) for r in raws]
    d_in = _track_inputs(w)
    keep = [_rectify_device(own, k, mx, my, raws[k], 3) for k in (0, 1)]
    out_a = distributed.alloc_device_outputs(TN, torch.device("cuda", 0))
    own.track_device(p, 0, 1, TN, *d_in, out_a)
    own.sync()
    for k in (2, 3):
        own.frame_upload(k, restated[k - 2], 3)
    out_b = distributed.alloc_device_outputs(TN, torch.device("cuda", 0))
    own.track_device(p, 2, 3, TN, *d_in, out_b)
    own.sync()
    a, b = _outputs(out_a, TN), _outputs(out_b, TN)
    print(f"{int(a['status'].sum())} of {TN} tracked, mean iterations {a['iters'].mean():.2f}")
    assert a["status"].sum() > TN // 2
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), name
    del keep


def test_capture_and_replay(rref):
    """[rectify -> pyramid -> track] as one graph over a fixed raw-frame buffer: every replay equals the direct call."""
    w = synth.make_workload("rectified", TW, TH, TN, seed=0x5EED0C02, half_patch=5, iterations=10, pyramids=3)
    p = capi.make_params(half_patch=5, iterations=10, pyramids=3, has_gyro=w.has_gyro, camera=w.camera)
    mx, my = ru.lens_maps(ru.STRONG, TW, TH)
    rp = capi.rectify_params_default(channels=3)
    frames = [_colour(w.img_cur), _colour(np.roll(w.img_cur, 1, axis=1)), _colour(w.img_ref)]
    c = capi.Context(0)
    stream = torch.cuda.Stream()
    try:
        with torch.cuda.stream(stream):
            c.set_stream(stream.cuda_stream)
            c.rectify_set_maps(mx, my)
            d_in = _track_inputs(w)
            d_raw = torch.zeros((TH, TW * 3), dtype=torch.uint8, device="cuda:0")
            out = distributed.alloc_device_outputs(TN, torch.device("cuda", 0))
            d_raw.copy_(_dev(_colour(w.img_ref).reshape(TH, TW * 3)))
            c.frame_rectify_device(0, rp, d_raw.data_ptr(), TW, TH, TW * 3, 3)      # the reference frame, once

            def work():
                c.frame_rectify_device(1, rp, d_raw.data_ptr(), TW, TH, TW * 3, 3)
                c.track_device(p, 0, 1, TN, *d_in, out)

            def run(frame, how):
                d_raw.copy_(_dev(frame.reshape(TH, TW * 3)))
                how()
                stream.synchronize()
                return _outputs(out, TN), c.frame_download_level(1, 0, TW, TH)
            direct = [run(f, work) for f in frames]
            for (o, lvl0), f in zip(direct, frames):
                assert np.array_equal(lvl0, ru.ref_rectify(rref, mx, my, f))
            assert direct[0][0]["pt_un"].tobytes() != direct[1][0]["pt_un"].tobytes()
            c.graph_begin()
            try:
                with pytest.raises(capi.PagkError):      # allocates and synchronises: not inside a capture
                    c.rectify_set_maps(mx, my)
                with pytest.raises(capi.PagkError):      # the host-buffer form neither
                    c.rectify(rp, frames[0])
                work()
            finally:
                gid = c.graph_end()
            for k in (1, 2, 0):
                o, lvl0 = run(frames[k], lambda: c.graph_launch(gid))
                assert np.array_equal(lvl0, direct[k][1]), k
                for name in o:
                    assert o[name].tobytes() == direct[k][0][name].tobytes(), (k, name)
            c.graph_destroy(gid)
            # the pinned form: the host-to-device copy of the raw frame is a node of the graph
            pinned = torch.zeros((TH, TW * 3), dtype=torch.uint8).pin_memory()
            pinned.numpy()[...] = frames[0].reshape(TH, TW * 3)
            c.frame_rectify_pinned(2, rp, pinned.data_ptr(), TW, TH, TW * 3, 3)      # sizes the staging buffer
            stream.synchronize()
            c.graph_begin()
            try:
                c.frame_rectify_pinned(2, rp, pinned.data_ptr(), TW, TH, TW * 3, 3)
            finally:
                gid = c.graph_end()
            for k in (1, 2):
                pinned.numpy()[...] = frames[k].reshape(TH, TW * 3)
                c.graph_launch(gid)
                stream.synchronize()
                assert np.array_equal(c.frame_download_level(2, 0, TW, TH), direct[k][1]), k
                d_raw.copy_(_dev(frames[k].reshape(TH, TW * 3)))
                work()
                stream.synchronize()
                for lvl in (1, 2):
                    assert np.array_equal(c.frame_download_level(2, lvl, TW, TH), c.frame_download_level(1, lvl, TW, TH)), (k, lvl)
            c.graph_destroy(gid)
    finally:
        c.set_stream(None)
        c.close()


# ---- the loop ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_detector", [False, True])
def test_sequence_tracker_on_raw_frames(rref, with_detector):
    """SequenceTracker(rectify=...) fed raw three-channel frames against the same tracker fed the restated rectified
    frames: graph mode, six frames."""
    nf, cap, target, ratio = 6, 160, 128, 0.8
    cam, imgs, _, _, rot9, rng = hu.rotating_sequence(synth, nf, TW, TH, 0x5EED0C03, (0.02, -0.015, 0.03))
    mx, my = ru.lens_maps(ru.MILD, TW, TH)
    raws = [_colour(im) for im in imgs]
    restated = [ru.ref_rectify(rref, mx, my, r) for r in raws]
    p = capi.make_params(half_patch=5, iterations=10, pyramids=3, has_gyro=True, camera=cam)
    fitp = capi.fit_params_default(seed=0x5EED0F17, iters_H=256, iters_F=128)
    det = capi.detect_params_default(min_distance=10.0) if with_detector else None
    u = rng.uniform(2 * 200)
    cand = np.stack([20 + u[0::2] * (TW - 40), 20 + u[1::2] * (TH - 40)], axis=1).astype(np.float32)
    lists = [None] * nf if with_detector else [cand] + [cand[::-1].copy()] * (nf - 1)

    def run(frames, rectify):
        sq = runtime.SequenceTracker(p, TW, TH, cap, target, ratio, fitp, detector=det, cand_cap=256, rectify=rectify)
        try:
            res = [sq.start(frames[0], lists[0])]
            used = []
            for k in range(1, nf):
                res.append(sq.step(frames[k], rot9[k - 1], lists[k], mode="graph"))
                used.append(sq.mode_used)
            got = [r.to_numpy() for r in res]
            sq.synchronize()
        finally:
            sq.close()
        assert used == ["direct", "direct", "graph", "graph", "graph"], used
        return got
    want = run(restated, None)
    got = run(raws, (mx, my, capi.rectify_params_default(channels=3), (TH, TW)))
    states = np.array([f["state"] for f in want])
    print(states[:, :5].tolist())
    assert states[0, 0] > target // 2 and (states[1:, 2] > 0).all(), "the sequence tracks nothing"
    for k in range(nf):
        assert np.array_equal(got[k]["state"], want[k]["state"]), (k, got[k]["state"], want[k]["state"])
        for name in ("keys", "keys_un", "keys_normal", "index_in_last", "live"):
            assert got[k][name].tobytes() == want[k][name].tobytes(), (k, name)
        if with_detector:
            assert np.array_equal(got[k]["info"], want[k]["info"]), k
    with pytest.raises(ValueError):
        runtime.SequenceTracker(p, TW, TH, cap, target, ratio, rectify=(mx[:-1], my[:-1], capi.rectify_params_default(), (TH, TW)))


# ---- argument errors ---------------------------------------------------------------------------------------------------
def test_argument_errors(own):
    E = capi.PAGK_E_ARG
    rp = capi.rectify_params_default()
    d = torch.zeros((40, 64 * 4), dtype=torch.uint8, device="cuda:0")

    def refused(call, *words):
        with pytest.raises(capi.PagkError) as e:
            call()
        assert e.value.code == E
        text = own.lib.pagk_last_error(own.h).decode()
        print(text)
        assert all(wd in text for wd in words), (text, words)
    refused(lambda: own.frame_rectify_device(0, rp, d.data_ptr(), 64, 40, 64, 1), "no maps")
    host, dst = np.zeros((40, 64), np.uint8), np.zeros((40, 64), np.uint8)
    refused(lambda: own._check(own.lib.pagk_rectify(own.h, C.byref(rp), host.ctypes.data, 64, 40, 64, dst.ctypes.data, 64),
                               "pagk_rectify"), "no maps")
    mx, my = ru.identity_maps(64, 40)
    own.rectify_set_maps(mx, my)
    own.frame_rectify_device(0, rp, d.data_ptr(), 64, 40, 64, 1)
    for cn in (0, 2, 5):
        refused(lambda: own.frame_rectify_device(0, capi.rectify_params_default(channels=cn), d.data_ptr(), 64, 40, 256, 1), "channels")
    refused(lambda: own.frame_rectify_device(0, capi.rectify_params_default(channels=3, gray_weight=(1, 2, 3)), d.data_ptr(),
                                             64, 40, 256, 1), "weights")
    refused(lambda: own.frame_rectify_device(0, capi.rectify_params_default(channels=3), d.data_ptr(), 64, 40, 191, 1), "src_step")
    refused(lambda: own.frame_rectify_device(0, rp, d.data_ptr(), 64, 40, 63, 1), "src_step")
    # a source beyond 16-bit tap coordinates (nothing is read before the check)
    refused(lambda: own.frame_rectify_device(0, rp, d.data_ptr(), 32768, 40, 32768, 1), "32767")
    refused(lambda: own.frame_rectify_device(0, rp, d.data_ptr(), 64, 32768, 64, 1), "32767")
    # the slot holds a frame of another size than the maps
    own.frame_upload(1, np.zeros((48, 64), np.uint8), 1)
    refused(lambda: own.frame_rectify_device(1, rp, d.data_ptr(), 64, 40, 64, 1), "slot 1", "64 x 48")
    pinned = torch.zeros((40, 64), dtype=torch.uint8).pin_memory()
    refused(lambda: own.frame_rectify_pinned(1, rp, pinned.data_ptr(), 64, 40, 64, 1), "slot 1")
    own.sync()
    assert np.array_equal(own.frame_download_level(0, 0, 64, 40), np.zeros((40, 64), np.uint8))   # slot 0 is untouched by all that


# ---- the example -------------------------------------------------------------------------------------------------------
def test_stream_graph_loop_rectifies_its_frames(built, tmp_path):
    """examples/stream_graph_loop.cpp --rectify runs, prints the lines of the plain loop, and still tracks."""
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
    nfd, nk = 5, 100
    cam, imgs, Rs, KRKs, _, rng = hu.rotating_sequence(synth, nfd, TW, TH, 0x5EED0900, (0.02, -0.015, 0.04))
    u = rng.uniform(2 * nk)
    kp = np.stack([40 + u[0::2] * (TW - 80), 40 + u[1::2] * (TH - 80)], axis=1).astype(np.float32)
    path = str(tmp_path / "seq.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<4i", nfd, TW, TH, nk))
        f.write(cam.K.astype(np.float32).tobytes())
        f.write(np.asarray(cam.dist[:4], np.float32).tobytes())
        for im in imgs:
            f.write(im.tobytes())
        f.write(kp.tobytes())
        for R in Rs:
            f.write(R.tobytes())
        for M in KRKs:
            f.write(M.tobytes())
    outs = {}
    for flags in ((), ("--rectify",)):
        r = subprocess.run([exe, *flags, path, "5", "10", "3"], capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, (flags, r.returncode, r.stdout, r.stderr)
        outs[flags] = r.stdout.strip().splitlines()
        print("\n".join(outs[flags]))
    plain, rect = outs[()], outs[("--rectify",)]
    assert len(rect) == len(plain) == nfd
    for a, b in zip(rect[:-1], plain[:-1]):                    # "pair k tracked a of b"
        assert a.split()[:3] == b.split()[:3] and a.split()[4] == "of" and len(a.split()) == len(b.split()) == 6
    assert rect[-1].split()[0] == "survivors" and rect[-1].split()[2] == "checksum"
    assert int(rect[-1].split()[1]) > nk // 2
