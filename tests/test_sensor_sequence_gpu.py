"""GPU tests of the sensor form of the sequence (pagk_sequence_*_sensor, runtime.DeviceSequence(sensor=...)) on the rotating
320 x 240 sequence of tests/test_rectify_gpu.py: a sensor sequence fed raw frames and IMU windows against a PLAIN sequence fed
the restated rectified frames (tests/rectify_ref.c) and the restated rot9 (tests/gyro_integrate_ref.c), byte for byte, for all
three arms, the candidate list and a detecting detector; one channel, padded rows, a raw frame larger than the rectified one;
graph against direct; the flow velocities against their numpy model; independence of what the workspaces held; the
refusals."""
import numpy as np
import pytest
import torch

import gyro_integrate_ref_util as gu
import handover_ref_util as hu
import rectify_ref_util as ru
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, runtime, synth

pytestmark = pytest.mark.gpu
TW, TH = 320, 240
NF, CAP, TARGET, RATIO = 6, 160, 128, 0.8
STEP = (0.02, -0.015, 0.03)
T0, DT = 100.0, 1.0 / 30.0
SET = ("keys", "keys_un", "keys_normal", "index_in_last", "live", "state", "info")
PAIR = ("status", "pt_predict", "pt_predict_un", "err")
ARMS = {"patchmatch": (capi.SEQ_PATCHMATCH, 0), "lk": (capi.SEQ_LK, 0), "lk-gyro": (capi.SEQ_LK, 1)}


def _colour(img):
    """A three-channel raw frame with the picture in every channel (shifted, inverted): the gray step has work to do."""
    return np.ascontiguousarray(np.stack([img, np.roll(img, 1, axis=1), 255 - np.roll(img, 2, axis=0)], axis=2))


def _padded(raw, pad=7):
    """The same frame with rows `pad` bytes further apart (step > src_width * channels)."""
    hs, row = raw.shape[0], raw.shape[1] * (1 if raw.ndim == 2 else raw.shape[2])
    buf = np.full((hs, row + pad), 0xA5, np.uint8)
    buf[:, :row] = raw.reshape(hs, row)
    v = buf[:, :row]
    return v if raw.ndim == 2 else v.reshape(raw.shape)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """Frames, maps, restated rectified frames, windows and their restated rot9: computed once and left unchanged.
    The windows hold a constant rate chosen so that the restated Rcl reproduces the scene's step rotation; measured on the
    CPU: max |Rcl - R_scene| = 6.0e-08, max |rot9 - rot9_scene| = 2.9e-05 (the pixel column of K Rcl K^-1)."""
    rref = ru.build_ref(tmp_path_factory.mktemp("rectify_ref"))
    gref = gu.build_ref(tmp_path_factory.mktemp("gyro_integrate_ref"))
    cam, imgs, Rs, _, rot9_scene, rng = hu.rotating_sequence(synth, NF, TW, TH, 0x5EED0C03, STEP)
    p = capi.make_params(half_patch=5, iterations=10, pyramids=3, has_gyro=True, camera=cam)
    times = [T0 + k * DT for k in range(NF)]
    windows = [None] + [dict(gu.constant_rate_window(STEP, times[k - 1], times[k]), camera=(p.fx, p.fy, p.cx, p.cy)) for k in range(1, NF)]
    restated9 = [None] + [gu.ref_integrate(gref, w) for w in windows[1:]]
    agree = max(float(np.abs(r[0] - R).max()) for r, R in zip(restated9[1:], Rs))
    agree9 = max(float(np.abs(r[1] - q).max()) for r, q in zip(restated9[1:], rot9_scene))
    print(f"windows against the scene: max |Rcl - R| = {agree:.3e}, max |rot9 - rot9_scene| = {agree9:.3e}")
    assert agree <= 4 * 6.0e-08 and agree9 <= 4 * 2.9e-05
    u = rng.uniform(2 * 200)
    cand = np.stack([20 + u[0::2] * (TW - 40), 20 + u[1::2] * (TH - 40)], axis=1).astype(np.float32)
    mx, my = ru.lens_maps(ru.MILD, TW, TH)
    gx, gy, _, _ = ru.grid_maps(TW, TH, 352, 250, 13 * TW + TH)
    kinds = {"rgb": (mx, my, [_colour(im) for im in imgs]),
             "gray": (mx, my, [np.ascontiguousarray(im) for im in imgs]),
             "rgb padded": (mx, my, [_padded(_colour(im)) for im in imgs]),
             "larger raw": (gx, gy, [ru.noise_raw(352, 250, 3, 77 + k) for k in range(NF)])}
    rect = {name: [ru.ref_rectify(rref, m_x, m_y, r) for r in raws] for name, (m_x, m_y, raws) in kinds.items()}
    return dict(cam=cam, p=p, times=times, windows=windows, rot9=[None] + [r[1] for r in restated9[1:]], kinds=kinds, rect=rect,
                cands=[cand] + [cand[::-1].copy()] * (NF - 1), lk=capi.lk_params_default(half_patch=5),
                fit=capi.fit_params_default(seed=0x5EED0F17, iters_H=256, iters_F=128), memo={})


def _sp(scene, arm, detector=0):
    tracker, flow = ARMS[arm]
    sp = capi.sequence_params_default(track=scene["p"], lk=scene["lk"], fit=scene["fit"], tracker=tracker, lk_initial_flow=flow,
                                      width=TW, height=TH, cap=CAP, target_n=TARGET, new_point_threshold=TARGET * RATIO,
                                      detector=detector, cand_cap=256, validate=1, sigma=1.0)
    if detector == 1:
        sp.harris = capi.detect_params_default(min_distance=10.0)
    return sp


def _sensor(scene, kind, **kw):
    if kind is None:                                             # frames arrive gray and rectified: the IMU half alone
        return capi.sequence_sensor_default(**kw)
    raw = scene["kinds"][kind][2][0]
    cn = 1 if raw.ndim == 2 else raw.shape[2]
    return capi.sequence_sensor_default(rectify=capi.rectify_params_default(channels=cn), raw=1, src_width=raw.shape[1],
                                        src_height=raw.shape[0], **kw)


def _window(w):
    return capi.imu_window(w["t_ref"], w["t_cur"], w["t"], w["w"], w["bias"])


def _loop(sq, scene, frames, sp, mode, sensor):
    lists = scene["cands"] if sp.detector == 0 else [None] * NF
    try:
        if sensor:
            sq.start(frames[0], lists[0], t=scene["times"][0])
        else:
            sq.start(frames[0], lists[0])
        out, pair, status, vel = [sq.read()], [None], [sq.status()], [sq.read_velocity() if sensor else None]
        for k in range(1, NF):
            if sensor:
                win, keep = _window(scene["windows"][k])
                sq.step(frames[k], None, lists[k], mode=mode, window=win)
            else:
                sq.step(frames[k], scene["rot9"][k], lists[k], mode=mode)
            status.append(sq.status())
            out.append(sq.read())
            pair.append(sq.read_pair())
            vel.append(sq.read_velocity() if sensor else None)
    finally:
        sq.close()
    return out, pair, status, vel


def _plain(scene, arm, detector, kind="rgb", mode="graph"):
    """The yardstick: a plain sequence fed the restated rectified frames and the restated rot9 (once per configuration)."""
    key = (arm, detector, kind, mode)
    if key not in scene["memo"]:
        sp = _sp(scene, arm, detector)
        scene["memo"][key] = _loop(runtime.DeviceSequence(sp), scene, scene["rect"][kind], sp, mode, False)
    return scene["memo"][key]


def _sensor_run(scene, arm, detector, kind="rgb", mode="graph", ctx=None, raw=True):
    sp = _sp(scene, arm, detector)
    c = capi.Context(0) if ctx is None else ctx
    try:
        if raw:
            c.rectify_set_maps(*scene["kinds"][kind][:2])
        frames = scene["kinds"][kind][2] if raw else scene["rect"][kind]
        sq = runtime.DeviceSequence(sp, ctx=c, sensor=_sensor(scene, kind if raw else None))
        return _loop(sq, scene, frames, sp, mode, True)
    finally:
        if ctx is None:
            c.close()


def _same(got, want):
    for k in range(NF):
        for name in SET:
            assert np.asarray(got[0][k][name]).tobytes() == np.asarray(want[0][k][name]).tobytes(), (k, name)
        if k:
            for name in PAIR:
                assert got[1][k][name].tobytes() == want[1][k][name].tobytes(), (k, name)


def _not_vacuous(run):
    states = np.array([f["state"] for f in run[0]])
    print("state words per frame:", states[:, :5].tolist())
    assert states[0, 0] > TARGET // 2 and (states[1:, 2] > 0).all(), "the sequence tracks nothing"


# ---- the sensor sequence against the plain sequence --------------------------------------------------------------------------
@pytest.mark.parametrize("detector", [0, 1], ids=["candidate-list", "harris"])
@pytest.mark.parametrize("arm", list(ARMS))
def test_sensor_sequence_equals_the_plain_sequence(scene, arm, detector):
    want = _plain(scene, arm, detector)
    got = _sensor_run(scene, arm, detector)
    _not_vacuous(want)
    _same(got, want)
    assert [s["last_was_graph"] for s in got[2]] == [False, False, False, True, True, True]     # direct, direct, graph x 3
    assert [s["graphs"] for s in got[2]] == [0, 0, 0, 1, 2, 2]
    assert [s["frames"] for s in got[2]] == list(range(1, NF + 1))


@pytest.mark.parametrize("kind", ["gray", "rgb padded", "larger raw"])
def test_other_raw_frames(scene, kind):
    """One channel; rows with padding; a raw frame (352 x 250) larger than the rectified one, so a swapped size is caught."""
    want = _plain(scene, "patchmatch", 0, kind)
    got = _sensor_run(scene, "patchmatch", 0, kind)
    if kind != "larger raw":                                     # (noise through random maps: nothing to track, every byte equal)
        _not_vacuous(want)
    _same(got, want)
    if kind == "rgb padded":                                     # the padding is not read: the results are those of the dense rows
        _same(got, _plain(scene, "patchmatch", 0, "rgb"))


def test_gray_rectified_frames_with_the_imu_half_alone(scene):
    got = _sensor_run(scene, "lk-gyro", 0, raw=False)
    _same(got, _plain(scene, "lk-gyro", 0))


@pytest.mark.parametrize("arm", list(ARMS))
def test_graph_equals_direct(scene, arm):
    graph = _sensor_run(scene, arm, 0, mode="graph")
    direct = _sensor_run(scene, arm, 0, mode="direct")
    _same(graph, direct)
    assert not any(s["last_was_graph"] for s in direct[2]) and all(s["graphs"] == 0 for s in direct[2])
    assert sum(s["last_was_graph"] for s in graph[2]) == NF - 3
    for k in range(NF):
        assert graph[3][k].tobytes() == direct[3][k].tobytes(), k


def test_velocities_equal_the_model(scene):
    frames, _, _, vel = _sensor_run(scene, "patchmatch", 0)
    assert not vel[0].any()                                      # the first frame has no pair
    moving = 0
    for k in range(1, NF):
        f, last = frames[k], frames[k - 1]
        want = gu.model_flow_velocity(CAP, int(f["state"][0]), f["keys_normal"], last["keys_normal"], f["index_in_last"],
                                      scene["times"][k], scene["times"][k - 1])
        assert vel[k].tobytes() == want.tobytes(), k
        top_up = (f["index_in_last"] < 0) | (np.arange(CAP) >= int(f["state"][0]))
        assert not vel[k][top_up].any(), k
        moving += int(np.count_nonzero(vel[k][~top_up].any(axis=1)))
    assert moving > TARGET                                       # survivors move: about |STEP| / DT in the normal plane
    # flow_velocity = 0: the call is refused, everything else is unchanged
    c = capi.Context(0)
    try:
        c.rectify_set_maps(*scene["kinds"]["rgb"][:2])
        sq = runtime.DeviceSequence(_sp(scene, "patchmatch"), ctx=c, sensor=_sensor(scene, "rgb", flow_velocity=0))
        try:
            sq.start(scene["kinds"]["rgb"][2][0], scene["cands"][0], t=T0)
            assert np.asarray(sq.read()["keys_un"]).tobytes() == np.asarray(frames[0]["keys_un"]).tobytes()
            with pytest.raises(capi.PagkError):
                sq.read_velocity()
        finally:
            sq.close()
    finally:
        c.close()


def test_result_does_not_depend_on_what_the_workspaces_held(scene):
    runs = []
    for word in (0x00000001, 0xffc0ffc0):
        c = capi.Context(0)
        try:
            c.selftest_fill_workspaces(word, True)
            runs.append(_sensor_run(scene, "lk-gyro", 0, ctx=c))
        finally:
            c.close()
    _same(runs[0], runs[1])
    _same(runs[0], _plain(scene, "lk-gyro", 0))
    for k in range(NF):
        assert runs[0][3][k].tobytes() == runs[1][3][k].tobytes(), k


# ---- the refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(scene):
    c = capi.Context(0)
    E = capi.PAGK_E_ARG
    mx, my, raws = scene["kinds"]["rgb"]
    rect, cand = scene["rect"]["rgb"], scene["cands"][0]
    sp, sensor = _sp(scene, "patchmatch"), _sensor(scene, "rgb", imu_cap=8)
    win = [None] + [_window(w) for w in scene["windows"][1:]]

    def refused(fn, *a, words=(), **kw):
        with pytest.raises(capi.PagkError) as e:
            fn(*a, **kw)
        assert e.value.code == E
        text = c.lib.pagk_last_error(c.h).decode()
        assert all(wd in text for wd in words), (text, words)
    try:
        refused(c.sequence_create_sensor, sp, sensor, words=("maps",))                 # missing maps
        c.rectify_set_maps(mx[:-8], my[:-8])
        refused(c.sequence_create_sensor, sp, sensor, words=("320 x 232", "320 x 240"))  # maps of another size
        c.rectify_set_maps(mx, my)
        c.sequence_create(sp)                                                          # a plain sequence: no _sensor call
        refused(c.sequence_start_sensor, raws[0], T0, cand, words=("plain sequence",))
        c.sequence_start(rect[0], cand)
        refused(c.sequence_step_sensor, raws[1], win[1][0], cand, words=("plain sequence",))
        refused(c.sequence_read_velocity, CAP)
        c.sequence_destroy()
        c.sequence_create_sensor(sp, sensor)                                           # a sensor sequence: no plain call
        refused(c.sequence_create_sensor, sp, sensor)                                  # create twice
        refused(c.sequence_start, rect[0], cand, words=("sensor sequence",))
        refused(c.sequence_step_sensor, raws[1], win[1][0], cand)                      # step before start
        refused(c.sequence_start_sensor, rect[0], T0, cand)                            # a gray frame where a raw one is due
        refused(c.sequence_start_sensor, raws[0], float("nan"), cand)
        c.sequence_start_sensor(raws[0], T0, cand)
        refused(c.sequence_step, rect[1], scene["rot9"][1], cand, words=("sensor sequence",))
        refused(c.sequence_step_sensor, raws[1], win[2][0], cand, words=("previous frame",))   # t_ref out of step
        long = gu.constant_rate_window(STEP, scene["times"][0], scene["times"][1], n=9)
        refused(c.sequence_step_sensor, raws[1], _window(long)[0], cand, words=("imu_cap 8",))  # a window beyond imu_cap
        bad = dict(scene["windows"][1], t_cur=scene["times"][0])
        refused(c.sequence_step_sensor, raws[1], _window(bad)[0], cand)                # t_cur <= t_ref
        assert c.sequence_status()["frames"] == 1                                      # nothing of this reached the sequence
        c.sequence_step_sensor(raws[1], win[1][0], scene["cands"][1], mode=capi.SEQ_DIRECT)
        assert c.sequence_read(CAP)["total"] > 0 and c.sequence_status()["frames"] == 2
        d_img = torch.zeros((TH, TW), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        c.frame_set_device(3, d_img.data_ptr(), TW, TH, TW, 3)                         # (sizes slot 3 for the captured call)
        c.sync()
        c.graph_begin()                                                                # any call inside a capture
        try:
            refused(c.sequence_step_sensor, raws[2], win[2][0], scene["cands"][2])
            refused(c.sequence_start_sensor, raws[0], T0, cand)
            refused(c.sequence_read_velocity, CAP)
            refused(c.sequence_create_sensor, sp, sensor)
            cam = capi.make_params(camera=scene["cam"])
            refused(c.gyro_integrate, np.eye(3), cam, win[1][0])
            c.frame_set_device(3, d_img.data_ptr(), TW, TH, TW, 3)
        finally:
            gid = c.graph_end()
        c.graph_destroy(gid)
        c.sequence_step_sensor(raws[2], win[2][0], scene["cands"][2], mode=capi.SEQ_DIRECT)
        assert c.sequence_status()["frames"] == 3
        want = _plain(scene, "patchmatch", 0, mode="direct")
        got = c.sequence_read(CAP)
        for name in SET:
            assert np.asarray(got[name]).tobytes() == np.asarray(want[0][2][name]).tobytes(), name
    finally:
        c.close()


# ---- the example -------------------------------------------------------------------------------------------------------------
def test_example_prints_the_state_words_of_the_python_run(built, scene, tmp_path):
    """examples/sequence_loop.cpp --sensor, built against the shipped headers and libraries: it reads image_file_list.txt and
    imu.txt through csrc/host/sequence_io.h and ImuWindow; its per-frame state words are those of the same files through
    host_api.load_imu / imu_windows and runtime.DeviceSequence(sensor=...)."""
    import os
    import struct
    import subprocess
    from pixel_aware_gyro_aided_klt_feature_tracker_amd import host_api
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = capi.PKG_DIR
    exe = str(tmp_path / "sequence_loop")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-DPAGK_EXAMPLE_SENSOR", "-I", os.path.join(root, "include"), "-I",
                    os.path.join(pkg, "csrc", "host"), os.path.join(root, "examples", "sequence_loop.cpp"), "-o", exe, "-L", pkg,
                    "-l:libpagk_tracker.so", "-l:libpagk_hip.so", f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    cam, p = scene["cam"], scene["p"]
    mx, my, raws = scene["kinds"]["rgb"]
    d = tmp_path / "seq"
    d.mkdir()
    period = 33_333_333
    stamps = [100_000_000_000 + k * period for k in range(NF)]
    (d / "image_file_list.txt").write_text("".join(f"/data/cam0/{s}.png\n" for s in stamps))
    for s, r in zip(stamps, raws):
        (d / f"{s}.raw").write_bytes(np.ascontiguousarray(r).tobytes())
    rate = (-np.asarray(STEP, np.float64) / (period * 1e-9)).astype(np.float32)      # constant: Rcl is the scene's step
    with open(d / "imu.txt", "w") as f:
        for s in range(stamps[0] - 12_000_000, stamps[-1] + 12_000_000, 5_000_000):   # 200 Hz
            f.write(f"{s} 0.0 9.81 0.0 {float(rate[0]):.9g} {float(rate[1]):.9g} {float(rate[2]):.9g}\n")
    bias = np.array([0.001, -0.002, 0.0005], np.float32)
    with open(d / "sensor.bin", "wb") as f:
        f.write(struct.pack("<6i", TW, TH, TW, TH, 3, 200))
        f.write(cam.K.astype(np.float32).tobytes() + np.asarray(cam.dist[:4], np.float32).tobytes())
        f.write(np.eye(3, dtype=np.float32).tobytes() + bias.tobytes())
        f.write(np.ascontiguousarray(mx, np.float32).tobytes() + np.ascontiguousarray(my, np.float32).tobytes())
        for c in scene["cands"]:
            assert c.shape == (200, 2)
            f.write(np.ascontiguousarray(c, np.float32).tobytes())
    r = subprocess.run([exe, str(d), str(TARGET), str(CAP), "--sensor", "--lk-gyro"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    lines = r.stdout.strip().splitlines()
    print("\n".join(lines), r.stderr.strip())
    # the same files through the Python layers; the example's configuration: the library's default fit, the file's camera
    times = [s * 1e-9 for s in stamps]
    imu = host_api.load_imu(str(d / "imu.txt"))
    first, counts = host_api.imu_windows(str(d / "imu.txt"), times)
    assert counts[0] == 0 and (counts[1:] >= 6).all() and (counts[1:] <= 8).all(), counts
    sp = _sp(scene, "lk-gyro")
    sp.fit, sp.cand_cap = capi.fit_params_default(), 200
    sp.track.n_dist_coef = 4
    sp.track.dist_coef[4] = 0.0
    c = capi.Context(0)
    try:
        c.rectify_set_maps(mx, my)
        sq = runtime.DeviceSequence(sp, ctx=c, sensor=_sensor(scene, "rgb"))
        try:
            sq.start(raws[0], scene["cands"][0], t=times[0])
            got = [sq.read()]
            for k in range(1, NF):
                rows = imu[first[k]:first[k] + counts[k]]
                win, keep = capi.imu_window(times[k - 1], times[k], rows[:, 6], rows[:, 3:6], bias)
                sq.step(raws[k], None, scene["cands"][k], mode="graph", window=win)
                got.append(sq.read())
        finally:
            sq.close()
    finally:
        c.close()
    _not_vacuous((got,))
    assert lines == [f"frame {k}: " + " ".join(str(int(v)) for v in g["state"][:5]) for k, g in enumerate(got)]
    assert f"{NF} frames, 2 graphs" in r.stderr
