"""GPU tests of the sensor form of the sequence group (pagk_sequence_group_*_sensor, runtime.DeviceSequenceGroup(sensor=...)):
k sensor sequences stepped together against k sensor sequences stepped alone (runtime.DeviceSequence(sp, sensor=...), each on
a context of its own) fed the same raw frames, windows and lists.  Every comparison is byte for byte: every array of read(),
read_pair() and read_velocity() after every frame.  The rigs are those of tests/group_sensor_cases.py; camera 0 of rig A is
also held against the CPU model (tests/sequence_model.run_sensor), so the group is pinned to the model and not only to the
library."""
import numpy as np
import pytest

import group_sensor_cases as gc
import sequence_model as sm
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, runtime

pytestmark = pytest.mark.gpu
NF = gc.NF
SET = ("keys", "keys_un", "keys_normal", "index_in_last", "live", "state", "info")
PAIR = ("status", "pt_predict", "pt_predict_un", "err")
E = capi.PAGK_E_ARG


@pytest.fixture(scope="module")
def rigs():
    """The rigs, computed once and left unchanged, and the single-camera runs by configuration."""
    return dict(A=gc.rig_a(), B0=gc.rig_b(0), B1=gc.rig_b(1), C=gc.rig_c(), singles={})


def _own_sensor(rig, cam, **kw):
    return gc.sensor_params(rig, Rbc=cam["rbc"], **kw)


def _lists(rig, cams, k):
    return None if rig["cfg"]["detector"] else [c["cands"][k] for c in cams]


def _snap(seq, pair: bool, vel: bool):
    return dict(set=seq.read(), pair=seq.read_pair() if pair else None, vel=seq.read_velocity() if vel else None)


def _alone(rig, cam, mode="graph", passes=1, nf=NF, first=0, seq=None, out=None):
    """One camera stepped alone on a context of its own: per pass and frame its snapshot."""
    sp, vel = gc.sequence_params(rig), bool(rig["flow_velocity"])
    own = seq is None
    if own:
        ctx = capi.Context(0)
        try:
            if cam["maps"] is not None:
                ctx.rectify_set_maps(*cam["maps"])
            seq = runtime.DeviceSequence(sp, ctx=ctx, sensor=_own_sensor(rig, cam))
        except Exception:
            ctx.close()
            raise
        seq._own = True
    out = [] if out is None else out
    try:
        for _ in range(passes):
            if first == 0:
                seq.start(cam["frames"][0], cam["cands"][0], t=cam["times"][0])
                out.append(_snap(seq, False, vel))
            for k in range(max(first, 1), nf):
                win, keep = gc.window(cam["windows"][k])
                seq.step(cam["frames"][k], None, cam["cands"][k], mode=mode, window=win)
                out.append(_snap(seq, True, vel))
    finally:
        if own:
            seq.close()
    return out


def _single(rigs, rig, j, cam=None, passes=1, tag=None):
    key = (rig["name"], j if tag is None else tag, passes)
    if key not in rigs["singles"]:
        rigs["singles"][key] = _alone(rig, rig["cameras"][j] if cam is None else cam, passes=passes)
    return rigs["singles"][key]


def _make(rig, cams):
    maps = None if rig["raw"] is None else [c["maps"] for c in cams]
    return runtime.DeviceSequenceGroup(gc.sequence_params(rig), len(cams), sensor=gc.sensor_params(rig),
                                       rbc=[c["rbc"] for c in cams], maps=maps)


def _start(g, rig, cams):
    g.start([c["frames"][0] for c in cams], _lists(rig, cams, 0), t=[c["times"][0] for c in cams])


def _step(g, rig, cams, k, mode, windows=None, lists="own"):
    wins = [gc.window(c["windows"][k]) for c in cams] if windows is None else windows
    g.step([c["frames"][k] for c in cams], windows=[w[0] for w in wins], cands=_lists(rig, cams, k) if lists == "own" else lists,
           mode=mode)


def _group(rig, cams, mode, passes=1, nf=NF, before_start=None):
    """The rig through a DeviceSequenceGroup -> (per camera: per pass and frame the snapshots, the status words per frame)."""
    vel = bool(rig["flow_velocity"])
    g = _make(rig, cams)
    out, status = [[] for _ in cams], []
    try:
        for _ in range(passes):
            if before_start:
                before_start(g)
            _start(g, rig, cams)
            status.append(g.status())
            for j in range(len(cams)):
                out[j].append(_snap(g.seqs[j], False, vel))
            for k in range(1, nf):
                _step(g, rig, cams, k, mode)
                status.append(g.status())
                for j in range(len(cams)):
                    out[j].append(dict(set=g.read(j), pair=g.read_pair(j), vel=g.read_velocity(j) if vel else None))
    finally:
        g.close()
    return out, status


def _same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        for name in SET:
            assert np.asarray(g["set"][name]).tobytes() == np.asarray(w["set"][name]).tobytes(), (what, k, name)
        assert (g["pair"] is None) == (w["pair"] is None) and (g["vel"] is None) == (w["vel"] is None), (what, k)
        for name in PAIR if g["pair"] is not None else ():
            assert np.asarray(g["pair"][name]).tobytes() == np.asarray(w["pair"][name]).tobytes(), (what, k, name)
        if g["vel"] is not None:
            assert g["vel"].tobytes() == w["vel"].tobytes(), (what, k, "velocity")


def _words(cam_frames):
    return [s["set"]["state"][:5].tolist() for s in cam_frames]


# ---- 1. rig A: FAST, raw colour, three cameras that differ in what a record carries -------------------------------------------
def test_rig_a_equals_three_sensor_sequences(rigs):
    rig = rigs["A"]
    cams = rig["cameras"]
    want = [_single(rigs, rig, j, passes=2) for j in range(3)]
    graph, gs = _group(rig, cams, "graph", passes=2)
    direct, ds = _group(rig, cams, "direct", passes=2)
    print("state words per camera and frame:", [_words(c[:NF]) for c in graph])
    for j in range(3):
        _same(graph[j], want[j], f"graph, camera {j}")
        _same(direct[j], graph[j], f"direct against graph, camera {j}")
    # member by member, batched, then each parity captured and replayed; the restart keeps the graphs
    assert [s["last_was_graph"] for s in gs] == [False, False, False] + [True] * (NF - 3) + [False] + [True] * (NF - 1)
    assert [s["graphs"] for s in gs] == [0, 0, 0, 1, 2] + [2] * (2 * NF - 5)
    assert [s["frames"] for s in gs] == 2 * list(range(1, NF + 1)) and all(s["k"] == 3 for s in gs)
    replays = [k for k, s in enumerate(gs) if s["last_was_graph"]]
    assert sum(1 for k in replays if (k % NF) % 2 == 1) >= 3 and sum(1 for k in replays if (k % NF) % 2 == 0) >= 3
    assert not any(s["last_was_graph"] or s["graphs"] for s in ds)
    # the rig is ragged on the device as in the model: frame 1 tops up camera 1 alone, camera 2 loses everything at its gray frame
    words = [_words(c[:NF]) for c in graph]
    assert words[0][1][3] == 0 and words[2][1][3] == 0 and words[1][1][3] > 0
    assert words[2][3][0] == 0 and words[2][4][2] == 0 and words[2][4][3] > 0
    assert any(s["vel"].any() for s in graph[1][1:NF])


# ---- 2. camera 0 of rig A against the CPU model -------------------------------------------------------------------------------
def test_camera_0_equals_the_cpu_model(rigs, tmp_path_factory):
    rig = rigs["A"]
    refs = sm.build_refs(tmp_path_factory.mktemp("group_sensor_model"))
    want = gc.model(refs, rig, 0)
    got, _ = _group(rig, rig["cameras"], "graph")
    for k, (g, w) in enumerate(zip(got[0], want)):
        for name in ("keys", "keys_un", "keys_normal", "index_in_last", "live", "state"):
            assert np.asarray(g["set"][name]).tobytes() == np.asarray(w[name]).tobytes(), (k, name)
        assert g["vel"].tobytes() == w["velocity"].tobytes(), (k, "velocity")
        if k:
            pair = w["pair"]
            n, rows = pair["n"], pair["defined"]
            assert g["pair"]["status"][:n].tobytes() == pair["status"].tobytes(), (k, "status")
            for name in ("pt_predict", "pt_predict_un"):
                assert g["pair"][name][:n][rows].tobytes() == pair[name][rows].tobytes(), (k, name)


# ---- 3. rig B in both switch settings, rig C ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["B0", "B1", "C"])
def test_lists_and_the_imu_half_alone(rigs, name):
    rig = rigs[name]
    cams = rig["cameras"]
    got, gs = _group(rig, cams, "graph")
    print("state words per camera and frame:", [_words(c) for c in got])
    for j in range(len(cams)):
        _same(got[j], _single(rigs, rig, j), f"rig {name}, camera {j}")
    assert [s["last_was_graph"] for s in gs] == [False, False, False] + [True] * (NF - 3)
    if name != "C":   # rows of the second block of 256 are live for the full camera, the sparse one holds fewer in every frame
        assert got[0][0]["set"]["state"][0] > 256 and all(a["set"]["state"][0] != b["set"]["state"][0] for a, b in zip(got[0], got[1]))
        if name == "B0":   # (survivors come first in a key set: only B0 keeps more than 256 of them, and they move)
            assert any(s["vel"][256:].any() for s in got[0][1:])
    else:
        with pytest.raises(capi.PagkError):
            g = _make(rig, cams)
            try:
                _start(g, rig, cams)
                g.read_velocity(0)                                                # flow_velocity = 0: nothing to read
            finally:
                g.close()


# ---- 4. k = 1 and k = 5 -----------------------------------------------------------------------------------------------------------
def test_one_camera_and_five(rigs):
    rig = rigs["A"]
    one, _ = _group(rig, rig["cameras"][:1], "direct")
    _same(one[0], _single(rigs, rig, 0, passes=2)[:NF], "k = 1")
    cams = [rig["cameras"][0]] + [gc.rolled_camera(rig, s) for s in (1, 2, 3, 4)]
    five, gs = _group(rig, cams, "direct")
    for j, cam in enumerate(cams):
        want = _single(rigs, rig, 0, passes=2)[:NF] if j == 0 else _single(rigs, rig, 0, cam=cam, tag=f"rolled {j}")
        _same(five[j], want, f"k = 5, camera {j}")
    assert all(s["k"] == 5 for s in gs) and five[1][2]["set"]["keys"].tobytes() != five[2][2]["set"]["keys"].tobytes()


# ---- 5. group, then alone ---------------------------------------------------------------------------------------------------------
def test_group_then_alone(rigs):
    rig = rigs["A"]
    cams = rig["cameras"]
    g = _make(rig, cams)
    got = [[] for _ in cams]
    try:
        _start(g, rig, cams)
        for j in range(3):
            got[j].append(_snap(g.seqs[j], False, True))
        for k in range(1, 4):
            _step(g, rig, cams, k, "graph")
            for j in range(3):
                got[j].append(_snap(g.seqs[j], True, True))
        g.dissolve()
        for j in range(3):                                        # ... and alone again from where it stands
            _alone(rig, cams[j], first=4, nf=6, seq=g.seqs[j], out=got[j])
    finally:
        g.close()
    for j in range(3):
        _same(got[j], _single(rigs, rig, j, passes=2)[:6], f"camera {j}")


# ---- 6. what the workspaces held --------------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_what_the_workspaces_held(rigs):
    rig = rigs["A"]
    words = iter((0x00000001, 0xffc0ffc0))

    def fill(g):                                                  # in front of both starts: the second finds the tables built
        word = next(words)
        for s in g.seqs:
            s.ctx.selftest_fill_workspaces(word, True)
    # (direct mode: the fill is refused while a graph of the context is alive; both tables are state and survive it)
    got, _ = _group(rig, rig["cameras"], "direct", passes=2, before_start=fill)
    for j in range(3):
        _same(got[j], _single(rigs, rig, j, passes=2), f"camera {j}")


# ---- 7. refusals, each followed by a step whose results are unaffected ------------------------------------------------------------
def test_refusals_leave_the_rig_as_it_was(rigs):
    rig = rigs["A"]
    cams = rig["cameras"]
    sp = gc.sequence_params(rig)
    want = [_single(rigs, rig, j, passes=2)[:4] for j in range(3)]
    ctxs, seqs, extra = [], [], []

    def sensor_seq(cam, **kw):
        ctx = capi.Context(0)
        ctx.rectify_set_maps(*cam["maps"])
        s = runtime.DeviceSequence(sp, ctx=ctx, sensor=_own_sensor(rig, cam, **kw))
        s._own = True
        return s

    def refused(fn, *a, words=(), **kw):
        with pytest.raises(capi.PagkError) as e:
            fn(*a, **kw)
        assert e.value.code == E and all(w in str(e.value) for w in words), e.value
    group = plain_group = None
    try:
        seqs = [sensor_seq(c) for c in cams]
        ctxs = [s.ctx for s in seqs]
        plain = [runtime.DeviceSequence(capi.sequence_params_default(width=160, height=120)) for _ in range(2)]
        other = sensor_seq(cams[0], imu_cap=32)
        extra = plain + [other]
        refused(capi.SequenceGroup, [ctxs[0], plain[0].ctx], sensor=True, words=("plain sequence",))
        refused(capi.SequenceGroup, [ctxs[0], other.ctx], sensor=True, words=("Rbc only",))      # imu_cap differs
        refused(capi.SequenceGroup, [ctxs[0], ctxs[1]], words=("sensor",))                       # the plain create on sensor sequences
        group = capi.SequenceGroup(ctxs, sensor=True)                                            # Rbc-only differences are accepted
        plain_group = capi.SequenceGroup([p.ctx for p in plain])
        lib = capi.load()
        assert lib.pagk_sequence_group_start_sensor(ctxs[0].h, None, None, None, None) == E
        assert lib.pagk_sequence_group_step_sensor(ctxs[0].h, None, None, None, None, capi.SEQ_DIRECT) == E
        got = [[] for _ in cams]
        frames = lambda k: [c["frames"][k] for c in cams]                                          # noqa: E731
        wins = lambda k: [gc.window(c["windows"][k]) for c in cams]                                # noqa: E731
        group.start_sensor(frames(0), [c["times"][0] for c in cams])
        for j in range(3):
            got[j].append(_snap(seqs[j], False, True))
        some = np.zeros((4, 2), np.float32)
        for k in range(1, 4):
            w = wins(k)
            ok = [x[0] for x in w]
            late = wins(k + 1)                                                                   # t_ref is the NEXT frame's
            refused(group.step_sensor, frames(k), [ok[0], late[1][0], ok[2]], words=("camera 1", "previous frame"))
            refused(group.step_sensor, frames(k), ok, [some] * 3)                                # a list with detector 2
            gray = [np.zeros((rig["cfg"]["height"], rig["cfg"]["width"]), np.uint8)] * 3
            refused(group.step, gray, None, [some] * 3, words=("sensor sequences",))             # the plain step on the sensor group
            refused(plain_group.step_sensor, [np.zeros((120, 160), np.uint8)] * 2, ok[:2], [some] * 2, words=("plain sequences",))
            refused(plain_group.start_sensor, [np.zeros((120, 160), np.uint8)] * 2, [0.0, 0.0], [some] * 2, words=("plain sequences",))
            refused(ctxs[1].sequence_step_sensor, cams[1]["frames"][k], ok[1], words=("group",))  # a member's own step
            refused(ctxs[0].sequence_start_sensor, cams[0]["frames"][0], cams[0]["times"][0], words=("group",))
            refused(ctxs[2].sequence_destroy, words=("group",))
            assert group.status()["frames"] == k                                                 # nothing was enqueued, nothing counted
            group.step_sensor(frames(k), ok, mode=capi.SEQ_GRAPH)
            for j in range(3):
                got[j].append(_snap(seqs[j], True, True))
        for j in range(3):
            _same(got[j], want[j], f"camera {j}")
    finally:
        for grp in (group, plain_group):
            if grp is not None and grp.alive:
                grp.destroy()
        for s in seqs + extra:
            s.close()


# ---- 8. the example ---------------------------------------------------------------------------------------------------------------
def test_example_prints_the_state_words_of_the_python_run(built, rigs, tmp_path):
    """examples/sequence_loop.cpp --sensor --cameras 3 --detect-fast, built against the shipped headers and libraries: camera j
    is fed the raw frame (k + j) mod n_frames and the windows of imu.txt; its state words are those of the same files through
    host_api.load_imu / imu_windows and runtime.DeviceSequenceGroup(sensor=...)."""
    import os
    import struct
    import subprocess
    from pixel_aware_gyro_aided_klt_feature_tracker_amd import host_api
    rig = rigs["A"]
    cam0, cfg = rig["cameras"][0], rig["cfg"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = capi.PKG_DIR
    exe = str(tmp_path / "sequence_loop")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-DPAGK_EXAMPLE_SENSOR", "-I", os.path.join(root, "include"), "-I",
                    os.path.join(pkg, "csrc", "host"), os.path.join(root, "examples", "sequence_loop.cpp"), "-o", exe, "-L", pkg,
                    "-l:libpagk_tracker.so", "-l:libpagk_hip.so", f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    W, H, (ws, hs, cn), nc = cfg["width"], cfg["height"], rig["raw"], 4
    mx, my = cam0["maps"]
    raws = cam0["frames"]
    d = tmp_path / "seq"
    d.mkdir()
    period = 33_333_333
    stamps = [100_000_000_000 + k * period for k in range(NF)]
    (d / "image_file_list.txt").write_text("".join(f"/data/cam0/{s}.png\n" for s in stamps))
    for s, r in zip(stamps, raws):
        (d / f"{s}.raw").write_bytes(np.ascontiguousarray(r).tobytes())
    rate = (-np.asarray(gc.STEP, np.float64) / (period * 1e-9)).astype(np.float32)     # constant: Rcl is the scene's step
    with open(d / "imu.txt", "w") as f:
        for s in range(stamps[0] - 12_000_000, stamps[-1] + 12_000_000, 5_000_000):    # 200 Hz
            f.write(f"{s} 0.0 9.81 0.0 {float(rate[0]):.9g} {float(rate[1]):.9g} {float(rate[2]):.9g}\n")
    bias = np.array([0.001, -0.002, 0.0005], np.float32)
    p = cfg["p"]
    K = np.array([p.fx, 0, p.cx, 0, p.fy, p.cy, 0, 0, 1], np.float32)
    with open(d / "sensor.bin", "wb") as f:
        f.write(struct.pack("<6i", W, H, ws, hs, cn, nc))
        f.write(K.tobytes() + np.asarray([p.dist_coef[i] for i in range(4)], np.float32).tobytes())
        f.write(np.eye(3, dtype=np.float32).tobytes() + bias.tobytes())
        f.write(np.ascontiguousarray(mx, np.float32).tobytes() + np.ascontiguousarray(my, np.float32).tobytes())
        for _ in range(NF):
            f.write(np.zeros((nc, 2), np.float32).tobytes())
    r = subprocess.run([exe, str(d), str(cfg["target_n"]), str(cfg["cap"]), "--sensor", "--cameras", "3", "--detect-fast"],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    lines = r.stdout.strip().splitlines()
    print("\n".join(lines), r.stderr.strip())
    # the same files through the Python layers; the example's configuration: the library's default fit, the file's camera
    times = [s * 1e-9 for s in stamps]
    imu = host_api.load_imu(str(d / "imu.txt"))
    first, counts = host_api.imu_windows(str(d / "imu.txt"), times)
    sp = gc.sequence_params(rig)
    sp.fit, sp.cand_cap = capi.fit_params_default(), nc
    sp.track.n_dist_coef = 4
    sp.track.dist_coef[4] = 0.0
    g = runtime.DeviceSequenceGroup(sp, 3, sensor=gc.sensor_params(rig), maps=[(mx, my)] * 3)
    want = []
    try:
        for k in range(NF):
            frames = [raws[(k + j) % NF] for j in range(3)]
            if k == 0:
                g.start(frames, None, t=[times[0]] * 3)
            else:
                rows = imu[first[k]:first[k] + counts[k]]
                wins = [capi.imu_window(times[k - 1], times[k], rows[:, 6], rows[:, 3:6], bias) for _ in range(3)]
                g.step(frames, windows=[w[0] for w in wins], mode="graph")
            want += [f"camera {j} frame {k}: " + " ".join(str(int(v)) for v in g.read(j)["state"][:5]) for j in range(3)]
    finally:
        g.close()
    assert lines == want
    assert any(int(ln.split()[-2]) > 0 for ln in lines[3:]), "no camera ever tops up"
    assert f"3 cameras, {NF} frames, 2 graphs" in r.stderr
