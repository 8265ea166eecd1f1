"""GPU tests of the sequence group (pagk_sequence_group_*, runtime.DeviceSequenceGroup): k cameras stepped together against
k independent single sequences (runtime.DeviceSequence, the code as it stood before the group) fed the same frames, rot9 and
candidates.  Every comparison is byte for byte: every array of read() and read_pair(), state and info, after every frame.
The rotating synthetic sequence of tests/test_sequence_gpu.py cut down to 320 x 240, h = 5, three levels, 7 frames."""
import os
import struct
import subprocess

import numpy as np
import pytest

import handover_ref_util as hu
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, runtime, synth

pytestmark = pytest.mark.gpu
W, H, NF = 320, 240, 7
CAP, TARGET, RATIO = 448, 400, 0.8
SET = ("keys", "keys_un", "keys_normal", "index_in_last", "live", "state", "info")
PAIR = ("status", "pt_predict", "pt_predict_un", "err")
E = capi.PAGK_E_ARG


@pytest.fixture(scope="module")
def scene():
    cam, imgs, Rs, KRKs, rot9, _ = hu.rotating_sequence(synth, NF, W, H, 0x5EED0A10, (0.035, -0.045, 0.03))
    lists = [np.ascontiguousarray(c * np.float32(0.5)) for c in hu.seq_candidates()]      # 500 points each, inside 320 x 240
    rng = np.random.default_rng(0x6A0B)
    many = [np.ascontiguousarray(rng.uniform((1, 1), (W - 2, H - 2), (3000, 2)).astype(np.float32)) for _ in range(NF)]
    return dict(cam=cam, imgs=imgs, rot9=rot9, cands=[lists[k % 4] for k in range(NF)], many=many,
                gray=np.full((H, W), 128, np.uint8), fit=capi.fit_params_default(seed=0x5EED0F17, iters_H=512, iters_F=256),
                singles={})


def _sp(scene, validate=1, gyro=1, cap=CAP, target=TARGET, cand_cap=1024, fit=None) -> capi.SequenceParams:
    p = capi.make_params(half_patch=5, iterations=10, pyramids=3, has_gyro=bool(gyro), camera=scene["cam"])
    return capi.sequence_params_default(track=p, fit=fit if fit is not None else scene["fit"], tracker=capi.SEQ_PATCHMATCH,
                                        width=W, height=H, cap=cap, target_n=target, new_point_threshold=target * RATIO,
                                        detector=0, cand_cap=cand_cap, validate=validate, sigma=1.0)


# ---- what each camera is fed: per frame (image, candidate list); rot9[k - 1] goes with frame k for every camera -------------
def _feed(scene, kind: str, nf: int = NF):
    imgs, cands = scene["imgs"], scene["cands"]
    if kind == "full":
        return [(imgs[k], cands[k]) for k in range(nf)]
    if kind == "sparse":      # 40 candidates, none on alternate frames: its top-up runs and its live count stays small
        return [(imgs[k], cands[k][:40] if k % 2 == 0 else cands[k][:0]) for k in range(nf)]
    if kind == "gray3":       # a constant-gray frame 3: every feature fails, nothing survives, then a full re-detection
        return [(scene["gray"] if k == 3 else imgs[k], cands[k]) for k in range(nf)]
    if kind == "shifted":     # the lists of the next frames
        return [(imgs[k], cands[(k + 1) % nf]) for k in range(nf)]
    if kind == "many":        # 3000 candidates a frame
        return [(imgs[k], scene["many"][k]) for k in range(nf)]
    if kind == "hundred":
        return [(imgs[k], scene["many"][k][:100]) for k in range(nf)]
    raise ValueError(kind)


def _snap(seq, pair: bool):
    return dict(set=seq.read(), pair=seq.read_pair() if pair else None)


def _single(scene, key, sp, kind: str, nf: int = NF, passes: int = 1):
    """One camera alone, in graph mode: per pass and frame read() and read_pair().  Computed once per configuration."""
    memo = scene["singles"]
    if (key, kind, nf, passes) in memo:
        return memo[(key, kind, nf, passes)]
    feed = _feed(scene, kind, nf)
    sq = runtime.DeviceSequence(sp)
    out = []
    try:
        for _ in range(passes):
            sq.start(*feed[0])
            out.append(_snap(sq, False))
            for k in range(1, nf):
                sq.step(feed[k][0], scene["rot9"][k - 1], feed[k][1], mode="graph")
                out.append(_snap(sq, True))
    finally:
        sq.close()
    memo[(key, kind, nf, passes)] = out
    return out


def _step_all(scene, g, feeds, k: int, mode: str):
    g.step([f[k][0] for f in feeds], [scene["rot9"][k - 1]] * len(feeds), [f[k][1] for f in feeds], mode=mode)


def _group(scene, sp, kinds, mode: str, nf: int = NF, passes: int = 1, before_start=None):
    """The rig through a DeviceSequenceGroup -> (per camera: per pass and frame the snapshots, the status words per frame)."""
    feeds = [_feed(scene, kind, nf) for kind in kinds]
    g = runtime.DeviceSequenceGroup(sp, len(kinds))
    out, status = [[] for _ in kinds], []
    try:
        if before_start:
            before_start(g)
        for _ in range(passes):
            g.start([f[0][0] for f in feeds], [f[0][1] for f in feeds])
            status.append(g.status())
            for j in range(len(kinds)):
                out[j].append(_snap(g.seqs[j], False))
            for k in range(1, nf):
                _step_all(scene, g, feeds, k, mode)
                status.append(g.status())
                for j in range(len(kinds)):
                    out[j].append(_snap(g.seqs[j], True))
    finally:
        g.close()
    return out, status


def _same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        for name in SET:
            assert np.asarray(g["set"][name]).tobytes() == np.asarray(w["set"][name]).tobytes(), (what, k, name)
        assert (g["pair"] is None) == (w["pair"] is None), (what, k)
        for name in PAIR if g["pair"] is not None else ():
            assert np.asarray(g["pair"][name]).tobytes() == np.asarray(w["pair"][name]).tobytes(), (what, k, name)


# ---- 1. the ragged rig --------------------------------------------------------------------------------------------------------
RIG = ("full", "sparse", "gray3")


@pytest.mark.parametrize("validate,gyro", [(1, 1), (0, 1), (1, 0)], ids=["validate-gyro", "gyro", "validate"])
def test_ragged_rig_equals_three_single_sequences(scene, validate, gyro):
    sp = _sp(scene, validate, gyro)
    key = ("rig", validate, gyro)
    want = [_single(scene, key, sp, kind, passes=2) for kind in RIG]
    graph, gs = _group(scene, sp, RIG, "graph", passes=2)
    direct, ds = _group(scene, sp, RIG, "direct", passes=2)
    states = [[s["set"]["state"][:5].tolist() for s in cam[:NF]] for cam in graph]
    print("state words per camera and frame:", states)
    for j, kind in enumerate(RIG):
        _same(graph[j], want[j], f"graph, camera {j} ({kind})")
        _same(direct[j], graph[j], f"direct against graph, camera {j} ({kind})")
    # the first step runs member by member, the second as batched launches, then each parity is captured and replayed; the
    # second pass (pagk_sequence_group_start again) keeps the graphs and replays from its first step on
    assert [s["last_was_graph"] for s in gs] == [False, False, False] + [True] * (NF - 3) + [False] + [True] * (NF - 1)
    assert [s["graphs"] for s in gs] == [0, 0, 0, 1, 2] + [2] * (2 * NF - 5)
    assert [s["frames"] for s in gs] == 2 * list(range(1, NF + 1)) and all(s["k"] == 3 for s in gs)
    replays = [k for k, s in enumerate(gs) if s["last_was_graph"]]
    assert sum(1 for k in replays if (k % NF) % 2 == 1) >= 3 and sum(1 for k in replays if (k % NF) % 2 == 0) >= 3
    assert not any(s["last_was_graph"] or s["graphs"] for s in ds)
    # the rig is ragged: camera 2 loses every feature at its gray frame, with and without validation, and detects anew;
    # camera 1 never holds more than its four lists of 40 candidates gave it
    assert states[2][3][2] == 0 and states[2][3][3] > 0 and states[2][2][0] > 8
    assert max(s[0] for s in states[1]) <= 4 * 40 and any(s[3] > 0 for s in states[1][1:])
    if gyro:
        assert all(s[2] > 8 for s in states[0][1:]), "the full camera keeps features when the prediction starts the tracker"


# ---- 2. more than one group of 1024, more than one round of 2048 ------------------------------------------------------------
def test_beyond_one_round(scene):
    sp = _sp(scene, cap=2200, target=2100, cand_cap=4096)
    kinds = ("many", "hundred")
    want = [_single(scene, "big", sp, kind, nf=4) for kind in kinds]
    got, gs = _group(scene, sp, kinds, "graph", nf=4)
    for j, kind in enumerate(kinds):
        _same(got[j], want[j], f"camera {j} ({kind})")
    totals = [[int(s["set"]["state"][0]) for s in cam] for cam in got]
    print("live features per camera and frame:", totals)
    # every kernel walks the cap of 2200 rows (two rounds of 2048, three groups of 1024); camera 0 fills them past one round,
    # camera 1 holds at most its four lists of 100 candidates
    assert totals[0][0] > 2048 and max(totals[1]) <= 4 * 100
    assert [s["last_was_graph"] for s in gs] == [False, False, False, True]


# ---- 3. k = 1, and k = 5 with two cameras fed alike -----------------------------------------------------------------------------
def test_one_camera_and_five(scene):
    sp = _sp(scene)
    key = ("rig", 1, 1)
    one, _ = _group(scene, sp, ("full",), "graph")
    _same(one[0], _single(scene, key, sp, "full", passes=2)[:NF], "k = 1")
    kinds = ("full", "sparse", "gray3", "shifted", "full")
    five, gs = _group(scene, sp, kinds, "graph")
    _same(five[4], five[0], "camera 4 against camera 0")
    for j, kind in enumerate(kinds):
        want = _single(scene, key, sp, kind, passes=2)[:NF] if kind in RIG else _single(scene, key, sp, kind)
        _same(five[j], want, f"k = 5, camera {j} ({kind})")
    assert all(s["k"] == 5 for s in gs)


# ---- 4. group, then alone -------------------------------------------------------------------------------------------------------
def test_group_then_alone(scene):
    sp = _sp(scene)
    key = ("rig", 1, 1)
    feeds = [_feed(scene, kind) for kind in RIG]
    want = [_single(scene, key, sp, kind, passes=2)[:6] for kind in RIG]
    g = runtime.DeviceSequenceGroup(sp, 3)
    got = [[] for _ in RIG]
    try:
        g.start([f[0][0] for f in feeds], [f[0][1] for f in feeds])
        for j in range(3):
            got[j].append(_snap(g.seqs[j], False))
        for k in range(1, 4):
            _step_all(scene, g, feeds, k, "graph")
            for j in range(3):
                got[j].append(_snap(g.seqs[j], True))
        for j in (0, 2):                                          # a member is stepped, started and destroyed through its group
            c = g.seqs[j].ctx
            for call in (lambda: c.sequence_step(feeds[j][4][0], scene["rot9"][3], feeds[j][4][1]),
                         lambda: c.sequence_start(*feeds[j][0]), c.sequence_destroy):
                with pytest.raises(capi.PagkError) as e:
                    call()
                assert e.value.code == E and "group" in str(e.value)
            assert c.sequence_status()["frames"] == 4 and g.seqs[j].read()["state"].tobytes() == got[j][-1]["set"]["state"].tobytes()
        g.dissolve()
        words = np.zeros(capi.SEQ_STATUS_WORDS, np.int32)
        assert capi.load().pagk_sequence_group_status(g.seqs[0].ctx.h, words.ctypes.data) == E     # the lead leads nothing now
        for k in (4, 5):                                          # ... and alone again from where it stands
            for j in range(3):
                g.seqs[j].step(feeds[j][k][0], scene["rot9"][k - 1], feeds[j][k][1], mode="graph")
                got[j].append(_snap(g.seqs[j], True))
    finally:
        g.close()
    for j, kind in enumerate(RIG):
        _same(got[j], want[j], f"camera {j} ({kind})")


# ---- 5. what the workspaces held --------------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_what_the_workspaces_held(scene):
    sp = _sp(scene)
    key = ("rig", 1, 1)
    runs = []
    for word in (0x00000001, 0xffc0ffc0):
        def fill(g, word=word):
            for s in g.seqs:
                s.ctx.selftest_fill_workspaces(word, True)
        runs.append(_group(scene, sp, RIG, "graph", before_start=fill)[0])
    for j, kind in enumerate(RIG):
        _same(runs[0][j], runs[1][j], f"camera {j} ({kind}), one word against the other")
        _same(runs[0][j], _single(scene, key, sp, kind, passes=2)[:NF], f"camera {j} ({kind})")


# ---- 6. refusals that need a device ---------------------------------------------------------------------------------------------
def test_refusals_leave_the_rig_as_it_was(scene):
    sp = _sp(scene)
    key = ("rig", 1, 1)
    feeds = [_feed(scene, kind) for kind in RIG]
    want = [_single(scene, key, sp, kind, passes=2)[:5] for kind in RIG]
    seqs = [runtime.DeviceSequence(sp) for _ in RIG]
    other = runtime.DeviceSequence(_sp(scene, cap=CAP + 1))                     # configured differently
    sensor = runtime.DeviceSequence(sp, sensor=capi.sequence_sensor_default())   # a sensor sequence
    ctxs = [s.ctx for s in seqs]
    group = None

    def refused(fn, *a, **kw):
        with pytest.raises(capi.PagkError) as e:
            fn(*a, **kw)
        assert e.value.code == E, e.value
        return str(e.value)
    try:
        assert "configured differently" in refused(capi.SequenceGroup, [ctxs[0], other.ctx])
        assert "sensor" in refused(capi.SequenceGroup, [ctxs[0], sensor.ctx])
        assert "twice" in refused(capi.SequenceGroup, [ctxs[0], ctxs[1], ctxs[0]])
        group = capi.SequenceGroup(ctxs)
        assert "group already" in refused(capi.SequenceGroup, [other.ctx, ctxs[1]])      # a member of two groups
        assert "group already" in refused(capi.SequenceGroup, [ctxs[2]])
        lib = capi.load()                                                          # NULL lists under a live lead
        assert lib.pagk_sequence_group_start(ctxs[0].h, None, None, None) == E
        assert lib.pagk_sequence_group_step(ctxs[0].h, None, None, None, None, capi.SEQ_DIRECT) == E
        assert lib.pagk_sequence_group_status(ctxs[0].h, None) == E and lib.pagk_sequence_group_status(ctxs[1].h, None) == E
        got = [[] for _ in RIG]
        imgs = lambda k: [np.ascontiguousarray(f[k][0]) for f in feeds]   # noqa: E731
        lists = lambda k: [f[k][1] for f in feeds]                        # noqa: E731
        refused(group.step, imgs(1), [scene["rot9"][0]] * 3, lists(1))            # before the start
        group.start(imgs(0), lists(0))
        for j in range(3):
            got[j].append(_snap(seqs[j], False))
        for k in range(1, 4):
            bad = imgs(k)
            bad[1] = np.zeros((H, W + 2), np.uint8)                               # one camera's frame has another size
            refused(group.step, bad, [scene["rot9"][k - 1]] * 3, lists(k))
            refused(group.step, imgs(k), None, lists(k))                          # this tracker predicts
            refused(group.step, imgs(k), [scene["rot9"][k - 1]] * 3, lists(k), mode=2)
            long_list = lists(k)
            long_list[2] = np.zeros((1025, 2), np.float32)                        # one camera's list is longer than cand_cap
            refused(group.step, imgs(k), [scene["rot9"][k - 1]] * 3, long_list)
            assert group.status()["frames"] == k                                  # nothing was enqueued, nothing counted
            group.step(imgs(k), [scene["rot9"][k - 1]] * 3, lists(k), mode=capi.SEQ_GRAPH)
            for j in range(3):
                got[j].append(_snap(seqs[j], True))
        # pagk_destroy of a member that is not the lead dissolves the group: the others step alone from where they stand
        ctxs[1].close()
        seqs[1]._open = False
        group.alive = False
        refused(capi.SequenceGroup.status, group)
        for j in (0, 2):
            seqs[j].step(feeds[j][4][0], scene["rot9"][3], feeds[j][4][1], mode="graph")
            got[j].append(_snap(seqs[j], True))
        for j in (0, 2):
            _same(got[j], want[j], f"camera {j} ({RIG[j]})")
        _same(got[1], want[1][:4], "camera 1 up to its destruction")
    finally:
        if group is not None and group.alive:
            group.destroy()
        for s in seqs + [other, sensor]:
            s.close()


# ---- 7. the example -------------------------------------------------------------------------------------------------------------
def test_example_prints_the_state_words_of_the_python_run(built, scene, tmp_path):
    """examples/sequence_loop.cpp --cameras 3, built against the shipped header and library: camera j is fed the file's frames
    and the candidate list of frame (k + j) mod n_frames; its state words are those of the same rig through the Python class."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = capi.PKG_DIR
    exe = str(tmp_path / "sequence_loop")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "sequence_loop.cpp"), "-o", exe, "-L", pkg, "-l:libpagk_hip.so",
                    f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    cam, nc = scene["cam"], 500
    path = str(tmp_path / "seq.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<4i", NF, W, H, nc))
        f.write(cam.K.astype(np.float32).tobytes())
        f.write(np.asarray(cam.dist[:4], np.float32).tobytes())
        for im in scene["imgs"]:
            f.write(np.ascontiguousarray(im).tobytes())
        for c in scene["cands"]:
            assert c.shape == (nc, 2)
            f.write(np.ascontiguousarray(c, np.float32).tobytes())
        for r in scene["rot9"]:
            f.write(np.ascontiguousarray(r, np.float32).tobytes())
    r = subprocess.run([exe, path, str(TARGET), str(CAP), "--cameras", "3"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    lines = r.stdout.strip().splitlines()
    print("\n".join(lines), r.stderr.strip())
    sp = _sp(scene, cand_cap=nc, fit=capi.fit_params_default())    # the example's configuration: the library's default fits
    g = runtime.DeviceSequenceGroup(sp, 3)
    want = []
    try:
        for k in range(NF):
            frames, lists = [scene["imgs"][k]] * 3, [scene["cands"][(k + j) % NF] for j in range(3)]
            if k == 0:
                g.start(frames, lists)
            else:
                g.step(frames, [scene["rot9"][k - 1]] * 3, lists, mode="graph")
            want += [f"camera {j} frame {k}: " + " ".join(str(int(v)) for v in g.read(j)["state"][:5]) for j in range(3)]
    finally:
        g.close()
    assert lines == want
    assert f"3 cameras, {NF} frames, 2 graphs" in r.stderr
