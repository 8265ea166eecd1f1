"""GPU tests of the result ring of a sequence (include/pagk.h "The result ring of a sequence"; kernel k_results_pack and
k_group_results_pack, csrc/pagk_results_kernel.h).  Every comparison is byte for byte.

The record of frame f against what pagk_sequence_read, pagk_sequence_read_pair and pagk_sequence_read_velocity return in
lock-step after frame f, on all cap rows; its ids, ages, n_new and next_id against tests/results_model.py on the frames of the
CPU model (tests/sequence_model.py); pipelined runs (no synchronising call between the hand-ins, frame k fetched after frame
k + depth - 1 was handed in) against the lock-step run's records; refusals; restarts; groups against sequences alone; the
example's pipelined loop against its lock-step loop."""
import os
import struct
import subprocess

import numpy as np
import pytest

import group_sensor_cases as gc
import results_cases as rcs
import results_model as rm
import sequence_cases as sc
import sequence_model as sm
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, runtime

pytestmark = pytest.mark.gpu
E = capi.PAGK_E_ARG
SET = ("keys", "keys_un", "keys_normal", "index_in_last", "live", "state", "info")
PAIR = ("status", "pt_predict", "pt_predict_un", "err")
ARRAYS = tuple(capi.RESULTS_ARRAYS) + ("state", "info")
SCALARS = ("frame", "cap", "n_live", "n_new", "next_id", "t")


# ---- feeds: what ONE sequence is handed, frame by frame ---------------------------------------------------------------------------
def scene_feed(scene) -> dict:
    """A row of the tables (tests/sequence_cases.py, tests/results_cases.py) as a feed."""
    r, nf = scene["row"], scene["row"]["nf"]
    lists = scene["cands"] if r["detector"] == 0 else [None] * nf
    if r["raw"] is not None:
        return dict(sp=sc.sequence_params(scene), sensor=sc.sensor_params(scene), maps=(scene["map_x"], scene["map_y"]),
                    frames=scene["raws"], cands=lists, windows=scene["windows"], times=scene["times"], rot9=None, nf=nf)
    rot9 = scene["rot9"] if (r["gyro"] or r["arm"] == "lk-gyro") else None
    return dict(sp=sc.sequence_params(scene), sensor=None, maps=None, frames=scene["imgs"], cands=lists, windows=None,
                times=[0.0] * nf, rot9=rot9, nf=nf)


def rig_feed(rig, cam) -> dict:
    """A camera of a rig of tests/group_sensor_cases.py as a feed."""
    own = capi.SequenceSensor.from_buffer_copy(gc.sensor_params(rig))
    own.Rbc = (capi.C.c_float * 9)(*[float(x) for x in np.asarray(cam["rbc"], np.float32).reshape(9)])
    return dict(sp=gc.sequence_params(rig), sensor=own, maps=cam["maps"], frames=cam["frames"], cands=cam["cands"],
                windows=cam["windows"], times=cam["times"], rot9=None, nf=len(cam["frames"]), rbc=cam["rbc"])


class Alone:
    """One feed through runtime.DeviceSequence on a context of its own."""

    def __init__(self, feed, results=None):
        self.feed, self.ctx = feed, capi.Context(0)
        try:
            if feed["maps"] is not None:
                self.ctx.rectify_set_maps(*feed["maps"])
            self.sq = runtime.DeviceSequence(feed["sp"], ctx=self.ctx, sensor=feed["sensor"], results=results)
        except Exception:
            self.ctx.close()
            raise

    def hand_in(self, k, mode="graph"):
        f = self.feed
        if k == 0:
            return self.sq.start(f["frames"][0], f["cands"][0], t=f["times"][0] if f["sensor"] is not None else None)
        if f["sensor"] is not None:
            w = f["windows"][k]
            win, keep = capi.imu_window(w["t_ref"], w["t_cur"], w["t"], w["w"], w["bias"])
            return self.sq.step(f["frames"][k], None, f["cands"][k], mode=mode, window=win)
        self.sq.step(f["frames"][k], None if f["rot9"] is None else f["rot9"][k - 1], f["cands"][k], mode=mode)

    def reads(self, k) -> dict:
        """What the three read calls deliver in lock-step after frame k, laid out as a record's arrays."""
        return lockstep_reads(self.sq, self.feed, k)

    def close(self):
        try:
            self.sq.close()
        finally:
            self.ctx.close()


def lockstep_reads(sq, feed, k) -> dict:
    cap = int(feed["sp"].cap)
    out = dict(sq.read())
    pair = sq.read_pair() if k >= 1 else dict(status=np.zeros(cap, np.uint8), pt_predict=np.zeros((cap, 2), np.float32),
                                              pt_predict_un=np.zeros((cap, 2), np.float32), err=np.zeros(cap, np.float32))
    out.update(pair)
    flows = feed["sensor"] is not None and feed["sensor"].flow_velocity
    out["velocity"] = sq.read_velocity() if flows else np.zeros((cap, 2), np.float32)
    return out


def same_record(a: dict, b: dict, what):
    for name in SCALARS:
        assert a[name] == b[name], (what, name, a[name], b[name])
    for name in ARRAYS:
        assert a[name].dtype == b[name].dtype and a[name].tobytes() == b[name].tobytes(), (what, name)


def check_record(rec, reads, feed, k, ids, what):
    """One record against the lock-step reads and the model's ids."""
    cap = int(feed["sp"].cap)
    for name in SET + PAIR + ("velocity",):
        assert rec[name].shape[0] == (cap if name not in ("state", "info") else 8), (what, name)
        assert rec[name].tobytes() == np.asarray(reads[name]).tobytes(), (what, name)
    assert (rec["frame"], rec["cap"], rec["n_live"]) == (k, cap, int(reads["state"][0])), what
    assert rec["t"] == (feed["times"][k] if feed["sensor"] is not None else 0.0), what
    if ids is not None:
        assert rec["track_id"].tobytes() == ids["track_id"].tobytes() and rec["age"].tobytes() == ids["age"].tobytes(), what
        assert (rec["n_new"], rec["next_id"]) == (ids["n_new"], ids["next_id"]), what


def lockstep(feed, mode, depth=4, ids=None, what=None, passes=1):
    """Hand in, read, fetch -- frame by frame.  Returns the records (the last pass's)."""
    a = Alone(feed, results=depth)
    try:
        for p in range(passes):
            recs = []
            for k in range(feed["nf"]):
                a.hand_in(k, mode)
                reads = a.reads(k)
                rec = a.sq.fetch(k)
                assert a.sq.poll(k) is True
                check_record(rec, reads, feed, k, None if ids is None else ids[k], (what, mode, p, k))
                recs.append(rec)
    finally:
        a.close()
    return recs


def pipelined(hand_in, fetch, nf, depth, passes=2, frame_of=lambda rec: rec["frame"]):
    """Per pass: every frame handed in with nothing synchronising in between; frame k fetched once frame k + depth - 1 is in."""
    out = []
    for _ in range(passes):
        recs = []
        for k in range(nf):
            hand_in(k)
            if k >= depth - 1:
                recs.append(fetch(k - depth + 1))
        recs += [fetch(k) for k in range(max(nf - depth + 1, 0), nf)]
        assert [frame_of(r) for r in recs] == list(range(nf))
        out.append(recs)
    return out


# ---- the expected values, computed once -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refs(built, tmp_path_factory):
    return sm.build_refs(tmp_path_factory.mktemp("results_model"))


@pytest.fixture(scope="module")
def table(refs):
    """name -> (scene, feed, the model's ids per frame), computed when first asked for and left unchanged."""
    memo = {}

    def get(name):
        if name not in memo:
            scene = rcs.scene(name)
            frames = sc.model(refs, scene)
            memo[name] = (scene, scene_feed(scene), rm.ids_of_frames(frames))
            print(f"{name}: state words {sc.words(frames)}, next_id {[g['next_id'] for g in memo[name][2]]}")
        return memo[name]
    return get


@pytest.fixture(scope="module")
def records(table):
    """name -> the records of the lock-step run in graph mode with depth 4 (every one checked against the reads and the model)."""
    memo = {}

    def get(name):
        if name not in memo:
            _, feed, ids = table(name)
            memo[name] = lockstep(feed, "graph", ids=ids, what=name)
        return memo[name]
    return get


# ---- 1. lock-step -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["graph", "direct"])
@pytest.mark.parametrize("name", rcs.LOCKSTEP)
def test_fetch_equals_the_reads_in_lock_step(table, records, name, mode):
    _, feed, ids = table(name)
    recs = records(name) if mode == "graph" else lockstep(feed, "direct", ids=ids, what=name)
    assert len(recs) == feed["nf"] and recs[0]["n_new"] == recs[0]["n_live"] and not recs[0]["status"].any()
    if name == "three-chunks-refill":       # ids issued in all three chunks of 1024 rows, behind a next_id above zero
        fresh = np.nonzero(recs[2]["index_in_last"][:recs[2]["n_live"]] < 0)[0]
        assert recs[1]["next_id"] > 0 and set((fresh // rcs.CHUNK).tolist()) == {0, 1, 2}
    if name == "sensor":
        assert any(r["velocity"].any() for r in recs[1:]) and recs[3]["t"] == feed["times"][3] != 0.0


# ---- 2. pipelined -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [4, 2])
@pytest.mark.parametrize("name", rcs.PIPELINED)
def test_pipelined_records_equal_the_lock_step_records(table, records, name, depth):
    _, feed, _ = table(name)
    want = records(name)
    a = Alone(feed, results=depth)
    try:
        # two passes of seven frames replay every parity at least three times; a row of four frames needs four passes for that
        passes = pipelined(lambda k: a.hand_in(k, "graph"), a.sq.fetch, feed["nf"], depth, passes=2 if feed["nf"] >= 7 else 4)
        st = a.sq.status()
    finally:
        a.close()
    assert st["results_depth"] == depth and st["graphs"] == 2 and st["last_was_graph"]
    for p, recs in enumerate(passes):
        for k, (g, w) in enumerate(zip(recs, want)):
            same_record(g, w, (name, depth, "pass", p, k))


# ---- 3. poll, fetch and the refusals ------------------------------------------------------------------------------------------------
def _refused(ctx, fn, *args):
    """The call is refused with PAGK_E_ARG and a text, which is returned."""
    with pytest.raises(capi.PagkError) as e:
        fn(*args)
    text = ctx.lib.pagk_last_error(ctx.h).decode()
    assert e.value.code == E and text, (e.value.code, text)
    return text


def test_poll_fetch_and_refusals(table, records):
    _, feed, _ = table("base")
    want = records("base")
    a = Alone(feed)                                   # no ring yet
    c = a.ctx
    try:
        assert a.sq.status()["results_depth"] == 0
        assert "no result ring" in _refused(c, c.sequence_fetch, 0)
        for depth in (1, 9, 0, -1):
            assert "depth" in _refused(c, c.sequence_results_create, depth)
        import torch
        row = table("base")[0]["row"]
        d_img = torch.from_numpy(np.ascontiguousarray(feed["frames"][0])).cuda()
        torch.cuda.synchronize()
        c.frame_set_device(3, d_img.data_ptr(), row["width"], row["height"], row["width"], 3)   # (sizes slot 3 for the captured call)
        c.sync()
        c.graph_begin()
        try:
            assert "pagk_graph_begin" in _refused(c, c.sequence_results_create, 4)             # inside a capture
            c.frame_set_device(3, d_img.data_ptr(), row["width"], row["height"], row["width"], 3)
        finally:
            gid = c.graph_end()
        c.graph_destroy(gid)
        c.sequence_results_create(4)
        assert "already" in _refused(c, c.sequence_results_create, 4)
        assert a.sq.status()["results_depth"] == 4
        _refused(c, c.sequence_fetch, 0)                          # nothing handed in yet
        for k in range(feed["nf"]):
            a.hand_in(k, "graph")
            assert "outside the ring" in _refused(c, c.sequence_fetch, k + 1)          # not yet handed in
            assert "outside the ring" in _refused(c, c.sequence_fetch, k - 4)          # frames_submitted - depth - 1
            _refused(c, c.sequence_poll, k + 1)
            if k == 2:
                _refused(c, c.sequence_results_create, 2)         # a second ring, and after a start
            rec = a.sq.fetch(k)                                   # every refusal is followed by a record that is unaffected
            assert a.sq.poll(k) is True
            same_record(rec, want[k], ("refusals", k))
            if k >= 3:
                same_record(a.sq.fetch(k - 3), want[k - 3], ("oldest", k))           # the oldest frame the ring holds
    finally:
        a.close()
    b = Alone(feed)                                   # a sequence that never gets a ring keeps refusing
    try:
        b.hand_in(0)
        b.hand_in(1)
        assert "no result ring" in _refused(b.ctx, b.ctx.sequence_fetch, 1)
        _refused(b.ctx, b.ctx.sequence_poll, 1)
        assert "after pagk_sequence_start" in _refused(b.ctx, b.ctx.sequence_results_create, 4)
    finally:
        b.close()


# ---- 4. what the workspaces held before --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["base", "sensor"])
def test_filled_workspaces_change_no_record(table, records, name):
    _, feed, _ = table(name)
    want = records(name)
    a = Alone(feed, results=4)
    try:
        a.ctx.selftest_fill_workspaces(0xFFFFFFFF, also_new=True)
        got = [(a.hand_in(k, "direct"), a.sq.fetch(k))[1] for k in range(feed["nf"])]
    finally:
        a.close()
    for k, (g, w) in enumerate(zip(got, want)):
        same_record(g, w, (name, "filled", k))


# ---- 5. restart ----------------------------------------------------------------------------------------------------------------------
def test_restart_begins_ids_at_zero_and_empties_the_ring(table, records):
    _, feed, _ = table("odd-gray3")
    want = records("odd-gray3")
    a = Alone(feed, results=4)
    try:
        for k in range(6):
            a.hand_in(k, "graph")
        assert a.sq.fetch(5)["next_id"] == want[5]["next_id"] > want[0]["next_id"]
        a.hand_in(0)                                                  # the restart, with frames 2 .. 5 in the ring
        for k in (1, 2, 3, 5):
            _refused(a.ctx, a.ctx.sequence_fetch, k)
        same_record(a.sq.fetch(0), want[0], "restarted 0")
        assert a.sq.fetch(0)["track_id"][:want[0]["n_live"]].tolist() == list(range(want[0]["n_live"]))
        for k in range(1, feed["nf"]):
            a.hand_in(k, "graph")
            same_record(a.sq.fetch(k), want[k], ("restarted", k))
    finally:
        a.close()


# ---- 6. groups ---------------------------------------------------------------------------------------------------------------------
def _ragged_feeds(table):
    """The ragged rig of three of the plain group (tests/test_sequence_shapes_gpu.py): the row "base", its feed with 10
    candidates on even frames and none on odd ones, its feed with a constant-gray frame 3."""
    scene, feed, _ = table("base")
    sparse = dict(feed, cands=[c[:10] if k % 2 == 0 else c[:0] for k, c in enumerate(feed["cands"])])
    gray = dict(feed, frames=[np.full_like(im, 128) if k == 3 else im for k, im in enumerate(feed["frames"])])
    return [feed, sparse, gray]


def _rig_a_feeds():
    rig = gc.rig_a()
    return [rig_feed(rig, cam) for cam in rig["cameras"]]


class Rig:
    """k feeds of one configuration through runtime.DeviceSequenceGroup."""

    def __init__(self, feeds, results):
        self.feeds, f0 = feeds, feeds[0]
        sensor = f0["sensor"] is not None
        self.g = runtime.DeviceSequenceGroup(f0["sp"], len(feeds), sensor=f0["sensor"],
                                             rbc=[f["rbc"] for f in feeds] if sensor else None,
                                             maps=[f["maps"] for f in feeds] if sensor and f0["maps"] is not None else None,
                                             results=results)

    def hand_in(self, k, mode="graph"):
        fs = self.feeds
        lists = None if fs[0]["cands"][k] is None else [f["cands"][k] for f in fs]
        if fs[0]["sensor"] is not None:
            if k == 0:
                return self.g.start([f["frames"][0] for f in fs], lists, t=[f["times"][0] for f in fs])
            wins = [gc.window(f["windows"][k]) for f in fs]
            return self.g.step([f["frames"][k] for f in fs], windows=[w[0] for w in wins], cands=lists, mode=mode)
        if k == 0:
            return self.g.start([f["frames"][0] for f in fs], lists)
        rot = None if fs[0]["rot9"] is None else [f["rot9"][k - 1] for f in fs]
        self.g.step([f["frames"][k] for f in fs], rot, lists, mode=mode)

    def close(self):
        self.g.close()


@pytest.fixture(scope="module")
def rigs(table):
    """rig -> (its feeds, per camera the records of its sequence stepped alone in lock-step with a ring)."""
    memo = {}

    def get(name):
        if name not in memo:
            feeds = _rig_a_feeds() if name == "A" else _ragged_feeds(table)
            memo[name] = (feeds, [lockstep(f, "graph", what=(name, j)) for j, f in enumerate(feeds)])
        return memo[name]
    return get


@pytest.mark.parametrize("mode", ["graph", "direct"])
@pytest.mark.parametrize("name", ["A", "ragged"])
def test_group_fetch_equals_the_sequence_alone(rigs, name, mode):
    feeds, want = rigs(name)
    r = Rig(feeds, results=4)
    try:
        for k in range(feeds[0]["nf"]):
            r.hand_in(k, mode)
            for j, f in enumerate(feeds):
                rec = r.g.fetch(j, k)
                assert r.g.poll(j, k) is True
                same_record(rec, want[j][k], (name, mode, "camera", j, k))
                check_record(rec, lockstep_reads(r.g.seqs[j], f, k), f, k, None, (name, mode, "reads", j, k))
        assert r.g.status()["k"] == len(feeds) and r.g.seqs[0].status()["results_depth"] == 4
    finally:
        r.close()
    assert len({w[-1]["next_id"] for w in want}) > 1                        # the cameras issue different numbers of ids


@pytest.mark.parametrize("depth", [4, 2])
@pytest.mark.parametrize("name", ["A", "ragged"])
def test_group_pipelined(rigs, name, depth):
    feeds, want = rigs(name)
    r = Rig(feeds, results=depth)
    try:
        passes = pipelined(lambda k: r.hand_in(k, "graph"), lambda k: [r.g.fetch(j, k) for j in range(len(feeds))],
                           feeds[0]["nf"], depth, frame_of=lambda cams: cams[0]["frame"])
    finally:
        r.close()
    for p, recs in enumerate(passes):
        assert len(recs) == feeds[0]["nf"]
        for k, cams in enumerate(recs):
            for j, rec in enumerate(cams):
                same_record(rec, want[j][k], (name, depth, "pass", p, "camera", j, k))


def test_group_of_one_and_a_mixture(rigs):
    feeds, want = rigs("ragged")
    r = Rig(feeds[:1], results=4)
    try:
        for k in range(feeds[0]["nf"]):
            r.hand_in(k, "graph")
            same_record(r.g.fetch(0, k), want[0][k], ("k = 1", k))
    finally:
        r.close()
    # members with and without a ring, and rings of two depths: refused with a text, and the contexts stay usable
    for depths in ((4, None), (None, 4), (4, 2)):
        seqs = [runtime.DeviceSequence(feeds[0]["sp"], results=d) for d in depths]
        try:
            with pytest.raises(capi.PagkError):
                capi.SequenceGroup([s.ctx for s in seqs])
            assert b"result ring" in seqs[0].ctx.lib.pagk_last_error(seqs[0].ctx.h)
        finally:
            for s in seqs:
                s.close()


def test_ids_continue_when_the_group_is_dissolved(rigs):
    feeds, want = rigs("ragged")
    r = Rig(feeds, results=4)
    try:
        for k in range(4):                                  # the start and three group steps
            r.hand_in(k, "graph")
        _refused(r.g.seqs[1].ctx, r.g.seqs[1].ctx.sequence_results_create, 4)      # while grouped
        r.g.dissolve()
        for k in (4, 5):                                    # two steps alone: the ids continue
            for j, f in enumerate(feeds):
                sq = r.g.seqs[j]
                sq.step(f["frames"][k], f["rot9"][k - 1], f["cands"][k], mode="graph")
                same_record(sq.fetch(k), want[j][k], ("alone again", j, k))
                same_record(sq.fetch(k - 2), want[j][k - 2], ("from the group's steps", j, k - 2))
    finally:
        r.close()


# ---- 7. the example ------------------------------------------------------------------------------------------------------------------
def _build_example(tmp_path, sensor: bool):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = capi.PKG_DIR
    exe = str(tmp_path / ("sequence_loop_sensor" if sensor else "sequence_loop"))
    extra = ["-DPAGK_EXAMPLE_SENSOR", "-I", os.path.join(pkg, "csrc", "host"), "-l:libpagk_tracker.so"] if sensor else []
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(root, "include"), *extra[:3],
                    os.path.join(root, "examples", "sequence_loop.cpp"), "-o", exe, "-L", pkg, *extra[3:], "-l:libpagk_hip.so",
                    f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def _both_loops(cmd):
    outs = []
    for flags in ([], ["--pipeline", "4"]):
        r = subprocess.run(cmd + flags, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, (flags, r.returncode, r.stdout, r.stderr)
        outs.append(r.stdout)
    return outs


def test_example_pipelined_prints_the_lock_step_lines_one_camera(table, tmp_path):
    scene, feed, _ = table("base")
    row, cam = scene["row"], scene["cam"]
    path = str(tmp_path / "seq.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<4i", row["nf"], row["width"], row["height"], row["n_cand"]))
        f.write(cam.K.astype(np.float32).tobytes() + np.asarray(cam.dist[:4], np.float32).tobytes())
        for im in scene["imgs"]:
            f.write(np.ascontiguousarray(im).tobytes())
        for c in scene["cands"]:
            f.write(np.ascontiguousarray(c, np.float32).tobytes())
        for r9 in scene["rot9"]:
            f.write(np.ascontiguousarray(r9, np.float32).tobytes())
    lock, pipe = _both_loops([_build_example(tmp_path, False), path, str(row["target_n"]), str(row["cap"])])
    lines = lock.strip().splitlines()
    assert lock == pipe and len(lines) == row["nf"] and lines[0].startswith("frame 0: ") and lines[-1].startswith(f"frame {row['nf'] - 1}: ")
    assert int(lines[0].split()[2]) == row["target_n"] and any(int(ln.split()[4]) > 0 for ln in lines[1:])      # filled, then tracked


def test_example_pipelined_prints_the_lock_step_lines_sensor_rig(tmp_path):
    rig = gc.rig_a()
    cam0, cfg, nf = rig["cameras"][0], rig["cfg"], gc.NF
    W, H, (ws, hs, cn), nc = cfg["width"], cfg["height"], rig["raw"], 4
    d = tmp_path / "seq"
    d.mkdir()
    period = 33_333_333
    stamps = [100_000_000_000 + k * period for k in range(nf)]
    (d / "image_file_list.txt").write_text("".join(f"/data/cam0/{s}.png\n" for s in stamps))
    for s, r in zip(stamps, cam0["frames"]):
        (d / f"{s}.raw").write_bytes(np.ascontiguousarray(r).tobytes())
    rate = (-np.asarray(gc.STEP, np.float64) / (period * 1e-9)).astype(np.float32)
    with open(d / "imu.txt", "w") as f:
        for s in range(stamps[0] - 12_000_000, stamps[-1] + 12_000_000, 5_000_000):
            f.write(f"{s} 0.0 9.81 0.0 {float(rate[0]):.9g} {float(rate[1]):.9g} {float(rate[2]):.9g}\n")
    p = cfg["p"]
    K = np.array([p.fx, 0, p.cx, 0, p.fy, p.cy, 0, 0, 1], np.float32)
    with open(d / "sensor.bin", "wb") as f:
        f.write(struct.pack("<6i", W, H, ws, hs, cn, nc))
        f.write(K.tobytes() + np.asarray([p.dist_coef[i] for i in range(4)], np.float32).tobytes())
        f.write(np.eye(3, dtype=np.float32).tobytes() + np.array([0.001, -0.002, 0.0005], np.float32).tobytes())
        f.write(np.ascontiguousarray(cam0["maps"][0], np.float32).tobytes() + np.ascontiguousarray(cam0["maps"][1], np.float32).tobytes())
        for _ in range(nf):
            f.write(np.zeros((nc, 2), np.float32).tobytes())
    lock, pipe = _both_loops([_build_example(tmp_path, True), str(d), str(cfg["target_n"]), str(cfg["cap"]), "--sensor", "--cameras", "3",
                              "--detect-fast"])
    lines = lock.strip().splitlines()
    assert lock == pipe and len(lines) == 3 * nf and lines[1].startswith("camera 1 frame 0: ")
    assert any(int(ln.split()[-2]) > 0 for ln in lines[3:]), "no camera ever tops up"
