#!/usr/bin/env python3
"""Frame time of the sequence the context owns (pagk_sequence_*, runtime.DeviceSequence) for its three arms -- PatchMatch,
Lucas-Kanade, Lucas-Kanade started from the gyro prediction -- against runtime.SequenceTracker in the same process, on
synth.config(1)-sized frames (752 x 480, 1000 keypoints).

Method: a rotating sequence of 9 frames is run once through every loop and the PatchMatch arm's key sets and state words
are compared with SequenceTracker's, byte for byte, before anything is reported (a mismatch is exit code 20).  Then every
loop steps through the frames again and again in graph mode; a window is `steps` steps between two host clock readings with
a synchronisation at both ends (the step calls themselves synchronise nothing), the loops take turns window by window, and
the figure is the median of seven windows with their minimum and maximum.  The process runs under a time limit of its own
(--limit seconds, a watchdog thread ends it with exit code 124).

    python tools/sequence_time.py --out profiles/sequence_time.json

With --sensor two more loops take their turns on the same frames: the sensor form of the sequence (pagk_sequence_*_sensor)
fed raw three-channel frames and IMU windows of eight samples, and a plain PatchMatch sequence fed the same frames rectified
in advance (tests/rectify_ref.c) with the rot9 of tests/gyro_integrate_ref.c; the two are compared byte for byte first.

    python tools/sequence_time.py --sensor --out profiles/sensor_sequence_time.json

With --cameras K the script measures a rig instead (runtime.DeviceSequenceGroup, pagk_sequence_group_*): (a) a group of K
cameras, (b) K sequences of the same configuration stepped one after another, each on its own context and replaying its own
graphs -- what a rig does without the group -- and (c) one of those sequences alone.  Camera j sees the frames and its own
rotation of the candidate list.  (a) and (b) are compared byte for byte on every array of every camera and frame first (a
mismatch is exit code 20); a step of (a) or (b) is one frame of the whole rig, and (b) is synchronised on all its contexts.

    python tools/sequence_time.py --cameras 8 --out profiles/sequence_group_time_k8.json

With --cameras K --sensor [--detect-fast] the rig is one of sensor sequences (pagk_sequence_group_*_sensor): raw RGB frames,
IMU windows and, with --detect-fast, the FAST top-up instead of the lists; the same three arms.
    python tools/sequence_time.py --cameras 8 --sensor --detect-fast

With --cameras K --lk | --lk-gyro [--sensor [--detect-fast]] the rig tracks with Lucas-Kanade (pagk_sequence_group_create_lk):
tracker type 0, the image-only baseline, or Lucas-Kanade started from the gyro prediction; the same three arms, (b) being what a
rig had before the Lucas-Kanade group.  With --only-c (plain rigs) arm (c), the single sequence, is measured alone; with --tree DIR
on the parent commit's built checkout, so that the single-camera path of the two commits is compared in one session.
    python tools/sequence_time.py --cameras 8 --lk-gyro

With --results DEPTH [--cameras K] the script measures what the loop costs when every frame's results are consumed (include/pagk.h
"The result ring of a sequence"), for one camera and, with --cameras K, for the group of K as well, PatchMatch with validation:
(a) a result ring of DEPTH blocks, frame k fetched (pagk_sequence_fetch, zero copy) after frame k + DEPTH - 1 was handed in;
(b) the calls there were before the ring, in lock-step: pagk_sequence_read and pagk_sequence_read_pair after every frame, into
arrays allocated once; (c) the loop that reads nothing.  First the records of (a) are compared byte for byte with the arrays of
(b) on every frame (exit code 20 on a mismatch), then the arms take turns window by window.  --only-c measures arm (c) alone and
touches nothing the ring added; with --tree DIR the package and the test helpers come from another built checkout, so the same
file measures (c) on the parent commit's tree in the same session.

    python tools/sequence_time.py --results 4 --cameras 8 --out profiles/sequence_results_time.json
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in sys.argv[1:-1]:   # (before the package is imported)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, N, NF = 752, 480, 1000, 9
CAP, RATIO = 1024, 0.8


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--limit", type=float, default=240.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sensor", action="store_true", help="add the sensor sequence and its plain counterpart")
    ap.add_argument("--cameras", type=int, default=0, help="measure a rig of K cameras: the group against K sequences in turn")
    ap.add_argument("--detect-fast", action="store_true", help="with --cameras K --sensor: the FAST top-up instead of the lists")
    ap.add_argument("--results", type=int, default=0, help="measure the loop with every frame read: a result ring of this depth")
    ap.add_argument("--only-c", action="store_true", help="with --results or --cameras K --lk: arm (c) alone")
    ap.add_argument("--lk", action="store_true", help="with --cameras K: the rig tracks with Lucas-Kanade (tracker type 0)")
    ap.add_argument("--lk-gyro", action="store_true", help="with --cameras K: Lucas-Kanade started from the gyro prediction")
    ap.add_argument("--tree", default=None, help="a built checkout to import the package and the test helpers from")
    a = ap.parse_args()
    threading.Timer(a.limit, lambda: os._exit(124)).start()

    import torch
    import handover_ref_util as hu
    from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, runtime, synth
    if not torch.cuda.is_available():
        print("no HIP device: nothing is measured", file=sys.stderr)
        os._exit(3)
    cam, imgs, Rs, KRKs, rot9, rng = hu.rotating_sequence(synth, NF, W, H, 0x5EED0B20, (0.004, -0.005, 0.006))
    u = rng.uniform(2 * 4 * N)
    cand = np.stack([8 + u[0::2] * (W - 16), 8 + u[1::2] * (H - 16)], axis=1).astype(np.float32)
    cands = [np.roll(cand, 97 * k, axis=0) for k in range(NF)]
    p = capi.make_params(half_patch=10, iterations=30, pyramids=3, has_gyro=True, camera=cam)
    fitp = capi.fit_params_default(seed=0x5EED0F17)

    def sp(tracker, flow):
        return capi.sequence_params_default(track=p, lk=capi.lk_params_default(), fit=fitp, tracker=tracker, lk_initial_flow=flow,
                                            width=W, height=H, cap=CAP, target_n=N, new_point_threshold=N * RATIO, detector=0,
                                            cand_cap=len(cand), validate=1, sigma=1.0)
    if a.results:
        return results(a, capi, runtime, sp(capi.SEQ_PATCHMATCH, 0), imgs, rot9, cands)
    if (a.lk or a.lk_gyro) and (not a.cameras or (a.lk and a.lk_gyro)):
        ap.error("--lk and --lk-gyro select the arm of a rig: one of them, with --cameras K")
    rig_sp = sp(capi.SEQ_LK, 1 if a.lk_gyro else 0) if a.lk or a.lk_gyro else sp(capi.SEQ_PATCHMATCH, 0)
    a.arm = "Lucas-Kanade started from the gyro prediction" if a.lk_gyro else "Lucas-Kanade" if a.lk else "PatchMatch"
    if a.cameras and a.sensor:
        return rig_sensor(a, capi, runtime, rig_sp, p, imgs, cands)
    if a.cameras:
        return rig(a, runtime, rig_sp, imgs, rot9, cands)
    arms = {"sequence PatchMatch": sp(capi.SEQ_PATCHMATCH, 0), "sequence LK": sp(capi.SEQ_LK, 0),
            "sequence LK gyro-started": sp(capi.SEQ_LK, 1)}

    # 1. results first
    st = runtime.SequenceTracker(p, W, H, CAP, N, RATIO, fitp, cand_cap=len(cand))
    want = [st.start(imgs[0], cands[0]).to_numpy()]
    for k in range(1, NF):
        want.append(st.step(imgs[k], rot9[k - 1], cands[k], mode="graph").to_numpy())
    st.synchronize()
    seqs = {name: runtime.DeviceSequence(s) for name, s in arms.items()}
    kept = {}
    for name, sq in seqs.items():
        sq.start(imgs[0], cands[0])
        got = [sq.read()]
        for k in range(1, NF):
            sq.step(imgs[k], rot9[k - 1], cands[k], mode="graph")
            got.append(sq.read())
        kept[name] = [int(g["state"][2]) for g in got[1:]]
        if name == "sequence PatchMatch":
            for k in range(NF):
                for key in ("keys", "keys_un", "keys_normal", "index_in_last", "live", "state"):
                    if np.asarray(got[k][key]).tobytes() != np.asarray(want[k][key]).tobytes():
                        print(f"frame {k}: {key} differs from SequenceTracker: nothing is reported", file=sys.stderr)
                        os._exit(20)
    print("results: the PatchMatch arm equals SequenceTracker on all", NF, "frames; survivors per frame:", kept)

    sensor_loops = {}
    if a.sensor:
        import tempfile
        import gyro_integrate_ref_util as gu
        import rectify_ref_util as ru
        tmp = tempfile.mkdtemp(prefix="pagk_sequence_time_")
        rref, gref = ru.build_ref(tmp), gu.build_ref(tmp)
        mx, my = ru.lens_maps(ru.MILD, W, H)
        raws = [np.ascontiguousarray(np.stack([im, np.roll(im, 1, axis=1), 255 - np.roll(im, 2, axis=0)], axis=2)) for im in imgs]
        rect = [ru.ref_rectify(rref, mx, my, r) for r in raws]
        dt = 1.0 / 30.0
        wins = [dict(gu.constant_rate_window((0.004, -0.005, 0.006), 50.0 + (k - 1) * dt, 50.0 + k * dt), camera=(p.fx, p.fy, p.cx, p.cy))
                for k in range(1, NF)]
        rot9_w = [gu.ref_integrate(gref, w)[1] for w in wins]
        cwin = [capi.imu_window(w["t_ref"], w["t_cur"], w["t"], w["w"], w["bias"]) for w in wins]
        sensor = capi.sequence_sensor_default(rectify=capi.rectify_params_default(channels=3), raw=1, src_width=W, src_height=H)
        c_sensor = capi.Context(0)
        c_sensor.rectify_set_maps(mx, my)
        sq_s = runtime.DeviceSequence(sp(capi.SEQ_PATCHMATCH, 0), ctx=c_sensor, sensor=sensor)
        sq_p = runtime.DeviceSequence(sp(capi.SEQ_PATCHMATCH, 0))
        sq_s.start(raws[0], cands[0], t=50.0)
        sq_p.start(rect[0], cands[0])
        for k in range(1, NF):
            sq_s.step(raws[k], None, cands[k], mode="graph", window=cwin[k - 1][0])
            sq_p.step(rect[k], rot9_w[k - 1], cands[k], mode="graph")
            gs, gp = sq_s.read(), sq_p.read()
            for key in ("keys", "keys_un", "keys_normal", "index_in_last", "live", "state"):
                if np.asarray(gs[key]).tobytes() != np.asarray(gp[key]).tobytes():
                    print(f"frame {k}: {key} of the sensor sequence differs from the plain one: nothing is reported", file=sys.stderr)
                    os._exit(20)
        print("results: the sensor sequence equals the plain sequence on rectified frames on all", NF, "frames")

        # a window restarts the sensor sequence: its time stamps go on from one frame to the next, the plain loop has none
        def sensor_step(k):
            if k == 1:
                sq_s.start(raws[0], cands[0], t=50.0)
            sq_s.step(raws[k], None, cands[k], mode="graph", window=cwin[k - 1][0])

        def plain_step(k):
            if k == 1:
                sq_p.start(rect[0], cands[0])
            sq_p.step(rect[k], rot9_w[k - 1], cands[k], mode="graph")
        sensor_loops = {"sensor sequence, raw RGB frames": (sensor_step, c_sensor.sync),
                        "plain sequence, frames rectified in advance": (plain_step, sq_p.ctx.sync)}

    # 2. windows taking turns (frame k of a window is frame 1 + k mod (NF - 1): both parities, every graph replayed)
    def window(step, sync):
        sync()
        t0 = time.perf_counter()
        for i in range(a.steps):
            k = 1 + i % (NF - 1)
            step(k)
        sync()
        return (time.perf_counter() - t0) / a.steps * 1e6

    loops = {"SequenceTracker": (lambda k: st.step(imgs[k], rot9[k - 1], cands[k], mode="graph", snapshot=False), st.synchronize)}
    for name, sq in seqs.items():
        loops[name] = ((lambda k, sq=sq: sq.step(imgs[k], rot9[k - 1], cands[k], mode="graph")), sq.ctx.sync)
    loops.update(sensor_loops)
    times = {name: [] for name in loops}
    for name, (step, sync) in loops.items():
        window(step, sync)                                     # warm-up
    for _ in range(a.windows):
        for name, (step, sync) in loops.items():
            times[name].append(window(step, sync))
    res = {"workload": f"{W}x{H}, {N} keypoints, h = 10, {a.steps} steps a window, {a.windows} windows taking turns",
           "unit": "us per frame (host clock around a window, synchronised at both ends)", "survivors_per_frame": kept, "loops": {}}
    if a.sensor:
        res["sensor_note"] = ("the two sensor loops restart at the first frame every 8 steps (one start per 8 steps is inside "
                              "their figures): a sensor sequence's time stamps must go on from frame to frame")
    for name, v in times.items():
        res["loops"][name] = dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1))
        print(f"{name:28s} {res['loops'][name]['median']:8.1f} us ({res['loops'][name]['min']:.1f} - {res['loops'][name]['max']:.1f})")
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    for sq in seqs.values():
        sq.close()
    st.close()
    os._exit(0)


def rig(a, runtime, sp, imgs, rot9, cands) -> int:
    """--cameras K: the group, K sequences one after another, one sequence."""
    K = a.cameras
    lists = [[np.roll(c, 13 * j, axis=0) for c in cands] for j in range(K)]      # camera j's candidate list of frame k
    if a.only_c:
        return rig_only_c(a, runtime, sp, imgs, rot9, lists[0])
    group = runtime.DeviceSequenceGroup(sp, K)
    singles = [runtime.DeviceSequence(sp) for _ in range(K)]
    names = ("keys", "keys_un", "keys_normal", "index_in_last", "live", "state", "info")
    pair = ("status", "pt_predict", "pt_predict_un", "err")

    # 1. results first: every array of every camera after every frame
    group.start([imgs[0]] * K, [lists[j][0] for j in range(K)])
    for j, sq in enumerate(singles):
        sq.start(imgs[0], lists[j][0])
    kept = []
    for k in range(NF):
        if k:
            group.step([imgs[k]] * K, [rot9[k - 1]] * K, [lists[j][k] for j in range(K)], mode="graph")
            for j, sq in enumerate(singles):
                sq.step(imgs[k], rot9[k - 1], lists[j][k], mode="graph")
        for j, sq in enumerate(singles):
            got, want = group.read(j), sq.read()
            both = [(n, got[n], want[n]) for n in names]
            if k:
                gp, wp = group.read_pair(j), sq.read_pair()
                both += [(n, gp[n], wp[n]) for n in pair]
            for n, g, w in both:
                if np.asarray(g).tobytes() != np.asarray(w).tobytes():
                    print(f"camera {j} frame {k}: {n} of the group differs from the sequence alone: nothing is reported", file=sys.stderr)
                    os._exit(20)
        kept.append(int(group.read(0)["state"][2]))
    print(f"results: the group of {K} equals {K} sequences alone on all {NF} frames; camera 0's survivors per frame: {kept[1:]}")

    # 2. windows taking turns; a step is one frame of the whole rig (arm c: of one camera)
    def window(step, sync):
        sync()
        t0 = time.perf_counter()
        for i in range(a.steps):
            step(1 + i % (NF - 1))
        sync()
        return (time.perf_counter() - t0) / a.steps * 1e6

    def step_group(k):
        group.step([imgs[k]] * K, [rot9[k - 1]] * K, [lists[j][k] for j in range(K)], mode="graph")

    def step_singles(k):
        for j, sq in enumerate(singles):
            sq.step(imgs[k], rot9[k - 1], lists[j][k], mode="graph")

    def sync_singles():
        for sq in singles:
            sq.ctx.sync()

    def sync_group():
        for sq in group.seqs:
            sq.ctx.sync()
    loops = {f"(a) group of {K}": (step_group, sync_group), f"(b) {K} sequences one after another": (step_singles, sync_singles),
             "(c) one sequence": (lambda k: singles[0].step(imgs[k], rot9[k - 1], lists[0][k], mode="graph"), singles[0].ctx.sync)}
    times = {name: [] for name in loops}
    for step, sync in loops.values():
        window(step, sync)                                     # warm-up
    for _ in range(a.windows):
        for name, (step, sync) in loops.items():
            times[name].append(window(step, sync))
    res = {"workload": f"{K} cameras, each {W}x{H}, {N} keypoints, {a.arm}, h = 10, validation on, graph mode, {a.steps} steps a "
                       f"window, {a.windows} windows taking turns",
           "unit": "us per rig frame for (a) and (b), per frame for (c) (host clock around a window, synchronised at both ends)",
           "group_status": group.status(), "loops": {}}
    for name, v in times.items():
        res["loops"][name] = dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1))
        print(f"{name:36s} {res['loops'][name]['median']:8.1f} us ({res['loops'][name]['min']:.1f} - {res['loops'][name]['max']:.1f})")
    ga, gb = res["loops"][f"(a) group of {K}"], res["loops"][f"(b) {K} sequences one after another"]
    res["a_range_below_b_range"] = bool(ga["max"] < gb["min"])
    try:   # the single path as the parent commit recorded it
        with open(os.path.join(ROOT, "profiles", "sequence_time.json")) as f:
            res["parent_one_sequence"] = json.load(f)["loops"]["sequence LK gyro-started" if a.lk_gyro else "sequence LK" if a.lk
                                                               else "sequence PatchMatch"]
    except (OSError, KeyError, ValueError):
        pass
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    group.close()
    for sq in singles:
        sq.close()
    os._exit(0)


def rig_only_c(a, runtime, sp, imgs, rot9, lists) -> int:
    """--cameras K --only-c: arm (c) of the rig, one sequence, alone (with --tree: on another built checkout)."""
    sq = runtime.DeviceSequence(sp)
    sq.start(imgs[0], lists[0])

    def window():
        sq.ctx.sync()
        t0 = time.perf_counter()
        for i in range(a.steps):
            k = 1 + i % (NF - 1)
            sq.step(imgs[k], rot9[k - 1], lists[k], mode="graph")
        sq.ctx.sync()
        return (time.perf_counter() - t0) / a.steps * 1e6
    window()                                                   # warm-up
    v = [window() for _ in range(a.windows)]
    res = {"workload": f"one camera, {W}x{H}, {N} keypoints, {a.arm}, h = 10, validation on, graph mode, {a.steps} steps a window, "
                       f"{a.windows} windows", "tree": ROOT if a.tree else "this", "unit": "us per frame",
           "loops": {"(c) one sequence": dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1))}}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    sq.close()
    os._exit(0)


def rig_sensor(a, capi, runtime, sp, p, imgs, cands) -> int:
    """--cameras K --sensor [--detect-fast]: the sensor group, K sensor sequences one after another on their own streams, one
    sensor sequence.  Raw RGB frames of 752 x 480 through the mild lens maps; camera j sees the frames rolled by 3 j columns, its
    own Rbc (a roll of 0.01 j about the optical axis) and, without --detect-fast, its own lists."""
    import gyro_integrate_ref_util as gu
    import rectify_ref_util as ru
    K = a.cameras
    if a.detect_fast:
        sp.detector, sp.cand_cap = 2, 0
    mx, my = ru.lens_maps(ru.MILD, W, H)
    raws = [[np.ascontiguousarray(np.stack([im, np.roll(im, 1, axis=1), 255 - np.roll(im, 2, axis=0)], axis=2))
             for im in (np.roll(im, 3 * j, axis=1) for im in imgs)] for j in range(K)]
    lists = [[np.roll(c, 13 * j, axis=0) for c in cands] for j in range(K)]
    rbc = [gu.rodrigues64((0.0, 0.0, 0.01 * j)).astype(np.float32) for j in range(K)]
    dt, t0 = 1.0 / 30.0, 50.0
    wins = [[capi.imu_window(w["t_ref"], w["t_cur"], w["t"], w["w"], w["bias"])
             for w in (gu.constant_rate_window(rbc[j].astype(np.float64) @ np.array((0.004, -0.005, 0.006)), t0 + (k - 1) * dt, t0 + k * dt)
                       for k in range(1, NF))] for j in range(K)]
    sensor = capi.sequence_sensor_default(rectify=capi.rectify_params_default(channels=3), raw=1, src_width=W, src_height=H)
    group = runtime.DeviceSequenceGroup(sp, K, sensor=sensor, rbc=rbc, maps=[(mx, my)] * K)
    singles = []
    for j in range(K):
        c = capi.Context(0)
        c.rectify_set_maps(mx, my)
        own = capi.SequenceSensor.from_buffer_copy(sensor)
        own.Rbc = (capi.C.c_float * 9)(*[float(x) for x in rbc[j].reshape(9)])
        singles.append(runtime.DeviceSequence(sp, ctx=c, sensor=own))
    names = ("keys", "keys_un", "keys_normal", "index_in_last", "live", "state", "info")
    pair = ("status", "pt_predict", "pt_predict_un", "err")
    cand = (lambda j, k: None) if a.detect_fast else (lambda j, k: lists[j][k])

    def group_frame(k):
        cs = None if a.detect_fast else [lists[j][k] for j in range(K)]
        if k == 0:
            group.start([raws[j][0] for j in range(K)], cs, t=[t0] * K)
        else:
            group.step([raws[j][k] for j in range(K)], windows=[wins[j][k - 1][0] for j in range(K)], cands=cs, mode="graph")

    def single_frame(j, k):
        if k == 0:
            singles[j].start(raws[j][0], cand(j, 0), t=t0)
        else:
            singles[j].step(raws[j][k], None, cand(j, k), mode="graph", window=wins[j][k - 1][0])

    # 1. results first: every array of every camera after every frame
    kept = []
    for k in range(NF):
        group_frame(k)
        for j in range(K):
            single_frame(j, k)
            got, want = group.read(j), singles[j].read()
            both = [(n, got[n], want[n]) for n in names] + [("velocity", group.read_velocity(j), singles[j].read_velocity())]
            if k:
                gp, wp = group.read_pair(j), singles[j].read_pair()
                both += [(n, gp[n], wp[n]) for n in pair]
            for n, g, w in both:
                if np.asarray(g).tobytes() != np.asarray(w).tobytes():
                    print(f"camera {j} frame {k}: {n} of the group differs from the sequence alone: nothing is reported", file=sys.stderr)
                    os._exit(20)
        kept.append([int(v) for v in group.read(0)["state"][:5]])
    print(f"results: the sensor group of {K} equals {K} sensor sequences alone on all {NF} frames; camera 0's state words: {kept}")

    # 2. windows taking turns; a step is one frame of the whole rig (arm c: of one camera).  A loop restarts at the first frame
    # every NF - 1 steps: a sensor sequence's time stamps go on from one frame to the next
    def window(step, sync):
        sync()
        t_0 = time.perf_counter()
        for i in range(a.steps):
            step(1 + i % (NF - 1))
        sync()
        return (time.perf_counter() - t_0) / a.steps * 1e6

    def step_group(k):
        if k == 1:
            group_frame(0)
        group_frame(k)

    def step_singles(k):
        for j in range(K):
            if k == 1:
                single_frame(j, 0)
            single_frame(j, k)

    def step_one(k):
        if k == 1:
            single_frame(0, 0)
        single_frame(0, k)

    def sync_singles():
        for sq in singles:
            sq.ctx.sync()

    def sync_group():
        for sq in group.seqs:
            sq.ctx.sync()
    loops = {f"(a) sensor group of {K}": (step_group, sync_group),
             f"(b) {K} sensor sequences one after another": (step_singles, sync_singles),
             "(c) one sensor sequence": (step_one, singles[0].ctx.sync)}
    times = {name: [] for name in loops}
    for step, sync in loops.values():
        window(step, sync)                                     # warm-up
    for _ in range(a.windows):
        for name, (step, sync) in loops.items():
            times[name].append(window(step, sync))
    res = {"workload": f"{K} cameras, each {W}x{H} maps from 3-channel raw frames, {N} keypoints, {a.arm}, h = 10, validation on, "
                       f"{'FAST top-up' if a.detect_fast else 'candidate lists'}, graph mode, {a.steps} steps a window, {a.windows} windows "
                       "taking turns; one start per 8 steps is inside every figure",
           "unit": "us per rig frame for (a) and (b), per frame for (c) (host clock around a window, synchronised at both ends)",
           "group_status": group.status(), "camera_0_state_words": kept, "loops": {}}
    for name, v in times.items():
        res["loops"][name] = dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1))
        print(f"{name:44s} {res['loops'][name]['median']:8.1f} us ({res['loops'][name]['min']:.1f} - {res['loops'][name]['max']:.1f})")
    ga, gb = res["loops"][f"(a) sensor group of {K}"], res["loops"][f"(b) {K} sensor sequences one after another"]
    res["a_range_below_b_range"] = bool(ga["max"] < gb["min"])
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    group.close()
    for sq in singles:
        sq._own = True
        sq.close()
    os._exit(0)


def results(a, capi, runtime, sp, imgs, rot9, cands) -> int:
    """--results DEPTH [--cameras K]: (a) the ring, pipelined, (b) read and read_pair in lock-step, (c) nothing read."""
    import ctypes as C
    D = a.results
    SET = ("keys", "keys_un", "keys_normal", "index_in_last", "live", "state", "info")
    PAIR = ("status", "pt_predict", "pt_predict_un", "err")
    out = {"workload": f"{W}x{H}, {N} keypoints, h = 10, validation on, graph mode, {a.steps} steps a window, {a.windows} windows "
                       f"taking turns; ring depth {D}", "tree": ROOT if a.tree else "this",
           "unit": "us per frame (of the whole rig for a group; host clock around a window, synchronised at both ends)"}

    class Rig:
        """K cameras (K = 0: one sequence, no group) with or without rings; camera j's list of frame k is rolled by 13 j."""

        def __init__(self, K, depth):
            self.K, self.n = K, max(K, 1)
            kw = {"results": depth} if depth else {}
            self.group = runtime.DeviceSequenceGroup(sp, K, **kw) if K else None
            self.seqs = self.group.seqs if K else [runtime.DeviceSequence(sp, **kw)]
            self.lists = [[np.roll(c, 13 * j, axis=0) for c in cands] for j in range(self.n)]
            self.handed = 0
            self.res = capi.SequenceResult() if depth else None
            self.arrays = dict(keys=np.zeros((CAP, 2), np.float32), keys_un=np.zeros((CAP, 2), np.float32),
                               keys_normal=np.zeros((CAP, 2), np.float32), index_in_last=np.zeros(CAP, np.int32),
                               live=np.zeros(CAP, np.uint8), state=np.zeros(8, np.int32), info=np.zeros(8, np.int32),
                               status=np.zeros(CAP, np.uint8), pt_predict=np.zeros((CAP, 2), np.float32),
                               pt_predict_un=np.zeros((CAP, 2), np.float32), err=np.zeros(CAP, np.float32))
            self.ptr = {k: v.ctypes.data for k, v in self.arrays.items()}

        def hand_in(self, k):
            if self.group:
                fr, ls = [imgs[k]] * self.K, [self.lists[j][k] for j in range(self.K)]
                self.group.start(fr, ls) if k == 0 else self.group.step(fr, [rot9[k - 1]] * self.K, ls, mode="graph")
            elif k == 0:
                self.seqs[0].start(imgs[0], self.lists[0][0])
            else:
                self.seqs[0].step(imgs[k], rot9[k - 1], self.lists[0][k], mode="graph")
            self.handed = 1 if k == 0 else self.handed + 1

        def read(self, j, pair=True):
            """pagk_sequence_read (and pagk_sequence_read_pair) of camera j into the arrays allocated once."""
            c, p = self.seqs[j].ctx, self.ptr
            c._check(c.lib.pagk_sequence_read(c.h, CAP, *(p[n] for n in SET)), "pagk_sequence_read")
            if pair:
                c._check(c.lib.pagk_sequence_read_pair(c.h, CAP, *(p[n] for n in PAIR)), "pagk_sequence_read_pair")
            return self.arrays

        def fetch(self, j, frame):
            c = self.seqs[j].ctx
            c._check(c.lib.pagk_sequence_fetch(c.h, frame, C.byref(self.res)), "pagk_sequence_fetch")
            return self.res

        def sync(self):
            for sq in self.seqs:
                sq.ctx.sync()

        def close(self):
            if self.group:
                self.group.close()
            else:
                self.seqs[0].close()

    def window(step, sync):
        sync()
        t0 = time.perf_counter()
        for i in range(a.steps):
            step(1 + i % (NF - 1))
        sync()
        return (time.perf_counter() - t0) / a.steps * 1e6

    for K in ([0] + ([a.cameras] if a.cameras else [])):
        title = f"group of {K}" if K else "one camera"
        arm_c = Rig(K, 0)
        arms = {"(c) nothing read": arm_c}
        if not a.only_c:
            arm_a, arm_b = Rig(K, D), Rig(K, 0)
            arms = {f"(a) ring of {D}, fetch of frame k after frame k + {D - 1}": arm_a, "(b) read + read_pair after every frame": arm_b,
                    "(c) nothing read": arm_c}
            # 1. results first: the lock-step arrays of (b) per frame and camera, then the records of (a), fetched pipelined
            want = []
            for k in range(NF):
                arm_b.hand_in(k)
                want.append([{n: v.copy() for n, v in arm_b.read(j, pair=k > 0).items()} for j in range(arm_b.n)])

            def compare(f):
                for j in range(arm_a.n):
                    rec = arm_a.seqs[j].fetch(f)
                    for n in SET + (PAIR if f else ()):
                        if rec[n].tobytes() != want[f][j][n].tobytes():
                            print(f"{title}: camera {j} frame {f}: {n} of the record differs from the lock-step read: nothing is reported",
                                  file=sys.stderr)
                            os._exit(20)
            for k in range(NF):
                arm_a.hand_in(k)
                if k >= D - 1:
                    compare(k - D + 1)
            for f in range(max(NF - D + 1, 0), NF):
                compare(f)
            for k in range(NF):
                arm_c.hand_in(k)
            for j in range(arm_c.n):
                last = arm_c.read(j)
                for n in SET + PAIR:
                    if last[n].tobytes() != want[NF - 1][j][n].tobytes():
                        print(f"{title}: camera {j}: {n} of the loop that reads nothing differs: nothing is reported", file=sys.stderr)
                        os._exit(20)
            print(f"results ({title}): every record of (a) equals the lock-step arrays of (b) on all {NF} frames, and (c) ends where (b) does")

            def step_a(k):
                arm_a.hand_in(k)
                f = arm_a.handed - D
                if f >= 0:
                    for j in range(arm_a.n):
                        arm_a.fetch(j, f)

            def step_b(k):
                arm_b.hand_in(k)
                for j in range(arm_b.n):
                    arm_b.read(j)
        loops = {}
        for name, r in arms.items():
            r.hand_in(0)                                           # every arm starts again: frame numbers from 0
            loops[name] = (step_a if name.startswith("(a)") else step_b if name.startswith("(b)") else r.hand_in, r.sync)
        times = {name: [] for name in loops}
        for step, sync in loops.values():
            window(step, sync)                                     # warm-up
        for _ in range(a.windows):
            for name, (step, sync) in loops.items():
                times[name].append(window(step, sync))
        block = {}
        for name, v in times.items():
            block[name] = dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1))
            print(f"{title}: {name:58s} {block[name]['median']:8.1f} us ({block[name]['min']:.1f} - {block[name]['max']:.1f})")
        if not a.only_c:
            ka, kb = [n for n in block if n.startswith("(a)")][0], [n for n in block if n.startswith("(b)")][0]
            block["a_range_below_b_range"] = bool(block[ka]["max"] < block[kb]["min"])
        out[title] = block
        for r in arms.values():
            r.close()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    os._exit(0)


if __name__ == "__main__":
    sys.exit(main())
