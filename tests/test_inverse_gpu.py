"""GPU tests of the template-Jacobian mode (include/pagk.h, pagk_params::inverse == PAGK_INVERSE_TEMPLATE): every entry point
against the plain-C restatement (tests/inverse_ref.c), bit for bit on every output of every feature -- pt_un, pt_dist, status,
pix_err, dist_pred, ncc, iters.  The restatement itself is held to the definition, the truth and the forward oracle by
tests/test_inverse_cpu.py; this file adds no tolerance."""
import numpy as np
import pytest
import torch

import handover_ref_util as hu
import inverse_ref_util as iu
import shape_cases as sc
from oracle import pagk_oracle as orc
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, distributed, runtime, synth
from route_runner import device_inputs, outputs
from util import assert_parity, params_for

pytestmark = pytest.mark.gpu

SHAPE2 = (96, 64, 2)
VARIANT = 8


def _track(c, p, w, **over):
    a = dict(img_ref=w.img_ref, img_cur=w.img_cur, pt_ref=w.pt_ref, pt_init=w.pt_init, affine=w.affine, status_in=w.status_in)
    a.update(over)
    got = c.track(p, a["img_ref"], a["img_cur"], a["pt_ref"], a["pt_init"], a["affine"], a["status_in"])
    ref = iu.track(p, a["img_ref"], a["img_cur"], a["pt_ref"], a["pt_init"], a["affine"], a["status_in"])
    return got, ref, int(a["pt_ref"].shape[0])


# ---- the shape matrix ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", iu.HALVES)
@pytest.mark.parametrize("shape", sc.SHAPES, ids=sc.shape_id)
def test_shape_matrix(ctx, shape, h):
    w = sc.workload(shape, h)
    for mode in sc.MODES:
        what = f"{sc.shape_id(shape)} h={h} {mode}"
        got = ctx.track(iu.shape_params(w, mode), w.img_ref, w.img_cur, w.pt_ref, w.pt_init, w.affine, w.status_in)
        assert ctx.last_variant() == VARIANT, what
        iu.assert_same(got, iu.restated(shape, h, mode), w.n, what)
        ctx.check_launch()


# ---- parameters and inputs at 96 x 64 with two levels -------------------------------------------------------------------------
def _five_coefficients(p):
    p.fx, p.fy, p.cx, p.cy = 80.0, 82.0, 47.5, 31.5
    for k, v in enumerate((-0.28, 0.07, 0.0012, -0.0008, 0.013)):
        p.dist_coef[k] = v
    p.n_dist_coef = 5


PARAM_CASES = {
    "illumination off": lambda p: setattr(p, "consider_illumination", 0),
    "affine off": lambda p: setattr(p, "consider_affine", 0),
    "no initial prediction": lambda p: setattr(p, "has_gyro_predict_initial", 0),
    "ncc": lambda p: setattr(p, "calculate_ncc", 1),
    "five distortion coefficients": _five_coefficients,
    "iterations 0": lambda p: setattr(p, "iterations", 0),
    "iterations 1": lambda p: setattr(p, "iterations", 1),
    "everything": lambda p: (setattr(p, "calculate_ncc", 1), _five_coefficients(p), setattr(p, "has_gyro_predict_initial", 0)),
}


@pytest.mark.parametrize("h", (5, 10))
@pytest.mark.parametrize("case", sorted(PARAM_CASES))
def test_parameters(ctx, case, h):
    w = sc.workload(SHAPE2, h)     # edge_fraction 0.3: patches with clamped taps
    for mode in sc.MODES:
        p = iu.shape_params(w, mode)
        PARAM_CASES[case](p)
        got, ref, n = _track(ctx, p, w)
        assert ctx.last_variant() == VARIANT
        iu.assert_same(got, ref, n, f"{case} h={h} {mode}")
        if case == "ncc":
            assert (ref["ncc"][:n][ref["status"][:n] > 0] != 1).any()
        if case == "five distortion coefficients":
            assert (ref["pt_dist"][:n] != ref["pt_un"][:n]).any()


@pytest.mark.parametrize("h", (5, 10))
def test_inputs(ctx, h):
    w = sc.workload(SHAPE2, h)
    p = iu.shape_params(w, "lean")
    # some status_in zero (more than the workload's own)
    status = w.status_in.copy()
    status[::3] = 0
    got, ref, n = _track(ctx, p, w, status_in=status)
    iu.assert_same(got, ref, n, f"status_in h={h}")
    assert (got["status"][:n][::3] == 0).all() and (got["iters"][:n][::3] == 0).all()
    # the flat rectangles: the NaN exit
    a, b, pt_ref, pt_init, st, idx = iu.flat_pair(w, h, w.pyramids)
    for iterations in (0, 1, 2, 20):
        p.iterations = iterations
        got, ref, n = _track(ctx, p, w, img_ref=a, img_cur=b, pt_ref=pt_ref, pt_init=pt_init, status_in=st)
        iu.assert_same(got, ref, n, f"flat rectangles h={h} iterations={iterations}")
        assert (got["status"][idx] == (1 if iterations == 0 else 0)).all()
    # n = 0, 1 and 67
    p = iu.shape_params(w, "both")
    before = iu.restated(SHAPE2, h, "both")
    for n in (0, 1, w.n):
        c = np.ascontiguousarray
        got = ctx.track(p, w.img_ref, w.img_cur, c(w.pt_ref[:n]), c(w.pt_init[:n]), c(w.affine[:n]), c(w.status_in[:n]))
        iu.assert_same(got, {k: before[k][:max(n, 1)] for k in iu.KEYS}, n, f"n={n} h={h}")
    ctx.check_launch()


# ---- entry points ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", (5, 10))
def test_entry_points(built, h):
    assert capi.has_variant(VARIANT)
    w = sc.workload(SHAPE2, h)
    stream, dev = torch.cuda.Stream(), torch.device("cuda", 0)
    c = capi.Context(0)
    try:
        for mode in sc.MODES:
            p = iu.shape_params(w, mode)
            ref = iu.restated(SHAPE2, h, mode)
            # pagk_track with every forcing selector in force: none applies
            for selector in (0, 1, 3, 5, 7):
                c.set_kernel(selector)
                try:
                    got = c.track(p, w.img_ref, w.img_cur, w.pt_ref, w.pt_init, w.affine, w.status_in)
                finally:
                    c.set_kernel(0)
                assert c.last_variant() == VARIANT and c.last_handover() == 0, (mode, selector)
                iu.assert_same(got, ref, w.n, f"track, pagk_set_kernel({selector}), {mode}")
            # pagk_track_pyr
            lv_r, lv_c = [w.img_ref], [w.img_cur]
            for _ in range(w.pyramids - 1):
                lv_r.append(orc.pyr_down(lv_r[-1]))
                lv_c.append(orc.pyr_down(lv_c[-1]))
            got = c.track_pyr(p, lv_r, lv_c, w.pt_ref, w.pt_init, w.affine, w.status_in)
            assert c.last_variant() == VARIANT
            iu.assert_same(got, ref, w.n, f"track_pyr {mode}")
        with torch.cuda.stream(stream):
            c.set_stream(stream.cuda_stream)
            c.frame_upload(0, w.img_ref, w.pyramids)
            c.frame_upload(1, w.img_cur, w.pyramids)
            d = device_inputs(w, dev)
            for mode in sc.MODES:
                p = iu.shape_params(w, mode)
                ref = iu.restated(SHAPE2, h, mode)
                # pagk_track_device
                out = distributed.alloc_device_outputs(w.n, dev)
                c.track_device(p, 0, 1, w.n, d[0], d[1], d[2], d[3], out)
                stream.synchronize()
                assert c.last_variant() == VARIANT
                iu.assert_same(outputs(out), ref, w.n, f"track_device {mode}")
                # a captured graph, replayed twice on changed inputs
                c.graph_begin()
                try:
                    c.track_device(p, 0, 1, w.n, d[0], d[1], d[2], d[3], out)
                finally:
                    gid = c.graph_end()
                perm = np.random.default_rng(7).permutation(w.n)
                for k, order in enumerate((perm, np.arange(w.n)[::-1].copy())):
                    src = [np.ascontiguousarray(x[order]) for x in (w.pt_ref, w.pt_init, w.affine, w.status_in)]
                    for t, x in zip(d, src):
                        t.copy_(torch.from_numpy(x).to(dev))
                    out["_buf"].zero_()
                    stream.synchronize()
                    c.graph_launch(gid)
                    stream.synchronize()
                    want = {name: np.ascontiguousarray(ref[name][:w.n][order]) for name in iu.KEYS}
                    iu.assert_same(outputs(out), want, w.n, f"graph replay {k} {mode}")
                c.graph_destroy(gid)
                for t, x in zip(d, (w.pt_ref, w.pt_init, w.affine, w.status_in)):
                    t.copy_(torch.from_numpy(x.copy()).to(dev))
                # pagk_track_device_fused: tracking and the next frame's pyramid, as two launches
                nxt = np.random.default_rng(0x1A7E + h).integers(0, 256, w.img_ref.shape, dtype=np.uint8)
                d_next = torch.from_numpy(nxt).to(dev)
                out = distributed.alloc_device_outputs(w.n, dev)
                height, width = w.img_ref.shape
                c.track_device_fused(p, 0, 1, w.n, d[0], d[1], d[2], d[3], out, 2, d_next.data_ptr(), width, height, width,
                                     w.pyramids)
                stream.synchronize()
                assert c.last_variant() == VARIANT
                iu.assert_same(outputs(out), ref, w.n, f"track_device_fused {mode}")
                lvl = nxt
                for l in range(1, w.pyramids):
                    lvl = orc.pyr_down(lvl)
                    assert np.array_equal(c.frame_download_level(2, l, width, height), lvl), f"fused: next-frame level {l}"
                out = distributed.alloc_device_outputs(w.n, dev)
                c.track_device(p, 1, 2, w.n, d[0], d[1], d[2], d[3], out)
                stream.synchronize()
                want = iu.track(p, w.img_cur, nxt, w.pt_ref, w.pt_init, w.affine, w.status_in)
                iu.assert_same(outputs(out), want, w.n, f"pair (cur, next) on the fused-built slot {mode}")
            c.check_launch()
    finally:
        c.set_stream(None)
        c.close()


@pytest.mark.parametrize("h", (5, 10))
def test_batch_runs_as_k_launches(built, h):
    ws = sc.batch_workloads(SHAPE2, h)     # streams of 1, 67 and 30 features on three frame sizes
    assert tuple(w.n for w in ws) == (1, 67, 30)
    stream, dev = torch.cuda.Stream(), torch.device("cuda", 0)
    ctxs = []
    try:
        with torch.cuda.stream(stream):
            for w in ws:
                c = capi.Context(0)
                ctxs.append(c)
                c.set_stream(stream.cuda_stream)
                c.frame_upload(0, w.img_ref, w.pyramids)
                c.frame_upload(1, w.img_cur, w.pyramids)
            d = [device_inputs(w, dev) for w in ws]
            for selector in (0, 7):          # a forced batch kernel does not apply either
                ctxs[0].set_kernel(selector)
                for mode in sc.MODES:
                    p = iu.shape_params(ws[0], mode)
                    outs = [distributed.alloc_device_outputs(w.n, dev) for w in ws]
                    capi.Context.track_device_batch(ctxs, p, [0] * 3, [1] * 3, [w.n for w in ws], [x[0] for x in d],
                                                    [x[1] for x in d], [x[2] for x in d], [x[3] for x in d], outs)
                    stream.synchronize()
                    for j, (w, out) in enumerate(zip(ws, outs)):
                        what = f"batch stream {j} ({w.n} features) {mode}, selector {selector}"
                        assert ctxs[j].last_variant() == VARIANT, what
                        iu.assert_same(outputs(out), iu.track_workload(w, p), w.n, what)
                        ctxs[j].check_launch()
    finally:
        for c in ctxs:
            c.set_stream(None)
            c.close()


# ---- determinism, and the forward path beside it ------------------------------------------------------------------------------
def test_two_runs_and_the_forward_path_around_them(built):
    w = sc.workload(SHAPE2, 10)
    fwd_p, inv_p = sc.params(w, "lean"), iu.shape_params(w, "lean")
    fwd_ref = sc.oracle(SHAPE2, 10, "lean")
    c = capi.Context(0)
    try:
        args = (w.img_ref, w.img_cur, w.pt_ref, w.pt_init, w.affine, w.status_in)
        assert_parity(c.track(fwd_p, *args), fwd_ref, w.n, exact=True, what="forward launch before")
        assert c.last_variant() == 0
        a = c.track(inv_p, *args)
        b = c.track(inv_p, *args)
        assert c.last_variant() == VARIANT
        iu.assert_same(a, b, w.n, "two runs")
        iu.assert_same(a, iu.restated(SHAPE2, 10, "lean"), w.n, "first run")
        assert_parity(c.track(fwd_p, *args), fwd_ref, w.n, exact=True, what="forward launch after")
        assert c.last_variant() == 0
        # the refused values are still refused, through a live context
        for bad in (1, 3):
            with pytest.raises(capi.PagkError) as e:
                c.track(capi.make_params(half_patch=10, iterations=20, pyramids=2, inverse=bad), *args)
            assert e.value.code == capi.PAGK_E_UNSUPPORTED
    finally:
        c.close()


# ---- runtime ------------------------------------------------------------------------------------------------------------------
def test_resident_tracker(built):
    w = sc.workload(SHAPE2, 10)
    p = iu.shape_params(w, "lean")
    ref = iu.restated(SHAPE2, 10, "lean")
    rt = runtime.ResidentTracker(p, device=0)
    try:
        rt.load_pair(w.img_ref, w.img_cur)
        rt.set_features(w.pt_ref, w.pt_init, w.affine, w.status_in)
        for mode in ("serial", "graph", "graph"):
            out = rt.step(mode=mode)
            rt.synchronize()
            assert rt.mode_used == mode and rt.ctx.last_variant() == VARIANT
            iu.assert_same(distributed.to_numpy(out), ref, w.n, f"ResidentTracker {mode}")
    finally:
        rt.close()


def test_sequence_tracker_graph_equals_direct(built):
    W, H, NF, CAP, TARGET, RATIO = 96, 64, 4, 96, 64, 0.8
    cam, imgs, Rs, KRKs, rot9, _ = hu.rotating_sequence(synth, NF, W, H, 0x5EED0A12, (0.01, -0.012, 0.02))
    lists = hu.seq_candidates()
    # the candidate lists (640 x 480) scaled into the frame
    cands = [np.ascontiguousarray(lists[k % 4] * np.float32([W / 640.0, H / 480.0])) for k in range(NF)]
    p = capi.make_params(half_patch=5, iterations=10, pyramids=2, has_gyro=True, camera=cam, inverse=capi.PAGK_INVERSE_TEMPLATE)
    fitp = capi.fit_params_default(seed=0x5EED0F17, iters_H=128, iters_F=64)
    results = {}
    for mode in ("graph", "direct"):
        sq = runtime.SequenceTracker(p, W, H, CAP, TARGET, RATIO, fitp)
        try:
            res = [sq.start(imgs[0], cands[0])]
            used = ["direct"]
            for k in range(1, NF):
                res.append(sq.step(imgs[k], rot9[k - 1], cands[k], mode=mode))
                used.append(sq.mode_used)
            got = [r.to_numpy() for r in res]
            sq.synchronize()
            assert sq.ctx.last_variant() == VARIANT
        finally:
            sq.close()
        if mode == "graph":
            assert used[-1] == "graph", used
        else:
            assert all(u == "direct" for u in used)
        results[mode] = got
    for k in range(NF):
        for name in runtime.FrameResult.FIELDS:
            assert results["graph"][k][name].tobytes() == results["direct"][k][name].tobytes(), (k, name)
    totals = [int(r["total"]) for r in results["graph"]]
    print("features per frame:", totals)
    assert totals[0] > 0 and totals[-1] > 0
    assert any(int(r["state"][2]) > 0 for r in results["graph"][1:]), "no frame carries a tracked feature over"


# ---- the example --------------------------------------------------------------------------------------------------------------
def test_stream_graph_loop_takes_the_flag(built, tmp_path):
    """examples/stream_graph_loop.cpp --inverse: the per-frame loop of the C ABI in this mode keeps its features."""
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
    Wd, Hd, NFd, NK = 320, 240, 4, 150
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
    lines = {}
    for flags in ((), ("--inverse",)):
        r = subprocess.run([exe, *flags, path, "5", "10", "3"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (flags, r.returncode, r.stdout, r.stderr)
        lines[flags] = r.stdout.strip().splitlines()
    inv = lines[("--inverse",)]
    print("\n".join(inv))
    assert len(inv) == NFd and inv[-1].startswith("survivors") and int(inv[-1].split()[1]) > 0.7 * NK
    assert inv != lines[()]          # (the mode's own results: the checksums differ from the forward loop's)
