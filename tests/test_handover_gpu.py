"""GPU tests of the device-side frame hand-over: pagk_post_filter_device against the host function, pagk_frame_handover
against the plain-C restatement (tests/frame_handover_ref.c), pagk_gyro_predict_device_live, runtime.SequenceTracker
against a host loop built from the older entry points, the codes with which the six pagk_frame_handover* forms refuse a
mistake, and examples/stream_graph_loop.cpp against stream_resident."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import handover_ref_util as hu
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, distributed, runtime, synth
from util import params_for

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 640, 480


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return hu.build_ref(tmp_path_factory.mktemp("handover_ref"))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _device_post_filter(ctx, half, st, pe, dp, pm, pmu, alias=False, fill=0.0):
    n = int(st.shape[0])
    nn = max(n, 1)
    d_st, d_pe, d_dp = _dev(np.resize(st, nn).astype(np.uint8)), _dev(np.resize(pe, nn)), _dev(np.resize(dp, nn))
    d_pm, d_pmu = _dev(np.resize(pm, (nn, 2)).astype(np.float32)), _dev(np.resize(pmu, (nn, 2)).astype(np.float32))
    d_out = d_st if alias else torch.full((nn,), 7, dtype=torch.uint8, device="cuda:0")
    d_pp = torch.full((nn, 2), fill, dtype=torch.float32, device="cuda:0")
    d_ppu = torch.full((nn, 2), fill, dtype=torch.float32, device="cuda:0")
    d_kept = torch.full((1,), -5, dtype=torch.int32, device="cuda:0")
    d_th = torch.zeros(2, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.post_filter_device(n, half, d_st, d_pe, d_dp, d_pm, d_pmu, d_out, d_pp, d_ppu, d_kept, d_th)
    ctx.sync()
    return dict(kept=int(d_kept.cpu()[0]), status=d_out.cpu().numpy()[:n], pt_predict=d_pp.cpu().numpy()[:n],
                pt_predict_un=d_ppu.cpu().numpy()[:n], thresholds=d_th.cpu().numpy())


def _check_post_filter(ctx, ref, half, st, pe, dp, pm, pmu, what, alias=False):
    got = _device_post_filter(ctx, half, st, pe, dp, pm, pmu, alias=alias)
    kept, mask, pp, ppu = capi.post_filter(half, st, pe, dp, pm, pmu)          # the host function
    r = hu.ref_post_filter(ref, half, st, pe, dp, pm, pmu)
    print(f"{what}: n = {st.shape[0]}, kept {got['kept']} (host {kept}), th_pix {got['thresholds'][0]!r} (restated {r['thresholds'][0]!r})")
    assert got["kept"] == kept == r["kept"], what
    assert np.array_equal(got["status"], mask), what
    assert got["pt_predict"].tobytes() == pp.tobytes() and got["pt_predict_un"].tobytes() == ppu.tobytes(), what
    assert got["thresholds"].tobytes() == r["thresholds"].tobytes(), what
    return got


@pytest.mark.parametrize("idx,n", [(1, 1000), (2, 2000), (3, 3000)])
def test_post_filter_device_on_real_outputs(ctx, ref, idx, n):
    w = synth.config(idx, n=n)
    p = params_for(w)
    o = ctx.track(p, w.img_ref, w.img_cur, w.pt_ref, w.pt_init, w.affine, w.status_in)
    a = [o[k][:w.n] for k in ("status", "pix_err", "dist_pred", "pt_dist", "pt_un")]
    got = _check_post_filter(ctx, ref, w.half_patch, *a, what=w.name)
    assert 0 < got["kept"] <= int(a[0].sum())
    _check_post_filter(ctx, ref, w.half_patch, *a, what=w.name + " (aliased status)", alias=True)


def _random_case(n, seed, p_true=0.8):
    rng = np.random.default_rng(seed)
    st = (rng.random(n) < p_true).astype(np.uint8)
    pe = (rng.random(n) * 10.0 ** rng.integers(-9, 2, n)).astype(np.float64)   # a sum that depends on its order
    dp = rng.random(n) * 30.0
    pm = rng.random((n, 2)).astype(np.float32) * 600
    return st, pe, dp, pm, (pm + np.float32(0.5)).astype(np.float32)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000, 20000])
def test_post_filter_device_sizes(ctx, ref, n):
    st, pe, dp, pm, pmu = _random_case(n, 100 + n)
    if n == 1:
        st[0] = 1
    _check_post_filter(ctx, ref, 5, st, pe, dp, pm, pmu, what=f"random n = {n}")
    _check_post_filter(ctx, ref, 10, st, pe * 0.01, dp, pm, pmu, what=f"random n = {n}, small errors, h = 10", alias=True)


def test_post_filter_device_all_false_and_nan(ctx, ref):
    st, pe, dp, pm, pmu = _random_case(3000, 7)
    got = _check_post_filter(ctx, ref, 5, np.zeros_like(st), pe, dp, pm, pmu, what="all status false")
    assert got["kept"] == 0 and got["thresholds"][0] == 5.0 and not got["status"].any()
    pe2 = pe.copy()
    pe2[np.flatnonzero(st)[11]] = np.nan
    got = _check_post_filter(ctx, ref, 5, st, pe2, dp, pm, pmu, what="one NaN pix_err")
    assert got["thresholds"][0] == 5.0
    pe3 = pe.copy()
    pe3[np.flatnonzero(st == 0)[3]] = np.nan     # a NaN behind a false status is not added
    got = _check_post_filter(ctx, ref, 5, st, pe3, dp, pm, pmu, what="NaN pix_err under a false status")
    assert np.isfinite(got["thresholds"][0])


def test_post_filter_device_leaves_other_entries_untouched(ctx, ref):
    st, pe, dp, pm, pmu = _random_case(2000, 9)
    got = _device_post_filter(ctx, 5, st, pe, dp, pm, pmu, fill=-777.0)
    init = np.full((2000, 2), -777.0, np.float32)
    r = hu.ref_post_filter(ref, 5, st, pe, dp, pm, pmu, pt_predict=init, pt_predict_un=init)
    assert got["pt_predict"].tobytes() == r["pt_predict"].tobytes() and got["pt_predict_un"].tobytes() == r["pt_predict_un"].tobytes()
    assert (got["pt_predict"][got["status"] == 0] == -777.0).all() and 0 < got["kept"] < 2000


# ---- hand-over -----------------------------------------------------------------------------------------------------
def _check_handover(ctx, ref, p, cap, target_n, thr, status, pp, ppu, cand, state=None, what=""):
    got = ctx.frame_handover(p, W, H, cap, target_n, thr, status, pp, ppu, cand, state=state)
    want = hu.ref_handover(ref, hu.camera_of(p), W, H, cap, target_n, thr, status, pp, ppu, cand, state=state)
    print(f"{what}: state {got['state'].tolist()} (restated {want['state'].tolist()})")
    assert hu.same_handover(got, want) == [], what
    return got


@pytest.mark.parametrize("k,n_surv", [(0, 300), (0, 400), (1, 300), (1, 400), (2, 300), (2, 400)])
def test_handover_on_the_superpoint_lists(ctx, ref, k, n_surv):
    lists = hu.seq_candidates()
    surv, cand = lists[k][:n_surv], lists[k + 1]
    p = capi.make_params(camera=synth.D435I)
    dist = (surv + np.float32([0.25, -0.5])).astype(np.float32)
    got = _check_handover(ctx, ref, p, 500, 500, 400.0, np.ones(n_surv, np.uint8), dist, surv, cand, what=f"lists {k}/{k + 1}, {n_surv} survivors")
    assert got["state"][2] == n_surv and got["state"][3] > 0 and 135 <= got["state"][4] <= 255


def test_handover_cases(ctx, ref):
    lists = hu.seq_candidates()
    p = capi.make_params(camera=synth.D435I)
    pd = capi.make_params(camera=synth.Camera(380.0, 381.0, 320.5, 239.5, (0.11, -0.05, 0.001, -0.002)))
    rng = np.random.default_rng(3)
    st = (rng.random(450) < 0.7).astype(np.uint8)
    un = np.stack([rng.random(450) * 640, rng.random(450) * 480], axis=1).astype(np.float32)
    ds = (un + rng.random((450, 2)).astype(np.float32)).astype(np.float32)
    none = np.zeros(0, np.uint8), np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32)
    # cap > target_n, status with holes, a distorting camera
    got = _check_handover(ctx, ref, pd, 1500, 400, 320.0, st, ds, un, lists[0], what="cap > target_n")
    assert got["state"][0] == 400 and got["state"][1] == 1 and got["state"][3] > 0
    assert np.abs(got["keys"][got["state"][2]:400] - got["keys_un"][got["state"][2]:400]).max() > 0.05
    # zero candidates
    got = _check_handover(ctx, ref, p, 450, 400, 320.0, st, ds, un, np.zeros((0, 2), np.float32), what="zero candidates")
    assert got["state"][3] == 0 and got["state"][4] == 0 and got["state"][1] == 0
    # total hits target_n exactly, with exactly as many acceptable candidates as are missing
    first = _check_handover(ctx, ref, p, 400, 400, 320.0, *none, lists[1], what="first frame")
    assert first["state"].tolist() == [400, 1, 0, 400, 0, 0, 0, 0]
    m = int(st[:400].sum())
    want = hu.ref_handover(ref, hu.camera_of(p), W, H, 400, 400, 320.0, st[:400], ds[:400], un[:400], lists[2])
    ok_idx = [j for j in range(500) if want["mask"][int(lists[2][j, 1]), int(lists[2][j, 0])]]
    exact = lists[2][:ok_idx[400 - m - 1] + 1]
    got = _check_handover(ctx, ref, p, 400, 400, 320.0, st[:400], ds[:400], un[:400], exact, what="total == target_n exactly")
    assert got["state"][0] == 400 and got["state"][1] == 1 and got["state"][3] == 400 - m
    # out-of-image candidates, the corners of the mask, flag persistence (no top-up with the flag up)
    bad = np.float32([[-1.0, 10.0], [640.0, 10.0], [10.0, 480.0], [10.0, -3.5], [np.nan, 5.0], [-0.5, -0.5], [639.9, 479.9]])
    got = _check_handover(ctx, ref, p, 420, 400, 320.0, *none, np.concatenate([bad, lists[3]]), what="out-of-image candidates")
    assert got["state"][4] == 5
    corners = np.float32([[0.4, 0.9], [639.6, 0.0], [0.0, 479.9], [639.9, 479.9]])
    got = _check_handover(ctx, ref, p, 16, 4, 3.2, np.ones(4, np.uint8), corners, corners, lists[0][:9], what="corners")
    assert int((got["mask"] == 0).sum()) == 4 * 196
    up = np.array([0, 1, 0, 0, 0, 0, 0, 0], np.int32)
    s350 = np.ones(350, np.uint8)
    got = _check_handover(ctx, ref, p, 400, 400, 320.0, s350, lists[1][:350], lists[1][:350], lists[2], state=up, what="flag up, above the threshold")
    assert got["state"][:4].tolist() == [350, 1, 350, 0] and got["state"][4] > 0
    got = _check_handover(ctx, ref, p, 400, 400, 320.0, s350, lists[1][:350], lists[1][:350], lists[2], what="flag down, above the threshold")
    assert got["state"][:4].tolist() == [400, 1, 350, 50]


def test_handover_device_is_capturable_and_checks_its_arguments(ref):
    c = capi.Context(0)
    stream = torch.cuda.Stream()
    try:
        p = capi.make_params(camera=synth.D435I)
        lists = hu.seq_candidates()
        cap = 512
        with torch.cuda.stream(stream):
            c.set_stream(stream.cuda_stream)
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda:0")  # noqa: E731
            d_st, d_pp, d_ppu = z(cap, torch.uint8), z((cap, 2), torch.float32), z((cap, 2), torch.float32)
            d_nc, d_cand = z(1, torch.int32), z((600, 2), torch.float32)
            outs = [z((cap, 2), torch.float32) for _ in range(3)]
            d_idx, d_live, d_state = z(cap, torch.int32), z(cap, torch.uint8), z(8, torch.int32)
            with pytest.raises(capi.PagkError):   # cap < target_n
                c._check(c.lib.pagk_frame_handover_device(c.h, p, W, H, 100, 400, 320.0, d_st.data_ptr(), d_pp.data_ptr(),
                                                          d_ppu.data_ptr(), 600, d_nc.data_ptr(), d_cand.data_ptr(),
                                                          outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                                          d_idx.data_ptr(), d_live.data_ptr(), None, d_state.data_ptr()), "cap")
            with pytest.raises(capi.PagkError):   # outputs alias the inputs
                c.frame_handover_device(p, W, H, cap, 400, 320.0, d_st, d_pp, d_ppu, 600, d_nc, d_cand, d_pp, d_ppu, outs[2],
                                        d_idx, d_live, None, d_state)

            def work():
                c.frame_handover_device(p, W, H, cap, 400, 320.0, d_st, d_pp, d_ppu, 600, d_nc, d_cand, outs[0], outs[1],
                                        outs[2], d_idx, d_live, None, d_state)
            work()                                   # sizes the context's mask
            stream.synchronize()
            c.graph_begin()
            try:
                with pytest.raises(capi.PagkError):  # the host-buffer form is not capturable
                    c.frame_handover(p, W, H, cap, 400, 320.0, np.zeros(1, np.uint8), np.zeros((1, 2)), np.zeros((1, 2)), lists[0])
                work()
            finally:
                gid = c.graph_end()
            state = np.zeros(8, np.int32)
            for k in range(3):                       # each replay reads that frame's inputs from device memory
                st = np.zeros(cap, np.uint8)
                st[:200 + 60 * k] = 1
                un = np.zeros((cap, 2), np.float32)
                un[:400] = lists[k][:400]
                d_st.copy_(_dev(st)), d_pp.copy_(_dev(un)), d_ppu.copy_(_dev(un))
                d_cand[:500].copy_(_dev(lists[k + 1])), d_nc.fill_(500)
                c.graph_launch(gid)
                stream.synchronize()
                want = hu.ref_handover(ref, hu.camera_of(p), W, H, cap, 400, 320.0, st, un, un, lists[k + 1], state=state)
                state = want["state"]
                assert np.array_equal(d_state.cpu().numpy(), state), k
                assert outs[1].cpu().numpy().tobytes() == want["keys_un"].tobytes() and outs[0].cpu().numpy().tobytes() == want["keys"].tobytes()
                assert outs[2].cpu().numpy().tobytes() == want["keys_normal"].tobytes()
                assert np.array_equal(d_idx.cpu().numpy(), want["index_in_last"]) and np.array_equal(d_live.cpu().numpy(), want["live"])
            c.graph_destroy(gid)
    finally:
        c.set_stream(None)
        c.close()


def test_host_api_wrappers(ctx, ref):
    from pixel_aware_gyro_aided_klt_feature_tracker_amd import host_api
    st, pe, dp, pm, pmu = _random_case(1500, 21)
    kept, mask, pp, ppu, th = host_api.post_filter_device(5, st, pe, dp, pm, pmu, ctx=ctx)
    want = capi.post_filter(5, st, pe, dp, pm, pmu)
    r = hu.ref_post_filter(ref, 5, st, pe, dp, pm, pmu)
    assert kept == want[0] and np.array_equal(mask, want[1]) and pp.tobytes() == want[2].tobytes() and ppu.tobytes() == want[3].tobytes()
    assert (th[0], th[1]) == (r["thresholds"][0], r["thresholds"][1])
    with pytest.raises(ValueError):
        host_api.post_filter_device(5, st, pe[:-1], dp, pm, pmu, ctx=ctx)
    lists = hu.seq_candidates()
    p = capi.make_params(camera=synth.D435I)
    got = host_api.frame_handover(p, W, H, 400, 400, 320.0, np.ones(300, np.uint8), lists[0][:300], lists[0][:300], lists[1], ctx=ctx)
    want = hu.ref_handover(ref, hu.camera_of(p), W, H, 400, 400, 320.0, np.ones(300, np.uint8), lists[0][:300], lists[0][:300], lists[1])
    assert hu.same_handover(got, want) == []


# ---- prediction with a live mask -----------------------------------------------------------------------------------
def test_predict_live(ctx, ref):
    w = synth.config(1, n=1000, edge_fraction=0.1)
    p = params_for(w)
    n = w.n
    K32 = synth.EUROC.K.astype(np.float32)
    R32 = synth.rodrigues(np.array((0.5, -1.0, 2.0)) * 0.05).astype(np.float32)
    Kinv32 = np.linalg.inv(K32.astype(np.float64)).astype(np.float32)
    KRK = ((K32.astype(np.float64) @ R32.astype(np.float64)).astype(np.float32).astype(np.float64) @ Kinv32.astype(np.float64)).astype(np.float32)
    d_rot = _dev(np.concatenate([KRK.reshape(-1)[:6], R32[2]]).astype(np.float32))
    d_ref = _dev(w.pt_ref)

    def run(live):
        pu, pd = torch.full((n, 2), -3.0, device="cuda:0"), torch.full((n, 2), -3.0, device="cuda:0")
        st, A = torch.full((n,), 9, dtype=torch.uint8, device="cuda:0"), torch.full((n, 4), -5.0, device="cuda:0")
        torch.cuda.synchronize()
        if live is None:
            ctx.gyro_predict_device_rot(p, w.img_ref.shape[1], w.img_ref.shape[0], d_rot, n, d_ref, pu, pd, st, A)
        else:
            ctx.gyro_predict_device_live(p, w.img_ref.shape[1], w.img_ref.shape[0], d_rot, n, d_ref, _dev(live), pu, pd, st, A)
        ctx.sync()
        return [t.cpu().numpy() for t in (pu, pd, st, A)]
    base = run(None)
    assert 0 < base[2].sum() < n or base[2].all()
    ones = run(np.ones(n, np.uint8))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(base, ones))
    live = (np.random.default_rng(1).random(n) < 0.6).astype(np.uint8)
    got = run(live)
    want = [a.copy() for a in base]
    ref.fhr_predict_live(n, live.ctypes.data, want[0].ctypes.data, want[1].ctypes.data, want[2].ctypes.data)
    want[3][live == 0] = -5.0     # affine untouched
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
    dead = live == 0
    assert not got[2][dead].any() and not got[0][dead].any() and not got[1][dead].any() and (got[3][dead] == -5.0).all()
    assert got[2][~dead].sum() == base[2][~dead].sum() > 0


# ---- a sequence ----------------------------------------------------------------------------------------------------
NF, CAP, TARGET, RATIO = 9, 448, 400, 0.8


def _host_loop(ctx, ref, p, fitp, cam, imgs, Rs, KRKs, cands):
    """The same frames through entry points that existed before the hand-over (pagk_gyro_predict_device,
    pagk_track_device, the host pagk_post_filter, pagk_geometry_validation_fit) plus the restated hand-over."""
    rcam = hu.camera_of(p)
    none = np.zeros(0, np.uint8), np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32)
    state = np.zeros(8, np.int32)
    frames = [hu.ref_handover(ref, rcam, W, H, CAP, TARGET, TARGET * RATIO, *none, cands[0], state=state)]
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
        frames.append(hu.ref_handover(ref, rcam, W, H, CAP, TARGET, TARGET * RATIO, st2, pp, ppu, cands[k], state=prev["state"]))
        frames[-1]["kept"], frames[-1]["validated"] = kept, int(st2.sum())
    return frames


def test_sequence_tracker_against_a_host_loop(ctx, ref):
    cam, imgs, Rs, KRKs, rot9, _ = hu.rotating_sequence(synth, NF, W, H, 0x5EED0A10, (0.035, -0.045, 0.03))
    lists = hu.seq_candidates()
    cands = [lists[k % 4] for k in range(NF)]
    p = capi.make_params(half_patch=5, iterations=10, pyramids=3, has_gyro=True, camera=cam)
    fitp = capi.fit_params_default(seed=0x5EED0F17, iters_H=512, iters_F=256)
    want = _host_loop(ctx, ref, p, fitp, cam, imgs, Rs, KRKs, cands)
    states = np.array([f["state"] for f in want])
    print("host loop, state words per frame [total, reach, survivors, added, rejected]:")
    for k, f in enumerate(want):
        print(f"  frame {k}: {f['state'][:5].tolist()} kept {f.get('kept')} validated {f.get('validated')}")
    # the sequence must exercise what it is here for
    assert any(states[k, 2] < states[k - 1, 0] for k in range(1, NF)), "no frame loses features"
    assert (states[1:, 3] > 0).any(), "no frame triggers the top-up"
    assert (states[1:, 4] > 0).any(), "no candidate is rejected by the mask"
    assert (states[1:, 0] == TARGET).any(), "no frame has total == target_n"
    assert (states[1:, 3] == 0).any(), "every frame tops up: the threshold rule is not exercised"

    results = {}
    for mode in ("graph", "direct"):
        sq = runtime.SequenceTracker(p, W, H, CAP, TARGET, RATIO, fitp)
        try:
            res = [sq.start(imgs[0], cands[0])]
            used = ["direct"]
            for k in range(1, NF):               # nothing is synchronised or read back inside this loop
                res.append(sq.step(imgs[k], rot9[k - 1], cands[k], mode=mode))
                used.append(sq.mode_used)
            got = [r.to_numpy() for r in res]
            sq.synchronize()
        finally:
            sq.close()
        if mode == "graph":
            assert used[1:3] == ["direct", "direct"] and all(u == "graph" for u in used[3:]), used
        else:
            assert all(u == "direct" for u in used)
        results[mode] = got
        for k in range(NF):
            g, wnt = got[k], want[k]
            print(f"{mode} frame {k}: state {g['state'][:5].tolist()}")
            assert np.array_equal(g["state"], wnt["state"]), (mode, k, g["state"], wnt["state"])
            for name in ("keys", "keys_un", "keys_normal", "index_in_last", "live"):
                assert g[name].tobytes() == np.asarray(wnt[name]).tobytes(), (mode, k, name)
            assert int(g["live"].sum()) == g["total"] == int(wnt["state"][0])
    for k in range(NF):
        for name in runtime.FrameResult.FIELDS:
            assert results["graph"][k][name].tobytes() == results["direct"][k][name].tobytes(), (k, name)


# ---- refusals ------------------------------------------------------------------------------------------------------
# What each of the six entry points returns for which mistake, and which code wins when two mistakes meet.  Every row is
# refused on the host, in front of the hand-over's first launch; the calls go to the C functions, because capi.Context
# raises ValueError on its own for some of them.
RW, RH, RCAP, RTARGET = 97, 80, 16, 8
R_ALL = ("given_dev", "given_host", "detect_dev", "detect_host", "fast_dev", "fast_host")
R_DEV, R_HOST = R_ALL[0::2], R_ALL[1::2]
R_GIVEN, R_DETECT, R_FAST = R_ALL[0:2], R_ALL[2:4], R_ALL[4:6]
R_NAMES = dict(given_dev="pagk_frame_handover_device", given_host="pagk_frame_handover",
               detect_dev="pagk_frame_handover_detect_device", detect_host="pagk_frame_handover_detect",
               fast_dev="pagk_frame_handover_fast_device", fast_host="pagk_frame_handover_fast")


def _refusal_rows(img61):
    """(mistake, forms, overrides of the valid call's arguments, code)"""
    A, U, nan = capi.PAGK_E_ARG, capi.PAGK_E_UNSUPPORTED, float("nan")
    fast8 = capi.fast_params_default(n_levels=8)
    low = dict(height=61, slot=0, img=img61, mask=None)   # (slot 0 and img61 are 97 x 61: too low for the FAST cell grid)
    rows = [("cap < target_n", R_ALL, dict(cap=RTARGET - 1), A),
            ("width 13", R_ALL, dict(width=13), A),
            ("height 13", R_ALL, dict(height=13), A),
            ("NaN threshold", R_ALL, dict(thr=nan), A),
            ("params NULL", R_ALL, dict(params=None), A),
            ("cand_cap > 0 with a NULL list", R_GIVEN, dict(cand_un=None), A),
            ("cand_cap < 0", R_GIVEN, dict(cand_cap=-1), A),
            ("n_cand NULL", R_GIVEN, dict(n_cand=None), A)]
    rows += [(name + " NULL", R_ALL, {name: None}, A)
             for name in ("status", "pt_predict", "pt_predict_un", "keys", "keys_un", "index_in_last", "live", "state")]
    rows += [("info NULL", ("detect_dev", "fast_dev"), dict(info=None), A),
             ("img NULL", ("detect_host", "fast_host"), dict(img=None), A),
             ("img of another size", ("detect_host", "fast_host"), dict(img=img61), A),
             ("keys == pt_predict", R_DEV, dict(keys="pt_predict"), A),
             ("keys_un == pt_predict_un", R_DEV, dict(keys_un="pt_predict_un"), A),
             ("slot -1", ("detect_dev", "fast_dev"), dict(slot=-1), A),
             ("slot 4", ("detect_dev", "fast_dev"), dict(slot=4), A),
             ("empty slot", ("detect_dev", "fast_dev"), dict(slot=2), A),
             ("slot of another size", ("detect_dev", "fast_dev"), dict(slot=0), A),
             ("det NULL", R_DETECT, dict(detect=None), A),
             ("quality_level NaN", R_DETECT, dict(detect=capi.detect_params_default(quality_level=nan)), A),
             ("fast NULL", R_FAST, dict(fast=None), A),
             ("ini_threshold 256", R_FAST, dict(fast=capi.fast_params_default(ini_threshold=256)), A),
             ("n_levels 8", R_FAST, dict(fast=fast8), U),
             ("61-pixel-high frame", R_FAST, low, A),
             ("n_features 0 with target_n 0", R_FAST, dict(target_n=0), A),
             # two at once: the parameter block is looked at after the geometry and the slot's range, before the rest
             ("n_levels 8 and a NaN threshold", R_FAST, dict(fast=fast8, thr=nan), A),
             ("n_levels 8 and slot -1", ("fast_dev",), dict(fast=fast8, slot=-1), A),
             ("n_levels 8 and keys NULL", R_FAST, dict(fast=fast8, keys=None), U),
             ("n_levels 8 and keys == pt_predict", ("fast_dev",), dict(fast=fast8, keys="pt_predict"), U),
             ("n_levels 8 and an empty slot", ("fast_dev",), dict(fast=fast8, slot=2), U),
             ("n_levels 8 and a 61-pixel-high frame", R_FAST, dict(low, fast=fast8), U)]
    return rows


def _refusal_args(form, img):
    """The arguments of a valid call: device tensors for the device forms, numpy arrays for the host forms."""
    if form in R_HOST:
        z, u8, f32, i32 = np.zeros, np.uint8, np.float32, np.int32
    else:
        z, u8, f32, i32 = (lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda:0")), torch.uint8, torch.float32, torch.int32
    return dict(params=capi.make_params(camera=synth.D435I), width=RW, height=RH, cap=RCAP, target_n=RTARGET, thr=6.0,
                status=z(RCAP, u8), pt_predict=z((RCAP, 2), f32), pt_predict_un=z((RCAP, 2), f32), cand_cap=4,
                n_cand=z(1, i32), cand_un=z((4, 2), f32), detect=capi.detect_params_default(), fast=capi.fast_params_default(),
                slot=1, img=img, keys=z((RCAP, 2), f32), keys_un=z((RCAP, 2), f32), keys_normal=z((RCAP, 2), f32),
                index_in_last=z(RCAP, i32), live=z(RCAP, u8), mask=z((RH, RW), u8), state=z(8, i32), info=z(8, i32))


def _refusal_call(c, form, a):
    import ctypes as C
    ptr = lambda k: capi._ptr(a[k])                          # noqa: E731
    ref = lambda s: None if s is None else C.byref(s)        # noqa: E731
    head = [c.h, ref(a["params"]), a["width"], a["height"], a["cap"], a["target_n"], a["thr"], ptr("status"), ptr("pt_predict"),
            ptr("pt_predict_un")]
    tail = [ptr(k) for k in ("keys", "keys_un", "keys_normal", "index_in_last", "live", "mask", "state")]
    fn = getattr(c.lib, R_NAMES[form])
    if form in R_GIVEN:
        return fn(*head, a["cand_cap"], ptr("n_cand"), ptr("cand_un"), *tail)
    frame = a["slot"] if form in R_DEV else None if a["img"] is None else C.byref(capi.image_view(a["img"]))
    return fn(*head, ref(a["detect" if form in R_DETECT else "fast"]), frame, *tail, ptr("info"))


def test_handover_refusals(built):
    rng = np.random.default_rng(97)
    img, img61 = rng.integers(0, 256, (RH, RW), dtype=np.uint8), rng.integers(0, 256, (61, RW), dtype=np.uint8)
    c = capi.Context(0)
    stream = torch.cuda.Stream()
    bad = []

    def expect(what, form, over, code):
        a = base[form]
        a = dict(a, **{k: a[v] if isinstance(v, str) else v for k, v in over.items()})
        got = _refusal_call(c, form, a)
        print(f"{what} | {form} | {got}")
        if got != code:
            bad.append((what, form, got, code))
        return got

    try:
        with torch.cuda.stream(stream):
            c.set_stream(stream.cuda_stream)
            c.frame_upload(0, img61, 1)
            c.frame_upload(1, img, 1)                          # (slot 2 stays empty)
            base = {form: _refusal_args(form, img) for form in R_ALL}
            torch.cuda.synchronize()
            for form in R_ALL:                                 # the arguments that the rows spoil are good ones
                expect("a valid call", form, {}, capi.PAGK_OK)
            c.sync()
            for what, forms, over, code in _refusal_rows(img61):
                for form in forms:
                    expect(what, form, over, code)
            c.graph_begin()
            try:
                for form in R_HOST:
                    if expect("under capture", form, {}, capi.PAGK_E_ARG) == capi.PAGK_E_ARG:
                        text = c.lib.pagk_last_error(c.h).decode()
                        print(f"    {text}")
                        if not text.startswith(R_NAMES[form] + " is not capturable"):
                            bad.append(("under capture: the message", form, text, R_NAMES[form]))
                expect("under capture: n_levels 8", "fast_host", dict(fast=capi.fast_params_default(n_levels=8)),
                       capi.PAGK_E_UNSUPPORTED)
                expect("under capture: width 13", "given_host", dict(width=13), capi.PAGK_E_ARG)
                for form in R_DEV:                             # (sized by the valid calls above)
                    expect("under capture: a valid call", form, {}, capi.PAGK_OK)
            finally:
                c.graph_destroy(c.graph_end())
            c.sync()
    finally:
        c.set_stream(None)
        c.close()
    assert bad == [], "(mistake, form, returned, expected): " + repr(bad)


# ---- examples ------------------------------------------------------------------------------------------------------
def test_stream_graph_loop_prints_what_stream_resident_prints(built, tmp_path):
    pkg = capi.PKG_DIR
    exes = {}
    for name in ("stream_resident", "stream_graph_loop"):
        exes[name] = str(tmp_path / name)
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I",
                        os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", name + ".cpp"), "-o", exes[name],
                        "-L", pkg, "-l:libpagk_hip.so", "-L", "/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{pkg}",
                        "-Wl,-rpath,/opt/rocm/lib"], check=True)
    # the input of the C++ demo-loop test: 5 frames of 320x240, 150 keypoints
    Wd, Hd, NFd, NK = 320, 240, 5, 150
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
    outs = {}
    for name, exe in exes.items():
        r = subprocess.run([exe, path, "5", "10", "3"], capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, (name, r.returncode, r.stdout, r.stderr)
        outs[name] = r.stdout.strip().splitlines()
    print("\n".join(outs["stream_graph_loop"]))
    assert len(outs["stream_resident"]) == NFd and outs["stream_resident"][-1].startswith("survivors")
    assert int(outs["stream_resident"][-1].split()[1]) > 0.7 * NK
    assert outs["stream_graph_loop"] == outs["stream_resident"]
