"""The device stages of the frame loop against the reference's OWN tracker text, compiled: every fixture of
tests/golden/ref_shim/tracker/ -- outputs of src/gyro_aided_tracker.cpp, compiled unchanged under its own header against the
project's stand-ins (oracle/ref_shim, tests/test_reference_tracker_cpu.py) -- goes through the device entry point of its stage,
and through the host form where there is one:

    pagk_gyro_integrate                                   Rcl and rot9 of every window
    pagk_gyro_predict_device / _device_rot                both methods, fed the fixture's rotation
    pagk_track, then pagk_post_filter / _post_filter_device
    pagk_geometry_scores(_device) with pagk_geometry_select, and pagk_geometry_validation
    pagk_find_near_neighbors / pagk_near_neighbors_device the lists in the reference's order, level 2 only where it ran
    pagk_match_features / pagk_match_features_device
    pagk_search_gyro_predict                              lists, matches and flow errors end to end

Every compared output is bit-identical to the compiled reference's, NaN positions included, and pagk_check_launch is clean
afterwards.  The tests read the committed fixtures only: neither the reference nor oracle/_ref.

Rows left out where the library defines what the reference leaves undefined ("Defined behaviour" of oracle/README.md): none.  The
case table keeps the compiled reference inside the image buffers of its stand-in cv::Mat, whose slack holds the zeros the library
defines, and free of NaN coordinates (checked on the CPU under AddressSanitizer, tests/test_reference_tracker_cpu.py).

Not compared: pagk_search_klt with the fixture's Lucas-Kanade result.  The entry point runs Lucas-Kanade itself and its ABI takes no
point, status or error input, so the `klt` fixture reaches the device only through pagk_gyro_integrate; the steps after
Lucas-Kanade are held to the compiled reference on the CPU (tests/associate_ref.c, which tests/test_associate_gpu.py holds
pagk_search_klt_device to).  The third row of mKRKinv and mvvFlowsPredictCorners are no outputs of the library."""
import numpy as np
import pytest

import reference_cases as rc
import reference_tracker_util as tu
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, host_api

pytestmark = pytest.mark.gpu
F = np.float32
BY_MODE = {m: [c.name for c in rc.TRACKER_CASES if c.mode == m] for m in ("track", "validate", "search", "klt")}
CAP = tu.LIST_CAP


def etype(name):
    """The eType of a track or search row of the table (the builders' defaults: 4 for make_track, 1 for the search cases)."""
    c = rc.tracker_case(name)
    return c.args.get("type_", 1 if c.mode == "search" else 4)


@pytest.fixture(scope="module")
def fixtures():
    """Every fixture, read once: name -> (inputs, the compiled reference's outputs), read-only."""
    out = {}
    for c in rc.TRACKER_CASES:
        inp, ref = rc.load_tracker_fixture(c.name)
        ref = tu.reference_view(ref)
        for a in list(inp.values()) + list(ref.values()):
            a.setflags(write=False)
        out[c.name] = (inp, ref)
    return out


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype}{got.shape}, the reference writes {want.dtype}{want.shape}"
    assert tu.same_bits(got, want), f"{what} differs from the compiled reference:\n{got}\n{want}"


def _dev(a):
    import torch
    a = np.array(a, copy=True, order="C")   # the fixtures are read-only
    return torch.from_numpy(a if a.size else np.zeros((1,) + a.shape[1:], a.dtype)).to(torch.device("cuda", 0))


def _window(inp):
    t, w = np.ascontiguousarray(inp["imu_t"], np.float64), np.ascontiguousarray(inp["imu_w"], F)
    win = capi.ImuWindow(float(inp["times"][0]), float(inp["times"][1]), len(t), t.ctypes.data, w.ctypes.data)
    win.bias[:] = [float(v) for v in inp["bias"]]
    win._keep = (t, w)
    return win


@pytest.mark.parametrize("name", BY_MODE["track"] + BY_MODE["search"] + BY_MODE["klt"])
def test_gyro_integrate(ctx, fixtures, name):
    inp, ref = fixtures[name]
    rcl, rot9 = ctx.gyro_integrate(inp["rbc"], tu.params_of(inp), _window(inp))
    same(rcl, ref["Rcl"], f"{name}: Rcl")
    same(rot9[:6].reshape(2, 3), ref["KRKinv01"], f"{name}: rows 0 and 1 of KRKinv")
    same(rot9[6:], ref["Rcl"][2], f"{name}: the third row of Rcl in rot9")
    ctx.check_launch()


def _gyro_state(inp, ref):
    """The tracker's state after GyroPredictFeatures as the fixture holds it: the prediction's own status is affine_set."""
    if tu.cfg_of(inp).type == 5:
        return inp["keys_ref_un"], inp["keys_ref"], ref["affine_set"]
    return ref["pt_gyro_predict_un"], ref["pt_gyro_predict"], ref["affine_set"]


@pytest.mark.parametrize("form", ["device", "device_rot"])
@pytest.mark.parametrize("name", [n for n in BY_MODE["track"] + BY_MODE["search"] if etype(n) != 5])
def test_gyro_predict(ctx, fixtures, name, form):
    import torch
    inp, ref = fixtures[name]
    c, params = tu.cfg_of(inp), tu.params_of(inp)
    n = inp["keys_ref_un"].shape[0]
    dev = torch.device("cuda", 0)
    d_ref = _dev(inp["keys_ref_un"])
    pu, pd = torch.full((n, 2), 7.0, device=dev), torch.full((n, 2), 7.0, device=dev)
    st, aff = torch.full((n,), 7, dtype=torch.uint8, device=dev), torch.zeros((n, 4), device=dev)
    torch.cuda.synchronize()
    if form == "device":
        ctx.gyro_predict_device(params, c.width, c.height, ref["KRKinv"], ref["Rcl"][2], n, d_ref, pu, pd, st, aff)
    else:
        rot = _dev(np.concatenate([ref["KRKinv"][:2].reshape(6), ref["Rcl"][2]]).astype(F))
        ctx.gyro_predict_device_rot(params, c.width, c.height, rot, n, d_ref, pu, pd, st, aff)
    ctx.sync()
    want_un, want_dist, want_status = _gyro_state(inp, ref)
    same(st.cpu().numpy(), want_status, f"{name}: status of the prediction")
    same(pu.cpu().numpy(), want_un, f"{name}: mvPtGyroPredictUn")
    same(pd.cpu().numpy(), want_dist, f"{name}: mvPtGyroPredict")
    same(aff.cpu().numpy(), ref["affine"], f"{name}: the affine matrices (untouched where the prediction left the image)")
    if c.type == 1:
        same(np.where(want_status[:, None] != 0, pu.cpu().numpy() - inp["keys_ref_un"], F(0)).astype(F), ref["flows_predict_un"], f"{name}: flows")
    ctx.check_launch()


@pytest.mark.parametrize("name", [n for n in BY_MODE["track"] + BY_MODE["search"] if etype(n) != 1])
def test_track_then_post_filter(ctx, fixtures, name):
    inp, ref = fixtures[name]
    c, params = tu.cfg_of(inp), tu.params_of(inp)
    n = inp["keys_ref_un"].shape[0]
    init_un, init_dist, status_in = _gyro_state(inp, ref)
    pm = ctx.track(params, np.ascontiguousarray(inp["img_ref"]), np.ascontiguousarray(inp["img_cur"]), np.ascontiguousarray(inp["keys_ref_un"]),
                   np.ascontiguousarray(init_un), np.ascontiguousarray(ref["affine"]), np.ascontiguousarray(status_in))
    for mine, theirs in (("pt_dist", "pm_pt"), ("pt_un", "pm_pt_un"), ("status", "pm_status"), ("pix_err", "pm_pix_err"),
                         ("dist_pred", "pm_dist_pred"), ("ncc", "pm_ncc")):
        same(pm[mine][:n], ref[theirs], f"{name}: {theirs}")
    host = capi.post_filter(c.half, pm["status"][:n], pm["pix_err"][:n], pm["dist_pred"][:n], pm["pt_dist"][:n], pm["pt_un"][:n])
    device = host_api.post_filter_device(c.half, pm["status"][:n], pm["pix_err"][:n], pm["dist_pred"][:n], pm["pt_dist"][:n], pm["pt_un"][:n], ctx=ctx)
    for label, (kept, status, pp, ppu) in (("pagk_post_filter", host[:4]), ("pagk_post_filter_device", device[:4])):
        on = np.asarray(status)[:, None] != 0
        assert int(kept) == int(ref["ret"][0]) or rc.tracker_case(name).mode == "search", f"{name}: {label} keeps {kept}"
        same(np.asarray(status, np.uint8), ref["status"], f"{name}: {label}: mvStatus")
        same(np.where(on, pp, init_dist).astype(F), ref["pt_predict"], f"{name}: {label}: mvPtPredict")   # other rows keep the prediction (:329-335)
        same(np.where(on, ppu, init_un).astype(F), ref["pt_predict_un"], f"{name}: {label}: mvPtPredictUn")
    ctx.check_launch()


@pytest.mark.parametrize("name", BY_MODE["validate"])
def test_geometry_validation(ctx, fixtures, name):
    import torch
    inp, ref = fixtures[name]
    H21, H12, F21 = inp["H21"], ref["H12"], inp["F21"]
    cnt, st, _ = ctx.geometry_validation(H21, H12, F21, inp["keys_ref_un"], inp["pt_predict_un"], inp["status"])
    assert cnt == int(ref["ret"][0])
    same(st, ref["status"], f"{name}: pagk_geometry_validation")
    on = np.flatnonzero(inp["status"])
    if len(on) > 8:   # the scoring loops by themselves, host and device form, under the reference's model choice (:460-481)
        p1, p2 = np.ascontiguousarray(inp["keys_ref_un"][on]), np.ascontiguousarray(inp["pt_predict_un"][on])
        inl_h, inl_f, score_h, score_f = ctx.geometry_scores(H21, H12, F21, p1, p2)
        dev = torch.device("cuda", 0)
        d_h, d_f = torch.full((len(on),), 7, dtype=torch.uint8, device=dev), torch.full((len(on),), 7, dtype=torch.uint8, device=dev)
        d_s = torch.zeros(2, device=dev)
        torch.cuda.synchronize()
        ctx.geometry_scores_device(H21, H12, F21, len(on), _dev(p1), _dev(p2), 1.0, d_h, d_f, d_s)
        ctx.sync()
        scores = d_s.cpu().numpy()
        for label, (ih, i_f, sh, sf) in (("pagk_geometry_scores", (inl_h, inl_f, score_h, score_f)),
                                         ("pagk_geometry_scores_device", (d_h.cpu().numpy(), d_f.cpu().numpy(), scores[0], scores[1]))):
            chosen = ih if capi.geometry_select(float(sh), float(sf)) else i_f
            full = inp["status"].copy()
            full[on] = chosen
            same(full, ref["status"], f"{name}: {label} with pagk_geometry_select")
            assert int(chosen.sum()) == int(ref["ret"][0])
    ctx.check_launch()


def _list_args(inp, ref):
    return (np.ascontiguousarray(inp["img_ref"]), np.ascontiguousarray(inp["img_cur"]), tu.cfg_of(inp).half, np.ascontiguousarray(inp["keys_ref"]),
            np.ascontiguousarray(ref["pt_predict_un"]), np.ascontiguousarray(ref["status"]), np.ascontiguousarray(ref["affine"]),
            np.ascontiguousarray(inp["keys_cur"]), np.ascontiguousarray(inp["keys_cur_un"]))


def _same_lists(got, ref, what):
    cap = ref["nbr_idx"].shape[1]
    same(got["count"], ref["nbr_count"], f"{what}: list sizes")
    assert int(ref["nbr_count"].max()) <= CAP
    live = np.arange(cap)[None, :] < ref["nbr_count"][:, None]   # beyond a list's end the reference has nothing
    for mine, theirs in (("idx", "nbr_idx"), ("dist", "nbr_dist"), ("ncc", "nbr_ncc")):
        same(np.where(live, got[mine][:, :cap], 0), np.where(live, ref[theirs], 0), f"{what}: {theirs}, in the reference's order")


def _same_matches(q, t, d, c, ref, what):
    k = int(ref["ret"][0])
    same(np.asarray(q[:k], np.int32), ref["match_query"], f"{what}: queryIdx")
    same(np.asarray(t[:k], np.int32), ref["match_train"], f"{what}: trainIdx")
    same(np.asarray(d[:k], F), ref["match_dist"], f"{what}: distance")
    same(np.asarray(c[:k], F), ref["match_ncc"], f"{what}: ncc")


@pytest.mark.parametrize("name", BY_MODE["search"])
def test_near_neighbors_and_match_features(ctx, fixtures, name):
    import torch
    inp, ref = fixtures[name]
    use_ncc, args = bool(tu.cfg_of(inp).ncc), _list_args(inp, ref)
    level2 = bool((ref["nbr_level"] == 2).any()) or int(ref["ret"][0]) < 100   # whether the reference searched again (:921)
    assert level2 == (int(ref["ret"][0]) < 100)
    # host form
    r = ctx.find_near_neighbors(*args, level=1, use_ncc=use_ncc, cap=CAP)
    assert r["rc"] == 0
    if level2:
        r2 = ctx.find_near_neighbors(*args, level=2, use_ncc=use_ncc, cap=CAP, count=r["count"])
        assert r2["rc"] == 0
        keep = r["count"] > 0
        same(np.where(keep, 1, np.where(r2["count"] > 0, 2, 0)).astype(np.int32), ref["nbr_level"][:, 0], f"{name}: the level a list was found at")
        for k in ("idx", "dist", "ncc"):
            r2[k][keep] = r[k][keep]
        r = r2
    _same_lists(r, ref, f"{name}: pagk_find_near_neighbors")
    # device form on resident frames: level 2 fills only the lists level 1 left empty (:793)
    n, m = args[3].shape[0], args[7].shape[0]
    dev = torch.device("cuda", 0)
    ctx.frame_upload(0, args[0], 3)
    ctx.frame_upload(1, args[1], 3)
    d = [_dev(a) for a in args[3:]]
    cnt, idx = torch.zeros(n, dtype=torch.int32, device=dev), torch.full((n, CAP), -1, dtype=torch.int32, device=dev)
    dist, ncc = torch.zeros((n, CAP), device=dev), torch.zeros((n, CAP), device=dev)
    torch.cuda.synchronize()
    for level in (1, 2) if level2 else (1,):
        ctx.near_neighbors_device(0, 1, args[2], n, d[0], d[1], d[2], d[3], m, d[4], d[5], level, float(2 * args[2]), use_ncc, CAP, cnt, idx, dist, ncc)
    ctx.sync()
    lists = dict(count=cnt.cpu().numpy(), idx=idx.cpu().numpy(), dist=dist.cpu().numpy(), ncc=ncc.cpu().numpy())
    _same_lists(lists, ref, f"{name}: pagk_near_neighbors_device")
    # MatchFeatures on the device's lists, host and device form
    _same_matches(*capi.match_features(lists["count"], lists["idx"], lists["dist"], lists["ncc"], use_ncc), ref, f"{name}: pagk_match_features")
    q, t = torch.full((n,), 7, dtype=torch.int32, device=dev), torch.full((n,), 7, dtype=torch.int32, device=dev)
    md, mc = torch.full((n,), 7.0, device=dev), torch.full((n,), 7.0, device=dev)
    k, info = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(capi.ASSOC_INFO_WORDS, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.match_features_device(capi.assoc_params_default(use_ncc=int(use_ncc)), n, m, CAP, cnt, idx, dist, ncc, q, t, md, mc, k, info)
    ctx.sync()
    assert int(k.cpu()[0]) == int(ref["ret"][0])
    _same_matches(q.cpu().numpy(), t.cpu().numpy(), md.cpu().numpy(), mc.cpu().numpy(), ref, f"{name}: pagk_match_features_device")
    ctx.check_launch()


@pytest.mark.parametrize("name", BY_MODE["search"])
def test_search_gyro_predict_end_to_end(ctx, fixtures, name):
    inp, ref = fixtures[name]
    use_ncc = bool(tu.cfg_of(inp).ncc)
    s = ctx.search_gyro_predict(*_list_args(inp, ref), ap=capi.assoc_params_default(use_ncc=int(use_ncc)), cap=CAP)
    assert s["rc"] == int(ref["ret"][0]) == s["n_matches"]
    _same_lists(dict(count=s["count"], idx=s["idx"], dist=s["dist_lists"], ncc=s["ncc_lists"]), ref, f"{name}: pagk_search_gyro_predict")
    _same_matches(s["query"], s["train"], s["dist"], s["ncc"], ref, f"{name}: pagk_search_gyro_predict")
    same(s["flows_err"], ref["flows_error_un"], f"{name}: mvFlowsErrorUn")
    ctx.check_launch()
