"""GPU tests of pyramidal Lucas-Kanade (tracker type 0): pagk_lk_pyramid_device, pagk_lk_track_device and pagk_lk_track against
the plain-C restatement (tests/lk_ref.c), bit for bit, on the smallest shapes at which each rule can go wrong; capture and
replay; a second table of edge cases (every k_lk_track<NPIX> at both ends of its window range, parameters off their defaults,
extreme contrast, unequal pitches, the pyramid kernel's grid); the argument checks on a live context;
GyroAidedTracker::TrackFeatures with type 0 through the C++ shell."""
import numpy as np
import pytest
import torch

import lk_ref_util as lu
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, host_api, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return lu.build_ref(tmp_path_factory.mktemp("lk_ref"))


@pytest.fixture(scope="module")
def shapes():
    return lu.shapes(synth)


EDGE = lu.edge_shapes(synth)          # the second table (built here for the test ids)
PYRAMIDS = lu.pyramid_shapes()


@pytest.fixture(scope="module")
def restated(ref, shapes):
    """name (of either table) -> the restatement of that shape, computed once and left unchanged."""
    memo = {}

    def get(name, n=None):
        c = shapes[name] if name in shapes else EDGE[name]
        n = c["n"] if n is None else n
        if (name, n) not in memo:
            memo[(name, n)] = lu.ref_track(ref, c["ref"], c["cur"], c["pts"], c["p"], c["cap"], n)
        return memo[(name, n)]
    return get


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _set_slot(ctx, slot, img, pitch=None, junk=None):
    """The image into a frame slot: uploaded, or read in place from the left columns of a wider device buffer (returned:
    the caller keeps it alive while the slot is used); right of the image 255, or seeded junk."""
    h, w = img.shape
    if pitch is None:
        ctx.frame_upload(slot, img, 1)
        return None
    if junk is None:
        keep = torch.full((h, pitch), 255, dtype=torch.uint8, device=DEV)
    else:
        keep = _dev(np.random.default_rng(junk).integers(0, 256, (h, pitch), dtype=np.uint8))
    keep[:, :w] = _dev(img)
    torch.cuda.synchronize()
    ctx.frame_set_device(slot, keep.data_ptr(), w, h, pitch, 1)
    return keep


def _lk(p: dict):
    return capi.lk_params_default(**p)


def _device_track(ctx, c, n=None, pitch=None, with_optional=True, with_count=True):
    """pagk_lk_pyramid_device on slots 0 and 1, then pagk_lk_track_device: every output pre-filled with junk.  pitch: None,
    one pitch for both slots, or the pair (reference, current) with junk right of the image.  A case may name other
    parameters for its pyramids ("pyr")."""
    lk = _lk(c["p"])
    if isinstance(pitch, tuple):
        keep = [_set_slot(ctx, s, img, pt, junk=80 + s) for s, img, pt in ((0, c["ref"], pitch[0]), (1, c["cur"], pitch[1]))]
    else:
        keep = [_set_slot(ctx, s, img, pitch) for s, img in ((0, c["ref"]), (1, c["cur"]))]
    lk_pyr = _lk(c["pyr"]) if c.get("pyr") else lk
    ctx.lk_pyramid_device(lk_pyr, 0)
    ctx.lk_pyramid_device(lk_pyr, 1)
    cap = max(len(c["pts"]), 1) if c["cap"] is None else c["cap"]
    n = (len(c["pts"]) if c["n"] is None else c["n"]) if n is None else n
    buf = np.zeros((cap, 2), np.float32)                  # (rows beyond the list: as the restatement's helper fills them)
    buf[:len(c["pts"])] = c["pts"]
    d_p, d_n = _dev(buf), (_dev(np.array([n], np.int32)) if with_count else None)
    d_o = torch.full((cap, 2), -7.0, dtype=torch.float32, device=DEV)
    d_s = torch.full((cap,), 0x5a, dtype=torch.uint8, device=DEV)
    d_r = torch.full((cap,), 0x5a, dtype=torch.uint8, device=DEV) if with_optional else None
    d_e = torch.full((cap,), -7.0, dtype=torch.float32, device=DEV)
    d_f = torch.full((cap, 2), -7.0, dtype=torch.float32, device=DEV) if with_optional else None
    d_i = torch.full((capi.LK_INFO_WORDS,), -7, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    ctx.lk_track_device(lk, 0, 1, cap, d_p, d_n, d_o, d_s, d_r, d_e, d_f, d_i)
    ctx.sync()
    out = dict(pt_out=d_o.cpu().numpy(), status=d_s.cpu().numpy(), err=d_e.cpu().numpy(), info=d_i.cpu().numpy())
    if with_optional:
        out.update(status_raw=d_r.cpu().numpy(), flow=d_f.cpu().numpy())
    del keep
    return out


# ---- the shapes ----------------------------------------------------------------------------------------------------------
SHAPES = ["48x36 h2: three levels, borders, non-finite", "96x64 h10: top level cut to 1", "40x24 h10: level 0 only",
          "33x31 h1: win 3, every parent odd", "160x120 h15: 961 pixels", "160x120 h5: cap 300, count 257"]


@pytest.mark.parametrize("name", SHAPES)
def test_track_device_equals_the_restatement(ctx, shapes, restated, name):
    c = shapes[name]
    pitch = c["ref"].shape[1] + 29 if name.startswith("96x64") else None       # one shape is read through a wider pitch
    got = _device_track(ctx, c, pitch=pitch)
    want = restated(name)
    print(f"{name}: info {got['info'][:6].tolist()} (restated {want['info'][:6].tolist()})")
    assert lu.differing(got, want) == []


def test_counts_and_the_zeroed_tail(ctx, shapes, restated):
    name = "160x120 h5: cap 300, count 257"
    c = shapes[name]
    for n in (0, 257, 1000, -3):             # the device count is clamped to [0, cap]
        got = _device_track(ctx, c, n=n)
        want = restated(name, n)
        assert lu.differing(got, want) == [], n
        k = min(max(n, 0), 300)
        assert got["info"][0] == k
        for key in ("pt_out", "status", "status_raw", "err", "flow"):
            assert not got[key][k:].any(), (n, key)
    got = _device_track(ctx, c, with_optional=False, with_count=False)      # no count: cap; no raw status, no flow
    want = restated(name, 300)
    assert lu.differing(got, want, ("pt_out", "status", "err", "info")) == []


@pytest.mark.parametrize("name", SHAPES[:2] + SHAPES[3:4])
def test_pyramid_levels_equal_the_restatement(ctx, ref, shapes, name):
    c = shapes[name]
    lk = _lk(c["p"])
    levels = lu.ref_levels(ref, c["cur"], c["p"])
    assert len(levels) - 1 == capi.lk_levels(c["cur"].shape[1], c["cur"].shape[0], lk) >= 1
    for pitch in (None, c["cur"].shape[1] + 13):
        keep = _set_slot(ctx, 2, c["cur"], pitch)
        ctx.lk_pyramid_device(lk, 2)
        for l in range(1, len(levels)):
            h, w = levels[l].shape
            assert np.array_equal(ctx.selftest_lk_level(2, l, w, h), levels[l]), (name, pitch, l)
            assert np.array_equal(ctx.selftest_lk_level(2, l, w, h, pitch=w + 5), levels[l]), (name, pitch, l)
        with pytest.raises(capi.PagkError):
            ctx.selftest_lk_level(2, len(levels), 8, 8)
        with pytest.raises(capi.PagkError):
            ctx.selftest_lk_level(2, 0, c["cur"].shape[1], c["cur"].shape[0])
        del keep


def test_host_form_equals_the_device_form(ctx, shapes, restated):
    for name in (SHAPES[0], SHAPES[5]):
        c = shapes[name]
        n = len(c["pts"])
        got = ctx.lk_track(c["ref"], c["cur"], c["pts"], _lk(c["p"]))
        want = restated(name, n)
        assert lu.differing(got, {k: (v if k == "info" else v[:n]) for k, v in want.items()}) == [], name
        assert (got["n"], got["raw"], got["kept"], got["top_level"]) == tuple(int(v) for v in want["info"][:4])
    c = shapes[SHAPES[1]]
    wide = [np.full((64, 96 + 11), 200, np.uint8) for _ in range(2)]                  # host images with a pitch
    wide[0][:, :96], wide[1][:, :96] = c["ref"], c["cur"]
    got = ctx.lk_track(wide[0][:, :96], wide[1][:, :96], c["pts"], _lk(c["p"]))
    assert lu.differing(got, restated(SHAPES[1])) == []
    empty = ctx.lk_track(c["ref"], c["cur"], np.zeros((0, 2), np.float32), _lk(c["p"]))
    assert empty["info"].tolist() == [0, 0, 0, 1, 0, 0, 0, 0] and empty["pt_out"].shape == (0, 2)
    via = host_api.lk_track(c["ref"], c["cur"], c["pts"], _lk(c["p"]), ctx=ctx)
    assert lu.differing(via, restated(SHAPES[1])) == []


# ---- the edge table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EDGE))
def test_edge_track_device_equals_the_restatement(ctx, restated, name):
    """Every case of lk_ref_util.edge_shapes() (tests/test_lk_cpu.py says which exits of the level loop they take): the name
    says the window and k_lk_track<NPIX>, or the parameter that left its default."""
    c = EDGE[name]
    got = _device_track(ctx, c, pitch=c["pitch"])
    want = restated(name)
    print(f"{name}: k_lk_track<{c['npix']}>, info {got['info'][:6].tolist()} (restated {want['info'][:6].tolist()})")
    bad = lu.differing(got, want)
    if bad:                                                # the first differing feature and why it left each level
        key = next(k for k in bad if k != "info") if bad != ["info"] else "info"
        if key != "info":
            k = int(np.flatnonzero([not lu.same_array(a, b) for a, b in zip(got[key], want[key])])[0])
            print(f"  {key}[{k}]: device {got[key][k]}, restated {want[key][k]}, pt_ref {c['pts'][k]}, why {want['why'][k].tolist()}")
    assert bad == []


@pytest.mark.parametrize("name", [n for n, c in EDGE.items() if c["host"]])
def test_edge_host_form_equals_the_restatement(ctx, restated, name):
    """pagk_lk_track on the smallest legal frame of every window and on every k_lk_track<4> case that needs no device slot
    of its own (pitches, deeper pyramids)."""
    c = EDGE[name]
    got = ctx.lk_track(c["ref"], c["cur"], c["pts"], _lk(c["p"]))
    want = restated(name)
    assert lu.differing(got, want) == []
    assert (got["n"], got["raw"], got["kept"], got["top_level"]) == tuple(int(v) for v in want["info"][:4])


@pytest.mark.parametrize("name", list(PYRAMIDS))
def test_pyramid_grid_equals_the_restatement(ctx, ref, name):
    """k_lk_pyrdown beyond its first 64 x 4 block in both directions: level widths 63, 64, 65, 128 and 129, level heights of
    every residue modulo 4, the source slot with and without a pitch."""
    img = PYRAMIDS[name]
    p = lu.params(half_patch=1, max_level=7)
    lk = _lk(p)
    levels = lu.ref_levels(ref, img, p)
    assert len(levels) - 1 == capi.lk_levels(img.shape[1], img.shape[0], lk) >= 1
    for pitch in (None, img.shape[1] + 13):
        keep = _set_slot(ctx, 2, img, pitch, junk=81)
        ctx.lk_pyramid_device(lk, 2)
        for l in range(1, len(levels)):
            h, w = levels[l].shape
            assert np.array_equal(ctx.selftest_lk_level(2, l, w, h), levels[l]), (name, pitch, l)
        del keep


# ---- capture -----------------------------------------------------------------------------------------------------------
def test_capture_pyramids_and_track_and_replay(ref):
    w, h, cap = 96, 64, 40
    frames = [lu.texture_pair(synth, w, h, 41, s)[1] for s in ((0, 0), (1.2, -0.7), (-2.1, 1.4))]
    pts = lu.interior_points(w, h, 37, 6, 42)
    p = lu.params(half_patch=4)
    lk = _lk(p)
    c = capi.Context(0)
    try:
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            c.set_stream(stream.cuda_stream)
            d_img = [torch.zeros((h, w + 16), dtype=torch.uint8, device=DEV) for _ in range(2)]
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)     # noqa: E731
            buf = np.zeros((cap, 2), np.float32)
            buf[:len(pts)] = pts
            d_p, d_n = _dev(buf), _dev(np.array([len(pts)], np.int32))
            outs = [z((cap, 2), torch.float32), z(cap, torch.uint8), z(cap, torch.uint8), z(cap, torch.float32),
                    z((cap, 2), torch.float32), z(capi.LK_INFO_WORDS, torch.int32)]
            d_img[0][:, :w] = _dev(frames[0])

            def work():
                for s in range(2):
                    c.frame_set_device(s, d_img[s].data_ptr(), w, h, w + 16, 1)
                    c.lk_pyramid_device(lk, s)
                c.lk_track_device(lk, 0, 1, cap, d_p, d_n, outs[0], outs[1], outs[2], outs[3], outs[4], outs[5])

            def result():
                stream.synchronize()
                o = [t.cpu().numpy() for t in outs]
                return dict(pt_out=o[0], status=o[1], status_raw=o[2], err=o[3], flow=o[4], info=o[5])

            def feed(k):
                d_img[1][:, :w] = _dev(frames[k])

            want = {k: lu.ref_track(ref, frames[0], frames[k], pts, p, cap) for k in (1, 2)}
            for k in (1, 2):                          # the direct calls (the first one sizes the pyramids' buffers)
                feed(k)
                work()
                assert lu.differing(result(), want[k]) == [], ("direct", k)
            c.graph_begin()
            try:
                with pytest.raises(capi.PagkError):   # the host-buffer forms are not capturable
                    c.lk_track(frames[0], frames[1], pts, lk)
                with pytest.raises(capi.PagkError):
                    c.selftest_lk_level(0, 1, (w + 1) // 2, (h + 1) // 2)
                work()
            finally:
                gid = c.graph_end()
            for k in (1, 2):                          # replayed twice, the second frame changed in place
                feed(k)
                for t in outs:
                    t.fill_(9)
                c.graph_launch(gid)
                assert lu.differing(result(), want[k]) == [], ("replay", k)
            c.graph_destroy(gid)
    finally:
        c.set_stream(None)
        c.close()


def test_capture_and_replay_half_patch_7(ref):
    """The pattern of test_capture_pyramids_and_track_and_replay on k_lk_track<4> (window 15, three levels): replayed twice,
    the current frame changed in place in between, each replay held to the restatement."""
    w, h, cap = 96, 80, 40
    frames = [lu.texture_pair(synth, w, h, 45, s)[1] for s in ((0, 0), (1.4, -0.9), (-1.8, 2.2))]
    pts = lu.mixed_points(w, h, 15, 37, 46, nonfinite=True)
    p = lu.params(half_patch=7)
    lk = _lk(p)
    c = capi.Context(0)
    try:
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            c.set_stream(stream.cuda_stream)
            d_img = [torch.full((h, w + 16), 0xa5, dtype=torch.uint8, device=DEV) for _ in range(2)]
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)     # noqa: E731
            buf = np.zeros((cap, 2), np.float32)
            buf[:len(pts)] = pts
            d_p, d_n = _dev(buf), _dev(np.array([len(pts)], np.int32))
            outs = [z((cap, 2), torch.float32), z(cap, torch.uint8), z(cap, torch.uint8), z(cap, torch.float32),
                    z((cap, 2), torch.float32), z(capi.LK_INFO_WORDS, torch.int32)]
            d_img[0][:, :w] = _dev(frames[0])

            def work():
                for s in range(2):
                    c.frame_set_device(s, d_img[s].data_ptr(), w, h, w + 16, 1)
                    c.lk_pyramid_device(lk, s)
                c.lk_track_device(lk, 0, 1, cap, d_p, d_n, outs[0], outs[1], outs[2], outs[3], outs[4], outs[5])

            def result():
                stream.synchronize()
                o = [t.cpu().numpy() for t in outs]
                return dict(pt_out=o[0], status=o[1], status_raw=o[2], err=o[3], flow=o[4], info=o[5])

            want = {k: lu.ref_track(ref, frames[0], frames[k], pts, p, cap) for k in (1, 2)}
            assert want[1]["info"][3] == 2 and lu.differing(want[1], want[2]) != []
            d_img[1][:, :w] = _dev(frames[1])
            work()                                    # the direct call sizes the pyramids' buffers
            assert lu.differing(result(), want[1]) == [], "direct"
            c.graph_begin()
            try:
                work()
            finally:
                gid = c.graph_end()
            for k in (2, 1):                          # replayed twice, the current frame changed in place
                d_img[1][:, :w] = _dev(frames[k])
                for t in outs:
                    t.fill_(9)
                c.graph_launch(gid)
                assert lu.differing(result(), want[k]) == [], ("replay", k)
            c.graph_destroy(gid)
    finally:
        c.set_stream(None)
        c.close()


# ---- arguments -----------------------------------------------------------------------------------------------------------
def test_arguments_are_checked_on_a_live_context(shapes):
    c0 = shapes[SHAPES[1]]
    c = capi.Context(0)
    try:
        ok = capi.lk_params_default()
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)     # noqa: E731
        d_p, d_o, d_s, d_e, d_i = z((16, 2), torch.float32), z((16, 2), torch.float32), z(16, torch.uint8), z(16, torch.float32), z(8, torch.int32)
        track = lambda lk, a=0, b=1, cap=16: c.lk_track_device(lk, a, b, cap, d_p, None, d_o, d_s, None, d_e, None, d_i)   # noqa: E731
        with pytest.raises(capi.PagkError) as e:                         # no frame in the slot
            c.lk_pyramid_device(ok, 0)
        assert e.value.code == capi.PAGK_E_ARG
        c.frame_upload(0, c0["ref"], 1)
        c.frame_upload(1, c0["cur"], 1)
        with pytest.raises(capi.PagkError) as e:                         # tracking before the pyramids were built
            track(ok)
        assert e.value.code == capi.PAGK_E_ARG and "pagk_lk_pyramid_device" in str(e.value)
        c.lk_pyramid_device(ok, 0)
        with pytest.raises(capi.PagkError):                              # ... one of them is not enough
            track(ok)
        c.lk_pyramid_device(ok, 1)
        track(ok)
        c.sync()
        for kw in (dict(half_patch=0), dict(half_patch=16), dict(max_level=8), dict(max_count=0), dict(epsilon=float("nan")),
                   dict(min_eig_threshold=-1.0), dict(err_threshold=float("nan"))):      # bad parameters
            bad = capi.lk_params_default(**kw)
            with pytest.raises(capi.PagkError) as e:
                track(bad)
            assert e.value.code == capi.PAGK_E_ARG, kw
            with pytest.raises(capi.PagkError):
                c.lk_pyramid_device(bad, 0)
            with pytest.raises(capi.PagkError):
                c.lk_track(c0["ref"], c0["cur"], c0["pts"], bad)
        for a, b, cap in ((-1, 1, 16), (0, 4, 16), (0, 1, 0), (0, 1, (1 << 24) + 1)):
            with pytest.raises(capi.PagkError):
                track(ok, a, b, cap)
        with pytest.raises(capi.PagkError):
            c.lk_pyramid_device(ok, 4)
        with pytest.raises(ValueError):
            c.lk_track_device(ok, 0, 1, 16, d_p, None, None, d_s, None, d_e, None, d_i)
        # a level 0 that is not larger than the window: 21 x 40 with win = 21, and 96 x 64 with win = 31 in one direction only
        small = np.zeros((40, 21), np.uint8)
        c.frame_upload(2, small, 1)
        with pytest.raises(capi.PagkError) as e:
            c.lk_pyramid_device(ok, 2)
        assert e.value.code == capi.PAGK_E_ARG
        with pytest.raises(capi.PagkError):
            c.lk_track(small, small, np.zeros((1, 2), np.float32), ok)
        c.lk_pyramid_device(capi.lk_params_default(half_patch=15), 0)    # 96 x 64 is larger than 31 x 31 ...
        c.frame_upload(3, np.zeros((31, 96), np.uint8), 1)
        with pytest.raises(capi.PagkError):                              # ... 96 x 31 is not
            c.lk_pyramid_device(capi.lk_params_default(half_patch=15), 3)
        c.frame_upload(3, np.zeros((48, 64), np.uint8), 1)               # frames of two sizes
        c.lk_pyramid_device(capi.lk_params_default(half_patch=5), 3)
        with pytest.raises(capi.PagkError):
            track(capi.lk_params_default(half_patch=5), 0, 3)
        c.frame_upload(1, np.zeros((48, 64), np.uint8), 1)               # a slot that changed its size lost its pyramid
        c.frame_upload(0, np.zeros((48, 64), np.uint8), 1)
        with pytest.raises(capi.PagkError):
            track(capi.lk_params_default(half_patch=5))
    finally:
        c.close()


# ---- the shell -----------------------------------------------------------------------------------------------------------
def _scene(n=200, seed=0x5EED0700):
    """The scene of tests/test_host_shell.py."""
    cam = synth.D435I
    w = synth.make_workload("host", 320, 240, n, seed=seed, half_patch=5, iterations=10, pyramids=3, camera=cam,
                            omega=(0.3, -0.4, 1.2), gyro_error=(0.003, -0.002, 0.004), edge_fraction=0.2)
    R = synth.rodrigues(np.array((0.003, -0.002, 0.004))) @ synth.rodrigues(np.array((0.3, -0.4, 1.2)) * 0.05)
    K = cam.K.astype(np.float32)
    return cam, w, R.astype(np.float32), K


def _distort(pts, K, dist):
    """DistortVecPoints (reference src/utils.cpp:49-76) in float32, one rounding per operation."""
    F = np.float32
    fx, fy, cx, cy = F(K[0, 0]), F(K[1, 1]), F(K[0, 2]), F(K[1, 2])
    fxi, fyi = F(1.0 / float(fx)), F(1.0 / float(fy))
    d = np.asarray(dist, np.float32)
    k1, k2, p1, p2 = d[0], d[1], d[2], d[3]
    k3 = d[4] if d.size == 5 else F(0)
    x, y = (pts[:, 0] - cx) * fxi, (pts[:, 1] - cy) * fyi
    r2 = x * x + y * y
    r4 = r2 * r2
    r6 = r4 * r2
    one, two = F(1), F(2)
    rad = one + k1 * r2 + k2 * r4 + k3 * r6
    xd = x * rad + two * p1 * x * y + p2 * (r2 + two * x * x)
    yd = y * rad + p1 * (r2 + two * y * y) + two * p2 * x * y
    return np.column_stack([fx * xd + cx, fy * yd + cy]).astype(np.float32)


@pytest.mark.parametrize("with_rcl", [False, True])
def test_shell_type_0_equals_the_restatement_and_the_filter(built, ref, with_rcl):
    cam, w, R32, K32 = _scene()
    ret, out = host_api.track_features(w.img_ref, w.img_cur, w.pt_ref, K32, cam.dist, type=0, half_patch=5,
                                       Rcl=R32 if with_rcl else None)
    want = lu.ref_track(ref, w.img_ref, w.img_cur, w.pt_ref, lu.params(half_patch=5))
    kept = want["status_raw"].astype(bool) & ~(want["err"] >= np.float32(12.0))             # :371-375
    print(f"type 0: returned {ret}, kept {int(kept.sum())} of {w.n} (raw {int(want['status_raw'].sum())})")
    assert ret == int(kept.sum()) == int(want["info"][2]) and 0 < ret
    assert np.array_equal(out["status"], kept.astype(np.uint8))
    assert lu.same_array(out["pt_predict_un"], want["pt_out"])
    assert lu.same_array(out["error"], want["err"])
    assert lu.same_array(out["flows_predict_un"], want["pt_out"] - w.pt_ref.astype(np.float32))
    assert lu.same_array(out["flows_predict_un"], want["flow"])
    with np.errstate(all="ignore"):
        assert lu.same_array(out["pt_predict"], _distort(want["pt_out"], K32, cam.dist))      # :379
    # the other types are untouched by the new branch: type 1 still returns its own count
    r1, _ = host_api.track_features(w.img_ref, w.img_cur, w.pt_ref, K32, cam.dist, type=1, half_patch=5, Rcl=R32)
    assert 0 < r1 < w.n
