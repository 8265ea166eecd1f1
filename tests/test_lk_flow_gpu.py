"""GPU tests of the flow form of pyramidal Lucas-Kanade: pagk_lk_track_flow (kernel k_lk_flow) against the plain-C restatement
tests/lk_flow_ref.c, byte for byte, on the flow edge table (every output pre-filled with junk); the identity with
pagk_lk_track on the whole edge table of tests/lk_ref_util.py; the same bytes from contexts whose workspaces were filled with
two different words; the argument checks on a live context."""
import ctypes as C

import numpy as np
import pytest

import lk_flow_ref_util as fu
import lk_ref_util as lu
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, host_api, synth

pytestmark = pytest.mark.gpu
TABLE = fu.flow_edge_shapes(synth)      # (built here for the test ids)
EDGE = lu.edge_shapes(synth)
OUT = ("pt_out", "pt_out_dist", "status", "status_raw", "err", "flow", "info")


@pytest.fixture(scope="module")
def flow_ref(tmp_path_factory):
    return fu.build_ref(tmp_path_factory.mktemp("lk_flow_ref"))


def _cam(c) -> capi.Params:
    """The case's camera as a pagk_params."""
    k = c["cam"]
    return capi.make_params(camera=synth.Camera(k["fx"], k["fy"], k["cx"], k["cy"], tuple(k["dist"][:k["n"]])))


def _flow(ctx, c, junk=0x5a):
    """pagk_lk_track_flow on the first n rows of a case of the flow table, called on arrays of exactly n rows that hold junk
    -> the outputs, n rows each."""
    n = c["n"]
    pts, init, live = (np.ascontiguousarray(c[k][:n]) for k in ("pts", "init", "live"))
    out = dict(pt_out=np.full((n, 2), -7, np.float32), pt_out_dist=np.full((n, 2), -7, np.float32),
               status=np.full(n, junk, np.uint8), status_raw=np.full(n, junk, np.uint8), err=np.full(n, -7, np.float32),
               flow=np.full((n, 2), -7, np.float32), info=np.full(capi.LK_INFO_WORDS, -7, np.int32))
    lk, cam = capi.lk_params_default(**c["p"]), _cam(c)
    ir, ic = capi.image_view(c["ref"]), capi.image_view(c["cur"])
    rc = ctx.lib.pagk_lk_track_flow(ctx.h, C.byref(lk), C.byref(cam), C.byref(ir), C.byref(ic), n, pts.ctypes.data, init.ctypes.data,
                                    live.ctypes.data, *(out[k].ctypes.data for k in OUT))
    assert rc == capi.PAGK_OK, ctx.lib.pagk_last_error(ctx.h)
    return out


def _rows(r: dict, n: int) -> dict:
    return {k: (v if k == "info" else v[:n]) for k, v in r.items()}


@pytest.mark.parametrize("name", list(TABLE))
def test_flow_equals_the_restatement(ctx, flow_ref, name):
    c = TABLE[name]
    want = fu.run_case(lambda *a, **kw: fu.ref_flow(flow_ref, *a, **kw), c)
    got = _flow(ctx, c)
    print(f"{name}: k_lk_flow<{c['npix']}>, info {got['info'][:7].tolist()} (restated {want['info'][:7].tolist()})")
    bad = lu.differing(got, _rows(want, c["n"]), OUT)
    for key in bad:
        if key != "info":
            k = int(np.flatnonzero([not lu.same_array(a, b) for a, b in zip(got[key], want[key])])[0])
            print(f"  {key}[{k}]: device {got[key][k]}, restated {want[key][k]}, pt_ref {c['pts'][k]}, pt_init {c['init'][k]}, "
                  f"status_in {c['live'][k]}, why {want['why'][k].tolist()}")
    assert bad == []
    assert got["info"][6] == (c["live"][:c["n"]] == 0).sum() > 0


@pytest.mark.parametrize("name", list(EDGE))
def test_identity_with_lk_track(ctx, name):
    """pt_init NULL or bit-equal to pt_ref, status_in NULL or all set: every output of pagk_lk_track, byte for byte; and the
    distorted point of every row is DistortVecPoints of its point."""
    c = EDGE[name]
    lk = capi.lk_params_default(**c["p"])
    want = ctx.lk_track(c["ref"], c["cur"], c["pts"], lk)
    h, w = c["ref"].shape
    cam = dict(fx=61.5, fy=59.25, cx=w / 2.0, cy=h / 2.0, dist=(-0.2834, 0.0739, 0.00019, 1.76e-05, -0.0112), n=5)
    cp = capi.make_params(camera=synth.Camera(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["dist"]))
    plain = ctx.lk_track_flow(c["ref"], c["cur"], c["pts"], lk)
    full = host_api.lk_track_flow(c["ref"], c["cur"], c["pts"], lk, cam=cp, pt_init=c["pts"].copy(),
                                  status_in=np.full(len(c["pts"]), 0x80, np.uint8), ctx=ctx)
    assert lu.differing(plain, want) == [] and "pt_out_dist" not in plain
    assert lu.differing(full, want) == [] and full["skipped"] == 0
    assert lu.same_array(full["pt_out_dist"], fu.model_distort(want["pt_out"], cam))


def test_rows_beyond_the_count_and_the_empty_call(ctx):
    c = next(iter(TABLE.values()))
    lk = capi.lk_params_default(**c["p"])
    empty = ctx.lk_track_flow(c["ref"], c["cur"], np.zeros((0, 2), np.float32), lk, cam=_cam(c))
    assert empty["info"].tolist() == [0, 0, 0, 0, 0, 0, 0, 0] and empty["pt_out_dist"].shape == (0, 2)
    off = ctx.lk_track_flow(c["ref"], c["cur"], c["pts"], lk, cam=_cam(c), status_in=np.zeros(len(c["pts"]), np.uint8))
    assert off["info"].tolist() == [len(c["pts"]), 0, 0, 0, 0, 0, len(c["pts"]), 0]
    for key in ("pt_out", "pt_out_dist", "status", "status_raw", "err", "flow"):
        assert not off[key].any(), key


def test_result_does_not_depend_on_what_the_workspaces_held(flow_ref):
    """Two contexts whose every block arrives filled with a word of its own (pagk_selftest_fill_workspaces, also_new = 1), the
    second filled once more between the cases: the same bytes, and those of the restatement."""
    names = [n for n in TABLE if "win9 " in n or "win31 " in n]
    assert len(names) == 4
    got = {}
    for word in (0x00000001, 0xffc0ffc0):
        x = capi.Context(0)
        try:
            x.selftest_fill_workspaces(word, True)
            for name in names:
                got[(word, name)] = _flow(x, TABLE[name], junk=word & 0xff)
                if word != 1:
                    x.selftest_fill_workspaces(word, True)
        finally:
            x.close()
    for name in names:
        c = TABLE[name]
        want = _rows(fu.run_case(lambda *a, **kw: fu.ref_flow(flow_ref, *a, **kw), c), c["n"])
        assert lu.differing(got[(1, name)], got[(0xffc0ffc0, name)], OUT) == [], name
        assert lu.differing(got[(1, name)], want, OUT) == [], name


def test_arguments_are_checked_on_a_live_context(ctx):
    c = next(iter(TABLE.values()))
    n = c["n"]
    lk, cam = capi.lk_params_default(**c["p"]), _cam(c)
    ir, ic = capi.image_view(c["ref"]), capi.image_view(c["cur"])
    pts = np.ascontiguousarray(c["pts"][:n])
    o2, o1, s1 = np.zeros((n, 2), np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint8)
    a = lambda x: x.ctypes.data     # noqa: E731

    def call(lk=lk, cam=cam, ref=ir, cur=ic, n=n, pt=a(pts), out=a(o2), dist=a(o2), st=a(s1), err=a(o1)):
        return ctx.lib.pagk_lk_track_flow(ctx.h, C.byref(lk) if lk else None, C.byref(cam) if cam else None,
                                          C.byref(ref) if ref else None, C.byref(cur) if cur else None, n, pt, None, None, out,
                                          dist, st, None, err, None, None)
    assert call() == capi.PAGK_OK
    assert call(cam=None, dist=None) == capi.PAGK_OK
    assert call(cam=None) == capi.PAGK_E_ARG                                  # a distorted point needs a camera
    assert call(cam=capi.make_params(half_patch=0)) == capi.PAGK_E_ARG        # ... one that passes pagk_params_check
    for kw in (dict(lk=None), dict(ref=None), dict(cur=None), dict(n=-1), dict(n=(1 << 24) + 1), dict(pt=None), dict(out=None),
               dict(st=None), dict(err=None), dict(lk=capi.lk_params_default(half_patch=16)),
               dict(lk=capi.lk_params_default(max_count=0)), dict(cur=capi.image_view(np.zeros((40, 44), np.uint8))),
               dict(lk=capi.lk_params_default(half_patch=15))):              # (a window larger than the frame)
        assert call(**kw) == capi.PAGK_E_ARG, list(kw)
    with pytest.raises(ValueError):
        ctx.lk_track_flow(c["ref"], c["cur"], c["pts"], lk, pt_init=c["pts"][:3])
    assert call() == capi.PAGK_OK                                             # the context serves the next call as usual


def test_flow_is_refused_inside_a_capture():
    """The host form synchronises: PAGK_E_ARG between pagk_graph_begin and pagk_graph_end, and the capture goes on."""
    import torch
    c = TABLE[[n for n in TABLE if "win9 " in n and "three levels" in n][0]]
    lk = capi.lk_params_default(**c["p"])
    x = capi.Context(0)
    try:
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            x.set_stream(stream.cuda_stream)
            x.frame_upload(0, c["ref"], 1)
            x.lk_pyramid_device(lk, 0)
            want = x.lk_track_flow(c["ref"], c["cur"], c["pts"], lk, pt_init=c["init"], status_in=c["live"])
            x.graph_begin()
            try:
                with pytest.raises(capi.PagkError) as e:
                    x.lk_track_flow(c["ref"], c["cur"], c["pts"], lk)
                assert e.value.code == capi.PAGK_E_ARG
                x.lk_pyramid_device(lk, 0)
            finally:
                gid = x.graph_end()
            x.graph_launch(gid)
            x.sync()
            x.graph_destroy(gid)
            again = x.lk_track_flow(c["ref"], c["cur"], c["pts"], lk, pt_init=c["init"], status_in=c["live"])
            assert lu.differing(again, want) == []
    finally:
        x.set_stream(None)
        x.close()
