"""The library-owned buffers that captured graphs point into (the table): each refuses to grow inside
a capture and while a graph of its context is alive -- PAGK_E_ARG before any launch, the graph's replays untouched --
and grows once the graph is gone.  One case per buffer, at the smallest shapes that make it grow."""
import numpy as np
import pytest
import torch

import detect_ref_util as du
import fit_ref_util as fu
import handover_ref_util as hu
import rectify_ref_util as ru
from oracle import pagk_oracle as orc
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, distributed, synth
from util import assert_parity, make_geometry_case, params_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp("workspace_refs")
    return dict(det=du.build_ref(d), hand=hu.build_ref(d), fit=fu.build_ref(d), rect=ru.build_ref(d))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _full(shape, dtype):
    return torch.full(shape, -7, dtype=dtype, device=DEV)


def _tensors(outs):
    """(reset, snapshot) of a case whose outputs (and in/out state) are device tensors."""
    init = [t.clone() for t in outs]
    return (lambda: [t.copy_(t0) for t, t0 in zip(outs, init)]), (lambda: [t.cpu().numpy().tobytes() for t in outs])


# Every case: (the buffer's name in the error text, small call, larger call, reset, snapshot, check of the larger call)
def _det(c, refs):
    imgs = [du.noise_image(64, 48, 1), du.noise_image(128, 96, 2)]
    for slot, im in enumerate(imgs):
        c.frame_upload(slot, im, 1)
    det, cap = capi.detect_params_default(min_distance=6.0), 64
    outs = [_full((cap, 2), torch.float32), _full((capi.DETECT_INFO_WORDS,), torch.int32)]

    def check():
        got = dict(corners=outs[0].cpu().numpy(), info=outs[1].cpu().numpy())
        want = du.ref_detect(refs["det"], imgs[1], None, cap, min_distance=6.0)
        assert want["n"] > 4 and du.same_detect(got, want) == []
    call = lambda slot: c.detect_corners_device(det, slot, None, cap, None, *outs)  # noqa: E731
    return ("the detector's workspace", lambda: call(0), lambda: call(1), *_tensors(outs), check)


def _hand(c, refs):
    p, cap, n_cand = capi.make_params(camera=synth.D435I), 48, 60
    sizes, host, dev = [(64, 48), (128, 96)], [], []
    for k, (w, h) in enumerate(sizes):
        rng = np.random.default_rng(k)
        un = (rng.random((cap, 2)) * [w, h]).astype(np.float32)
        host.append(((rng.random(cap) < 0.5).astype(np.uint8), un + np.float32(0.25), un,
                     (rng.random((n_cand, 2)) * [w, h]).astype(np.float32)))
        dev.append([_dev(a) for a in host[k][:3]] + [_dev(np.int32([n_cand])), _dev(host[k][3])])
    names = ("keys", "keys_un", "keys_normal", "index_in_last", "live", "state")
    outs = [_full((cap, 2), torch.float32) for _ in range(3)] + [_full((cap,), torch.int32), _full((cap,), torch.uint8),
                                                                 torch.zeros(8, dtype=torch.int32, device=DEV)]

    def call(k):
        c.frame_handover_device(p, *sizes[k], cap, cap, float(cap), *dev[k][:3], n_cand, *dev[k][3:], *outs[:5], None, outs[5])

    def check():
        want = hu.ref_handover(refs["hand"], hu.camera_of(p), *sizes[1], cap, cap, float(cap), *host[1])
        assert want["state"][3] > 0   # (candidates were taken: the mask was read)
        assert [n for n, t in zip(names, outs) if t.cpu().numpy().tobytes() != want[n].tobytes()] == []
    return ("the hand-over's mask", lambda: call(0), lambda: call(1), *_tensors(outs), check)


def _fit(c, refs):
    kw = dict(seed=5, iters_H=64, iters_F=64)
    scenes = [make_geometry_case(7 + n, n, planar=False) for n in (16, 64)]
    pts = [[_dev(g["pts1"]), _dev(g["pts2"])] for g in scenes]
    outs = [_full((27,), torch.float64), _full((64,), torch.uint8), _full((64,), torch.uint8),
            _full((capi.FIT_INFO_WORDS,), torch.int32), _full((128,), torch.int32)]

    def check():
        want = fu.ref_fit(refs["fit"], fu.params(**kw), scenes[1]["pts1"], scenes[1]["pts2"])
        got = [t.cpu().numpy() for t in outs]
        assert got[0].tobytes() == want["models"].tobytes() and np.array_equal(got[3], want["info"])
        assert np.array_equal(got[1], want["mask_H"]) and np.array_equal(got[2], want["mask_F"])
        assert np.array_equal(got[4], want["hyp_counts"])
    call = lambda k: c.geometry_fit_device(capi.fit_params_default(**kw), (16, 64)[k], *pts[k], None, *outs)  # noqa: E731
    return ("the geometry fit's workspace", lambda: call(0), lambda: call(1), *_tensors(outs), check)


def _rect(c, refs):
    mx, my, _, _ = ru.grid_maps(64, 48, 64, 48, 3)
    c.rectify_set_maps(mx, my)
    raws = [ru.noise_raw(64, 48, 1, 1), ru.noise_raw(128, 96, 1, 2)]
    pinned = [torch.from_numpy(np.ascontiguousarray(r)).pin_memory() for r in raws]
    rp = capi.rectify_params_default(channels=1)

    def call(k, slot):
        c.frame_rectify_pinned(slot, rp, pinned[k].data_ptr(), raws[k].shape[1], raws[k].shape[0], raws[k].shape[1], 1)
    call(0, 1)   # slot 1 exists from here on: all the larger call lacks is the staging buffer
    c.sync()

    def check():
        assert np.array_equal(c.frame_download_level(1, 0, 64, 48), ru.ref_rectify(refs["rect"], mx, my, raws[1]))
    return ("the raw frame's staging buffer", lambda: call(0, 0), lambda: call(1, 1),
            lambda: c.frame_upload(0, np.zeros((48, 64), np.uint8), 1), lambda: c.frame_download_level(0, 0, 64, 48).tobytes(),
            check)


def _track(c, kernel, what, prime=None):
    w = synth.make_workload("workspaces", 320, 240, 64, seed=0x5EED5A0C, half_patch=10, iterations=30, pyramids=3)
    p = params_for(w)
    c.frame_upload(0, w.img_ref, 3)
    c.frame_upload(1, w.img_cur, 3)
    d = [_dev(a) for a in (w.pt_ref, w.pt_init, w.affine, w.status_in)]
    out = distributed.alloc_device_outputs(64, DEV)
    call = lambda n: c.track_device(p, 0, 1, n, *d, out)  # noqa: E731
    if prime:        # another variant sizes the buffers that are not this case's
        c.set_kernel(prime)
        call(64)
        c.sync()
    c.set_kernel(kernel)

    def check():
        ref = orc.track(p, w.img_ref, w.img_cur, w.pt_ref, w.pt_init, w.affine, w.status_in, nthreads=4)
        assert_parity(distributed.to_numpy(out), ref, 64, exact=True, what=what)
        assert c.last_variant() == kernel and (prime is None or c.last_handover() > 0)
    return (what, lambda: call(8), lambda: call(64), *_tensors([out["_buf"]]), check)


CASES = {
    "det": _det, "hand": _hand, "fit": _fit, "rect_stage": _rect,
    "quad_ws and lv": lambda c, refs: _track(c, 7, "the quad kernel's workspace"),
    # every feature leaves the four-features-per-wave kernel after three iterations: the continuation buffers are in use
    "susp": lambda c, refs: _track(c, 5, "the continuation buffers", prime=7),
}


@pytest.mark.parametrize("name", list(CASES))
def test_a_buffer_under_a_graph_does_not_move(built, refs, monkeypatch, name):
    if name == "susp":
        monkeypatch.setenv("PAGK_QUAD_BUDGET", "3")
        monkeypatch.setenv("PAGK_SUSPEND_LONE", "0")
    c = capi.Context(0)
    try:
        what, small, large, reset, snapshot, check = CASES[name](c, refs)

        def run(fn):
            reset()
            torch.cuda.synchronize()
            fn()
            c.sync()
            return snapshot()

        def refused(word):
            with pytest.raises(capi.PagkError) as e:
                large()
            assert e.value.code == capi.PAGK_E_ARG and word in str(e.value) and what in str(e.value), str(e.value)
        first = run(small)
        c.graph_begin()
        try:
            refused("capture")
            small()
        finally:
            gid = c.graph_end()
        assert run(lambda: c.graph_launch(gid)) == first
        refused("graph")
        assert run(lambda: c.graph_launch(gid)) == first
        c.graph_destroy(gid)
        run(large)
        check()
    finally:
        c.close()
