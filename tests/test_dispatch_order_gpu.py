"""The dispatch order of the 4-wave kernels (csrc/pagk_order.h): workgroup b runs the feature with the b-th largest hint.  The order
moves no arithmetic, so whatever the hints say every output is the oracle's bit for bit and equals the launch in index order; what is
tested beyond that is that the array the device builds is the permutation the rule promises, and that a launch is handed it only when
the host's conservative rule allows."""

import functools

import numpy as np
import pytest
import torch

from oracle import pagk_oracle as orc
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, distributed, runtime, synth

from util import assert_parity, params_for

pytestmark = pytest.mark.gpu

KEY_MAX = 127
INT32_MAX, INT32_MIN = 2**31 - 1, -2**31
DEAD = (3, 17, 255, 256, 299, 650, 699)   # features that come in with status 0: they must still be written (and leave hint 0)


def restated(hints):
    """The rule of csrc/pagk_order.h: a stable sort of the hints clamped to [0, 127], descending, ties in index order."""
    return np.argsort(-np.clip(np.asarray(hints, np.int64), 0, KEY_MAX), kind="stable").astype(np.int32)


@functools.lru_cache(maxsize=None)
def case(h, penalty, frames=1):
    """A 160 x 120 pair, 3 levels, 700 features (a launch of three layers on 256 CUs; its first 300 are the two-layer launch), a
    quarter of them near the border, seven that come in with status 0.  h = 10: the headline instantiation (pipelined body), h = 7:
    the one-round body at five workgroups per CU, penalty: the generic instantiation.  The oracle runs once per case and frame:
    frame 0 is the pair's own current image, frames 1 and 2 (the graph test) are that image shifted and the reference image itself."""
    w = synth.make_workload(f"order_h{h}_{int(penalty)}", 160, 120, 700, seed=0x5EED0D00 + 2 * h + int(penalty), half_patch=h,
                            iterations=30, pyramids=3, edge_fraction=0.25, penalty=penalty)
    w.status_in[list(DEAD)] = 0
    p = params_for(w)
    curs = [w.img_cur, np.ascontiguousarray(np.roll(w.img_cur, (1, 2), (0, 1))), w.img_ref.copy()][:frames]
    refs = []
    for cur in curs:
        ref = orc.track(p, w.img_ref, cur, w.pt_ref, w.pt_init, w.affine, w.status_in, nthreads=8)
        for a in ref.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        refs.append(ref)
    return w, p, curs, refs


def tracker(w, p, n):
    rt = runtime.ResidentTracker(p, device=0)
    rt.load_pair(w.img_ref, w.img_cur)
    rt.set_features(w.pt_ref[:n], w.pt_init[:n], w.affine[:n], w.status_in[:n])
    return rt


def outputs(rt, n):
    rt.synchronize()
    return {name: rt.out[name][:n].cpu().numpy() for name, _, _ in distributed.FIELDS}


def hint_sets(n, own):
    rng = np.random.default_rng(n)
    anything = rng.integers(INT32_MIN, INT32_MAX, n, endpoint=True).astype(np.int32)
    anything[::7] = INT32_MAX
    anything[3::11] = -5
    anything[5::13] = rng.integers(0, 40, anything[5::13].shape[0])
    # (None: what the launch before left -- the features' own counts, two launches in a row)
    return (("all zero", np.zeros(n, np.int32)), ("own counts", None), ("own counts again", None), ("any int32", anything),
            ("all equal", np.full(n, 17, np.int32)))


def run_sequence(w, p, ref, n, on):
    """One resident tracker through the five hint sets, pyramid and tracking launch issued one by one so that the order can be read
    between them.  Returns what every launch wrote."""
    rt = tracker(w, p, n)
    seen = []
    try:
        assert rt.ctx.dispatch_order_enabled() == on
        own = ref["iters"][:n]
        for what, hints in hint_sets(n, own):
            if hints is None:
                hints = own
                assert np.array_equal(rt.ctx.prio_hint_get(n), own), what
            else:
                rt.ctx.prio_hint_set(hints)
            with torch.cuda.stream(rt.main):
                rt.rebuild_current_pyramid(1)        # ... whose leading workgroup sorts the hints
                order, in_force = rt.ctx.dispatch_order_get(n)
                rt.track_shard(1)
            assert rt.ctx.last_variant() == 0
            assert np.array_equal(np.sort(order), np.arange(n)), f"{what}: the order is not a permutation of [0, {n})"
            if on:
                assert in_force, what
                assert np.array_equal(order, restated(hints)), f"{what}: not the stable descending order of the clamped hints"
            else:
                assert not in_force and np.array_equal(order, np.arange(n)), what
            got = outputs(rt, n)
            assert_parity(got, ref, n, exact=True, what=f"{n} features, order {'on' if on else 'off'}, hints {what}")
            assert np.array_equal(got["iters"], own) and np.array_equal(rt.ctx.prio_hint_get(n), own), what
            assert not got["status"][[i for i in DEAD if i < n]].any() and not own[[i for i in DEAD if i < n]].any()
            assert not rt.ctx.dispatch_order_get(n)[1], f"{what}: the launch rewrote the hints, its order is history"
            seen.append(got)
    finally:
        rt.close()
    return seen


@pytest.mark.parametrize("n", [300, 700])
@pytest.mark.parametrize("h,penalty", [(10, False), (7, False), (10, True)])
def test_no_order_changes_a_bit(monkeypatch, h, penalty, n):
    w, p, _, (ref,) = case(h, penalty)
    assert ref["iters"][:n].max() > 14 and len(set(ref["iters"][:n].tolist())) > 8, "the case needs a spread of counts to sort"
    monkeypatch.setenv("PAGK_DISPATCH_ORDER", "0")
    off = run_sequence(w, p, ref, n, on=False)
    monkeypatch.delenv("PAGK_DISPATCH_ORDER")
    on = run_sequence(w, p, ref, n, on=True)
    for k, (a, b) in enumerate(zip(on, off)):
        for name in a:
            assert a[name].tobytes() == b[name].tobytes(), f"hint set {k}: {name} differs between order on and off"


def test_replays_rebuild_the_order_from_the_counts_before_them():
    n = 700
    w, p, curs, refs = case(10, False, frames=3)
    rt = tracker(w, p, n)
    try:
        # the first step's warm-up launch tracks frame 0 directly, so replay 1 sorts frame 0's counts; replay k + 1 those of replay k
        before = [refs[0]["iters"], refs[0]["iters"], refs[1]["iters"]]
        assert not np.array_equal(restated(before[1]), restated(before[2])), "the frames must change the order"
        for k in range(3):
            rt.set_current_image(curs[k])
            rt.step(mode="graph")
            assert rt.mode_used == "graph"
            got = outputs(rt, n)
            assert_parity(got, refs[k], n, exact=True, what=f"replay {k + 1}")
            order, in_force = rt.ctx.dispatch_order_get(n)
            assert np.array_equal(order, restated(before[k][:n])), f"replay {k + 1}: the order its tracking node ran"
            assert not in_force   # (between replays the host knows of no build: a direct launch here would run in index order)
            assert np.array_equal(rt.ctx.prio_hint_get(n), refs[k]["iters"][:n])
    finally:
        rt.close()


def test_a_replay_on_another_stream_than_the_arrays_waits_and_stays_right():
    """The captured step holds the order's build and its reader.  While the array is bound to the stream of the last replay, a pyramid on
    another stream builds no order, and a replay there waits for the device first: the result is the oracle's either way."""
    n = 700
    w, p, _, (ref,) = case(10, False)
    rt = tracker(w, p, n)
    try:
        for _ in range(2):
            rt.step(mode="graph")
        assert rt.mode_used == "graph"
        assert_parity(outputs(rt, n), ref, n, exact=True, what="replays on the capture's stream")   # (torch's sync: the library saw none)
        gid = rt._graphs["graph"][0]
        rt.ctx.graph_launch(gid)                          # ... in flight on `main`
        rt.ctx.set_stream(rt.side.cuda_stream)
        try:
            rt.rebuild_current_pyramid(2)                 # on `side`: no order workgroup under the replay's tracking node
            rt.ctx.graph_launch(gid)                      # the same graph on `side`: waits for `main`'s replay first
            assert_parity(outputs(rt, n), ref, n, exact=True, what="replay on another stream")
            order, _ = rt.ctx.dispatch_order_get(n)
            assert np.array_equal(order, restated(ref["iters"][:n]))
            assert np.array_equal(rt.ctx.prio_hint_get(n), ref["iters"][:n])
        finally:
            rt.ctx.set_stream(rt.main.cuda_stream)
        rt.step(mode="graph")
        assert_parity(outputs(rt, n), ref, n, exact=True, what="back on the capture's stream")
    finally:
        rt.close()


def test_a_host_buffer_call_runs_in_index_order():
    n = 700
    w, p, _, (ref,) = case(10, False)
    rt = tracker(w, p, n)
    try:
        for _ in range(2):
            rt.step(mode="serial")
        assert_parity(outputs(rt, n), ref, n, exact=True, what="resident sequence")
        with torch.cuda.stream(rt.main):
            rt.rebuild_current_pyramid(1)
        assert rt.ctx.dispatch_order_get(n)[1]          # an order is built and waiting ...
        got = rt.ctx.track(p, w.img_ref, w.img_cur, w.pt_ref, w.pt_init, w.affine, w.status_in)   # ... and the host arrays are new features
        assert_parity(got, ref, n, exact=True, what="host-buffer call behind a resident sequence")
        assert not rt.ctx.dispatch_order_get(n)[1]
        assert not rt.ctx.prio_hint_get(n).any()
        with torch.cuda.stream(rt.main):
            rt.rebuild_current_pyramid(1)               # zeroed hints: nothing to sort, nothing in force
        assert not rt.ctx.dispatch_order_get(n)[1]
        rt.step(mode="serial")
        assert_parity(outputs(rt, n), ref, n, exact=True, what="resident launch behind the host-buffer call")
    finally:
        rt.close()


def test_the_five_per_cu_build_follows_the_order_too():
    """1025-1280 features at h = 10 run k_track_block5 (one round at five workgroups per CU): it reads the order like the others."""
    n = 1100
    w = synth.make_workload("order_block5", 160, 120, n, seed=0x5EED0D55, half_patch=10, iterations=30, pyramids=3, edge_fraction=0.25)
    w.status_in[[3, 1099]] = 0
    p = params_for(w)
    ref = orc.track(p, w.img_ref, w.img_cur, w.pt_ref, w.pt_init, w.affine, w.status_in, nthreads=8)
    rt = tracker(w, p, n)
    try:
        hints = np.random.default_rng(5).integers(0, 60, n).astype(np.int32)
        rt.ctx.prio_hint_set(hints)
        with torch.cuda.stream(rt.main):
            rt.rebuild_current_pyramid(1)
            order, in_force = rt.ctx.dispatch_order_get(n)
            rt.track_shard(1)
        assert in_force and np.array_equal(order, restated(hints))
        assert_parity(outputs(rt, n), ref, n, exact=True, what="1100 features, five workgroups per CU")
    finally:
        rt.close()
