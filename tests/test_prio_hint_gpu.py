"""The hint of the 4-wave kernels' issue priorities (csrc/pagk_prio.h): a feature slot whose previous launch ran more iterations than
PAGK_PRIO_HINT starts at priority 3.  s_setprio moves no arithmetic, so whatever the hints say every output is the oracle's bit for bit;
what is tested beyond that is the bookkeeping -- who writes the hints, who clears them, who moves them."""

import functools

import numpy as np
import pytest
import torch

from oracle import pagk_oracle as orc
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, distributed, runtime, synth

from util import assert_parity, params_for

pytestmark = pytest.mark.gpu

N = 40


@functools.lru_cache(maxsize=None)
def case(h):
    """A 96 x 64 pair, 3 levels, 40 features: a quarter of them near the border (clamped sampling), two that come in with status 0.
    h = 10 and h = 8 run the pipelined body, h = 5 the serial one.  The oracle's result is computed once per patch size."""
    w = synth.make_workload(f"hint_h{h}", 96, 64, N, seed=0x5EED0700 + h, half_patch=h, iterations=30, pyramids=3, edge_fraction=0.25)
    w.status_in[[3, 17]] = 0
    p = params_for(w)
    ref = orc.track(p, w.img_ref, w.img_cur, w.pt_ref, w.pt_init, w.affine, w.status_in, nthreads=4)
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return w, p, ref


def tracker(w, p):
    rt = runtime.ResidentTracker(p, device=0)
    rt.load_pair(w.img_ref, w.img_cur)
    rt.set_features(w.pt_ref, w.pt_init, w.affine, w.status_in)
    return rt


def outputs(rt, n=N):
    rt.synchronize()
    return {name: rt.out[name][:n].cpu().numpy() for name, _, _ in distributed.FIELDS}


def default_threshold():
    c = capi.Context(0)
    try:
        return c.prio_hint_threshold()
    finally:
        c.close()


@pytest.mark.parametrize("h", [10, 8, 5])
@pytest.mark.parametrize("threshold", ["0", "1", "default"])
def test_no_hint_changes_a_bit(monkeypatch, h, threshold):
    w, p, ref = case(h)
    if threshold == "default":
        monkeypatch.delenv("PAGK_PRIO_HINT", raising=False)
    else:
        monkeypatch.setenv("PAGK_PRIO_HINT", threshold)
    rt = tracker(w, p)
    try:
        assert rt.ctx.prio_hint_threshold() == (default_threshold() if threshold == "default" else int(threshold))
        rng = np.random.default_rng(h)
        for what, hints in (("all 0", np.zeros(N, np.int32)), ("all 1000", np.full(N, 1000, np.int32)),
                            ("random", rng.integers(0, 40, N).astype(np.int32)), ("exact", None)):
            if hints is None:   # what the launch before left: the features' own counts
                rt.step(mode="serial")
                rt.synchronize()
                assert np.array_equal(rt.ctx.prio_hint_get(N), ref["iters"][:N])
            else:
                rt.ctx.prio_hint_set(hints)
            rt.step(mode="serial")
            assert rt.ctx.last_variant() == 0
            assert_parity(outputs(rt), ref, N, exact=True, what=f"h = {h}, PAGK_PRIO_HINT={threshold}, hints {what}")
    finally:
        rt.close()


@functools.lru_cache(maxsize=None)
def crowded_case(h):
    """The same small pair with 600 features: more workgroups than the device has CUs, so that there is somebody to outrank.  A launch
    of a workgroup per CU or fewer stores its counts but is handed threshold 0 (pagk_hip.hip, launch_track), so the 40-feature cases
    above never load a hint: THIS is where a workgroup reads its entry and runs boosted.  h = 10 and h = 8 are the pipelined body's
    two-round instantiations; h = 12 (three sampling rounds) is the serial body with the rule on."""
    w = synth.make_workload(f"hint_crowded_h{h}", 96, 64, 600, seed=0x5EED0770 + h, half_patch=h, iterations=30, pyramids=3,
                            edge_fraction=0.25)
    w.status_in[[3, 17, 599]] = 0
    p = params_for(w)
    ref = orc.track(p, w.img_ref, w.img_cur, w.pt_ref, w.pt_init, w.affine, w.status_in, nthreads=8)
    return w, p, ref


@pytest.mark.parametrize("h", [10, 8, 12])
@pytest.mark.parametrize("threshold", ["0", "1", "default"])
def test_no_hint_changes_a_bit_where_workgroups_share_a_cu(monkeypatch, h, threshold):
    w, p, ref = crowded_case(h)
    assert ref["iters"][:w.n].max() > 14, "the case needs features past the default threshold"
    if threshold == "default":
        monkeypatch.delenv("PAGK_PRIO_HINT", raising=False)
    else:
        monkeypatch.setenv("PAGK_PRIO_HINT", threshold)
    rt = tracker(w, p)
    try:
        rng = np.random.default_rng(5)
        half = np.where(np.arange(w.n) % 2 == 0, 1000, 0).astype(np.int32)   # every other workgroup boosted
        for what, hints in (("all 0", np.zeros(w.n, np.int32)), ("all 1000", np.full(w.n, 1000, np.int32)), ("every other one", half),
                            ("random", rng.integers(0, 40, w.n).astype(np.int32)), ("exact", None)):
            if hints is not None:
                rt.ctx.prio_hint_set(hints)
            rt.step(mode="serial")
            assert rt.ctx.last_variant() == 0
            assert_parity(outputs(rt, w.n), ref, w.n, exact=True, what=f"600 features, h = {h}, PAGK_PRIO_HINT={threshold}, hints {what}")
            assert np.array_equal(rt.ctx.prio_hint_get(w.n), ref["iters"][:w.n])
    finally:
        rt.close()


@pytest.mark.parametrize("h", [10, 5])
def test_a_launch_leaves_its_iteration_counts(h):
    w, p, ref = case(h)
    rt = tracker(w, p)
    try:
        rt.ctx.prio_hint_set(np.full(N + 8, 777, np.int32))
        rt.step(mode="serial")
        got = outputs(rt)
        hints = rt.ctx.prio_hint_get(N + 8)
        assert np.array_equal(hints[:N], got["iters"]) and np.array_equal(got["iters"], ref["iters"][:N])
        # status 0 in (the two forced ones, and whatever the gyro prediction threw out near the border): no forecast; everyone else ran
        assert not w.status_in[3] and not w.status_in[17] and w.status_in.sum() >= N // 2
        assert np.array_equal(hints[:N] == 0, w.status_in == 0)
        assert np.all(hints[N:] == 777)                                             # slots past the launch: untouched
    finally:
        rt.close()


def test_replays_feed_each_other():
    w, p, ref = case(10)
    rt = tracker(w, p)
    try:
        seen = []
        for k in range(3):
            rt.step(mode="graph")
            assert rt.mode_used == "graph"
            seen.append(outputs(rt))
            assert np.array_equal(rt.ctx.prio_hint_get(N), seen[-1]["iters"]), f"hints after replay {k + 1}"
        assert_parity(seen[0], ref, N, exact=True, what="replay 1")
        for k in (1, 2):
            for name in seen[0]:
                assert seen[k][name].tobytes() == seen[0][name].tobytes(), f"replay {k + 1}: {name}"
    finally:
        rt.close()


def test_installing_features_clears_the_hints():
    w, p, _ = case(10)
    rt = tracker(w, p)
    try:
        rt.step(mode="serial")
        rt.synchronize()
        assert rt.ctx.prio_hint_get(N).max() > 0
        rt.set_features(w.pt_ref, w.pt_init, w.affine, w.status_in)       # same shape: the arrays are rewritten in place
        assert not rt.ctx.prio_hint_get(N).any()
        rt.ctx.prio_hint_set(np.full(N, 1000, np.int32))
        rt.set_features(w.pt_ref[:32], w.pt_init[:32], w.affine[:32], w.status_in[:32])   # another shape: new arrays
        assert not rt.ctx.prio_hint_get(N).any()
    finally:
        rt.close()
    # the host-buffer call installs its own arrays: whatever the slots held, within the launch and past it, is forgotten, and the
    # call keeps no counts of its own (its features are new in every call)
    c = capi.Context(0)
    try:
        c.prio_hint_set(np.full(N + 8, 1000, np.int32))
        c.track(p, w.img_ref, w.img_cur, w.pt_ref, w.pt_init, w.affine, w.status_in)
        assert not c.prio_hint_get(N + 8).any()
    finally:
        c.close()


def test_the_sharded_host_call_clears_the_hints_of_its_rank():
    w, p, ref = case(10)
    g = capi.Multi([0])
    try:
        c = g.ctx(0)
        c.prio_hint_set(np.full(N + 8, 1000, np.int32))
        got = g.track_sharded(p, w.img_ref, w.img_cur, w.pt_ref, w.pt_init, w.affine, w.status_in)
        assert_parity(got, ref, N, exact=True, what="pagk_track_sharded")
        assert not c.prio_hint_get(N + 8).any()
    finally:
        g.close()


def test_the_handover_moves_a_survivors_hint():
    cap, W, H = 64, 640, 480
    c = capi.Context(0)
    stream = torch.cuda.Stream()
    try:
        p = capi.make_params(camera=synth.D435I)
        rng = np.random.default_rng(11)
        status = np.zeros(cap, np.uint8)
        status[[0, 2, 3, 9, 10, 31, 40, 41, 63]] = 1          # the survivors, in slot order
        un = np.stack([40 + rng.random(cap) * 560, 40 + rng.random(cap) * 400], axis=1).astype(np.float32)
        cand = np.stack([20 + rng.random(30) * 600, 20 + rng.random(30) * 440], axis=1).astype(np.float32)
        hints = (100 + np.arange(cap)).astype(np.int32)
        with torch.cuda.stream(stream):
            c.set_stream(stream.cuda_stream)
            dev = lambda a: torch.from_numpy(a).to("cuda:0")   # noqa: E731
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda:0")   # noqa: E731
            d_st, d_un, d_cand, d_nc = dev(status), dev(un), dev(cand), dev(np.array([30], np.int32))
            outs = [z((cap, 2), torch.float32) for _ in range(3)]
            d_idx, d_live, d_state = z(cap, torch.int32), z(cap, torch.uint8), z(8, torch.int32)
            c.prio_hint_set(hints)
            c.frame_handover_device(p, W, H, cap, cap, float(cap), d_st, d_un, d_un, 30, d_nc, d_cand, outs[0], outs[1], outs[2],
                                    d_idx, d_live, None, d_state)
            stream.synchronize()
        state, idx = d_state.cpu().numpy(), d_idx.cpu().numpy()
        m = int(status.sum())
        assert state[2] == m and state[3] > 0, "the pattern needs survivors and topped-up features"
        got = c.prio_hint_get(cap)
        assert np.array_equal(idx[:m], np.flatnonzero(status))
        assert np.array_equal(got[:m], hints[idx[:m]]), "a survivor's hint sits at its new index"
        assert not got[m:].any(), "new and unused slots carry no hint"
    finally:
        c.close()


def test_a_sharded_tracker_keeps_the_hints_of_its_block(monkeypatch):
    import socket
    import torch.distributed as dist
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    distributed.FORCE_COLLECTIVE = True
    try:
        w, p, ref = case(10)
        rt = tracker(w, p)
        res = rt.step()
        assert isinstance(res, distributed.Gathered)
        rt.synchronize()
        torch.cuda.synchronize()
        assert_parity(distributed.to_numpy(res), ref, N, exact=True, what="gathered")
        hints = rt.ctx.prio_hint_get(N + 24)
        assert np.array_equal(hints[:rt.hi - rt.lo], ref["iters"][rt.lo:rt.hi]) and not hints[rt.hi - rt.lo:].any()
        rt.close()
    finally:
        distributed.FORCE_COLLECTIVE = False
        dist.destroy_process_group()
