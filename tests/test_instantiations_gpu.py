"""Every tracking-kernel instantiation of the build against the CPU oracle, generic builds included.

One case per (route, half patch) of tests/track_routes.py; inside each case four parameter modes: lean, penalty only,
every solver_variant bit only, both.  The last three run the generic instantiations (the only ones a host built against
another Eigen, or a tracker with regularization_penalty, ever runs).  Bar: every output bit-identical to the oracle with
the same alternatives; the variant and the hand-over the row names; the context's error word clear afterwards.

The workload (instantiation_cases.py) is the smallest at which these kernels can still go wrong: 67 features (no
multiple of 4, more than one wave of the thread kernel) on 320 x 240 with three levels, 30 % of them at the image edge
(the clamped samplers), a few switched off on input, and two that start on their reference position (0 / 0 under the
penalty: a NaN row beside healthy rows of the same quad wave).  check_not_vacuous asserts on the oracle's outputs that
the generic modes differ from the lean one, so a generic kernel that ignored its parameters would fail here.

The rows force their variant with pagk_set_kernel; test_auto_selection_reaches_each_variant leaves the selector at 0 and
lets the launch size decide, on the same workload."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import pagk_oracle as orc
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, distributed

import instantiation_cases as cases
import track_routes as tr
from util import assert_parity, needs_variant

pytestmark = pytest.mark.gpu


def _cases():
    out = []
    for r in tr.ROUTES:
        if not r.test.startswith("test_instantiations_gpu.py"):
            continue
        marks = [needs_variant(r.needs_variant)] if r.needs_variant else []
        out += [pytest.param(r.name, h, marks=marks, id=f"{r.name}-h{h}") for h in r.halves]
    return out


def _after_launch(c, r, variant, what):
    assert c.last_variant() == variant, f"{what}: ran variant {c.last_variant()}, the row names {variant}"
    handed = c.last_handover()
    assert (handed > 0) == r.handover, f"{what}: {handed} features handed over, the row says hand-over = {r.handover}"
    c.check_launch()   # raises when a wave of the launch gave up a wait: the error word must be clear


def _run_track(c, r, h):
    """Host-buffer entry point: every selector of the row x every mode."""
    w = cases.workload(h)
    for selector, variant in zip(r.selectors, r.variants):
        for mode in cases.MODES:
            what = f"{r.name} h={h} kernel {selector} {mode}"
            c.set_kernel(selector)
            try:
                got = c.track(cases.params(w, mode), w.img_ref, w.img_cur, w.pt_ref, w.pt_init, w.affine, w.status_in)
            finally:
                c.set_kernel(0)
            assert_parity(got, cases.oracle(h, mode), w.n, exact=True, what=what)
            _after_launch(c, r, variant, what)


def _device_inputs(w, dev):
    # (copies: the shared arrays are read-only)
    return [torch.from_numpy(x.copy()).to(dev) for x in (w.pt_ref, w.pt_init, w.affine, w.status_in)]


def _run_fused(r, h):
    """pagk_track_device_fused: the tracked outputs, and every level of the slot that the same launch built from another
    frame (a new one per mode, so that no mode can pass on the levels the one before it left)."""
    w = cases.workload(h)
    stream, dev = torch.cuda.Stream(), torch.device("cuda", 0)
    c = capi.Context(0)
    try:
        with torch.cuda.stream(stream):
            c.set_stream(stream.cuda_stream)
            c.frame_upload(0, w.img_ref, cases.PYRAMIDS)
            c.frame_upload(1, w.img_cur, cases.PYRAMIDS)
            d = _device_inputs(w, dev)
            for k, mode in enumerate(cases.MODES):
                what = f"{r.name} h={h} {mode}"
                nxt = np.random.default_rng(16 * h + k).integers(0, 256, (cases.HEIGHT, cases.WIDTH), dtype=np.uint8)
                d_next = torch.from_numpy(nxt).to(dev)
                out = distributed.alloc_device_outputs(w.n, dev)
                c.track_device_fused(cases.params(w, mode), 0, 1, w.n, d[0], d[1], d[2], d[3], out, 2, d_next.data_ptr(),
                                     cases.WIDTH, cases.HEIGHT, cases.WIDTH, cases.PYRAMIDS)
                stream.synchronize()
                got = {name: out[name].cpu().numpy() for name, _, _ in distributed.FIELDS}
                assert_parity(got, cases.oracle(h, mode), w.n, exact=True, what=what)
                lvl = nxt
                for l in range(1, cases.PYRAMIDS):   # (level 0 of a slot is the caller's own image)
                    lvl = orc.pyr_down(lvl)
                    assert np.array_equal(c.frame_download_level(2, l, cases.WIDTH, cases.HEIGHT), lvl), f"{what}: next-frame pyramid level {l}"
                _after_launch(c, r, r.variants[0], what)
                # ... and the slot is usable as the next pair's current frame (its level 0 taps included)
                out = distributed.alloc_device_outputs(w.n, dev)
                c.track_device(cases.params(w, mode), 1, 2, w.n, d[0], d[1], d[2], d[3], out)
                stream.synchronize()
                ref = cases.run_oracle(w, mode, pair=(w.img_cur, nxt))
                got = {name: out[name].cpu().numpy() for name, _, _ in distributed.FIELDS}
                assert_parity(got, ref, w.n, exact=True, what=f"{what}: pair (cur, next) on the fused-built slot")
                _after_launch(c, r, r.variants[0], what)
    finally:
        c.set_stream(None)
        c.close()


def _run_batch(r, h):
    """pagk_track_device_batch: three streams (1, 67 and 30 features, two frame sizes) as one launch of the lead context;
    every stream's outputs against that stream's own oracle run."""
    ws = cases.batch_workloads(h)
    stream, dev = torch.cuda.Stream(), torch.device("cuda", 0)
    ctxs = []
    try:
        with torch.cuda.stream(stream):
            for w in ws:
                c = capi.Context(0)
                ctxs.append(c)
                c.set_stream(stream.cuda_stream)
                c.frame_upload(0, w.img_ref, cases.PYRAMIDS)
                c.frame_upload(1, w.img_cur, cases.PYRAMIDS)
            ctxs[0].set_kernel(r.selectors[0])
            d = [_device_inputs(w, dev) for w in ws]
            for mode in cases.MODES:
                outs = [distributed.alloc_device_outputs(w.n, dev) for w in ws]
                capi.Context.track_device_batch(ctxs, cases.params(ws[0], mode), [0] * 3, [1] * 3, [w.n for w in ws],
                                                [x[0] for x in d], [x[1] for x in d], [x[2] for x in d], [x[3] for x in d], outs)
                stream.synchronize()
                for j, (w, out, ref) in enumerate(zip(ws, outs, cases.batch_oracles(h, mode))):
                    what = f"{r.name} h={h} {mode}, stream {j} ({w.n} features)"
                    got = {name: out[name].cpu().numpy() for name, _, _ in distributed.FIELDS}
                    assert_parity(got, ref, w.n, exact=True, what=what)
                    _after_launch(ctxs[j], r, r.variants[0], what)
    finally:
        for c in ctxs:
            c.set_stream(None)
            c.close()


def test_auto_selection_reaches_each_variant(monkeypatch):
    """Selector 0 on the matrix's own workload (h = 5, lean), under thresholds small enough for 67 features to cross:
    the launch size, pagk_set_concurrency and calculate_ncc pick variants 0, 3, 7, 5 and 3.  Every launch bit-exact
    against the oracle run on the same features."""
    for var, value in (("PAGK_WAVE_MIN", "20"), ("PAGK_QUAD_MIN", "30"), ("PAGK_LEVELS_MIN", "40"), ("PAGK_QUAD_BUDGET", "0")):
        monkeypatch.setenv(var, value)
    w = cases.workload(5)

    def first(n):
        return w if n == w.n else dataclasses.replace(w, pt_ref=w.pt_ref[:n], pt_init=w.pt_init[:n], affine=w.affine[:n],
                                                      status_in=w.status_in[:n], pt_true=w.pt_true[:n])
    c = capi.Context(0)
    try:
        # (features, contexts sharing the device, calculate_ncc) -> variant
        for n, streams, ncc, variant in ((10, 1, 0, 0), (25, 1, 0, 3), (67, 1, 0, 7), (67, 2, 0, 5), (67, 1, 1, 3)):
            what = f"auto selection: {n} features, concurrency {streams}, ncc {ncc}"
            wn, p = first(n), cases.params(w, "lean")
            p.calculate_ncc = ncc
            ref = cases.oracle(5, "lean") if (n, ncc) == (w.n, 0) else orc.track(
                p, wn.img_ref, wn.img_cur, wn.pt_ref, wn.pt_init, wn.affine, wn.status_in, nthreads=8)
            c.set_concurrency(streams)
            got = c.track(p, wn.img_ref, wn.img_cur, wn.pt_ref, wn.pt_init, wn.affine, wn.status_in)
            assert_parity(got, ref, n, exact=True, what=what)
            assert c.last_variant() == variant, f"{what}: ran variant {c.last_variant()}, expected {variant}"
            assert c.last_handover() == 0, what
            c.check_launch()
    finally:
        c.close()


@pytest.mark.parametrize("name,h", _cases())
def test_route(request, monkeypatch, name, h):
    r = tr.route(name)
    cases.check_not_vacuous(h, continuation=r.handover)
    for var, value in r.env:
        monkeypatch.setenv(var, value)
    if r.entry == "track_device_fused":
        _run_fused(r, h)
    elif r.entry == "track_device_batch":
        _run_batch(r, h)
    elif r.env:   # a context of its own, created under the row's environment
        c = capi.Context(0)
        try:
            _run_track(c, r, h)
        finally:
            c.close()
    else:
        _run_track(request.getfixturevalue("ctx"), r, h)

