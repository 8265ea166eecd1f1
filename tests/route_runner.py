"""Runs one row of tests/track_routes.py on one workload and holds every launch against the CPU oracle: shared by the
instantiation matrix (test_instantiations_gpu.py: every kernel at one geometry) and the shape matrix (test_shapes_gpu.py:
every route over pyramid depths and frame sizes).

A `Case` is what differs between the two: the workload(s), the parameter modes, where the oracle's results come from and
which variant each selector of the row is expected to run.  The bar is the same: every output bit-identical to the oracle
under the same alternatives, the variant and the hand-over the row names, the context's error word clear afterwards."""
import dataclasses
import typing

import numpy as np
import torch

from oracle import pagk_oracle as orc
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, distributed


@dataclasses.dataclass(frozen=True)
class Case:
    what: str                       # prefix of every message
    w: typing.Any                   # the workload (synth.Workload); its arrays are shared and read-only
    modes: tuple                    # names of the parameter modes
    params: typing.Callable         # (workload, mode) -> pagk_params
    oracle: typing.Callable         # mode -> the oracle's outputs on `w`
    run_oracle: typing.Callable     # (workload, mode, pair=None) -> the oracle's outputs on another workload / image pair
    variants: tuple                 # pagk_last_variant expected per selector of the row
    next_seed: int = 0              # fused route: seed of the next frames (one per mode)
    batch: tuple = ()               # batch route: the three streams' workloads (`w` is one of them)
    batch_oracles: typing.Callable = None   # mode -> the oracle's outputs per stream
    batch_variants: tuple = ()      # pagk_last_variant expected per stream


def after_launch(c, handover, variant, what):
    assert c.last_variant() == variant, f"{what}: ran variant {c.last_variant()}, expected {variant}"
    handed = c.last_handover()
    assert (handed > 0) == handover, f"{what}: {handed} features handed over, the row says hand-over = {handover}"
    c.check_launch()   # raises when a wave of the launch gave up a wait: the error word must be clear


def outputs(out):
    return {name: out[name].cpu().numpy() for name, _, _ in distributed.FIELDS}


def device_inputs(w, dev):
    # (copies: the shared arrays are read-only)
    return [torch.from_numpy(x.copy()).to(dev) for x in (w.pt_ref, w.pt_init, w.affine, w.status_in)]


def run_track(c, r, case):
    """Host-buffer entry point: every selector of the row x every mode."""
    from util import assert_parity
    w = case.w
    for selector, variant in zip(r.selectors, case.variants):
        for mode in case.modes:
            what = f"{case.what} kernel {selector} {mode}"
            c.set_kernel(selector)
            try:
                got = c.track(case.params(w, mode), w.img_ref, w.img_cur, w.pt_ref, w.pt_init, w.affine, w.status_in)
            finally:
                c.set_kernel(0)
            assert_parity(got, case.oracle(mode), w.n, exact=True, what=what)
            after_launch(c, r.handover, variant, what)


def run_fused(r, case):
    """pagk_track_device_fused: the tracked outputs, and every level of the slot that the same call built from another
    frame of the workload's size and depth (a new one per mode, so that no mode can pass on the levels the one before it
    left); then the pair (current, next) on that slot."""
    from util import assert_parity
    w = case.w
    height, width = w.img_ref.shape
    stream, dev = torch.cuda.Stream(), torch.device("cuda", 0)
    c = capi.Context(0)
    try:
        with torch.cuda.stream(stream):
            c.set_stream(stream.cuda_stream)
            c.frame_upload(0, w.img_ref, w.pyramids)
            c.frame_upload(1, w.img_cur, w.pyramids)
            d = device_inputs(w, dev)
            for k, mode in enumerate(case.modes):
                what = f"{case.what} {mode}"
                nxt = np.random.default_rng(case.next_seed + k).integers(0, 256, (height, width), dtype=np.uint8)
                d_next = torch.from_numpy(nxt).to(dev)
                out = distributed.alloc_device_outputs(w.n, dev)
                c.track_device_fused(case.params(w, mode), 0, 1, w.n, d[0], d[1], d[2], d[3], out, 2, d_next.data_ptr(),
                                     width, height, width, w.pyramids)
                stream.synchronize()
                assert_parity(outputs(out), case.oracle(mode), w.n, exact=True, what=what)
                lvl = nxt
                for l in range(1, w.pyramids):   # (level 0 of a slot is the caller's own image)
                    lvl = orc.pyr_down(lvl)
                    assert np.array_equal(c.frame_download_level(2, l, width, height), lvl), f"{what}: next-frame pyramid level {l}"
                after_launch(c, r.handover, case.variants[0], what)
                # ... and the slot is usable as the next pair's current frame (its level 0 taps included)
                out = distributed.alloc_device_outputs(w.n, dev)
                c.track_device(case.params(w, mode), 1, 2, w.n, d[0], d[1], d[2], d[3], out)
                stream.synchronize()
                ref = case.run_oracle(w, mode, pair=(w.img_cur, nxt))
                assert_parity(outputs(out), ref, w.n, exact=True, what=f"{what}: pair (cur, next) on the fused-built slot")
                after_launch(c, r.handover, case.variants[0], what)
    finally:
        c.set_stream(None)
        c.close()


def run_batch(r, case):
    """pagk_track_device_batch: the streams of case.batch as one call on the lead context; every stream's outputs against
    that stream's own oracle run."""
    from util import assert_parity
    ws = case.batch
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
            ctxs[0].set_kernel(r.selectors[0])
            d = [device_inputs(w, dev) for w in ws]
            for mode in case.modes:
                outs = [distributed.alloc_device_outputs(w.n, dev) for w in ws]
                capi.Context.track_device_batch(ctxs, case.params(ws[0], mode), [0] * len(ws), [1] * len(ws), [w.n for w in ws],
                                                [x[0] for x in d], [x[1] for x in d], [x[2] for x in d], [x[3] for x in d], outs)
                stream.synchronize()
                for j, (w, out, ref) in enumerate(zip(ws, outs, case.batch_oracles(mode))):
                    what = f"{case.what} {mode}, stream {j} ({w.n} features)"
                    assert_parity(outputs(out), ref, w.n, exact=True, what=what)
                    after_launch(ctxs[j], r.handover, case.batch_variants[j], what)
    finally:
        for c in ctxs:
            c.set_stream(None)
            c.close()


def run_route(request, monkeypatch, r, case, env=None):
    """The row `r` on `case`, in a context created under the row's environment (`env` replaces r.env)."""
    env = r.env if env is None else env
    for var, value in env:
        monkeypatch.setenv(var, value)
    if r.entry == "track_device_fused":
        run_fused(r, case)
    elif r.entry == "track_device_batch":
        run_batch(r, case)
    elif env:   # a context of its own, created under the row's environment
        c = capi.Context(0)
        try:
            run_track(c, r, case)
        finally:
            c.close()
    else:
        run_track(request.getfixturevalue("ctx"), r, case)
