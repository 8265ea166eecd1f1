"""Every tracking route over pyramid depths and frame sizes, against the CPU oracle.

test_instantiations_gpu.py runs every kernel instantiation at one geometry (320 x 240, three levels, the coarsest level
larger than the largest patch).  Here the rows of tests/track_routes.py run on the shapes of tests/shape_cases.py: one
level, two, PAGK_MAX_PYRAMIDS = 8; levels smaller than the patch (every tap clamped, the `interior` test false for the
whole level), 2 x 1 and 1 x 1 levels, odd parents inside every route; a frame slot deeper than the parameters.  One case
per (route, shape); inside it the row's half patches in two modes, lean and penalty plus every solver_variant bit.

Bar: every output bit-identical to the oracle under the same alternatives; pagk_last_variant as the row and select_variant
say (a forced 7 runs 5 on a single level); the hand-over the row names; the context's error word clear after every launch.
shape_cases.check_not_vacuous asserts on the oracle's outputs alone that at least 60 of the 67 features are live and
tracked, that the two modes differ, and, on the continuation routes, that most features run past the budget."""
import pytest
import torch

from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, distributed

import route_runner as rr
import shape_cases as cases
import track_routes as tr
from util import assert_parity, needs_variant

pytestmark = pytest.mark.gpu

_MATRIX_ROUTES = [r for r in tr.ROUTES if r.test.startswith("test_instantiations_gpu.py")]


def _params(routes, values, ident):
    out = []
    for r in routes:
        marks = [needs_variant(r.needs_variant)] if r.needs_variant else []
        out += [pytest.param(r.name, v, marks=marks, id=f"{r.name}-{ident(v)}") for v in values]
    return out


def _env(r, levels):
    """The row's environment; the continuation routes' budget follows the depth (shape_cases.budget)."""
    return tuple((var, str(cases.budget(levels)) if (var == "PAGK_QUAD_BUDGET" and r.handover) else value) for var, value in r.env)


def _case(r, shape, h):
    levels = shape[2]
    variants = cases.expected_variants(r.name, levels)
    batch = r.entry == "track_device_batch"
    ws = cases.batch_workloads(shape, h) if batch else ()
    # a batch on a single level is not one launch: every stream runs on its own context, of which only the lead was given
    # the row's selector; the others choose by launch size (the 4-wave kernel at these sizes)
    batch_variants = ((variants[0],) * len(ws) if levels >= 2 else (variants[0],) + (0,) * (len(ws) - 1)) if batch else ()
    return rr.Case(what=f"{r.name} {cases.shape_id(shape)} h={h}", w=cases.workload(shape, h), modes=tuple(cases.MODES),
                   params=cases.params, oracle=lambda mode: cases.oracle(shape, h, mode), run_oracle=cases.run_oracle,
                   variants=variants, next_seed=0x5A00 + 16 * h + shape[0], batch=ws,
                   batch_oracles=lambda mode: cases.batch_oracles(shape, h, mode), batch_variants=batch_variants)


@pytest.mark.parametrize("name,shape", _params(_MATRIX_ROUTES, cases.SHAPES, cases.shape_id))
def test_route_on_shape(request, monkeypatch, name, shape):
    r = tr.route(name)
    for h in cases.halves(name):
        cases.check_not_vacuous(cases.workload(shape, h), cases.budget(shape[2]) if r.handover else None)
        rr.run_route(request, monkeypatch, r, _case(r, shape, h), env=_env(r, shape[2]))


@pytest.mark.parametrize("name", cases.DEEP_ROUTES)
def test_slot_deeper_than_the_parameters(monkeypatch, name):
    """pagk_track_device accepts slots with more levels than pagk_params::pyramids: the launch reads the first `pyramids`
    levels of each and gives what the oracle gives with `pyramids` levels."""
    r = tr.route(name)
    width, height, slot_levels = cases.DEEP_SLOT
    for var, value in r.env:
        monkeypatch.setenv(var, value)
    stream, dev = torch.cuda.Stream(), torch.device("cuda", 0)
    c = capi.Context(0)
    try:
        with torch.cuda.stream(stream):
            c.set_stream(stream.cuda_stream)
            c.set_kernel(r.selectors[0])
            for h in cases.halves(name):
                w = cases.deep_workload(h)
                assert w.pyramids == cases.DEEP_PARAMS < slot_levels and w.img_ref.shape == (height, width)
                cases.check_not_vacuous(w)
                c.frame_upload(0, w.img_ref, slot_levels)
                c.frame_upload(1, w.img_cur, slot_levels)
                d = rr.device_inputs(w, dev)
                for mode in cases.MODES:
                    what = f"{name} h={h} {mode}: {slot_levels}-level slots, {w.pyramids}-level parameters"
                    out = distributed.alloc_device_outputs(w.n, dev)
                    c.track_device(cases.params(w, mode), 0, 1, w.n, d[0], d[1], d[2], d[3], out)
                    stream.synchronize()
                    assert_parity(rr.outputs(out), cases.oracle_of(w, mode), w.n, exact=True, what=what)
                    rr.after_launch(c, r.handover, r.variants[0], what)
    finally:
        c.set_stream(None)
        c.close()
