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

import pytest

from oracle import pagk_oracle as orc
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi

import instantiation_cases as cases
import route_runner as rr
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


def _case(r, h):
    """The row's case at half patch `h`: the matrix's one workload, its four modes, the variants the row names."""
    ws = cases.batch_workloads(h) if r.entry == "track_device_batch" else ()
    return rr.Case(what=f"{r.name} h={h}", w=cases.workload(h), modes=tuple(cases.MODES), params=cases.params,
                   oracle=lambda mode: cases.oracle(h, mode), run_oracle=cases.run_oracle, variants=r.variants,
                   next_seed=16 * h, batch=ws, batch_oracles=lambda mode: cases.batch_oracles(h, mode),
                   batch_variants=(r.variants[0],) * len(ws))


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
    rr.run_route(request, monkeypatch, r, _case(r, h))

