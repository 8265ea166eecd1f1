"""The HIP path against the reference's OWN text, compiled: every fixture of tests/golden/ref_shim/ -- the six outputs that the
reference's src/patch_match.cpp and src/utils.cpp wrote, built unchanged against the project's stand-ins (see
tests/test_reference_build_cpu.py and oracle/README.md) -- through pagk_track and through every row of tests/track_routes.py
whose constraints admit the case's parameters.  Bar: all six outputs bit-identical to the reference's, NaN patterns included;
the variant and the hand-over the row names; the context's error word clear.

Reads the fixtures only: neither the reference's sources nor oracle/_ref/ are touched here.

Which rows admit a case (admits() below, from csrc/pagk_select.h and the rows' own comments):
  * the row is built for the case's half patch, and it is parity-exact (the relaxed-order experiment is not);
  * rows that force four features per wave (selectors 5 and 7, the batch included) have no NCC epilogue: with calculate_ncc
    such a launch runs variant 3, which the `wave` row covers;
  * the continuation rows need a feature that iterates past their budget of 3: not on the constant-gray frames, where every
    live feature leaves in its first iteration;
  * the fused row builds its pyramid in the tracking launch for even parents and at most 4 levels."""
import functools
import types

import numpy as np
import pytest

from oracle import pagk_oracle as orc

import reference_cases as rc
import route_runner as rr
import track_routes as tr
from util import assert_parity, needs_variant

pytestmark = pytest.mark.gpu

MODE = "reference"   # one parameter mode: the case's own parameters, solver_variant 0


@functools.lru_cache(maxsize=None)
def fixture(name):
    params, inp, out, _ = rc.load_fixture(name)
    for a in list(inp.values()) + list(out.values()):
        a.setflags(write=False)   # shared by every row
    c = rc.case(name)
    w = types.SimpleNamespace(name=name, n=c.n, pyramids=c.pyramids, half_patch=c.half_patch, params=params, **inp)
    return c, w, out


def admits(r, c):
    if c.half_patch not in r.halves or not r.test.startswith("test_instantiations_gpu.py"):
        return False
    if c.ncc and any(s in (5, 7) for s in r.selectors):
        return False
    if r.handover and c.content != "texture":
        return False
    if r.entry == "track_device_fused":
        parents = [(c.width >> l, c.height >> l) for l in range(c.pyramids - 1)]
        return c.pyramids <= 4 and all(w % 2 == 0 and h % 2 == 0 for w, h in parents)
    return True


def _rows():
    out = []
    for name in rc.committed_cases():
        c = rc.case(name)
        for r in tr.ROUTES:
            if admits(r, c):
                marks = [needs_variant(r.needs_variant)] if r.needs_variant else []
                out.append(pytest.param(name, r.name, marks=marks, id=f"{name}-{r.name}"))
    return out


def test_every_case_is_admitted_by_the_4_wave_row():
    assert all(admits(tr.route("block"), rc.case(name)) for name in rc.committed_cases())


@pytest.mark.parametrize("name", rc.committed_cases())
def test_default_route(ctx, name):
    """pagk_track with the selector left alone: the launch size decides.  The padded-rows case goes through pagk_image.step,
    the five-coefficient case through n_dist_coef = 5."""
    c, w, want = fixture(name)
    assert w.img_ref.strides[0] == (c.step or c.width) and w.params.n_dist_coef == max(4, len(c.dist))
    got = ctx.track(w.params, w.img_ref, w.img_cur, w.pt_ref, w.pt_init, w.affine, w.status_in)
    assert_parity(got, want, c.n, exact=True, what=f"{name}: default route against the compiled reference")
    for k in rc.OUTPUTS:
        assert got[k][:c.n].dtype == want[k].dtype and np.array_equal(got[k][:c.n], want[k], equal_nan=True), f"{name}: {k}"
    ctx.check_launch()


def _run_oracle(w, mode, pair=None):
    """(the fused row's second launch, on the slot it built: another image pair, which no fixture holds)"""
    img_ref, img_cur = pair or (w.img_ref, w.img_cur)
    return orc.track(w.params, img_ref, img_cur, w.pt_ref, w.pt_init, w.affine, w.status_in, nthreads=8)


@pytest.mark.parametrize("name,route", _rows())
def test_route(request, monkeypatch, name, route):
    c, w, want = fixture(name)
    r = tr.route(route)
    batch = (w, w) if r.entry == "track_device_batch" else ()
    case = rr.Case(what=f"{name} through {route}, against the compiled reference", w=w, modes=(MODE,),
                   params=lambda wl, mode: wl.params, oracle=lambda mode: want, run_oracle=_run_oracle, variants=r.variants,
                   next_seed=0x5E51 + c.seed % 4096, batch=batch, batch_oracles=lambda mode: (want,) * len(batch),
                   batch_variants=(r.variants[0],) * len(batch))
    rr.run_route(request, monkeypatch, r, case)


@pytest.mark.parametrize("name", [c.name for c in rc.NCC_CASES])
def test_device_ncc(ctx, name):
    """pagk_ncc_free and the NCC column of pagk_find_near_neighbors against the free NCC overloads of src/utils.cpp as the
    compiled reference evaluated them, border points included."""
    c = rc.ncc_case(name)
    inp, by_images, by_values, _ = rc.load_ncc_fixture(name)
    n = inp["pt_ref"].shape[0]
    affine = inp["affine"] if c.use_affine else None
    got = ctx.ncc_free(inp["img_ref"], inp["img_cur"], c.half_patch, inp["pt_ref"], inp["pt_cur"], affine)
    assert got.dtype == by_images.dtype and np.array_equal(got, by_images), f"{name}: pagk_ncc_free, rows {np.flatnonzero(got != by_images)[:8]}"
    # every current point as the one detection within radius 0 of its own prediction: list i holds j = i alone
    assert len(np.unique(inp["pt_cur"], axis=0)) == n
    nb = ctx.find_near_neighbors(inp["img_ref"], inp["img_cur"], c.half_patch, inp["pt_ref"], inp["pt_cur"], np.ones(n, np.uint8),
                                 affine, inp["pt_cur"], inp["pt_cur"], level=1, radius_unit=0.0, use_ncc=True, cap=4)
    assert nb["rc"] == 0 and np.array_equal(nb["count"], np.ones(n, np.int32)) and np.array_equal(nb["idx"][:, 0], np.arange(n))
    assert np.array_equal(nb["dist"][:, 0], np.zeros(n, np.float32))
    assert np.array_equal(nb["ncc"][:, 0], by_values), f"{name}: pagk_find_near_neighbors, rows {np.flatnonzero(nb['ncc'][:, 0] != by_values)[:8]}"
