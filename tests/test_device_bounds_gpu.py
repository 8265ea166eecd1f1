"""Every device entry point on guarded, exact-length device arrays (tests/arena.py), one case per row of
tests/device_forms.py and shape.

The parity tests compare the bytes an array is documented to have and nothing else; their device arrays come out of one
packed buffer or out of torch's caching allocator, where a write one row past n lands in a neighbour and a read past the
end returns some other tensor's bytes.  Here every caller array is exactly its documented length with a guard band on both
sides, and every case
  1. runs the call under guard fill A: no guard damaged; every output payload byte-identical to the restatement the
     module's own GPU test uses; rows the header says are left untouched still hold the sentinel; inputs unchanged;
  2. rewrites the guards with fill B, resets the outputs and runs again: the same bytes (a read outside an array that
     steers a result shows here), no guard damaged;
  3. runs once more with each optional output NULL: the others unchanged.
The expected bytes never come from another call into the library."""
import dataclasses

import numpy as np
import pytest
import torch

import arena as ar
import associate_ref_util as au
import detect_ref_util as du
import device_forms as df
import fast_ref_util as fu
import fit_ref_util as ftu
import handover_ref_util as hu
import instantiation_cases as cases
import inverse_ref_util as iu
import lk_ref_util as lu
import orb_ref_util as ou
import pose_ref_util as pu
import rectify_ref_util as ru
import shape_cases as sc
import track_routes as tr
from oracle import pagk_oracle as orc
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, synth
from util import make_geometry_case, needs_variant

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "f64": torch.float64, "u8": torch.uint8, "i32": torch.int32}
NP = {"f32": np.float32, "f64": np.float64, "u8": np.uint8, "i32": np.int32}
F32, I32, U8, F64 = np.float32, np.int32, np.uint8, np.float64
DEV = "cuda:0"
COUNTS = (0, 1, 65)   # test_host_forms_gpu.COUNTS
W, H = 97, 80         # the 97 x 80 texture


# ---- the engine --------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Plan:
    """One call on arena arrays.  `arrays`: (device_forms.Arr, key, payload or shape) -- inputs and in/out arrays come with
    their payload, outputs with their shape; `key` names the array in the arena and in `want`.  `run(views, null)` issues the
    call with the views (None for the keys in `null`) and returns after the context has been synchronised and its error
    word checked.  `want`: key -> the expected payload, or a function of the sentinel array (the payload an untouched output
    holds under the current fill) that returns it -- for outputs with rows the call leaves alone."""
    what: str
    arrays: list
    run: object
    want: dict
    optional: tuple = ()


def _build(plan, which="A"):
    a = ar.Arena(DEV, which=which)
    for arr, key, data in plan.arrays:
        if arr.role == "out":
            a.out(key, DT[arr.dtype], data, arr.kind)
        elif arr.role == "inout":
            a.inout(key, np.ascontiguousarray(data, NP[arr.dtype]), arr.kind)
        elif isinstance(data, tuple) and data[0] == "image":
            a.image(key, data[1], data[2])
        else:
            a.inp(key, np.ascontiguousarray(data, NP[arr.dtype]), arr.kind)
    return a


def _expected(a, plan, key):
    w = plan.want[key]
    e = a.entries[key]
    got = w(a.sentinel(key)) if callable(w) else w
    got = np.ascontiguousarray(got, a.sentinel(key).dtype)
    assert got.size * got.itemsize == e.nbytes, f"{plan.what}: the restatement's {key} is not the documented length"
    return got


def _launch(a, plan, null=()):
    views = {key: (None if key in null else a.arg(key)) for _, key, _ in plan.arrays}
    torch.cuda.synchronize()      # the fills are torch's; the call runs on the context's stream
    plan.run(views, null)
    torch.cuda.synchronize()


def _assert_state(a, plan, what, null=()):
    assert a.damaged() == {}, f"{what}: guard bytes written (array: byte offsets relative to it)"
    for arr, key, _ in plan.arrays:
        if arr.role == "in":
            continue
        got = a.payload(key)
        if key in null:
            assert got.tobytes() == a.sentinel(key).tobytes() or arr.role == "inout", f"{what}: {key} is NULL in the call and was written"
            continue
        want = _expected(a, plan, key)
        if got.tobytes() != want.tobytes():
            bad = np.nonzero(got.reshape(-1).view(np.uint8) != want.reshape(-1).view(np.uint8))[0]
            raise AssertionError(f"{what}: {key} differs from the restatement in {bad.size} bytes, the first at byte {int(bad[0])}"
                                 f" (element {int(bad[0]) // got.itemsize} of {got.size})")
    assert a.inputs_unchanged() == [], f"{what}: input payloads written"


def check(plan):
    a = _build(plan, "A")
    _launch(a, plan)
    _assert_state(a, plan, f"{plan.what}, fill A")
    first = {key: a.payload(key) for arr, key, _ in plan.arrays if arr.role != "in"}
    a.refill("B")
    a.reset_outputs()
    _launch(a, plan)
    _assert_state(a, plan, f"{plan.what}, fill B")
    for arr, key, _ in plan.arrays:
        # rows that hold a result are the same bytes under both fills; rows left alone hold the fill they were given
        if arr.role != "in" and not callable(plan.want[key]):
            assert a.payload(key).tobytes() == first[key].tobytes(), f"{plan.what}: {key} depends on the guard fill"
    for key in plan.optional:
        a.reset_outputs()
        _launch(a, plan, null=(key,))
        _assert_state(a, plan, f"{plan.what}, {key} = NULL", null=(key,))
    return a


def test_the_arena_on_the_device(built):
    """The checks of test_arena_cpu.py once on device memory: a planted byte behind an array, one in front of it, one inside
    the payload, under both fills."""
    for which in ("A", "B"):
        a = ar.Arena(DEV, capacity=1 << 16, which=which)
        v = a.out("res", torch.float32, (3, 2), "float")
        a.inp("n", np.array([3], I32), "index")
        assert v.is_cuda and v.data_ptr() % 256 == 0 and a.damaged() == {}
        e = a.entries["res"]
        for off in (24, -1, 5):
            a.raw[a.base + e.off + off] = 0x5A
        torch.cuda.synchronize()
        assert a.damaged() == {"res": [-1, 24]} and a.inputs_unchanged() == []


# ---- trackers ----------------------------------------------------------------------------------------------------------------
TRACK = df.form("pagk_track_device")
OUT_KEYS = ("pt_un", "pt_dist", "status", "pix_err", "dist_pred", "ncc", "iters")
TRACK_OPTIONAL = ("pt_dist", "pix_err", "dist_pred", "ncc", "iters")


def _arr(form, name):
    return next(a for a in form.arrays if a.name == name)


def _track_arrays(form, w, n, prefix=""):
    """The four inputs and seven outputs of a tracking call on the first n features of workload `w`."""
    s = dict(n=n)
    ins = dict(d_pt_ref_un=w.pt_ref[:n], d_pt_init_un=w.pt_init[:n], d_affine=w.affine[:n], d_status_in=w.status_in[:n])
    arrays = []
    for name, data in ins.items():
        arr = _arr(form, name)
        assert data.size == df.length(arr, s)
        arrays.append((arr, prefix + name, data))
    for k in OUT_KEYS:
        arr = _arr(form, "d_out." + k)
        cols = 2 if k in ("pt_un", "pt_dist") else 1
        assert df.length(arr, s) == n * cols
        arrays.append((arr, prefix + k, (n, 2) if cols == 2 else (n,)))
    return arrays


def _track_want(ref, n, prefix=""):
    return {prefix + k: np.asarray(ref[k])[:n] for k in OUT_KEYS}


def _track_args(v, prefix=""):
    return ([v[prefix + k] for k in ("d_pt_ref_un", "d_pt_init_un", "d_affine", "d_status_in")],
            {k: v[prefix + k] for k in OUT_KEYS})


def _after(c, variant, handover, what):
    c.sync()
    if variant is None:   # (no feature, no launch to name)
        return c.check_launch()
    assert c.last_variant() == variant, f"{what}: ran variant {c.last_variant()}, expected {variant}"
    handed = c.last_handover()
    assert (handed > 0) == handover, f"{what}: {handed} features handed over, expected hand-over = {handover}"
    c.check_launch()


def _track_plan(c, what, w, p, ref, n, variant, handover, selector=0):
    def run(v, null):
        d, out = _track_args(v)
        c.set_kernel(selector)
        try:
            c.track_device(p, 0, 1, n, d[0], d[1], d[2], d[3], out)
        finally:
            c.set_kernel(0)
        _after(c, variant, handover, what)
    return Plan(what, _track_arrays(TRACK, w, n), run, _track_want(ref, n), TRACK_OPTIONAL)


def _route_cases():
    out = []
    for r in tr.ROUTES:
        if not r.test.startswith("test_instantiations_gpu.py"):
            continue
        marks = [needs_variant(r.needs_variant)] if r.needs_variant else []
        out += [pytest.param(r.name, h, marks=marks, id=f"{r.name}-h{h}") for h in r.halves]
    return out


ROUTE_MODES = ("lean", "both")


def _uploaded(c, w):
    c.frame_upload(0, w.img_ref, w.pyramids)
    c.frame_upload(1, w.img_cur, w.pyramids)


@pytest.mark.parametrize("name,h", _route_cases())
def test_track_route(built, request, monkeypatch, name, h):
    """Every row of track_routes.ROUTES that the instantiation matrix runs, on its workload (320 x 240, three levels, 67
    features: the last quad wave has spare rows), through the DEVICE forms with every array in the arena -- also the rows
    whose own test goes through pagk_track, whose staging block would hide an overrun."""
    r = tr.route(name)
    cases.check_not_vacuous(h, continuation=r.handover)
    for var, value in r.env:
        monkeypatch.setenv(var, value)
    w = cases.workload(h)
    if r.entry == "track_device_batch":
        return _batch(r, h)
    c = capi.Context(0) if (r.env or r.entry != "track") else request.getfixturevalue("ctx")
    try:
        _uploaded(c, w)
        for selector, variant in zip(r.selectors, r.variants):
            for k, mode in enumerate(ROUTE_MODES):
                what = f"{name} h={h} kernel {selector} {mode}"
                p, ref = cases.params(w, mode), cases.oracle(h, mode)
                if r.entry == "track_device_fused":
                    check(_fused_plan(c, what, w, p, ref, variant, 16 * h + k, pad=13 * (1 - k)))
                else:
                    check(_track_plan(c, what, w, p, ref, w.n, variant, r.handover, selector))
    finally:
        if c is not request.getfixturevalue("ctx"):
            c.close()


FUSED = df.form("pagk_track_device_fused")


def _fused_plan(c, what, w, p, ref, variant, seed, pad):
    """pagk_track_device_fused: the tracked outputs, and the pyramid of the next frame (an arena image, rows `pad` bytes
    wider than the frame) built into slot 2 by the same call."""
    height, width = w.img_ref.shape
    step = width + pad
    nxt = np.random.default_rng(seed).integers(0, 256, (height, width), dtype=np.uint8)
    arr = _arr(FUSED, "d_next")
    assert df.length(arr, dict(width=width, height=height, step=step)) == ar.image_length(width, height, step)

    def run(v, null):
        d, out = _track_args(v)
        c.track_device_fused(p, 0, 1, w.n, d[0], d[1], d[2], d[3], out, 2, v["d_next"].data_ptr(), width, height, step, w.pyramids)
        _after(c, variant, False, what)
        lvl = nxt
        for l in range(1, w.pyramids):
            lvl = orc.pyr_down(lvl)
            assert np.array_equal(c.frame_download_level(2, l, width, height), lvl), f"{what}: next-frame pyramid level {l}"
    return Plan(what, _track_arrays(FUSED, w, w.n) + [(arr, "d_next", ("image", nxt, step))], run, _track_want(ref, w.n),
                TRACK_OPTIONAL)


BATCH = df.form("pagk_track_device_batch")


def _batch(r, h):
    """pagk_track_device_batch: streams of 1, 67 and 30 features as one launch, every stream's arrays in the arena."""
    ws = cases.batch_workloads(h)
    assert [w.n for w in ws] == [1, 67, 30]
    ctxs = [capi.Context(0) for _ in ws]
    try:
        for c, w in zip(ctxs, ws):
            _uploaded(c, w)
        for mode in ROUTE_MODES:
            what = f"batch h={h} {mode}"
            p, refs = cases.params(ws[0], mode), cases.batch_oracles(h, mode)
            arrays, want = [], {}
            for j, (w, ref) in enumerate(zip(ws, refs)):
                arrays += _track_arrays(BATCH, w, w.n, f"s{j}.")
                want.update(_track_want(ref, w.n, f"s{j}."))

            def run(v, null):
                args = [_track_args(v, f"s{j}.") for j in range(len(ws))]
                ctxs[0].set_kernel(r.selectors[0])
                try:
                    capi.Context.track_device_batch(ctxs, p, [0] * len(ws), [1] * len(ws), [w.n for w in ws],
                                                    [d[0] for d, _ in args], [d[1] for d, _ in args], [d[2] for d, _ in args],
                                                    [d[3] for d, _ in args], [o for _, o in args])
                finally:
                    ctxs[0].set_kernel(0)
                for j, c in enumerate(ctxs):
                    _after(c, r.variants[0], r.handover, f"{what}, stream {j}")
            check(Plan(what, arrays, run, want, tuple(f"s1.{k}" for k in TRACK_OPTIONAL)))
    finally:
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("h", iu.HALVES)
def test_track_template_jacobian(ctx, h):
    """Variant 8 (inverse == PAGK_INVERSE_TEMPLATE, k_inv_wave) on 96 x 64 with two levels, against tests/inverse_ref.c."""
    shape = (96, 64, 2)
    w = sc.workload(shape, h)
    _uploaded(ctx, w)
    for mode in sc.MODES:
        check(_track_plan(ctx, f"template Jacobian h={h} {mode}", w, iu.shape_params(w, mode), iu.restated(shape, h, mode),
                          w.n, 8, False))


@pytest.mark.parametrize("selector,variant", [(0, 0), (3, 3)])
def test_track_ncc(ctx, selector, variant):
    """calculate_ncc: the ncc field holds results (not all 1) and stays inside its array."""
    w = cases.workload(5)
    p = cases.params(w, "lean")
    p.calculate_ncc = 1
    ref = orc.track(p, w.img_ref, w.img_cur, w.pt_ref, w.pt_init, w.affine, w.status_in, nthreads=8)
    assert (ref["ncc"][:w.n][ref["status"][:w.n] > 0] != 1).any()
    _uploaded(ctx, w)
    check(_track_plan(ctx, f"ncc kernel {selector}", w, p, ref, w.n, variant, False, selector))


@pytest.mark.parametrize("selector,variant", [(0, 0), (1, 1), (3, 3), (5, 5), (7, 7)])
@pytest.mark.parametrize("n", [0, 1])
def test_track_one_and_none(built, monkeypatch, n, selector, variant):
    """n = 1: one row of every output.  n = 0: every output untouched (zero-length arrays: only guards around the pointer)."""
    monkeypatch.setenv("PAGK_QUAD_BUDGET", "0")
    w = cases.workload(5)
    c = capi.Context(0)
    try:
        _uploaded(c, w)
        for mode in ROUTE_MODES:
            ref = cases.oracle(5, mode)   # features are independent: the first row of the 67-feature run
            plan = _track_plan(c, f"n={n} kernel {selector} {mode}", w, cases.params(w, mode), ref, n, variant if n else None, False,
                               selector)
            if n == 0:
                plan.want = {k: (lambda s: s) for k in plan.want}
            check(plan)
    finally:
        c.close()


# ---- everything else ---------------------------------------------------------------------------------------------------------
# The smallest inputs of each module's own GPU test; counts from test_host_forms_gpu.COUNTS; where a form has a capacity it
# is strictly larger than the count the restatement returns, so that a tail exists (asserted on the restatement's result).
class Refs:
    """The plain-C restatements, each built once."""

    def __init__(self, tmp):
        self.tmp, self.libs = tmp, {}

    def __getattr__(self, name):
        mod = dict(handover=hu, detect=du, fast=fu, orb=ou, lk=lu, fit=ftu, pose=pu, assoc=au, rectify=ru)[name]
        if name not in self.libs:
            self.libs[name] = mod.build_ref(self.tmp.mktemp(name + "_ref"))
        return self.libs[name]


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    return Refs(tmp_path_factory)


@pytest.fixture(scope="module")
def tex():
    return ou.images(synth)["97x80 texture"]


def _form_plan(what, function, scalars, ins, outs, run, want, optional=(), counts=None):
    """A Plan from a row of the table: `ins` name -> payload (or ("image", img, step)), `outs` name -> shape; the lengths
    are checked against the row's expressions for `scalars`.  `counts`: output name -> the count the restatement reports
    for it; its rows at and beyond the count must be what the row's `tail` says."""
    form = df.form(function)
    arrays = []
    for name, data in list(ins.items()) + list(outs.items()):
        arr = _arr(form, name)
        size = (ar.image_length(data[1].shape[1], data[1].shape[0], data[2]) if isinstance(data, tuple) and data and data[0] == "image"
                else int(np.prod(data)) if name in outs and arr.role == "out" else int(np.asarray(data).size))
        assert size == df.length(arr, scalars), f"{function}: {name} has {size} elements, the table says {df.length(arr, scalars)}"
        assert (name in outs) == (arr.role == "out") or arr.role == "inout", (function, name)
        arrays.append((arr, name, data))
    assert set(want) == {n for a, n, _ in arrays if a.role != "in"}, f"{function}: an output without a restatement"
    tailed = {a.name for a, _, _ in arrays if a.tail is not None and a.tail != "untouched"}
    assert tailed <= set(counts or {}), f"{function}: the table gives {sorted(tailed - set(counts or {}))} a tail and the case no count"
    for name, k in (counts or {}).items():
        rows = np.asarray(want[name])
        assert (rows[k:] == _arr(form, name).tail).all(), f"{function}: the restatement's {name} beyond row {k} is not the table's tail"
    return Plan(what, arrays, run, want, optional)


def _own():
    return capi.Context(0)


def _levels(img, count):
    out = [np.ascontiguousarray(img)]
    for _ in range(count - 1):
        out.append(orc.pyr_down(out[-1]))
    return out


# -- frames
@pytest.mark.parametrize("pad", [0, 13])
def test_frame_set_device(built, tex, pad):
    c = _own()
    try:
        step = W + pad

        def run(v, null):
            c.frame_set_device(2, v["d_data"].data_ptr(), W, H, step, 3)
            c.sync()
            c.check_launch()
            for l, want in enumerate(_levels(tex, 3)):
                assert np.array_equal(c.frame_download_level(2, l, W, H), want), f"level {l}"
        check(_form_plan(f"frame_set_device step {step}", "pagk_frame_set_device", dict(width=W, height=H, step=step),
                         dict(d_data=("image", tex, step)), {}, run, {}))
    finally:
        c.close()


@pytest.mark.parametrize("pad", [0, 13])
def test_frame_set_device_batch(built, tex, pad):
    """Three contexts' frames as one call: an even frame, the 97 x 80 texture (odd parents) and a 160 x 120 one."""
    imgs = [du.noise_image(96, 64, 3), tex, ou.images(synth)["160x120 texture"]]
    ctxs = [_own() for _ in imgs]
    try:
        form = df.form("pagk_frame_set_device_batch")
        arrays = [(form.arrays[0], f"s{j}.d_data", ("image", im, im.shape[1] + pad)) for j, im in enumerate(imgs)]

        def run(v, null):
            capi.Context.frame_set_device_batch(ctxs, [1] * 3, [v[f"s{j}.d_data"].data_ptr() for j in range(3)],
                                                [im.shape[1] for im in imgs], [im.shape[0] for im in imgs],
                                                [im.shape[1] + pad for im in imgs], 3)
            for c, im in zip(ctxs, imgs):
                c.sync()
                c.check_launch()
                for l, want in enumerate(_levels(im, 3)):
                    assert np.array_equal(c.frame_download_level(1, l, im.shape[1], im.shape[0]), want), (im.shape, l)
        check(Plan(f"frame_set_device_batch pad {pad}", arrays, run, {}))
    finally:
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("pad", [0, 5])
def test_frame_rectify_device(built, refs, pad, cn):
    ws, hs = 64, 40
    mx, my, _, _ = ru.grid_maps(70, 37, ws, hs, 7)
    raw = ru.noise_raw(ws, hs, cn, 100 + cn, pad=pad)
    want0 = ru.ref_rectify(refs.rectify, mx, my, raw)
    assert want0.any()
    rows, step = np.ascontiguousarray(np.asarray(raw).reshape(hs, ws * cn)), ws * cn + pad
    c = _own()
    try:
        c.rectify_set_maps(mx, my)
        rp = capi.rectify_params_default(channels=cn)

        def run(v, null):
            c.frame_rectify_device(0, rp, v["d_raw"].data_ptr(), ws, hs, step, 2)
            c.sync()
            c.check_launch()
            for l, want in enumerate(_levels(want0, 2)):
                assert np.array_equal(c.frame_download_level(0, l, 70, 37), want), f"level {l}"
        check(_form_plan(f"frame_rectify_device cn {cn} step {step}", "pagk_frame_rectify_device",
                         dict(src_width=ws, src_height=hs, src_step=step, channels=cn), dict(d_raw=("image", rows, step)), {}, run, {}))
    finally:
        c.close()


# -- prediction
def _case_predict(n):
    w = cases.workload(5)
    p = cases.params(w, "lean")
    Rp = synth.rodrigues(np.array((0.004, -0.003, 0.006))) @ synth.rodrigues(np.array((0.5, -1.0, 2.0)) * 0.05)
    K32 = w.camera.K.astype(F32)

    def mul(a, b):
        return (a.astype(F64) @ b.astype(F64)).astype(F32)
    KRK = mul(mul(K32, Rp.astype(F32)), np.linalg.inv(K32.astype(F64)).astype(F32))
    r3 = Rp.astype(F32)[2]
    pt = np.ascontiguousarray(w.pt_ref[:n])
    height, width = w.img_ref.shape
    pu_, pd_, st, A = orc.gyro_predict(p, width, height, w.half_patch, KRK, r3, pt)
    return p, width, height, KRK, r3, pt, pu_, pd_, st, A


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("form", ["", "_rot", "_live"])
def test_gyro_predict_device(ctx, refs, form, n):
    p, width, height, KRK, r3, pt, pu_, pd_, st, A = _case_predict(n)
    if n == 65:
        assert 0 < int(st.sum()) < n          # rows the prediction leaves the image in: status 0, affine untouched
    pu_, pd_, st = pu_.copy(), pd_.copy(), st.copy()
    ins = dict(d_pt_ref_un=pt)
    if form:
        ins = dict(d_rot=np.concatenate([KRK.reshape(-1)[:6], r3]).astype(F32), **ins)
    live = None
    if form == "_live":
        live = (np.random.default_rng(1).random(n) < 0.6).astype(U8)
        ins["d_live"] = live
        refs.handover.fhr_predict_live(n, live.ctypes.data, pu_.ctypes.data, pd_.ctypes.data, st.ctypes.data)
    before = np.full((n, 4), -5.0, F32)
    written = (st > 0) if live is None else ((st > 0) & (live > 0))
    want = dict(d_pt_predict_un=pu_, d_pt_predict=pd_, d_status=st, d_affine=np.where(written[:, None], A, before))

    def run(v, null):
        args = (n, v["d_pt_ref_un"]) + ((v["d_live"],) if form == "_live" else ()) + (
            v["d_pt_predict_un"], v["d_pt_predict"], v["d_status"], v["d_affine"])
        if form == "":
            ctx.gyro_predict_device(p, width, height, KRK, r3, *args)
        elif form == "_rot":
            ctx.gyro_predict_device_rot(p, width, height, v["d_rot"], *args)
        else:
            ctx.gyro_predict_device_live(p, width, height, v["d_rot"], *args)
        ctx.sync()
        ctx.check_launch()
    function = {"": "pagk_gyro_predict_device", "_rot": "pagk_gyro_predict_device_rot", "_live": "pagk_gyro_predict_device_live"}[form]
    check(_form_plan(f"{function} n={n}", function, dict(n=n), ins,
                     dict(d_pt_predict_un=(n, 2), d_pt_predict=(n, 2), d_status=(n,), d_affine=before), run, want, ("d_affine",)))


# -- Step 3
@pytest.mark.parametrize("n", COUNTS)
def test_post_filter_device(ctx, refs, n):
    rng = np.random.default_rng(100 + n)
    st = (rng.random(n) < 0.8).astype(U8)
    st[:1] = 1
    pe = (rng.random(n) * 10.0 ** rng.integers(-9, 2, n)).astype(F64)
    dp = rng.random(n) * 30.0
    pm = rng.random((n, 2)).astype(F32) * 600
    pmu = (pm + F32(0.5)).astype(F32)
    init = np.full((n, 2), -777.0, F32)
    r = hu.ref_post_filter(refs.handover, 5, st, pe, dp, pm, pmu, pt_predict=init if n else None, pt_predict_un=init if n else None)
    if n == 65:
        assert 0 < r["kept"] < n
    want = dict(d_status_out=r["status"], d_pt_predict=r["pt_predict"][:n], d_pt_predict_un=r["pt_predict_un"][:n],
                d_kept=np.array([r["kept"]], I32), d_thresholds=r["thresholds"])

    def run(v, null):
        ctx.post_filter_device(n, 5, v["d_status_pm"], v["d_pix_err"], v["d_dist_pred"], v["d_pt_pm"], v["d_pt_pm_un"],
                               v["d_status_out"], v["d_pt_predict"], v["d_pt_predict_un"], v["d_kept"], v["d_thresholds"])
        ctx.sync()
        ctx.check_launch()
    check(_form_plan(f"post_filter_device n={n}", "pagk_post_filter_device", dict(n=n),
                     dict(d_status_pm=st, d_pix_err=pe, d_dist_pred=dp, d_pt_pm=pm, d_pt_pm_un=pmu),
                     dict(d_status_out=(n,), d_pt_predict=init, d_pt_predict_un=init, d_kept=(1,), d_thresholds=(2,)),
                     run, want, ("d_thresholds",)))


# -- hand-overs
CAP, TARGET, THRESHOLD = 80, 70, 60.0
HANDOVER_OUT = ("keys", "keys_un", "keys_normal", "index_in_last", "live", "mask", "state")


def _handover_inputs(cap):
    """status / pt_predict / pt_predict_un of cap features (two thirds alive), a state with reach_flag set
    (test_host_forms_gpu._handover_inputs)."""
    rng = np.random.default_rng(17 + cap)
    st = (rng.random(cap) < 0.66).astype(U8)
    un = np.column_stack([rng.uniform(0, W, cap), rng.uniform(0, H, cap)]).astype(F32)
    pp = (un + F32([0.25, -0.5])).astype(F32)
    state = np.zeros(8, I32)
    state[1] = 1
    return st, pp, un, state


def _handover_plan(what, function, scalars, extra_in, call, want, info):
    st, pp, un, state = _handover_inputs(CAP)
    ins = dict(d_status=st, d_pt_predict=pp, d_pt_predict_un=un, **extra_in)
    outs = dict(d_keys=(CAP, 2), d_keys_un=(CAP, 2), d_keys_normal=(CAP, 2), d_index_in_last=(CAP,), d_live=(CAP,), d_mask=(H, W),
                d_state=state)
    if info:
        outs["d_info"] = (8,)
    total = int(want["state"][0])
    assert 1 <= total < CAP and int(want["state"][2]) >= 1, "a tail with nothing in front of it is vacuous"
    assert not want["keys"][total:].any() and (want["index_in_last"][total:] == -1).all()
    w = {"d_" + k: want[k] for k in HANDOVER_OUT + (("info",) if info else ())}
    return _form_plan(what, function, dict(cap=CAP, width=W, height=H, **scalars), ins, outs, call, w,
                      ("d_keys_normal", "d_mask"), {k: total for k in ("d_keys", "d_keys_un", "d_keys_normal", "d_index_in_last")})


def _handover_tail(v):
    return [v["d_" + k] for k in HANDOVER_OUT]


@pytest.mark.parametrize("n_cand", COUNTS)
def test_frame_handover_device(ctx, refs, n_cand):
    p = capi.make_params(camera=synth.generic_camera(W, H))
    st, pp, un, state = _handover_inputs(CAP)
    cand_cap = 70
    cand = np.zeros((cand_cap, 2), F32)
    cand[:n_cand] = lu.interior_points(W, H, n_cand, 2, 5)
    want = hu.ref_handover(refs.handover, hu.camera_of(p), W, H, CAP, TARGET, THRESHOLD, st, pp, un, cand[:n_cand], state=state)
    if n_cand == 65:
        assert want["state"][3] >= 1

    def run(v, null):
        ctx.frame_handover_device(p, W, H, CAP, TARGET, THRESHOLD, v["d_status"], v["d_pt_predict"], v["d_pt_predict_un"], cand_cap,
                                  v["d_n_cand"], v["d_cand_un"], *_handover_tail(v))
        ctx.sync()
        ctx.check_launch()
    check(_handover_plan(f"frame_handover_device n_cand={n_cand}", "pagk_frame_handover_device", dict(cand_cap=cand_cap),
                         dict(d_n_cand=np.array([n_cand], I32), d_cand_un=cand), run, want, False))


def _restated_handover(refs, p, img, detector):
    """The composition that defines the fused calls, made of the two restatements (test_detect_gpu.py, test_fast_gpu.py)."""
    st, pp, un, state = _handover_inputs(CAP)
    cam, none = hu.camera_of(p), np.zeros((0, 2), F32)
    first = hu.ref_handover(refs.handover, cam, W, H, CAP, TARGET, THRESHOLD, st, pp, un, none, state=state)
    m, reach = int(first["state"][2]), int(state[1])
    assert (m < THRESHOLD or not reach) and TARGET - m > 0, "the top-up must run"
    if detector == "harris":
        d = du.ref_detect(refs.detect, img, first["mask"], TARGET - m, cap=CAP, min_distance=5.0)
        cand = d["corners"][:d["n"]]
    else:
        d = fu.ref_detect(refs.fast, img, None, TARGET)
        cand = d["keypoints"][:d["n"]]
    assert d["n"] >= 1
    out = hu.ref_handover(refs.handover, cam, W, H, CAP, TARGET, THRESHOLD, st, pp, un, cand, state=state)
    out["info"] = d["info"]
    assert out["state"][3] >= 1
    return out


@pytest.mark.parametrize("detector", ["harris", "fast"])
def test_frame_handover_with_detector_device(built, refs, tex, detector):
    p = capi.make_params(camera=synth.generic_camera(W, H))
    want = _restated_handover(refs, p, tex, detector)
    dp = capi.detect_params_default(min_distance=5.0) if detector == "harris" else capi.fast_params_default()
    c = _own()
    try:
        c.frame_upload(0, tex, 1)
        fn = c.frame_handover_detect_device if detector == "harris" else c.frame_handover_fast_device

        def run(v, null):
            fn(p, W, H, CAP, TARGET, THRESHOLD, v["d_status"], v["d_pt_predict"], v["d_pt_predict_un"], dp, 0, *_handover_tail(v),
               v["d_info"])
            c.sync()
            c.check_launch()
        name = "pagk_frame_handover_detect_device" if detector == "harris" else "pagk_frame_handover_fast_device"
        check(_handover_plan(f"{name}", name, {}, {}, run, want, True))
    finally:
        c.close()


# -- detectors
@pytest.mark.parametrize("max_corners", COUNTS)
@pytest.mark.parametrize("masked", [False, True])
def test_detect_corners_device(ctx, refs, tex, max_corners, masked):
    mask = du.holes_mask(W, H, 12) if masked else None
    det = capi.detect_params_default(min_distance=5.0)
    want = du.ref_detect(refs.detect, tex, mask, max_corners, cap=CAP, min_distance=5.0)
    assert want["n"] == min(max_corners, want["n"]) < CAP and (max_corners == 0 or want["n"] >= 1)
    ctx.frame_upload(2, tex, 1)
    ins = dict(d_max_corners=np.array([max_corners], I32))
    if masked:
        ins["d_mask"] = mask

    def run(v, null):
        ctx.detect_corners_device(det, 2, v.get("d_mask"), CAP, v["d_max_corners"], v["d_corners"], v["d_info"])
        ctx.sync()
        ctx.check_launch()
    check(_form_plan(f"detect_corners_device max {max_corners} masked {masked}", "pagk_detect_corners_device", dict(cap=CAP, W=W, H=H),
                     ins, dict(d_corners=(CAP, 2), d_info=(8,)), run, dict(d_corners=want["corners"], d_info=want["info"]),
                     counts=dict(d_corners=want["n"])))


@pytest.mark.parametrize("n_features", COUNTS[1:])
@pytest.mark.parametrize("masked", [False, True])
def test_detect_fast_device(ctx, refs, n_features, masked):
    img = du.noise_image(62, 62, 3)
    mask = du.holes_mask(62, 62, 6) if masked else None
    cap = fu.ref_bounds(refs.fast, 62, 62, n_features)[1] + 7
    want = fu.ref_detect(refs.fast, img, mask, n_features, cap=cap)
    assert 1 <= want["n"] < cap
    ctx.frame_upload(2, img, 1)
    fp = capi.fast_params_default(n_features=n_features)

    def run(v, null):
        ctx.detect_fast_device(fp, 2, v.get("d_mask"), cap, v["d_keypoints"], v["d_response"], v["d_info"])
        ctx.sync()
        ctx.check_launch()
    check(_form_plan(f"detect_fast_device N {n_features} masked {masked}", "pagk_detect_fast_device", dict(cap=cap, W=62, H=62),
                     dict(d_mask=mask) if masked else {}, dict(d_keypoints=(cap, 2), d_response=(cap,), d_info=(8,)), run,
                     dict(d_keypoints=want["keypoints"], d_response=want["response"], d_info=want["info"]), ("d_response",),
                     dict(d_keypoints=want["n"], d_response=want["n"])))


# -- ORB
@pytest.mark.parametrize("n", COUNTS)
def test_orb_describe_device(ctx, refs, tex, n):
    pattern = ou.seeded_pattern()
    ctx.orb_set_pattern(pattern)
    ctx.frame_upload(2, tex, 1)
    kp = np.zeros((CAP, 2), F32)
    kp[:65] = ou.many_keypoints(W, H, 65)
    want = ou.ref_describe(refs.orb, tex, pattern, kp, cap=CAP, n=n)
    assert want["info"][0] + want["info"][1] == n and (n < 65 or want["info"][0] >= 1)
    orb = capi.orb_params_default()

    def run(v, null):
        ctx.orb_describe_device(orb, 2, CAP, v["d_keypoints"], v["d_n"], v["d_angle"], v["d_desc"], v["d_info"])
        ctx.sync()
        ctx.check_launch()
    check(_form_plan(f"orb_describe_device n={n}", "pagk_orb_describe_device", dict(cap=CAP), dict(d_keypoints=kp, d_n=np.array([n], I32)),
                     dict(d_angle=(CAP,), d_desc=(CAP, 32), d_info=(8,)), run,
                     dict(d_angle=want["angle"], d_desc=want["desc"], d_info=want["info"]), ("d_angle",), dict(d_angle=n, d_desc=n)))


@pytest.mark.parametrize("nq,nt", [(0, 65), (65, 0), (1, 1), (1, 65), (65, 65)])
def test_orb_match_device(ctx, refs, nq, nt):
    cap_q, cap_t = 80, 70
    dq, dt = np.zeros((cap_q, 32), U8), np.zeros((cap_t, 32), U8)
    dq[:65], dt[:65] = ou.random_descriptors(65, 1), ou.random_descriptors(65, 2)
    for k in range(0, 65, 2):
        dt[k] = ou.flip_bits(dq[k], 3 + k % 40, k)   # near rows: matches above and below the distance filter
    want = ou.ref_match(refs.orb, dq, dt, cap_q=cap_q, nq=nq, nt=nt)
    orb = capi.orb_params_default()

    def run(v, null):
        ctx.orb_match_device(orb, cap_q, v["d_desc_q"], v["d_nq"], cap_t, v["d_desc_t"], v["d_nt"], v["d_train_idx"], v["d_distance"],
                             v["d_keep"], v["d_info"])
        ctx.sync()
        ctx.check_launch()
    check(_form_plan(f"orb_match_device {nq} x {nt}", "pagk_orb_match_device", dict(cap_q=cap_q, cap_t=cap_t),
                     dict(d_desc_q=dq, d_nq=np.array([nq], I32), d_desc_t=dt, d_nt=np.array([nt], I32)),
                     dict(d_train_idx=(cap_q,), d_distance=(cap_q,), d_keep=(cap_q,), d_info=(8,)), run,
                     {"d_" + k: want[k] for k in ou.MATCH_KEYS}, counts=dict(d_train_idx=nq, d_distance=nq, d_keep=nq)))


# -- Lucas-Kanade
LK = dict(half_patch=10)


def _lk_case():
    a, b = lu.texture_pair(synth, 96, 64, 22, (-1.6, 1.1))
    pts = np.zeros((CAP, 2), F32)
    pts[:65] = lu.interior_points(96, 64, 65, 10, 23)
    return a, b, pts


def test_lk_pyramid_device(ctx, refs):
    """The row without a caller array: the levels it builds for a slot, against the restatement."""
    a, _, _ = _lk_case()
    ctx.frame_upload(0, a, 1)
    ctx.lk_pyramid_device(capi.lk_params_default(**LK), 0)
    ctx.sync()
    ctx.check_launch()
    levels = lu.ref_levels(refs.lk, a, lu.params(**LK))
    assert len(levels) >= 2
    for l in range(1, len(levels)):
        hh, ww = levels[l].shape
        assert np.array_equal(ctx.selftest_lk_level(0, l, ww, hh), levels[l]), l


@pytest.mark.parametrize("n", COUNTS)
def test_lk_track_device(ctx, refs, n):
    a, b, pts = _lk_case()
    lk = capi.lk_params_default(**LK)
    want = lu.ref_track(refs.lk, a, b, pts, lu.params(**LK), cap=CAP, n=n)
    assert want["info"][0] == n and (n < 65 or want["info"][2] >= 1)
    for slot, img in ((0, a), (1, b)):
        ctx.frame_upload(slot, img, 1)
        ctx.lk_pyramid_device(lk, slot)

    def run(v, null):
        ctx.lk_track_device(lk, 0, 1, CAP, v["d_pt_ref"], v["d_n"], v["d_pt_out"], v["d_status"], v["d_status_raw"], v["d_err"],
                            v["d_flow"], v["d_info"])
        ctx.sync()
        ctx.check_launch()
    check(_form_plan(f"lk_track_device n={n}", "pagk_lk_track_device", dict(cap=CAP), dict(d_pt_ref=pts, d_n=np.array([n], I32)),
                     dict(d_pt_out=(CAP, 2), d_status=(CAP,), d_status_raw=(CAP,), d_err=(CAP,), d_flow=(CAP, 2), d_info=(8,)), run,
                     {"d_" + k: want[k] for k in lu.KEYS}, ("d_status_raw", "d_flow"),
                     {k: n for k in ("d_pt_out", "d_status", "d_status_raw", "d_err", "d_flow")}))


# -- geometry
def _correspondences(n):
    """n points under a homography plus noise; every fifth one an outlier (test_host_forms_gpu._correspondences)."""
    rng = np.random.default_rng(41)
    p1 = np.column_stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)])
    Hm = np.array([[1.01, 0.02, 3.0], [-0.015, 0.99, -2.0], [1e-5, -2e-5, 1.0]])
    q = np.column_stack([p1, np.ones(n)]) @ Hm.T
    p2 = q[:, :2] / q[:, 2:] + rng.normal(0, 0.3, (n, 2))
    p2[::5] += rng.uniform(-40, 40, p2[::5].shape)
    return np.ascontiguousarray(p1, F32), np.ascontiguousarray(p2, F32), Hm


@pytest.mark.parametrize("n", COUNTS)
def test_geometry_scores_device(ctx, n):
    p1, p2, Hm = _correspondences(n)
    H21, H12 = np.ascontiguousarray(Hm), np.ascontiguousarray(np.linalg.inv(Hm))
    F21 = np.ascontiguousarray([[0, -1e-4, 0.01], [1e-4, 0, -0.02], [-0.01, 0.02, 0.3]], F64)
    inH, sH = orc.check_homography(H21, H12, p1, p2, 1.0)
    inF, sF = orc.check_fundamental(F21, p1, p2, 1.0)
    if n == 65:
        assert 1 <= int(inH.sum()) < n

    def run(v, null):
        ctx.geometry_scores_device(H21, H12, F21, n, v["d_pts1"], v["d_pts2"], 1.0, v["d_inliers_H"], v["d_inliers_F"], v["d_scores"])
        ctx.sync()
        ctx.check_launch()
    check(_form_plan(f"geometry_scores_device n={n}", "pagk_geometry_scores_device", dict(n=n), dict(d_pts1=p1, d_pts2=p2),
                     dict(d_inliers_H=(n,), d_inliers_F=(n,), d_scores=(2,)), run,
                     dict(d_inliers_H=inH[:n], d_inliers_F=inF[:n], d_scores=np.array([sH, sF], F32))))


FIT = dict(seed=7, iters_H=96, iters_F=48)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("with_status", [False, True])
def test_geometry_fit_device(ctx, refs, n, with_status):
    p1, p2, _ = _correspondences(n)
    st = (np.arange(n) % 7 != 3).astype(U8) if with_status else None
    want = ftu.ref_fit(refs.fit, ftu.params(**FIT), p1, p2, st)
    if n == 65:
        assert want["H"]["status"] == 1 and want["H"]["best_count"] >= 30
    fp = capi.fit_params_default(**FIT)

    def run(v, null):
        ctx.geometry_fit_device(fp, n, v["d_pts1"], v["d_pts2"], v.get("d_status"), v["d_models"], v["d_mask_H"], v["d_mask_F"],
                                v["d_info"], v["d_hyp_counts"])
        ctx.sync()
        ctx.check_launch()
    ins = dict(d_pts1=p1, d_pts2=p2, **(dict(d_status=st) if with_status else {}))
    check(_form_plan(f"geometry_fit_device n={n} status {with_status}", "pagk_geometry_fit_device", dict(n=n, iters_H=96, iters_F=48), ins,
                     dict(d_models=(27,), d_mask_H=(n,), d_mask_F=(n,), d_info=(12,), d_hyp_counts=(144,)), run,
                     dict(d_models=want["models"], d_mask_H=want["mask_H"], d_mask_F=want["mask_F"], d_info=want["info"],
                          d_hyp_counts=want["hyp_counts"]), ("d_mask_H", "d_mask_F", "d_hyp_counts")))


@pytest.mark.parametrize("n", COUNTS)
def test_geometry_validation_device(ctx, refs, n):
    p1, p2, _ = _correspondences(n)
    st = (np.arange(n) % 7 != 3).astype(U8)
    fit = ftu.ref_fit(refs.fit, ftu.params(**FIT), p1, p2, st)
    if n == 65:
        assert fit["H"]["status"] == 1 and fit["F"]["status"] == 1
        cnt, st_out, score = orc.geometry_validation(fit["H21"], fit["H12"], fit["F21"], p1, p2, st, 1.0)
        assert 8 < cnt < int(st.sum())
    else:          # at most 8 points take part: nothing changes, both outputs 0
        cnt, st_out, score = 0, st.copy(), F32(0)
    fp = capi.fit_params_default(**FIT)

    def run(v, null):
        ctx.geometry_validation_device(fp, n, v["d_pt_ref_un"], v["d_pt_predict_un"], v["d_status"], 1.0, v["d_cnt"], v["d_score"])
        ctx.sync()
        ctx.check_launch()
    check(_form_plan(f"geometry_validation_device n={n}", "pagk_geometry_validation_device", dict(n=n),
                     dict(d_pt_ref_un=p1, d_pt_predict_un=p2), dict(d_status=st, d_cnt=(1,), d_score=(1,)), run,
                     dict(d_status=st_out, d_cnt=np.array([cnt], I32), d_score=np.array([score], F32))))


# -- pose
SMALL_FIT = dict(iters_H=32, iters_F=32)   # test_pose_gpu.SMALL_FIT
ITERS_E = 17


def _pose_want(refs, seed, p1, p2, st):
    pose = pu.ref_pose(refs.pose, pu.params(seed=seed, iters_E=ITERS_E), p1, p2, st, cand_counts=True)
    fit = ftu.ref_fit(refs.fit, ftu.params(seed=seed, **SMALL_FIT), p1, p2, st)
    return pose, fit


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("with_status", [False, True])
def test_pose_2d2d_device(ctx, refs, n, with_status):
    g = make_geometry_case(700, 65, outlier_fraction=0.25, noise_px=0.3, planar=False, translation=pu.WIDE)
    p1, p2 = np.ascontiguousarray(g["pts1"][:n]), np.ascontiguousarray(g["pts2"][:n])
    st = (np.arange(n) % 7 != 3).astype(U8) if with_status else None
    pose, fit = _pose_want(refs, 11, p1, p2, st)
    if n == 65:
        assert pose["info"]["status"] == 1 and int(pose["mask_pose"].sum()) >= 1
    pp = capi.pose_params_default(seed=11, fit=capi.fit_params_default(seed=11, **SMALL_FIT), iters_E=ITERS_E)

    def run(v, null):
        ctx.pose_2d2d_device(pp, pu.F, pu.CX, pu.CY, n, v["d_pts1"], v["d_pts2"], v.get("d_status"), v["d_models"], v["d_pose"],
                             v["d_mask_H"], v["d_mask_F"], v["d_mask_E"], v["d_mask_pose"], v["d_fit_info"], v["d_pose_info"],
                             v["d_cand_counts"])
        ctx.sync()
        ctx.check_launch()
    ins = dict(d_pts1=p1, d_pts2=p2, **(dict(d_status=st) if with_status else {}))
    check(_form_plan(f"pose_2d2d_device n={n} status {with_status}", "pagk_pose_2d2d_device", dict(n=n, iters_E=ITERS_E), ins,
                     dict(d_models=(27,), d_pose=(21,), d_mask_H=(n,), d_mask_F=(n,), d_mask_E=(n,), d_mask_pose=(n,), d_fit_info=(12,),
                          d_pose_info=(16,), d_cand_counts=(ITERS_E, 10)), run,
                     dict(d_models=fit["models"], d_pose=pose["pose"], d_mask_H=fit["mask_H"], d_mask_F=fit["mask_F"],
                          d_mask_E=pose["mask_E"], d_mask_pose=pose["mask_pose"], d_fit_info=fit["info"], d_pose_info=pose["pose_info"],
                          d_cand_counts=pose["cand_counts"]),
                     ("d_mask_H", "d_mask_F", "d_mask_E", "d_mask_pose", "d_cand_counts")))


@pytest.mark.parametrize("nq", COUNTS)
def test_pose_from_matches_device(ctx, refs, nq):
    """The gather of the header in numpy (pts1[q] = kp_ref[q], pts2[q] = kp_cur[train_idx[q]], status[q] = q < nq && keep[q] &&
    0 <= train_idx[q] < nt), then the restatements of pagk_pose_2d2d_device with n = cap_q."""
    cap_q, cap_t, nt = 80, 70, 65
    g = make_geometry_case(701, 65, outlier_fraction=0.25, noise_px=0.3, planar=False, translation=pu.WIDE)
    rng = np.random.default_rng(5)
    perm = rng.permutation(65)
    kp_ref, kp_cur = np.zeros((cap_q, 2), F32), np.zeros((cap_t, 2), F32)
    kp_ref[:65], kp_cur[perm] = g["pts1"], g["pts2"]
    idx = np.zeros(cap_q, I32)
    idx[:65] = perm
    idx[3], idx[9], idx[12] = -1, nt, cap_t + 5      # no match; beyond the live count; beyond the array
    keep = (rng.random(cap_q) < 0.9).astype(U8)
    q = np.arange(cap_q)
    st = ((q < nq) & (keep > 0) & (idx >= 0) & (idx < nt)).astype(U8)
    p2 = np.ascontiguousarray(kp_cur[np.clip(idx, 0, cap_t - 1)])
    pose, fit = _pose_want(refs, 11, kp_ref, p2, st)
    if nq == 65:
        assert pose["info"]["status"] == 1
    pp = capi.pose_params_default(seed=11, fit=capi.fit_params_default(seed=11, **SMALL_FIT), iters_E=ITERS_E)

    def run(v, null):
        ctx.pose_from_matches_device(pp, pu.F, pu.CX, pu.CY, cap_q, v["d_kp_ref"], v["d_nq"], cap_t, v["d_kp_cur"], v["d_nt"],
                                     v["d_train_idx"], v["d_keep"], v["d_models"], v["d_pose"], v["d_mask_H"], v["d_mask_F"],
                                     v["d_mask_E"], v["d_mask_pose"], v["d_fit_info"], v["d_pose_info"])
        ctx.sync()
        ctx.check_launch()
    check(_form_plan(f"pose_from_matches_device nq={nq}", "pagk_pose_from_matches_device", dict(cap_q=cap_q, cap_t=cap_t),
                     dict(d_kp_ref=kp_ref, d_nq=np.array([nq], I32), d_kp_cur=kp_cur, d_nt=np.array([nt], I32), d_train_idx=idx,
                          d_keep=keep),
                     dict(d_models=(27,), d_pose=(21,), d_mask_H=(cap_q,), d_mask_F=(cap_q,), d_mask_E=(cap_q,), d_mask_pose=(cap_q,),
                          d_fit_info=(12,), d_pose_info=(16,)), run,
                     dict(d_models=fit["models"], d_pose=pose["pose"], d_mask_H=fit["mask_H"], d_mask_F=fit["mask_F"],
                          d_mask_E=pose["mask_E"], d_mask_pose=pose["mask_pose"], d_fit_info=fit["info"], d_pose_info=pose["pose_info"]),
                     ("d_mask_H", "d_mask_F", "d_mask_E", "d_mask_pose")))


# -- neighbours and association
NBR_CAP = 16


def _neighbour_inputs(n, m=65):
    """test_host_forms_gpu._neighbour_inputs: the 97 x 80 texture pair, n reference keypoints, m current ones."""
    ref, cur = lu.texture_pair(synth, W, H, 31, (0.7, -0.4))
    kr = lu.interior_points(W, H, n, 8, 3)
    pu_ = (kr + F32([0.7, -0.4])).astype(F32)
    kc = np.concatenate([pu_[:m // 2] + F32([1.5, 0.5]), lu.interior_points(W, H, m - min(n, m // 2), 8, 4)]).astype(F32)
    st = (np.arange(n) % 5 != 2).astype(U8)
    aff = np.tile(F32([1.02, 0.01, -0.01, 0.98]), (n, 1))
    return ref, cur, np.ascontiguousarray(kr), pu_, np.ascontiguousarray(kc), st, np.ascontiguousarray(aff)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("with_affine", [False, True])
def test_near_neighbors_device(ctx, n, with_affine):
    ref, cur, kr, pu_, kc, st, aff = _neighbour_inputs(n)
    m = int(kc.shape[0])
    want = orc.find_near_neighbors(ref, cur, 5, kr, pu_, st, aff if with_affine else None, kc, kc, level=1, radius_unit=10.0,
                                   cap=NBR_CAP)
    assert want["rc"] == 0 and (n < 65 or 1 <= want["count"].max() < NBR_CAP)
    ctx.frame_upload(0, ref, 1)
    ctx.frame_upload(1, cur, 1)
    init = dict(d_count=np.zeros(n, I32), d_nbr_idx=np.full((n, NBR_CAP), -1, I32), d_nbr_dist=np.zeros((n, NBR_CAP), F32),
                d_nbr_ncc=np.zeros((n, NBR_CAP), F32))      # in/out: the entries beyond a list's count keep the caller's content

    def run(v, null):
        ctx.near_neighbors_device(0, 1, 5, n, v["d_keys_ref"], v["d_pt_predict_un"], v["d_status"], v.get("d_affine"), m,
                                  v["d_keys_cur"], v["d_keys_cur_un"], 1, 10.0, 1, NBR_CAP, v["d_count"], v["d_nbr_idx"],
                                  v["d_nbr_dist"], v["d_nbr_ncc"])
        ctx.sync()
        ctx.check_launch()
    ins = dict(d_keys_ref=kr, d_pt_predict_un=pu_, d_status=st, d_keys_cur=kc, d_keys_cur_un=kc, **(dict(d_affine=aff) if with_affine else {}))
    check(_form_plan(f"near_neighbors_device n={n} affine {with_affine}", "pagk_near_neighbors_device", dict(n=n, m=m, cap=NBR_CAP), ins,
                     init, run, dict(d_count=want["count"][:n], d_nbr_idx=want["idx"][:n], d_nbr_dist=want["dist"][:n],
                                     d_nbr_ncc=want["ncc"][:n])))


@pytest.mark.parametrize("n", COUNTS)
def test_match_features_device(ctx, refs, n):
    m, cap = 65, 8
    count, idx, dist, ncc = au.random_lists(0x3A7 + n, n, m, cap)
    want = au.ref_match(refs.assoc, count, idx, dist, ncc, m)
    k = int(want["k"])
    assert (n < 65 or 1 <= k < n) and (want["query"][k:] == -1).all()
    ap = capi.assoc_params_default()

    def run(v, null):
        ctx.match_features_device(ap, n, m, cap, v["d_count"], v["d_nbr_idx"], v["d_nbr_dist"], v["d_nbr_ncc"], v["d_match_query"],
                                  v["d_match_train"], v["d_match_dist"], v["d_match_ncc"], v["d_n_matches"], v["d_info"])
        ctx.sync()
        ctx.check_launch()
    check(_form_plan(f"match_features_device n={n}", "pagk_match_features_device", dict(n=n, cap=cap),
                     dict(d_count=count, d_nbr_idx=idx, d_nbr_dist=dist, d_nbr_ncc=ncc),
                     dict(d_match_query=(n,), d_match_train=(n,), d_match_dist=(n,), d_match_ncc=(n,), d_n_matches=(1,), d_info=(8,)), run,
                     dict(d_match_query=want["query"], d_match_train=want["train"], d_match_dist=want["dist"], d_match_ncc=want["ncc"],
                          d_n_matches=np.array([k], I32), d_info=want["info"]), ("d_match_dist", "d_match_ncc"),
                     {name: k for name in ("d_match_query", "d_match_train", "d_match_dist", "d_match_ncc")}))


def _restated_search(refs, ref, cur, kr, pu_, st, aff, kc, min_matches, ru_):
    """Steps 2 and 3 of SearchByGyroPredict from the oracle's neighbour search and the restated MatchFeatures: level 1, choose
    and compact, level 2 for the empty lists when fewer than min_matches came out, choose and compact again."""
    m = int(kc.shape[0])
    args = (ref, cur, 5, kr, pu_, st, aff, kc, kc)
    lists = orc.find_near_neighbors(*args, level=1, radius_unit=ru_, cap=NBR_CAP)
    assert lists["rc"] == 0
    match = au.ref_match(refs.assoc, lists["count"], lists["idx"], lists["dist"], lists["ncc"], m, keys_cur_un=kc, pt_pred=pu_)
    ran2 = int(int(match["k"]) < min_matches)
    if ran2:
        r2 = orc.find_near_neighbors(*args, level=2, radius_unit=ru_, cap=NBR_CAP, count=lists["count"])
        assert r2["rc"] == 0
        keep = lists["count"] > 0
        for key in ("idx", "dist", "ncc"):
            r2[key][keep] = lists[key][keep]
        lists = r2
        match = au.ref_match(refs.assoc, lists["count"], lists["idx"], lists["dist"], lists["ncc"], m, keys_cur_un=kc, pt_pred=pu_)
    match["info"] = match["info"].copy()
    match["info"][5] = ran2
    return lists, match, ran2


@pytest.mark.parametrize("min_matches", [0, 100])
@pytest.mark.parametrize("n", COUNTS)
def test_search_gyro_predict_device(ctx, refs, n, min_matches):
    ref, cur, kr, pu_, kc, st, aff = _neighbour_inputs(n)
    m, ru_ = int(kc.shape[0]), 3.0
    lists, match, ran2 = _restated_search(refs, ref, cur, kr, pu_, st, aff, kc, min_matches, ru_)
    k = int(match["k"])
    assert ran2 == int(min_matches > 0) and (n < 65 or 1 <= k < n) and lists["count"].max(initial=0) < NBR_CAP
    ctx.frame_upload(0, ref, 1)
    ctx.frame_upload(1, cur, 1)
    ap = capi.assoc_params_default(min_matches=min_matches)
    live = np.arange(NBR_CAP)[None, :] < lists["count"][:n, None]      # the entries of a list; the others are left untouched

    def lists_of(key):
        return lambda s: np.where(live, lists[key][:n], s)

    def run(v, null):
        ctx.search_gyro_predict_device(ap, 0, 1, 5, n, v["d_keys_ref"], v["d_pt_predict_un"], v["d_status"], v["d_affine"], m,
                                       v["d_keys_cur"], v["d_keys_cur_un"], v["d_m"], ru_, NBR_CAP, v["d_count"], v["d_nbr_idx"],
                                       v["d_nbr_dist"], v["d_nbr_ncc"], v["d_match_query"], v["d_match_train"], v["d_match_dist"],
                                       v["d_match_ncc"], v["d_n_matches"], v["d_flows_err"], v["d_info"])
        ctx.sync()
        ctx.check_launch()
    check(_form_plan(f"search_gyro_predict_device n={n} min_matches {min_matches}", "pagk_search_gyro_predict_device",
                     dict(n=n, m=m, cap=NBR_CAP),
                     dict(d_keys_ref=kr, d_pt_predict_un=pu_, d_status=st, d_affine=aff, d_keys_cur=kc, d_keys_cur_un=kc,
                          d_m=np.array([m], I32)),
                     dict(d_count=(n,), d_nbr_idx=(n, NBR_CAP), d_nbr_dist=(n, NBR_CAP), d_nbr_ncc=(n, NBR_CAP), d_match_query=(n,),
                          d_match_train=(n,), d_match_dist=(n,), d_match_ncc=(n,), d_n_matches=(1,), d_flows_err=(n, 2), d_info=(8,)),
                     run,
                     dict(d_count=lists["count"][:n], d_nbr_idx=lists_of("idx"), d_nbr_dist=lists_of("dist"), d_nbr_ncc=lists_of("ncc"),
                          d_match_query=match["query"], d_match_train=match["train"], d_match_dist=match["dist"],
                          d_match_ncc=match["ncc"], d_n_matches=np.array([k], I32), d_flows_err=match["flows"], d_info=match["info"]),
                     ("d_match_dist", "d_match_ncc", "d_flows_err"),
                     {name: k for name in ("d_match_query", "d_match_train", "d_match_dist", "d_match_ncc")}))


@pytest.mark.parametrize("n", COUNTS)
def test_search_klt_device(ctx, refs, n):
    """pagk_lk_track_device's restatement, then the restated association on its points."""
    a, b, pts = _lk_case()
    m = 65
    track = lu.ref_track(refs.lk, a, b, pts, lu.params(**LK), cap=CAP, n=n)
    rng = np.random.default_rng(8)
    kc = (track["pt_out"][:m] + rng.normal(0, 1.5, (m, 2))).astype(F32)     # detections near the tracked points, some beyond 4 px
    kc[::4] = lu.interior_points(96, 64, len(kc[::4]), 3, 9)
    want = au.ref_klt(refs.assoc, CAP, n, track["status"], track["pt_out"], pts, kc)
    k = int(want["k"])
    assert (n < 65 or 1 <= k < n) and (want["query"][k:] == -1).all()
    lk, ap = capi.lk_params_default(**LK), capi.assoc_params_default()
    for slot, img in ((0, a), (1, b)):
        ctx.frame_upload(slot, img, 1)
        ctx.lk_pyramid_device(lk, slot)

    def run(v, null):
        ctx.search_klt_device(lk, ap, 0, 1, CAP, v["d_keys_ref"], v["d_n"], m, v["d_keys_cur"], v["d_m"], v["d_pt_out"], v["d_status"],
                              v["d_err"], v["d_match_query"], v["d_match_train"], v["d_match_dist"], v["d_disparity"],
                              v["d_n_matches"], v["d_stats"], v["d_info"], v["d_lk_info"])
        ctx.sync()
        ctx.check_launch()
    check(_form_plan(f"search_klt_device n={n}", "pagk_search_klt_device", dict(cap=CAP, m=m),
                     dict(d_keys_ref=pts, d_n=np.array([n], I32), d_keys_cur=kc, d_m=np.array([m], I32)),
                     dict(d_pt_out=(CAP, 2), d_status=(CAP,), d_err=(CAP,), d_match_query=(CAP,), d_match_train=(CAP,),
                          d_match_dist=(CAP,), d_disparity=(CAP,), d_n_matches=(1,), d_stats=(8,), d_info=(8,), d_lk_info=(8,)), run,
                     dict(d_pt_out=track["pt_out"], d_status=track["status"], d_err=track["err"], d_match_query=want["query"],
                          d_match_train=want["train"], d_match_dist=want["dist"], d_disparity=want["disparity"],
                          d_n_matches=np.array([k], I32), d_stats=want["stats"], d_info=want["info"], d_lk_info=track["info"]),
                     ("d_match_dist",),
                     dict(d_pt_out=n, d_status=n, d_err=n, d_match_query=k, d_match_train=k, d_match_dist=k, d_disparity=k)))
