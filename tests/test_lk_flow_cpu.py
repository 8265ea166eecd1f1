"""CPU tests of the flow form of pyramidal Lucas-Kanade (pagk_lk_track_flow, kernel k_lk_flow): the plain-C restatement
tests/lk_flow_ref.c against a numpy model of the addendum in include/pagk.h, byte for byte, on the flow edge table; the
identity with tests/lk_ref.c (flags = 0) on the whole edge table of tests/lk_ref_util.py; that the flow table is not vacuous;
the boundary (header, bindings, argument checks that need no device); the restatement under the sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lk_flow_ref_util as fu
import lk_ref_util as lu
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, host_api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pixel_aware_gyro_aided_klt_feature_tracker_amd", "csrc")


@pytest.fixture(scope="module")
def flow_ref(tmp_path_factory):
    return fu.build_ref(tmp_path_factory.mktemp("lk_flow_ref"))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return lu.build_ref(tmp_path_factory.mktemp("lk_ref"))


@pytest.fixture(scope="module")
def table():
    return fu.flow_edge_shapes(synth)


@pytest.fixture(scope="module")
def restated(flow_ref, table):
    """(name, flow) -> the restatement of a case of the flow table, computed once and left unchanged."""
    memo = {}

    def get(name, flow=True):
        if (name, flow) not in memo:
            memo[(name, flow)] = fu.run_case(lambda *a, **kw: fu.ref_flow(flow_ref, *a, **kw), table[name], flow)
        return memo[(name, flow)]
    return get


# ---- the boundary --------------------------------------------------------------------------------------------------------
def test_header_declares_and_capi_binds_the_flow_form(built):
    hdr = open(os.path.join(ROOT, "include", "pagk.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = capi.load()
    name = "pagk_lk_track_flow"
    assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name) and len(getattr(lib, name).argtypes) == 16
    assert re.search(r"\bint " + name + r"\s*\(", code)
    decl = hdr.index("int " + name + "(")
    comment = hdr[:decl].rsplit("/*", 1)[1]
    assert "src/gyro_aided_tracker.cpp:353-380" in comment and comment.rstrip().endswith("*/")
    assert not re.search(r"device\s+pointer", comment)
    params = re.search(r"int " + name + r"\((.*?)\);", code, flags=re.S).group(1)
    names = [p.split()[-1].lstrip("*") for p in params.split(",")]
    assert names == ["ctx", "params", "cam", "ref", "cur", "n", "pt_ref", "pt_init", "status_in", "pt_out", "pt_out_dist", "status",
                     "status_raw", "err", "flow", "info"]
    assert not any(p.startswith("d_") for p in names)
    assert "#define PAGK_VERSION 303" in hdr
    # the addendum stands in the Lucas-Kanade section, behind the definition it amends, whose sentences are all still there
    section = hdr[hdr.index("Pyramidal Lucas-Kanade: tracker type 0"):hdr.index("typedef struct pagk_lk_params")]
    for word in ("OPTFLOW_USE_INITIAL_FLOW", "next = pt_init 2^-L", "status_in", "tests/lk_flow_ref.c", "src/utils.cpp:49-76",
                 ":131-139", ":364-365", "byte for byte", "At the top level next = prev", "NOT claimed", "EXACT integers"):
        assert word in section, word
    assert "Not provided: OPTFLOW_USE_INITIAL_FLOW" not in hdr
    assert callable(capi.Context.lk_track_flow) and callable(host_api.lk_track_flow)


def test_one_body_and_a_chooser_of_its_own():
    """Both kernels are the text of csrc/pagk_lk_body.h, included once in each (the file says why it is text and not a
    function); the flow chooser mirrors lk_kernel outside the text tests/test_lk_cpu.py pins."""
    hdr = open(os.path.join(CSRC, "pagk_lk_kernel.h")).read()
    kernels = re.findall(r"__global__[^\n]*void (k_lk_(?:track|flow))\((\w+) (\w)\)\n\{\n(.*?)\n\}\n", hdr, flags=re.S)
    assert [(k[0], k[1]) for k in kernels] == [("k_lk_track", "LkTrackArgs"), ("k_lk_flow", "LkFlowArgs")]
    for name, _, _, text in kernels:
        flow = int(name == "k_lk_flow")
        lines = [ln.strip() for ln in text.split("\n")]
        assert lines[-3:] == [f"#define PAGK_LK_FLOW {flow}", '#include "pagk_lk_body.h"', "#undef PAGK_LK_FLOW"], name
        assert len(lines) == 3 + flow, name                       # nothing but the include (and the flow kernel's `a`)
    body = open(os.path.join(CSRC, "pagk_lk_body.h")).read()
    assert "#pragma once" not in body and "lk_wave_sum" in body and "lk_distort_point(f, nx, ny, ox, oy)" in body
    assert body.count("#if PAGK_LK_FLOW") == 4 and "k_track_" not in hdr + body and "__syncthreads" not in hdr + body
    host = open(os.path.join(CSRC, "pagk_hip.hip")).read()
    pinned = host[host.index("LkKernel lk_kernel(int win)"):host.index("int lk_track_slots(")]
    assert "k_lk_flow" not in pinned
    chooser = host[host.index("LkFlowKernel lk_flow_kernel(int win)"):host.index("int lk_flow_slots(")]
    assert "switch (lk_npix(win))" in chooser
    assert re.findall(r"case (\d+): return k_lk_flow<(\d+)>;", chooser) == [(str(n), str(n)) for n in (1, 2, 4, 8)]
    assert re.findall(r"default: return k_lk_flow<(\d+)>;", chooser) == ["16"]
    assert "hipLaunchKernelGGL(lk_flow_kernel(f.t.win)," in host


def test_null_arguments_are_refused_without_a_device(built):
    lib = capi.load()
    p, cam = capi.lk_params_default(), capi.make_params(camera=synth.D435I)
    one = np.zeros(16, np.float32)
    img = capi.image_view(np.zeros((64, 64), np.uint8))
    a = one.ctypes.data
    call = lambda ctx, lk, ref, cur: lib.pagk_lk_track_flow(ctx, lk, C.byref(cam), ref, cur, 1, a, a, a, a, a, a, a, a, a, a)  # noqa: E731
    assert call(None, C.byref(p), C.byref(img), C.byref(img)) == capi.PAGK_E_ARG
    assert lib.pagk_lk_track_flow(None, None, None, None, None, 0, *([None] * 10)) == capi.PAGK_E_ARG


def test_parameter_check_matrix(built):
    """Every field of pagk_lk_params the flow form reads, at both ends of its range and one step outside."""
    ok = [dict(half_patch=1), dict(half_patch=15), dict(max_level=0), dict(max_level=7), dict(max_count=1), dict(epsilon=0.0),
          dict(min_eig_threshold=0.0), dict(err_threshold=0.0)]
    bad = [dict(half_patch=0), dict(half_patch=16), dict(max_level=-1), dict(max_level=8), dict(max_count=0), dict(epsilon=-1e-9),
           dict(epsilon=float("nan")), dict(epsilon=float("inf")), dict(min_eig_threshold=-1.0),
           dict(min_eig_threshold=float("inf")), dict(err_threshold=-1.0), dict(err_threshold=float("nan"))]
    for kw in ok:
        assert capi.lk_params_check(capi.lk_params_default(**kw)) == capi.PAGK_OK, kw
    for kw in bad:
        assert capi.lk_params_check(capi.lk_params_default(**kw)) == capi.PAGK_E_ARG, kw
    # the camera comes from a pagk_params, which has to pass its own check
    assert capi.params_check(capi.make_params(camera=synth.D435I)) == capi.PAGK_OK
    assert capi.params_check(capi.make_params(half_patch=0)) == capi.PAGK_E_ARG


# ---- restatement against model ---------------------------------------------------------------------------------------------
def test_restatement_and_model_agree_on_the_flow_table(table, restated):
    for name, c in table.items():
        r = restated(name)
        m = fu.run_case(fu.model_flow, c)
        assert lu.differing(r, m, fu.KEYS + ("iters", "why")) == [], name
        n, cap = c["n"], c["cap"]
        assert r["info"][0] == n < cap and r["info"][7] == 0, name
        skipped = (c["live"][:n] == 0)
        assert r["info"][6] == skipped.sum() > 0, name
        assert r["info"][1] == r["status_raw"].sum() and r["info"][2] == r["status"].sum(), name
        zero = np.ones(cap, bool)
        zero[:n] = skipped
        for key in ("pt_out", "pt_out_dist", "status", "status_raw", "err", "flow", "iters", "why"):
            assert not r[key][zero].any(), (name, key)                    # rows beyond the count and skipped rows alike
        assert not r["status_raw"][:n][skipped].any() and r["why"][:n][~skipped, 0].all(), name


def test_flow_table_is_what_it_says(table, restated):
    wins = {}
    cams = set()
    for name, c in table.items():
        h, w = c["ref"].shape
        win = 2 * c["p"]["half_patch"] + 1
        assert c["npix"] == lu.NPIX_OF_WIN[win] and f"win{win} npix{c['npix']} {c['kind']}" in name, name
        top = restated(name)["info"][3]
        assert (top, (w, h) == (win + 1, win + 1)) == ((0, True) if c["kind"] == "minimal" else (2, False)), name
        wins.setdefault(win, set()).add(c["kind"])
        cams.add((c["cam"]["n"], c["cam"]["dist"][0] == 0))
        n = c["n"]
        d = c["init"][:n] - c["pts"][:n]
        live = c["live"][:n] != 0
        finite = np.isfinite(c["pts"][:n]).all(axis=1)
        assert 0 < (~live).sum() < n // 2, name                            # a mix of status_in values
        with np.errstate(invalid="ignore"):
            kinds = [(d == 0).all(axis=1), (np.abs(d) < 1).all(axis=1) & (d != 0).all(axis=1), (d < -1).all(axis=1),
                     (d >= 2 * win).all(axis=1), np.isinf(c["init"][:n]).any(axis=1), np.isnan(c["init"][:n]).any(axis=1)]
        for kind, rows in zip(fu.OFFSETS, kinds):
            assert (rows & live & (finite | (kind in ("inf", "nan")))).sum() >= 2, (name, kind)   # every offset on live rows
    assert wins == {win: {"minimal", "three levels"} for win in (3, 7, 9, 11, 13, 15, 17, 21, 23, 31)}
    assert cams == {(4, False), (5, False), (5, True)}                     # four, five coefficients, and k1 == 0


def test_flow_table_is_not_vacuous(table, restated):
    """On the restatement: the initial point changes some result; some feature is lost out of range at level 0 in flow mode
    alone; status_in skips rows; the far initial point leaves the top level of a three-level frame at its first tile; the
    distorted point differs from the point where the camera distorts and equals it where k1 == 0."""
    moved = lost_only_in_flow = skipped = far_top = distorted = copied = 0
    for name, c in table.items():
        f, z = restated(name), restated(name, flow=False)
        n = c["n"]
        live = c["live"][:n] != 0
        both = live & (f["status_raw"][:n] == 1) & (z["status_raw"][:n] == 1)
        moved += int((f["pt_out"][:n][both] != z["pt_out"][:n][both]).any(axis=1).sum())
        lost_only_in_flow += int((live & (f["why"][:n, 0] == lu.RANGE) & (z["why"][:n, 0] != lu.RANGE) &
                                  (z["why"][:n, 0] != lu.TEMPLATE)).sum())
        skipped += int(f["info"][6])
        assert z["info"][6] == 0, name
        if c["kind"] == "three levels":
            far = np.arange(n) % len(fu.OFFSETS) == fu.OFFSETS.index("far")
            far_top += int((live & far & (f["why"][:n, 2] == lu.RANGE) & (f["iters"][:n] == 0)).sum())
        tracked = live & np.isfinite(f["pt_out"][:n]).all(axis=1)
        same = (f["pt_out_dist"][:n][tracked] == f["pt_out"][:n][tracked]).all(axis=1)
        if c["cam"]["dist"][0] == 0:
            assert same.all(), name
            copied += int(same.sum())
        else:
            distorted += int((~same).sum())
    print(f"moved {moved}, lost to range in flow mode alone {lost_only_in_flow}, skipped {skipped}, far at the top level "
          f"{far_top}, distorted {distorted}, copied {copied}")
    assert moved > 0 and lost_only_in_flow > 0 and skipped > 0 and far_top > 0 and distorted > 0 and copied > 0


def test_identity_with_the_flags_0_restatement_on_its_whole_edge_table(flow_ref, ref):
    """pt_init = pt_ref (given and NULL) and no mask (NULL and all ones): tests/lk_flow_ref.c equals tests/lk_ref.c on every
    case of lk_ref_util.edge_shapes(), the record of every level's exit included."""
    for name, c in lu.edge_shapes(synth).items():
        want = lu.ref_track(ref, c["ref"], c["cur"], c["pts"], c["p"], c["cap"], c["n"])
        got = fu.ref_flow(flow_ref, c["ref"], c["cur"], c["pts"], c["p"], cap=c["cap"], n=c["n"])
        assert lu.differing(got, want, lu.KEYS + ("iters", "why")) == [], name
        got = fu.ref_flow(flow_ref, c["ref"], c["cur"], c["pts"], c["p"], pt_init=c["pts"].copy(),
                          status_in=np.full(len(c["pts"]), 3, np.uint8), cap=c["cap"], n=c["n"])
        assert lu.differing(got, want, lu.KEYS + ("iters", "why")) == [], name
        assert got["info"][6] == 0


def test_distortion_by_hand(flow_ref):
    """One point through DistortVecPoints in Python floats rounded per operation, against the restatement's pt_out_dist."""
    a, _ = lu.texture_pair(synth, 48, 36, 8)
    pts = np.array([[40.5, 6.25]], np.float32)
    cam = dict(fx=61.5, fy=59.25, cx=23.5, cy=17.75, dist=(-0.2834, 0.0739, 0.00019, 1.76e-05, -0.0112), n=5)
    r = fu.ref_flow(flow_ref, a, a, pts, lu.params(half_patch=2), cam=cam)
    assert r["status_raw"][0] == 1 and lu.same_array(r["pt_out"], pts)
    F = np.float32
    fx, fy, cx, cy = (F(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    k1, k2, p1, p2, k3 = (F(v) for v in cam["dist"])
    x, y = (F(40.5) - cx) * F(1.0 / float(fx)), (F(6.25) - cy) * F(1.0 / float(fy))
    r2 = x * x + y * y
    r4 = r2 * r2
    r6 = r4 * r2
    rad = F(1) + k1 * r2 + k2 * r4 + k3 * r6
    xd = x * rad + F(2) * p1 * x * y + p2 * (r2 + F(2) * x * x)
    yd = y * rad + p1 * (r2 + F(2) * y * y) + F(2) * p2 * x * y
    assert lu.same_array(r["pt_out_dist"], np.array([[fx * xd + cx, fy * yd + cy]], np.float32))
    assert not lu.same_array(r["pt_out_dist"], r["pt_out"])
    four = dict(cam, n=4)                                                       # k3 is read with five coefficients only
    r4c = fu.ref_flow(flow_ref, a, a, pts, lu.params(half_patch=2), cam=four)
    assert not lu.same_array(r4c["pt_out_dist"], r["pt_out_dist"])
    assert lu.same_array(r4c["pt_out_dist"], fu.model_distort(pts, four))


# ---- sanitizers ----------------------------------------------------------------------------------------------------------
def test_flow_restatement_runs_clean_under_the_sanitizers(tmp_path):
    """A stand-alone program (tests/lk_flow_sanitize.c: its own main, compiled together with tests/lk_flow_ref.c) runs the
    restatement on frames of the flow table's sizes under AddressSanitizer and UBSan, every array in a heap block of exactly
    its size."""
    exe = str(tmp_path / "lk_flow_sanitize")
    subprocess.run(["gcc", "-std=c99", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "lk_flow_sanitize.c"),
                    os.path.join(ROOT, "tests", "lk_flow_ref.c"), "-o", exe, "-lm"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "20 frames" in r.stdout, r.stdout
