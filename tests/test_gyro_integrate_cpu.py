"""CPU tests of the gyro integration (include/pagk.h "Gyro integration", kernel k_gyro_integrate): the plain-C restatement
tests/gyro_integrate_ref.c against a numpy model of the definition, byte for byte, on the edge table; that the table reaches
every case and branch; the restatement against an f64 Rodrigues product of the same window; pagk_imu_window_check; the
boundary (header, bindings, argument checks that need no device); the restatement under the sanitizers."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import gyro_integrate_ref_util as gu
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, host_api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return gu.build_ref(tmp_path_factory.mktemp("gyro_integrate_ref"))


@pytest.fixture(scope="module")
def table():
    return gu.edge_table()


@pytest.fixture(scope="module")
def restated(ref, table):
    """name -> (Rcl, rot9) of the restatement, computed once and left unchanged."""
    return {name: gu.ref_integrate(ref, c) for name, c in table.items()}


def _window(c):
    return capi.imu_window(c["t_ref"], c["t_cur"], c["t"], c["w"], c["bias"])


# ---- the definition ------------------------------------------------------------------------------------------------------
def test_restatement_equals_the_numpy_model_on_the_edge_table(table, restated):
    for name, c in table.items():
        assert restated[name] is not None, name
        rcl, rot9 = gu.model_integrate(c)
        assert restated[name][0].tobytes() == rcl.tobytes(), name
        assert restated[name][1].tobytes() == rot9.tobytes(), name


def test_the_edge_table_reaches_every_case_and_branch(table, restated):
    counts = {len(c["t"]) for c in table.values()}
    assert {0, 1, 2, 3, 4, 5, 64} <= counts                      # n = 1: the fourth case; 2: first and last; >= 3: all of them
    for name in ("0 samples", "1 samples"):
        assert np.array_equal(restated[name][0], np.eye(3, dtype=np.float32)), name
    f32 = np.float32

    def d_of(name):                                              # the angle of the single step of a two-sample case
        c = table[name]
        g = (c["w"][0] - c["bias"]).astype(np.float64) * np.float64(f32(c["t_cur"] - c["t_ref"]))
        x, y, z = g.astype(f32)
        return float(np.sqrt((x * x + y * y) + z * z))
    assert d_of("d below 1e-4") < 1e-4 <= d_of("d just above 1e-4") < 1.001e-4
    quadrant = lambda d: int(d * float.fromhex("0x1.45f306dc9c883p-1") + 0.5) & 3     # noqa: E731
    assert {quadrant(d_of(n)) for n in ("d 0.8 rad", "d 2 rad", "d 3.5 rad", "d 5 rad", "d 7 rad")} == {0, 1, 2, 3}
    # the small-angle branch is I + W with Rbc = I: Rcl is its transpose, antisymmetric off the diagonal, exactly
    small = restated["d below 1e-4"][0]
    assert np.array_equal(np.diag(small), np.ones(3, f32)) and np.array_equal(small - np.eye(3, dtype=f32), -(small - np.eye(3, dtype=f32)).T)
    assert table["bias"]["bias"].any() and not np.array_equal(table["Rbc not I"]["Rbc"], np.eye(3, dtype=f32))
    assert table["t_0 = t_ref"]["t"][0] == table["t_0 = t_ref"]["t_ref"]
    gaps = np.diff(table["5 samples"]["t"])
    assert gaps.max() > 1.2 * gaps.min()                         # uneven spacing
    # every product matters: Rbc and the camera change the result
    assert restated["Rbc not I"][0].tobytes() != gu.model_integrate(dict(table["Rbc not I"], Rbc=gu.EYE))[0].tobytes()
    assert restated["other camera"][1].tobytes() != gu.model_integrate(dict(table["other camera"], camera=gu.CAMERA))[1].tobytes()


def test_restatement_against_an_f64_rodrigues_product(table, restated):
    """Not vacuous: Rcl of the restatement against the same window with every step and product in f64 (libm's sin and cos).
    Measured here on the CPU: the largest |difference| of an element over the table is 4.90e-07 (the 64-sample window; the
    f32 chain's error grows with the number of steps: 2.3e-08 for one step of the generic windows, 8.8e-08 for four).  The
    bound is 4 x that maximum."""
    bound = 4 * 4.90e-07
    worst = 0.0
    for name, c in table.items():
        want = gu.rcl_f64(c)
        err = float(np.abs(restated[name][0].astype(np.float64) - want).max())
        print(f"{name}: {len(c['t'])} samples, max |Rcl - f64| = {err:.3e}")
        worst = max(worst, err)
        assert err <= bound, (name, err)
        if np.array_equal(c["Rbc"], gu.EYE):                      # (an Rbc rounded to f32 is orthogonal to 1e-7 only)
            assert np.abs(want @ want.T - np.eye(3)).max() < 1e-12, name
    print(f"worst {worst:.3e}, bound {bound:.3e}")
    # ... and the rotations are rotations worth the name: far from I by much more than the bound
    assert np.abs(restated["5 samples"][0] - np.eye(3)).max() > 1e-3
    assert np.abs(restated["d 2 rad"][0] - np.eye(3)).max() > 0.5


def test_rot9_is_k_rcl_kinv_and_the_third_row(table, restated):
    for name, c in table.items():
        rcl, rot9 = restated[name]
        fx, fy, cx, cy = c["camera"]
        K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)
        want = K @ rcl.astype(np.float64) @ np.linalg.inv(K)
        assert np.abs(rot9[:6].astype(np.float64) - want.reshape(-1)[:6]).max() <= 2e-4 * max(1.0, np.abs(want).max() / 100), name
        assert rot9[6:].tobytes() == rcl[2].tobytes(), name


# ---- the window checks -----------------------------------------------------------------------------------------------------
def test_imu_window_check_refuses_what_the_definition_refuses(built, ref, table):
    lib = capi.load()
    for name, (c, cap) in gu.refused_windows().items():
        win, keep = _window(c)
        assert capi.imu_window_check(win, cap) == capi.PAGK_E_ARG, name
        assert gu.ref_window_check(ref, c, cap) == -1, name
    for name, c in table.items():                                 # one accepted window per case, and many more
        win, keep = _window(c)
        assert capi.imu_window_check(win) == capi.PAGK_OK, name
        assert gu.ref_window_check(ref, c) == 0, name
        assert capi.imu_window_check(win, max(len(c["t"]), 1)) == capi.PAGK_OK, name     # exactly imu_cap samples
    assert lib.pagk_imu_window_check(None, 64) == capi.PAGK_E_ARG
    win, keep = _window(table["5 samples"])
    win.t = None                                                  # samples announced, no array
    assert capi.imu_window_check(win) == capi.PAGK_E_ARG
    win, keep = _window(table["5 samples"])
    win.n = -1
    assert capi.imu_window_check(win) == capi.PAGK_E_ARG
    with pytest.raises(ValueError):
        capi.imu_window(0.0, 1.0, [0.0, 0.5], np.zeros((3, 3)))


def test_null_arguments_are_refused_without_a_device(built, table):
    lib = capi.load()
    win, keep = _window(table["5 samples"])
    cam = capi.make_params()
    a = np.zeros(16, np.float32).ctypes.data
    assert lib.pagk_gyro_integrate(None, a, C.byref(cam), C.byref(win), a, a) == capi.PAGK_E_ARG
    assert lib.pagk_gyro_integrate(None, None, None, None, None, None) == capi.PAGK_E_ARG


# ---- the boundary ----------------------------------------------------------------------------------------------------------
def test_header_defines_the_section_and_capi_binds_it(built):
    hdr = open(os.path.join(ROOT, "include", "pagk.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = capi.load()
    for name, names in (("pagk_imu_window_check", ["window", "imu_cap"]),
                        ("pagk_gyro_integrate", ["ctx", "Rbc[9]", "camera", "window", "Rcl", "rot9"])):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name) and len(getattr(lib, name).argtypes) == len(names), name
        params = re.search(r"\bint " + name + r"\s*\((.*?)\);", code, flags=re.S).group(1)
        got = [p.split()[-1].lstrip("*") for p in params.split(",")]
        assert got == names and not any(p.startswith("d_") for p in got), (name, got)
        decl = hdr.index("int " + name + "(")
        comment = hdr[:decl].rsplit("/*", 1)[1]
        assert comment.rstrip().endswith("*/") and "src/gyro_aided_tracker.cpp:5" in comment, name
        assert not re.search(r"device\s+pointer", comment), name
    section = hdr[hdr.index("Gyro integration: the IMU window"):hdr.index("typedef struct pagk_imu_window")]
    for word in ("src/gyro_aided_tracker.cpp:511-587", ":530-555", ":564-587", ":560", ":518", "tests/gyro_integrate_ref.c",
                 "bit for bit", "NOT claimed", "steering", "rounded once to f32", "f64 accumulator starting at 0", "k ascending",
                 "(double)d < 1e-4", "correctly rounded", "cofactor", "pagk_gyro_predict_device_rot", "never reaches the device",
                 "#define PAGK_IMU_MAX_SAMPLES 64"):
        assert word in section, word
    assert "#define PAGK_VERSION 303" in hdr and capi.IMU_MAX_SAMPLES == 64
    assert callable(capi.Context.gyro_integrate) and callable(host_api.gyro_integrate)
    # the struct against a compiled C probe
    fields = [f for f, _ in capi.ImuWindow._fields_]
    assert fields == ["t_ref", "t_cur", "n", "t", "w", "bias"]


def test_imu_window_layout_matches_a_c_probe(built, tmp_path):
    fields = [f for f, _ in capi.ImuWindow._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pagk.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(pagk_imu_window));\n' +
                   "".join(f'    printf("%zu %zu\\n", offsetof(pagk_imu_window, {f}), sizeof(((pagk_imu_window *)0)->{f}));\n'
                           for f in fields) + "    return 0;\n}\n")
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    assert int(lines[0]) == C.sizeof(capi.ImuWindow)
    for f, line in zip(fields, lines[1:]):
        d = getattr(capi.ImuWindow, f)
        assert (d.offset, d.size) == tuple(int(v) for v in line.split()), f


def test_the_kernel_has_its_resource_row():
    import __graft_entry__ as g
    assert g.RESOURCE_CLAIMS["k_gyro_integrate"][1] == 0 and g.RESOURCE_CLAIMS["k_flow_velocity"][1] == 0     # no spill
    src = open(os.path.join(ROOT, "pixel_aware_gyro_aided_klt_feature_tracker_amd", "csrc", "pagk_gyro_kernel.h")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code and "asm" not in code
    assert not re.search(r"\b(sinf?|cosf?|sincosf?|__sinf|__cosf)\s*\(", code)     # no library sine or cosine
    host = open(os.path.join(ROOT, "pixel_aware_gyro_aided_klt_feature_tracker_amd", "csrc", "pagk_hip.hip")).read()
    assert host.count("hipLaunchKernelGGL(k_gyro_integrate, dim3(1), dim3(64)") == 2      # one wavefront, in both callers


# ---- the restatement under the sanitizers -----------------------------------------------------------------------------------
def test_restatement_under_the_sanitizers(ref, table, restated, tmp_path):
    """tests/gyro_integrate_sanitize.c, a program of its own, compiled together with the restatement under
    -fsanitize=address,undefined: the whole edge table and every refused window on exact-length heap arrays; its output is
    the restatement's, byte for byte."""
    cases = [(name, c, 64) for name, c in table.items()] + [(n, c, cap) for n, (c, cap) in gu.refused_windows().items()]
    path = tmp_path / "table.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for _, c, cap in cases:
            f.write(np.ascontiguousarray(c["Rbc"], np.float32).tobytes() + np.asarray(c["camera"], np.float32).tobytes())
            f.write(struct.pack("<ddii", c["t_ref"], c["t_cur"], len(c["t"]), cap))
            f.write(c["t"].tobytes() + c["w"].tobytes() + np.asarray(c["bias"], np.float32).tobytes())
    exe = str(tmp_path / "gyro_integrate_sanitize")
    subprocess.run(["gcc", "-std=c99", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Werror", gu.SANITIZE_SRC, gu.REF_SRC, "-o", exe, *gu.ORACLE_LINK, "-lm"],
                   check=True)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(cases) + 1 and lines[-1].startswith("velocity ")
    for (name, c, cap), line in zip(cases, lines):
        words = line.split()
        if name in table:
            assert words[:2] == ["0", "0"], name
            got = np.array([int(w, 16) for w in words[2:]], np.uint32).view(np.float32)
            assert got[:9].tobytes() == restated[name][0].tobytes() and got[9:].tobytes() == restated[name][1].tobytes(), name
        else:
            assert words[:2] == ["-1", "-1"] and set(words[2:]) == {"00000000"}, name
    v = np.array([int(w, 16) for w in lines[-1].split()[1:]], np.uint32).view(np.float32).reshape(5, 2)
    j = np.arange(5, dtype=np.float32)
    cur = np.stack([np.float32(0.01) * j, np.float32(-0.02) * j], axis=1)
    last = np.stack([np.float32(0.015) * j, np.full(5, 0.005, np.float32)], axis=1)
    idx = np.array([4, -1, 2, 1, 0], np.int32)
    assert v.tobytes() == gu.model_flow_velocity(5, 4, cur, last, idx, 2.5, 2.25).tobytes()
    assert v[0].any() and not v[1].any() and not v[4].any()
