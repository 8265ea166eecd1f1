"""Test helpers of the gyro integration (include/pagk.h "Gyro integration") and of the sensor sequence's flow velocity: the
plain-C restatement (tests/gyro_integrate_ref.c) built and loaded with ctypes, an independent numpy model written from the
definition (float32 / float64 scalars, matrices as arrays), an f64 Rodrigues product of the same window (what the f32 chain
approximates), the edge table, and constant-rate windows that reproduce a given rotation."""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SRC = os.path.join(HERE, "gyro_integrate_ref.c")
SANITIZE_SRC = os.path.join(HERE, "gyro_integrate_sanitize.c")
ORACLE_DIR = os.path.join(HERE, "..", "oracle")
# the matrix product, the inverse and the sine / cosine live in the oracle library (one definition, oracle/pagk_oracle.h)
ORACLE_LINK = ["-L", ORACLE_DIR, "-l:libpagk_oracle.so", f"-Wl,-rpath,{os.path.abspath(ORACLE_DIR)}"]
F, D = np.float32, np.float64
MAX_SAMPLES = 64
CAMERA = (382.613, 382.1, 320.183, 236.455)          # fx fy cx cy
EYE = np.eye(3, dtype=np.float32)


def build_ref(out_dir):
    from oracle import pagk_oracle
    pagk_oracle.build()   # the oracle library, when it is missing or older than its source
    so = os.path.join(str(out_dir), "gyro_integrate_ref.so")
    subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                    REF_SRC, *ORACLE_LINK, "-lm"], check=True)
    lib = C.CDLL(so)
    vp, i32, f32, f64 = C.c_void_p, C.c_int32, C.c_float, C.c_double
    lib.gyro_ref_one_step.restype = None
    lib.gyro_ref_one_step.argtypes = [vp, vp, f32, vp]
    lib.gyro_ref_window_check.restype = i32
    lib.gyro_ref_window_check.argtypes = [f64, f64, i32, vp, vp, vp, i32]
    lib.gyro_ref_integrate.restype = i32
    lib.gyro_ref_integrate.argtypes = [vp, f32, f32, f32, f32, f64, f64, i32, vp, vp, vp, vp, vp]
    lib.gyro_ref_flow_velocity.restype = None
    lib.gyro_ref_flow_velocity.argtypes = [i32, i32, vp, vp, vp, f64, f64, vp]
    return lib


def case(t_ref, t_cur, t, w, bias=(0.0, 0.0, 0.0), Rbc=EYE, camera=CAMERA) -> dict:
    t = np.ascontiguousarray(t, D).reshape(-1)
    w = np.ascontiguousarray(w, F).reshape(-1, 3)
    assert t.shape[0] == w.shape[0]
    return dict(t_ref=float(t_ref), t_cur=float(t_cur), t=t, w=w, bias=np.asarray(bias, F), Rbc=np.ascontiguousarray(Rbc, F),
                camera=tuple(float(F(v)) for v in camera))


def ref_integrate(lib, c: dict):
    """The restatement -> (Rcl 3 x 3, rot9), or None for a window it refuses."""
    rcl, rot9 = np.zeros(9, F), np.zeros(9, F)
    rbc = np.ascontiguousarray(c["Rbc"], F).reshape(9)
    rc = lib.gyro_ref_integrate(rbc.ctypes.data, *c["camera"], c["t_ref"], c["t_cur"], len(c["t"]), c["t"].ctypes.data,
                                c["w"].ctypes.data, c["bias"].ctypes.data, rcl.ctypes.data, rot9.ctypes.data)
    return None if rc else (rcl.reshape(3, 3), rot9)


def ref_window_check(lib, c: dict, imu_cap: int = MAX_SAMPLES) -> int:
    return int(lib.gyro_ref_window_check(c["t_ref"], c["t_cur"], len(c["t"]), c["t"].ctypes.data, c["w"].ctypes.data,
                                         c["bias"].ctypes.data, imu_cap))


# ---- the numpy model -------------------------------------------------------------------------------------------------------
_S = (-1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04, 2.75573137070700676789e-06,
      -2.50507602534068634195e-08, 1.58969099521155010221e-10)
_C = (4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05, -2.75573143513906633035e-07,
      2.08757232129817482790e-09, -1.13596475577881948265e-11)


def model_sin_cos(x: float):
    """The f64 algorithm of the header's "steering" paragraph on Python floats (IEEE f64, one rounding per operation)."""
    v = x * float.fromhex("0x1.45f306dc9c883p-1") + 0.5
    k = int(min(v, 2147483647.0))
    t = (x - k * float.fromhex("0x1.921fb544p+0")) - k * float.fromhex("0x1.0b4611a626331p-34")
    z = t * t
    ps = _S[5]
    for a in _S[4::-1]:
        ps = a + z * ps
    pc = _C[5]
    for a in _C[4::-1]:
        pc = a + z * pc
    s = t + t * (z * ps)
    c = 1.0 - z * (0.5 - z * pc)
    return ((s, c), (c, -s), (-s, -c), (-c, s))[k & 3]


def model_mul3(a, b):
    out = np.zeros((3, 3), F)
    for r in range(3):
        for c in range(3):
            s = 0.0
            for k in range(3):
                s = s + float(a[r, k]) * float(b[k, c])
            out[r, c] = F(s)
    return out


def model_inv3(m):
    a = np.asarray(m, D)
    cof = lambda i, j, k, l: float(a[i, j]) * float(a[k, l])   # noqa: E731
    det = (float(a[0, 0]) * (cof(1, 1, 2, 2) - cof(1, 2, 2, 1)) - float(a[0, 1]) * (cof(1, 0, 2, 2) - cof(1, 2, 2, 0))
           + float(a[0, 2]) * (cof(1, 0, 2, 1) - cof(1, 1, 2, 0)))
    d = 1.0 / det if det != 0.0 else 0.0
    o = [(cof(1, 1, 2, 2) - cof(1, 2, 2, 1)) * d, (cof(0, 2, 2, 1) - cof(0, 1, 2, 2)) * d, (cof(0, 1, 1, 2) - cof(0, 2, 1, 1)) * d,
         (cof(1, 2, 2, 0) - cof(1, 0, 2, 2)) * d, (cof(0, 0, 2, 2) - cof(0, 2, 2, 0)) * d, (cof(0, 2, 1, 0) - cof(0, 0, 1, 2)) * d,
         (cof(1, 0, 2, 1) - cof(1, 1, 2, 0)) * d, (cof(0, 1, 2, 0) - cof(0, 0, 2, 1)) * d, (cof(0, 0, 1, 1) - cof(0, 1, 1, 0)) * d]
    return np.array(o, D).astype(F).reshape(3, 3)


def model_one_step(av, bias, tstep):
    with np.errstate(all="ignore"):
        g = (np.asarray(av, F) - np.asarray(bias, F)).astype(D) * D(F(tstep))
        x, y, z = g.astype(F)
        d2 = (x * x + y * y) + z * z
        d = np.sqrt(d2)
        zero = F(0)
        W = np.array([[zero, -z, y], [z, zero, -x], [-y, x, zero]], F)
        if float(d) < 1e-4:
            return EYE + W
        WW = model_mul3(W, W)
        sn, cs = model_sin_cos(float(d))
        s, c = float(F(sn)), float(F(1) - F(cs))
        R = np.zeros((3, 3), F)
        for r in range(3):
            for q in range(3):
                R[r, q] = F((float(EYE[r, q]) + float(W[r, q]) * s / float(d)) + float(WW[r, q]) * c / float(d2))
        return R


def _steps(c: dict, f32: bool):
    """(angVel, tstep) per step: the four cases of :530-555, in f32 as the definition has them or in f64."""
    t, w, t_ref, t_cur = c["t"], c["w"], D(c["t_ref"]), D(c["t_cur"])
    T = F if f32 else D
    n = len(t) - 1
    half = T(0.5)
    for i in range(n):
        w0, w1 = w[i].astype(T), w[i + 1].astype(T)
        if i == 0 and i < n - 1:
            tab, tini = T(t[i + 1] - t[i]), T(t[i] - t_ref)
            yield ((w0 + w1) - (w1 - w0) * (tini / tab)) * half, T(t[i + 1] - t_ref)
        elif i < n - 1:
            yield (w0 + w1) * half, T(t[i + 1] - t[i])
        elif i > 0:
            tab, tend = T(t[i + 1] - t[i]), T(t[i + 1] - t_cur)
            yield ((w0 + w1) - (w1 - w0) * (tend / tab)) * half, T(t_cur - t[i])
        else:
            yield w0, T(t_cur - t_ref)


def model_integrate(c: dict):
    """The numpy model -> (Rcl, rot9)."""
    dR = EYE.copy()
    with np.errstate(all="ignore"):
        for av, tstep in _steps(c, True):
            dR = model_mul3(dR, model_one_step(av, c["bias"], tstep))
    Rbc = np.asarray(c["Rbc"], F).reshape(3, 3)
    Rcl = model_mul3(model_mul3(Rbc.T, dR.T), Rbc)
    fx, fy, cx, cy = c["camera"]
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], F)
    KRK = model_mul3(model_mul3(K, Rcl), model_inv3(K))
    return Rcl, np.concatenate([KRK.reshape(-1)[:6], Rcl[2]]).astype(F)


def rodrigues64(v) -> np.ndarray:
    v = np.asarray(v, D)
    th = float(np.linalg.norm(v))
    Wm = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], D)
    if th < 1e-12:
        return np.eye(3) + Wm
    return np.eye(3) + math.sin(th) / th * Wm + (1.0 - math.cos(th)) / (th * th) * (Wm @ Wm)


def rcl_f64(c: dict) -> np.ndarray:
    """The same window with every step and every product in f64 (Rodrigues' formula, libm): what the f32 chain approximates."""
    dR = np.eye(3)
    for av, tstep in _steps(c, False):
        dR = dR @ rodrigues64((av - c["bias"].astype(D)) * tstep)
    Rbc = np.asarray(c["Rbc"], D).reshape(3, 3)
    return Rbc.T @ dR.T @ Rbc


# ---- the edge table ------------------------------------------------------------------------------------------------------
def _window(n: int, seed: int, t_ref=100.0, dt=1.0 / 30.0, rate=0.6, uneven=True, first_at_ref=False):
    """n samples around [t_ref, t_ref + dt]: the first at or before t_ref, the last at or behind t_cur, as the demo's windows."""
    rng = np.random.default_rng(seed)
    t_cur = t_ref + dt
    if n == 0:
        return t_ref, t_cur, np.zeros(0, D), np.zeros((0, 3), F)
    lead = 0.0 if first_at_ref else 0.0011
    if n == 1:
        t = np.array([t_ref - lead], D)
    else:
        u = np.linspace(0.0, 1.0, n)
        if uneven and n > 2:
            u[1:-1] += rng.uniform(-0.3, 0.3, n - 2) / (n - 1)
        t = (t_ref - lead) + u * (dt + lead + 0.0017)
    w = (rng.normal(0.0, rate, (n, 3))).astype(F)
    return t_ref, t_cur, t, w


def edge_table() -> dict:
    Rbc = rodrigues64((0.01, -0.02, 1.57)).astype(F)
    out = {}
    for n in (0, 1, 2, 3, 4, 5, 64):
        out[f"{n} samples"] = case(*_window(n, 10 + n))
    out["64 samples, fast"] = case(*_window(64, 99, rate=4.0), bias=(0.01, -0.02, 0.005), Rbc=Rbc)
    dt = 1.0 / 30.0
    # one step (two samples): angVel = w0, tstep = (float)dt; d on both sides of 1e-4 and in every quadrant of the sine
    for name, d in (("d below 1e-4", 0.99e-4), ("d just above 1e-4", 1.0001e-4), ("d 0", 0.0), ("d 2 rad", 2.0),
                    ("d 3.5 rad", 3.5), ("d 5 rad", 5.0), ("d 7 rad", 7.0), ("d 0.8 rad", 0.8)):
        axis = np.array([0.6, -0.48, 0.64])
        out[name] = case(50.0, 50.0 + dt, [50.0 - 0.001, 50.0 + dt + 0.001], np.outer([1.0, 0.3], axis * d / dt))
    out["bias"] = case(*_window(5, 21), bias=(0.013, -0.007, 0.021))
    out["even spacing"] = case(*_window(7, 22, uneven=False))
    out["t_0 = t_ref"] = case(*_window(6, 23, first_at_ref=True))
    out["Rbc not I"] = case(*_window(5, 24), Rbc=Rbc)
    out["Rbc not I, bias, 64"] = case(*_window(64, 25), bias=(-0.004, 0.002, 0.001), Rbc=Rbc)
    out["large time stamps"] = case(*_window(9, 26, t_ref=1.6e9 + 0.123456))
    out["samples inside the pair only"] = case(10.0, 10.05, [10.01, 10.02, 10.04], np.full((3, 3), 0.5))
    out["other camera"] = case(*_window(4, 27), camera=(191.3, 190.9, 160.35, 118.95), Rbc=Rbc)
    return out


def refused_windows() -> dict:
    """name -> (case, imu_cap): every refusal of the definition."""
    nan, inf = float("nan"), float("inf")
    ok = _window(5, 31)

    def edit(**kw):
        t_ref, t_cur, t, w = ok
        c = case(t_ref, t_cur, t.copy(), w.copy())
        for k, v in kw.items():
            if k == "t":
                c["t"][v[0]] = v[1]
            elif k == "w":
                c["w"][v[0], v[1]] = v[2]
            else:
                c[k] = v
        return c
    return {"more than imu_cap": (edit(), 4), "65 samples": (case(*_window(65, 32)), 64), "imu_cap 0": (edit(), 0),
            "imu_cap 65": (edit(), 65), "nan time": (edit(t=(2, nan)), 64), "inf time": (edit(t=(4, inf)), 64),
            "nan rate": (edit(w=(1, 2, nan)), 64), "inf rate": (edit(w=(0, 0, -inf)), 64),
            "equal times": (edit(t=(2, ok[2][1])), 64), "decreasing times": (edit(t=(3, ok[2][1] - 1e-3)), 64),
            "t_cur = t_ref": (edit(t_cur=ok[0]), 64), "t_cur < t_ref": (edit(t_cur=ok[0] - 0.01), 64),
            "nan t_ref": (edit(t_ref=nan), 64), "inf t_cur": (edit(t_cur=inf), 64),
            "nan bias": (edit(bias=np.array([0, nan, 0], F)), 64)}


# ---- windows of a scene ----------------------------------------------------------------------------------------------------
def constant_rate_window(step_vec, t_ref: float, t_cur: float, n: int = 8):
    """A window whose integration gives Rcl = rodrigues(step_vec) for Rbc = I: Rcl = dR^T, so the constant rate is
    -step_vec / (t_cur - t_ref); with a constant rate every case of :530-555 has angVel = the rate, and the step times add
    up to t_cur - t_ref.  Samples a little before t_ref to a little behind t_cur, unevenly spaced."""
    dt = t_cur - t_ref
    u = np.linspace(0.0, 1.0, n)
    u[1:-1] += 0.2 / (n - 1) * np.cos(np.arange(1, n - 1))
    t = (t_ref - 0.05 * dt) + u * (1.1 * dt)
    w = np.tile((-np.asarray(step_vec, D) / dt).astype(F), (n, 1))
    return case(t_ref, t_cur, t, w)


def model_flow_velocity(cap, live, normal_cur, normal_last, index_in_last, t_cur, t_last) -> np.ndarray:
    """Section "flow velocity" of the header in numpy: an f32 difference, an f64 quotient rounded once."""
    v = np.zeros((cap, 2), F)
    idx = np.asarray(index_in_last[:cap])
    rows = np.nonzero((np.arange(cap) < live) & (idx >= 0))[0]
    diff = np.asarray(normal_cur, F)[rows] - np.asarray(normal_last, F)[idx[rows]]
    v[rows] = (diff.astype(D) / (D(t_cur) - D(t_last))).astype(F)
    return v
