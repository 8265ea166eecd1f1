"""Test helpers of the device RANSAC fits: the plain-C restatement (tests/geometry_fit_ref.c) built and loaded with
ctypes, the ground truth of a make_geometry_case scene, and scene variants (status masks, collinear input)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SRC = os.path.join(HERE, "geometry_fit_ref.c")
INFO_FIELDS = ("status", "best", "best_count", "refit_count", "valid", "adaptive")


class RefParams(C.Structure):   # pagk_fit_params
    _fields_ = [("seed", C.c_uint64), ("iters_H", C.c_int32), ("iters_F", C.c_int32), ("thresh_H", C.c_double),
                ("thresh_F", C.c_double), ("conf_H", C.c_double), ("conf_F", C.c_double)]


def build_ref(out_dir: str):
    """gcc -O2 -ffp-contract=off (one rounding per operation, like the library) -> ctypes library."""
    so = os.path.join(str(out_dir), "geometry_fit_ref.so")
    subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                    REF_SRC, "-lm"], check=True)
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.gfr_fit.restype = C.c_int32
    lib.gfr_fit.argtypes = [C.POINTER(RefParams), C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.gfr_sample.restype = C.c_int
    lib.gfr_sample.argtypes = [C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, vp]
    lib.gfr_splitmix64.restype = C.c_uint64
    lib.gfr_splitmix64.argtypes = [C.c_uint64]
    lib.gfr_draw.restype = C.c_uint32
    lib.gfr_draw.argtypes = [C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32]
    lib.gfr_adaptive.restype = C.c_int32
    lib.gfr_adaptive.argtypes = [C.c_int32, C.c_int32, C.c_int, C.c_double]
    lib.gfr_log.restype = C.c_double
    lib.gfr_log.argtypes = [C.c_double]
    return lib


def params(seed=1, iters_H=2000, iters_F=1000, thresh_H=3.0, thresh_F=3.0, conf_H=0.995, conf_F=0.99) -> RefParams:
    return RefParams(seed, iters_H, iters_F, thresh_H, thresh_F, conf_H, conf_F)


def ref_fit(lib, p, pts1, pts2, status=None) -> dict:
    """The restatement's fit, in the layout of capi.Context.geometry_fit (hyp_counts included)."""
    pts1 = np.ascontiguousarray(pts1, np.float32).reshape(-1, 2)
    pts2 = np.ascontiguousarray(pts2, np.float32).reshape(-1, 2)
    n = pts1.shape[0]
    st = None if status is None else np.ascontiguousarray(status, np.uint8)
    models = np.zeros(27, np.float64)
    mH, mF = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
    info = np.zeros(12, np.int32)
    hc = np.zeros(p.iters_H + p.iters_F, np.int32)
    m = lib.gfr_fit(C.byref(p), n, pts1.ctypes.data, pts2.ctypes.data, None if st is None else st.ctypes.data,
                    models.ctypes.data, mH.ctypes.data, mF.ctypes.data, info.ctypes.data, hc.ctypes.data)
    return dict(m=m, models=models, H21=models[:9].reshape(3, 3), H12=models[9:18].reshape(3, 3),
                F21=models[18:].reshape(3, 3), mask_H=mH[:n], mask_F=mF[:n], info=info, hyp_counts=hc,
                H=dict(zip(INFO_FIELDS, info[:6].tolist())), F=dict(zip(INFO_FIELDS, info[6:].tolist())))


def ref_samples(lib, seed, model, m, first, count) -> np.ndarray:
    s = 8 if model else 4
    out = np.zeros((count, s), np.int32)
    row = np.zeros(s, np.int32)
    for i in range(count):
        lib.gfr_sample(seed, model, first + i, m, row.ctypes.data)
        out[i] = row
    return out


# ---- ground truth --------------------------------------------------------------------------------------------------
def transfer_error(H, p1, p2):
    """|p2 - H p1| in pixels (f64)."""
    q = np.c_[p1.astype(np.float64), np.ones(len(p1))] @ H.T
    return np.hypot(p2[:, 0] - q[:, 0] / q[:, 2], p2[:, 1] - q[:, 1] / q[:, 2])


def epipolar_error(F, p1, p2):
    """max of the two point-to-epipolar-line distances in pixels (f64)."""
    x1 = np.c_[p1.astype(np.float64), np.ones(len(p1))]
    x2 = np.c_[p2.astype(np.float64), np.ones(len(p2))]
    l2, l1 = x1 @ F.T, x2 @ F
    num = np.abs(np.sum(x2 * l2, axis=1))
    return np.maximum(num / np.hypot(l2[:, 0], l2[:, 1]), num / np.hypot(l1[:, 0], l1[:, 1]))


def normalised(M):
    """M / ||M||_F with the sign that makes its largest |entry| positive (models are defined up to scale)."""
    M = np.asarray(M, np.float64)
    M = M / np.linalg.norm(M)
    return M * np.sign(M.flat[np.argmax(np.abs(M))])


def collinear_case(n=64, seed=3):
    rng = np.random.default_rng(seed)
    t = rng.uniform(0, 400, n)
    p1 = np.c_[50 + t, 80 + 0.5 * t].astype(np.float32)
    p2 = (p1 + np.float32([3.0, -2.0])).astype(np.float32)
    return p1, p2
