"""Test helpers of the frame hand-over: the plain-C restatement (tests/frame_handover_ref.c) built and loaded with ctypes,
the reference's SuperPoint candidate lists (tests/golden/seq) and a synthetic rotating-camera sequence."""
from __future__ import annotations

import ctypes as C
import glob
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SRC = os.path.join(HERE, "frame_handover_ref.c")
STATE_WORDS = 8


class RefCamera(C.Structure):   # fhr_camera
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("dist_coef", C.c_float * 5), ("n_dist_coef", C.c_int32)]


def build_ref(out_dir: str):
    """gcc -O2 -ffp-contract=off (one rounding per operation, like the library) -> ctypes library."""
    so = os.path.join(str(out_dir), "frame_handover_ref.so")
    subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                    REF_SRC, "-lm"], check=True)
    lib = C.CDLL(so)
    vp, i32 = C.c_void_p, C.c_int32
    lib.fhr_post_filter.restype = i32
    lib.fhr_post_filter.argtypes = [i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.fhr_hole_origin.restype = None
    lib.fhr_hole_origin.argtypes = [C.c_float, C.c_float, i32, i32, C.POINTER(i32), C.POINTER(i32)]
    lib.fhr_handover.restype = None
    lib.fhr_handover.argtypes = [C.POINTER(RefCamera), i32, i32, i32, i32, C.c_double, vp, vp, vp, i32, vp, vp, vp, vp,
                                 vp, vp, vp, vp]
    lib.fhr_predict_live.restype = None
    lib.fhr_predict_live.argtypes = [i32, vp, vp, vp, vp]
    return lib


def camera_of(params) -> RefCamera:
    """The camera fields of a capi.Params."""
    c = RefCamera(params.fx, params.fy, params.cx, params.cy)
    for k in range(5):
        c.dist_coef[k] = params.dist_coef[k]
    c.n_dist_coef = params.n_dist_coef
    return c


def ref_post_filter(lib, half_patch, status_pm, pix_err, dist_pred, pt_pm, pt_pm_un, pt_predict=None,
                    pt_predict_un=None) -> dict:
    """The restatement's Step 3; pt_predict(_un) start from the given arrays (zeros by default), so that the entries
    of non-survivors can be compared too."""
    st = np.ascontiguousarray(status_pm, np.uint8)
    n = st.shape[0]
    pe, dp = np.ascontiguousarray(pix_err, np.float64), np.ascontiguousarray(dist_pred, np.float64)
    pm, pmu = np.ascontiguousarray(pt_pm, np.float32), np.ascontiguousarray(pt_pm_un, np.float32)
    out = np.zeros(max(n, 1), np.uint8)
    pp = np.zeros((max(n, 1), 2), np.float32) if pt_predict is None else np.array(pt_predict, np.float32, copy=True)
    ppu = np.zeros((max(n, 1), 2), np.float32) if pt_predict_un is None else np.array(pt_predict_un, np.float32, copy=True)
    th = np.zeros(2, np.float64)
    kept = lib.fhr_post_filter(n, half_patch, st.ctypes.data, pe.ctypes.data, dp.ctypes.data, pm.ctypes.data,
                               pmu.ctypes.data, out.ctypes.data, pp.ctypes.data, ppu.ctypes.data, th.ctypes.data)
    return dict(kept=kept, status=out[:n], pt_predict=pp[:n], pt_predict_un=ppu[:n], thresholds=th)


def ref_handover(lib, cam: RefCamera, width, height, cap, target_n, new_point_threshold, status, pt_predict,
                 pt_predict_un, candidates, state=None) -> dict:
    """The restatement's hand-over in the layout of capi.Context.frame_handover."""
    def pad(a, dtype, w):
        out = np.zeros((cap, w) if w > 1 else (cap,), dtype)
        a = np.asarray(a, dtype).reshape((-1, w) if w > 1 else (-1,))
        out[:a.shape[0]] = a
        return out
    st, pp, ppu = pad(status, np.uint8, 1), pad(pt_predict, np.float32, 2), pad(pt_predict_un, np.float32, 2)
    cand = np.ascontiguousarray(candidates, np.float32).reshape(-1, 2)
    cbuf = np.zeros((max(cand.shape[0], 1), 2), np.float32)
    cbuf[:cand.shape[0]] = cand
    state = np.zeros(STATE_WORDS, np.int32) if state is None else np.array(state, np.int32, copy=True)
    out = dict(keys=np.zeros((cap, 2), np.float32), keys_un=np.zeros((cap, 2), np.float32),
               keys_normal=np.zeros((cap, 2), np.float32), index_in_last=np.zeros(cap, np.int32),
               live=np.zeros(cap, np.uint8), mask=np.zeros((height, width), np.uint8), state=state)
    lib.fhr_handover(C.byref(cam), width, height, cap, target_n, float(new_point_threshold), st.ctypes.data,
                     pp.ctypes.data, ppu.ctypes.data, cand.shape[0], cbuf.ctypes.data, out["keys"].ctypes.data,
                     out["keys_un"].ctypes.data, out["keys_normal"].ctypes.data, out["index_in_last"].ctypes.data,
                     out["live"].ctypes.data, out["mask"].ctypes.data, state.ctypes.data)
    return out


HANDOVER_ARRAYS = ("keys", "keys_un", "keys_normal", "index_in_last", "live", "mask", "state")


def same_handover(a: dict, b: dict) -> list:
    """Names of the arrays whose bytes differ."""
    return [k for k in HANDOVER_ARRAYS if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()]


def seq_candidates() -> list:
    """The reference's four SuperPoint lists "idx, x, y" (src/frame.cpp:222-240), 500 points each at 640x480."""
    out = []
    for path in sorted(glob.glob(os.path.join(HERE, "golden", "seq", "1*.txt"))):
        rows = [ln.split(",") for ln in open(path).read().splitlines() if ln.strip()]
        out.append(np.array([[float(r[1]), float(r[2])] for r in rows], np.float32))
    assert len(out) == 4 and all(c.shape == (500, 2) for c in out)
    return out


def rotating_sequence(synth, n_frames, width, height, seed, step_vec):
    """One synth.Texture warped by an accumulating rotation (the recipe of the C++ demo-loop test): images, the float32
    rotation of every pair, the 9 floats [rows 0-1 of K R K^-1, third row of R] the prediction reads, and the generator
    (for keypoints drawn behind the texture, as that test draws them)."""
    cam = synth.D435I
    rng = synth.SplitMix64(seed)
    tex = synth.Texture(rng)
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    K = cam.K
    Kinv = np.linalg.inv(K)
    step = synth.rodrigues(np.array(step_vec))
    imgs, Rs, Racc = [], [], np.eye(3)
    for k in range(n_frames):
        Hi = np.linalg.inv(K @ Racc @ Kinv)
        den = Hi[2, 0] * xx + Hi[2, 1] * yy + Hi[2, 2]
        sx = (Hi[0, 0] * xx + Hi[0, 1] * yy + Hi[0, 2]) / den
        sy = (Hi[1, 0] * xx + Hi[1, 1] * yy + Hi[1, 2]) / den
        imgs.append(np.clip(np.rint((1.0 + 0.01 * k) * tex(sx, sy) + k), 0, 255).astype(np.uint8))
        if k:
            Rs.append(step.astype(np.float32))
        Racc = step @ Racc
    K32 = K.astype(np.float32)
    Kinv32 = np.linalg.inv(K32.astype(np.float64)).astype(np.float32)

    def mul32(a, b):
        return (a.astype(np.float64) @ b.astype(np.float64)).astype(np.float32)
    KRKs = [mul32(mul32(K32, R), Kinv32) for R in Rs]
    rot9 = [np.concatenate([KRK.reshape(-1)[:6], R[2]]).astype(np.float32) for KRK, R in zip(KRKs, Rs)]
    return cam, imgs, Rs, KRKs, rot9, rng
