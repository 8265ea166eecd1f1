"""ctypes loader for the CPU oracle (oracle/libpagk_oracle.so).

TEST INFRASTRUCTURE ONLY: import this from tests/, __graft_entry__.smoke() and
bench.py's cpu_baseline leg, nowhere else.  The product never loads it.
What is pinned to the reference and what is not: see pagk_oracle.h.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from pixel_aware_gyro_aided_klt_feature_tracker_amd.capi import (Image, Outputs, Params, alloc_outputs, image_view,
                                                                 outputs_struct)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libpagk_oracle.so")
_lib = None


def build(force: bool = False) -> str:
    src = os.path.join(HERE, "pagk_oracle.c")
    if force or not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < os.path.getmtime(src):
        subprocess.run(["make", "-C", HERE, "libpagk_oracle.so"], check=True, capture_output=True)
    return LIB_PATH


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build()
        lib = C.CDLL(LIB_PATH)
        vp, i32, P = C.c_void_p, C.c_int32, C.POINTER
        lib.pagk_oracle_pyr_down.restype = C.c_int
        lib.pagk_oracle_pyr_down.argtypes = [vp, i32, i32, C.c_int64, vp]
        lib.pagk_oracle_sample.restype = C.c_int
        lib.pagk_oracle_sample.argtypes = [P(Image), i32, vp, vp]
        lib.pagk_oracle_track.restype = C.c_int
        lib.pagk_oracle_track.argtypes = [P(Params), P(Image), P(Image), i32, vp, vp, vp, vp, P(Outputs), i32]
        lib.pagk_oracle_track_pyr.restype = C.c_int
        lib.pagk_oracle_track_pyr.argtypes = [P(Params), i32, P(Image), P(Image), i32, vp, vp, vp, vp, P(Outputs), i32]
        lib.pagk_oracle_post_filter.restype = C.c_int
        lib.pagk_oracle_post_filter.argtypes = [i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
        lib.pagk_oracle_gyro_predict.restype = C.c_int
        lib.pagk_oracle_gyro_predict.argtypes = [P(Params), i32, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp]
        lib.pagk_oracle_log.restype = C.c_double
        lib.pagk_oracle_log.argtypes = [C.c_double]
        lib.pagk_oracle_inv_log_max_dist.restype = C.c_float
        lib.pagk_oracle_inv_log_max_dist.argtypes = [C.c_float, i32]
        lib.pagk_oracle_set_alternatives.restype = None
        lib.pagk_oracle_set_alternatives.argtypes = [C.c_uint32]
        lib.pagk_oracle_llt_solve4.restype = C.c_double
        lib.pagk_oracle_llt_solve4.argtypes = [vp, vp, vp]
        f32 = C.c_float
        lib.pagk_oracle_check_homography.restype = C.c_int
        lib.pagk_oracle_check_homography.argtypes = [vp, vp, i32, vp, vp, f32, vp, P(f32)]
        lib.pagk_oracle_check_fundamental.restype = C.c_int
        lib.pagk_oracle_check_fundamental.argtypes = [vp, i32, vp, vp, f32, vp, P(f32)]
        lib.pagk_oracle_geometry_select.restype = C.c_int
        lib.pagk_oracle_geometry_select.argtypes = [f32, f32]
        lib.pagk_oracle_geometry_validation.restype = C.c_int
        lib.pagk_oracle_geometry_validation.argtypes = [vp, vp, vp, i32, vp, vp, vp, f32, P(f32)]
        lib.pagk_oracle_ncc_free.restype = f32
        lib.pagk_oracle_ncc_free.argtypes = [P(Image), P(Image), i32, f32, f32, f32, f32, vp]
        lib.pagk_oracle_find_near_neighbors.restype = C.c_int
        lib.pagk_oracle_find_near_neighbors.argtypes = [P(Image), P(Image), i32, i32, vp, vp, vp, vp, i32, vp, vp, i32, f32,
                                                        i32, i32, vp, vp, vp, vp]
        lib.pagk_oracle_match_features.restype = C.c_int
        lib.pagk_oracle_match_features.argtypes = [i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp]
        lib.pagk_oracle_mat_inv3d.restype = None
        lib.pagk_oracle_mat_inv3d.argtypes = [vp, vp]
        # pagk_oracle_cv.h: OpenCV's arithmetic under the reference's ORB extractor
        i64 = C.c_int64
        lib.pagk_oracle_fast9.restype = C.c_int
        lib.pagk_oracle_fast9.argtypes = [vp, i64, i32, i32, i32, i32, vp]
        lib.pagk_oracle_resize_linear.restype = C.c_int
        lib.pagk_oracle_resize_linear.argtypes = [vp, i32, i32, i64, vp, i32, i32, i64]
        lib.pagk_oracle_border_reflect101.restype = C.c_int
        lib.pagk_oracle_border_reflect101.argtypes = [vp, i64, i32, i32, i32, i32]
        lib.pagk_oracle_blur7.restype = C.c_int
        lib.pagk_oracle_blur7.argtypes = [vp, i32, i32, i64, vp, vp, i64]
        lib.pagk_oracle_fast_atan2.restype = f32
        lib.pagk_oracle_fast_atan2.argtypes = [f32, f32]
        lib.pagk_oracle_pow_int.restype = C.c_double
        lib.pagk_oracle_pow_int.argtypes = [C.c_double, C.c_double, vp]
        lib.pagk_oracle_sin_cos.restype = None
        lib.pagk_oracle_sin_cos.argtypes = [C.c_double, vp, vp]
        _lib = lib
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data


def pyr_down(img: np.ndarray) -> np.ndarray:
    h, w = img.shape
    out = np.zeros((int(h * 0.5), int(w * 0.5)), np.uint8)
    rc = load().pagk_oracle_pyr_down(img.ctypes.data, w, h, img.strides[0], out.ctypes.data)
    if rc:
        raise RuntimeError(f"pagk_oracle_pyr_down: {rc}")
    return out


def sample(img: np.ndarray, xy: np.ndarray) -> np.ndarray:
    """PatchMatch::GetPixelValue (reference src/patch_match.cpp:391-406) on `img` (a row-strided view keeps its stride) at the
    (x, y) rows of `xy` -> float32 per row."""
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    n = int(xy.shape[0])
    out = np.zeros(max(n, 1), np.float32)
    iv = image_view(img)
    rc = load().pagk_oracle_sample(C.byref(iv), n, _p(xy), _p(out))
    if rc:
        raise RuntimeError(f"pagk_oracle_sample: {rc}")
    return out[:n]


def track(params: Params, img_ref, img_cur, pt_ref, pt_init, affine, status_in, nthreads: int = 1, out=None):
    n = int(pt_ref.shape[0])
    out = out if out is not None else alloc_outputs(n)
    ir, ic = image_view(img_ref), image_view(img_cur)
    o = outputs_struct(out)
    rc = load().pagk_oracle_track(C.byref(params), C.byref(ir), C.byref(ic), n, _p(pt_ref), _p(pt_init), _p(affine),
                                  _p(status_in), C.byref(o), nthreads)
    if rc:
        raise RuntimeError(f"pagk_oracle_track: {rc}")
    return out


def track_pyr(params: Params, ref_levels, cur_levels, pt_ref, pt_init, affine, status_in, nthreads: int = 1):
    n = int(pt_ref.shape[0])
    out = alloc_outputs(n)
    L = len(ref_levels)
    r = (Image * L)(*[image_view(a) for a in ref_levels])
    c = (Image * L)(*[image_view(a) for a in cur_levels])
    o = outputs_struct(out)
    rc = load().pagk_oracle_track_pyr(C.byref(params), L, r, c, n, _p(pt_ref), _p(pt_init), _p(affine),
                                      _p(status_in), C.byref(o), nthreads)
    if rc:
        raise RuntimeError(f"pagk_oracle_track_pyr: {rc}")
    return out


def post_filter(half_patch: int, status_pm, pix_err, dist_pred, pt_pm, pt_pm_un):
    n = int(status_pm.shape[0])
    status = np.zeros(max(n, 1), np.uint8)
    pp = np.zeros((max(n, 1), 2), np.float32)
    ppu = np.zeros((max(n, 1), 2), np.float32)
    rc = load().pagk_oracle_post_filter(n, half_patch, _p(status_pm), _p(pix_err), _p(dist_pred), _p(pt_pm),
                                        _p(pt_pm_un), _p(status), _p(pp), _p(ppu))
    if rc < 0:
        raise RuntimeError(f"pagk_oracle_post_filter: {rc}")
    return rc, status[:n], pp[:n], ppu[:n]


def gyro_predict(cam_params: Params, width, height, half_patch, KRKinv, r3, pt_ref):
    n = int(pt_ref.shape[0])
    KRKinv = np.ascontiguousarray(KRKinv, np.float32)
    r3 = np.ascontiguousarray(r3, np.float32)
    pu = np.zeros((n, 2), np.float32)
    pd = np.zeros((n, 2), np.float32)
    st = np.zeros(n, np.uint8)
    A = np.zeros((n, 4), np.float32)
    rc = load().pagk_oracle_gyro_predict(C.byref(cam_params), width, height, half_patch, KRKinv.ctypes.data,
                                         r3.ctypes.data, n, pt_ref.ctypes.data, pu.ctypes.data, pd.ctypes.data,
                                         st.ctypes.data, A.ctypes.data)
    if rc < 0:
        raise RuntimeError(f"pagk_oracle_gyro_predict: {rc}")
    return pu, pd, st, A


def set_alternatives(flags: int) -> None:
    """Switch the restatement's guesses about Eigen's associations (same bits as pagk_params::solver_variant; 16 = the
    pyramid's fixed-point path).  Global: reset to 0 after use."""
    load().pagk_oracle_set_alternatives(int(flags))


def llt_solve4(H: np.ndarray, b: np.ndarray):
    H = np.ascontiguousarray(H, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    x = np.zeros(4, np.float64)
    nrm = load().pagk_oracle_llt_solve4(H.ctypes.data, b.ctypes.data, x.ctypes.data)
    return x, nrm


def _mat3(M):
    M = np.ascontiguousarray(M, np.float64)
    assert M.size == 9
    return M


def check_homography(H21, H12, pts1, pts2, sigma=1.0):
    """CheckHomography scoring loop (reference src/gyro_aided_tracker.cpp:620-676) -> (inliers, score)."""
    H21, H12 = _mat3(H21), _mat3(H12)
    pts1 = np.ascontiguousarray(pts1, np.float32).reshape(-1, 2)
    pts2 = np.ascontiguousarray(pts2, np.float32).reshape(-1, 2)
    n = pts1.shape[0]
    inl = np.zeros(max(n, 1), np.uint8)
    sc = C.c_float(0)
    rc = load().pagk_oracle_check_homography(H21.ctypes.data, H12.ctypes.data, n, _p(pts1), _p(pts2), sigma,
                                             _p(inl), C.byref(sc))
    if rc < 0:
        raise RuntimeError(f"pagk_oracle_check_homography: {rc}")
    return inl[:n], np.float32(sc.value)


def check_fundamental(F21, pts1, pts2, sigma=1.0):
    """CheckFundamental scoring loop (reference src/gyro_aided_tracker.cpp:704-768) -> (inliers, score)."""
    F21 = _mat3(F21)
    pts1 = np.ascontiguousarray(pts1, np.float32).reshape(-1, 2)
    pts2 = np.ascontiguousarray(pts2, np.float32).reshape(-1, 2)
    n = pts1.shape[0]
    inl = np.zeros(max(n, 1), np.uint8)
    sc = C.c_float(0)
    rc = load().pagk_oracle_check_fundamental(F21.ctypes.data, n, _p(pts1), _p(pts2), sigma, _p(inl), C.byref(sc))
    if rc < 0:
        raise RuntimeError(f"pagk_oracle_check_fundamental: {rc}")
    return inl[:n], np.float32(sc.value)


def geometry_select(score_H, score_F) -> bool:
    return bool(load().pagk_oracle_geometry_select(float(score_H), float(score_F)))


def geometry_validation(H21, H12, F21, pt_ref_un, pt_predict_un, status, sigma=1.0):
    """GeometryValidation bookkeeping (reference src/gyro_aided_tracker.cpp:429-480) -> (cnt, status, score)."""
    H21, H12, F21 = _mat3(H21), _mat3(H12), _mat3(F21)
    p1 = np.ascontiguousarray(pt_ref_un, np.float32).reshape(-1, 2)
    p2 = np.ascontiguousarray(pt_predict_un, np.float32).reshape(-1, 2)
    st = np.array(status, np.uint8, copy=True)
    ts = C.c_float(0)
    rc = load().pagk_oracle_geometry_validation(H21.ctypes.data, H12.ctypes.data, F21.ctypes.data, st.shape[0],
                                                _p(p1), _p(p2), _p(st), sigma, C.byref(ts))
    if rc < 0:
        raise RuntimeError(f"pagk_oracle_geometry_validation: {rc}")
    return rc, st, np.float32(ts.value)


def ncc_free(img_ref, img_cur, half_patch, pt_ref, pt_cur, A=None) -> np.float32:
    """Free NCC over the free GetPixelValue (reference src/utils.cpp:166-200, include/utils.h:32-46)."""
    ir, ic = image_view(img_ref), image_view(img_cur)
    A = None if A is None else np.ascontiguousarray(A, np.float32).reshape(4)
    return np.float32(load().pagk_oracle_ncc_free(C.byref(ir), C.byref(ic), half_patch, float(pt_ref[0]), float(pt_ref[1]),
                                                  float(pt_cur[0]), float(pt_cur[1]), _p(A)))


def find_near_neighbors(img_ref, img_cur, half_patch, keys_ref, pt_predict_un, status, affine, keys_cur, keys_cur_un,
                        level=1, radius_unit=None, use_ncc=True, cap=64, count=None):
    """FindAndSortNearNeighbor (reference src/gyro_aided_tracker.cpp:788-851) -> dict(count, idx, dist, ncc, rc)."""
    n, m = int(keys_ref.shape[0]), int(keys_cur.shape[0])
    ir, ic = image_view(img_ref), image_view(img_cur)
    count = np.zeros(max(n, 1), np.int32) if count is None else np.array(count, np.int32, copy=True)
    idx = np.full((max(n, 1), cap), -1, np.int32)
    dist = np.zeros((max(n, 1), cap), np.float32)
    ncc = np.zeros((max(n, 1), cap), np.float32)
    ru = float(2 * half_patch) if radius_unit is None else float(radius_unit)
    rc = load().pagk_oracle_find_near_neighbors(C.byref(ir), C.byref(ic), half_patch, n, _p(keys_ref), _p(pt_predict_un),
                                                _p(status), _p(affine), m, _p(keys_cur), _p(keys_cur_un), level, ru,
                                                int(use_ncc), cap, _p(count), _p(idx), _p(dist), _p(ncc))
    return dict(count=count[:n], idx=idx[:n], dist=dist[:n], ncc=ncc[:n], rc=rc)


def match_features(count, idx, dist, ncc, use_ncc=True):
    """MatchFeatures (reference src/gyro_aided_tracker.cpp:949-1008) -> (query, train, dist, ncc) arrays."""
    n = int(count.shape[0])
    cap = int(idx.shape[1]) if idx.ndim == 2 else 1
    q = np.zeros(max(n, 1), np.int32)
    t = np.zeros(max(n, 1), np.int32)
    d = np.zeros(max(n, 1), np.float32)
    c = np.zeros(max(n, 1), np.float32)
    idx, dist, ncc = (np.ascontiguousarray(a) for a in (idx, dist, ncc))
    count = np.ascontiguousarray(count, np.int32)
    k = load().pagk_oracle_match_features(n, cap, _p(count), _p(idx), _p(dist), _p(ncc), int(use_ncc), _p(q), _p(t),
                                          _p(d), _p(c))
    if k < 0:
        raise RuntimeError(f"pagk_oracle_match_features: {k}")
    return q[:k], t[:k], d[:k], c[:k]


def mat_inv3d(M) -> np.ndarray:
    """The 3 x 3 f64 inverse the stand-in cv::Mat::inv() uses for H21.inv() (reference src/gyro_aided_tracker.cpp:598) -> 9 doubles."""
    M, out = _mat3(M), np.zeros(9, np.float64)
    load().pagk_oracle_mat_inv3d(M.ctypes.data, out.ctypes.data)
    return out


# ---- pagk_oracle_cv.h ------------------------------------------------------------------------------------------------------
def fast9(sub: np.ndarray, threshold: int) -> np.ndarray:
    """cv::FAST(sub, keys, threshold, true) -> (n, 3) int32 rows of x, y, score; sub may be a view with a row stride."""
    sub = np.asarray(sub, np.uint8)
    assert sub.strides[1] == 1
    h, w = sub.shape
    cap = ((w + 1) // 2) * ((h + 1) // 2) + 1
    out = np.zeros((cap, 3), np.int32)
    n = load().pagk_oracle_fast9(sub.ctypes.data, sub.strides[0], w, h, int(threshold), cap, out.ctypes.data)
    assert n >= 0
    return out[:n].copy()


def resize_linear(src: np.ndarray, dw: int, dh: int) -> np.ndarray:
    src = np.asarray(src, np.uint8)
    assert src.strides[1] == 1
    dst = np.zeros((dh, dw), np.uint8)
    assert load().pagk_oracle_resize_linear(src.ctypes.data, src.shape[1], src.shape[0], src.strides[0], dst.ctypes.data, dw, dh, dw) == 0
    return dst


def border_reflect101(img: np.ndarray, border: int, fill: int = -1) -> np.ndarray:
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    buf = np.zeros((h + 2 * border, w + 2 * border), np.uint8)
    buf[border:border + h, border:border + w] = img
    assert load().pagk_oracle_border_reflect101(buf.ctypes.data, buf.strides[0], w, h, border, fill) == 0
    return buf


def blur7(img: np.ndarray, weights=(54, 49, 34, 18)) -> np.ndarray:
    img = np.asarray(img, np.uint8)
    assert img.strides[1] == 1
    h, w = img.shape
    wt, out = np.array(weights, np.int32), np.zeros((h, w), np.uint8)
    assert load().pagk_oracle_blur7(img.ctypes.data, w, h, img.strides[0], wt.ctypes.data, out.ctypes.data, w) == 0
    return out


def fast_atan2(y, x) -> np.float32:
    return np.float32(load().pagk_oracle_fast_atan2(float(np.float32(y)), float(np.float32(x))))


def pow_int(base: float, n: float):
    """-> the repeated product, or None where n is no integer in [0, 64]"""
    ok = C.c_int32(0)
    p = load().pagk_oracle_pow_int(float(base), float(n), C.addressof(ok))
    return float(p) if ok.value else None


def sin_cos(x: float):
    sn, cs = C.c_double(0), C.c_double(0)
    load().pagk_oracle_sin_cos(float(x), C.addressof(sn), C.addressof(cs))
    return sn.value, cs.value
