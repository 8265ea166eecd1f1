"""Test helpers of the rectification (include/pagk.h "rectification"): the plain-C restatement (tests/rectify_ref.c) built
and loaded with ctypes, an independent whole-array numpy model written from the header's text -- in OpenCV's table form,
with the saturated weight, so that it also checks the header's claim that both forms give the same bytes --, a numpy f64
model of pagk_undistort_maps, and the maps and raw frames of the tests."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SRC = os.path.join(HERE, "rectify_ref.c")
GRAY_WEIGHT, GRAY_SHIFT = (4899, 9617, 1868), 14     # CV_RGB2GRAY on R, G, B, OpenCV 3.4 (the header's defaults)
CHANNELS = (1, 3, 4)

# two cameras at 640 x 480 (fx, fy, cx, cy, dist = k1 k2 p1 p2 k3, the camera the rectified image is seen through)
MILD = dict(fx=382.6, fy=382.1, cx=320.7, cy=237.9, dist=(-0.0563, 0.0641, -0.0008, 0.0003, -0.0205), new_camera=None)
# k1 = -0.28 seen through a wider camera: the corners of the rectified image look beyond the sensor (the black border)
STRONG = dict(fx=461.6, fy=460.3, cx=325.2, cy=241.4, dist=(-0.28, 0.07, 0.0002, -0.0001, 0.0),
              new_camera=(300.0, 300.0, 320.0, 240.0))


def build_ref(out_dir: str):
    """gcc -O2 -ffp-contract=off -> ctypes library."""
    so = os.path.join(str(out_dir), "rectify_ref.so")
    subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                    REF_SRC, "-lm"], check=True)
    lib = C.CDLL(so)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    lib.rcr_rectify.restype = i32
    lib.rcr_rectify.argtypes = [vp, vp, i32, i32, i64, vp, i32, i32, i64, i32, vp, i32, vp, i64]
    return lib


def raw_dims(raw: np.ndarray):
    """(Ws, Hs, cn, step) of a raw frame: Hs x Ws (one channel) or Hs x Ws x cn, rows possibly strided."""
    assert raw.dtype == np.uint8 and raw.ndim in (2, 3) and raw.strides[-1] == 1
    cn = 1 if raw.ndim == 2 else raw.shape[2]
    assert raw.ndim == 2 or raw.strides[1] == cn
    return raw.shape[1], raw.shape[0], cn, raw.strides[0]


def ref_rectify(lib, map_x, map_y, raw, weights=GRAY_WEIGHT, shift=GRAY_SHIFT) -> np.ndarray:
    """The restatement: the rectified gray image of the maps' shape."""
    mx, my = np.ascontiguousarray(map_x, np.float32), np.ascontiguousarray(map_y, np.float32)
    assert mx.ndim == 2 and mx.shape == my.shape
    ws, hs, cn, step = raw_dims(raw)
    gw = (C.c_int32 * 3)(*weights)
    dst = np.zeros(mx.shape, np.uint8)
    rc = lib.rcr_rectify(mx.ctypes.data, my.ctypes.data, mx.shape[1], mx.shape[0], mx.strides[0], raw.ctypes.data, ws, hs,
                         step, cn, gw, shift, dst.ctypes.data, dst.strides[0])
    assert rc == 0
    return dst


# ---- the numpy model: whole-array operations, OpenCV's table form ------------------------------------------------------
def model_fixed(m):
    """-> (valid, ix, f): rne(m * 32) split into the saturated integer tap and the 5-bit fraction."""
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.asarray(m, np.float32) * np.float32(32)
        valid = np.isfinite(p) & (np.abs(p) < np.float32(2.0 ** 31))
    s = np.rint(np.where(valid, p, np.float32(0))).astype(np.int64)        # np.rint: ties to even
    return valid, np.clip(s >> 5, -32768, 32767), s & 31


def model_rectify(map_x, map_y, raw, weights=GRAY_WEIGHT, shift=GRAY_SHIFT) -> np.ndarray:
    ws, hs, cn, _ = raw_dims(raw)
    src = np.asarray(raw).reshape(hs, ws, cn).astype(np.int64)
    vx, ix, fx = model_fixed(map_x)
    vy, iy, fy = model_fixed(map_y)
    # the interpolation table of OpenCV's remap: weights (1 - fx/32)(1 - fy/32) ... scaled by 2^15, saturated to 16 bits
    tab = [np.minimum((a * b) * 32, 32767) for a, b in (((32 - fx), (32 - fy)), (fx, (32 - fy)), ((32 - fx), fy), (fx, fy))]
    padded = np.zeros((hs + 2, ws + 2, cn), np.int64)                       # BORDER_CONSTANT 0 as a ring of zeros
    padded[1:-1, 1:-1] = src

    def tap(dx, dy):
        x, y = np.clip(ix + dx + 1, 0, ws + 1), np.clip(iy + dy + 1, 0, hs + 1)
        return padded[y, x]                                                 # H x W x cn
    acc = sum(tap(dx, dy) * t[..., None] for (dx, dy), t in zip(((0, 0), (1, 0), (0, 1), (1, 1)), tab))
    v = (acc + (1 << 14)) >> 15
    v[~(vx & vy)] = 0
    if cn == 1:
        return v[..., 0].astype(np.uint8)
    g = (v[..., 0] * weights[0] + v[..., 1] * weights[1] + v[..., 2] * weights[2] + (1 << (shift - 1))) >> shift
    return g.astype(np.uint8)


def model_gray(raw, weights=GRAY_WEIGHT, shift=GRAY_SHIFT) -> np.ndarray:
    """The gray formula on a 3- or 4-channel image."""
    a = np.asarray(raw).astype(np.int64)
    return ((a[..., 0] * weights[0] + a[..., 1] * weights[1] + a[..., 2] * weights[2] + (1 << (shift - 1))) >> shift).astype(np.uint8)


def model_undistort_maps(fx, fy, cx, cy, dist, width, height, new_camera=None):
    """pagk_undistort_maps in numpy f64, the header's operation order (numpy never fuses a multiply with an add)."""
    d = list(dist) + [0.0] * (5 - len(dist))
    k1, k2, p1, p2, k3 = (np.float64(v) for v in d)
    nfx, nfy, ncx, ncy = (np.float64(v) for v in (new_camera if new_camera is not None else (fx, fy, cx, cy)))
    fx, fy, cx, cy = (np.float64(v) for v in (fx, fy, cx, cy))
    r, c = np.mgrid[0:height, 0:width].astype(np.float64)
    x, y = (c - ncx) / nfx, (r - ncy) / nfy
    x2, y2 = x * x, y * y
    r2, xy2 = x2 + y2, (2.0 * x) * y
    kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = (x * kr + p1 * xy2) + p2 * (r2 + 2.0 * x2)
    yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * xy2
    return (fx * xd + cx).astype(np.float32), (fy * yd + cy).astype(np.float32)


# ---- maps and raw frames -----------------------------------------------------------------------------------------------
def noise_raw(ws: int, hs: int, cn: int, seed: int, pad: int = 0) -> np.ndarray:
    """Bytes in [1, 255] (a 0 in a result is then a border or a "no pixel"), rows ws * cn + pad bytes apart."""
    buf = np.random.default_rng(seed).integers(1, 256, (hs, ws * cn + pad), dtype=np.uint8)
    v = buf[:, :ws * cn]
    return v if cn == 1 else v.reshape(hs, ws, cn)


def grid_maps(w: int, h: int, ws: int, hs: int, seed: int):
    """Map values k / 64 with k uniform over [-3, ws + 3] x [-3, hs + 3]: every odd k is an exact tie of map * 32."""
    rng = np.random.default_rng(seed)
    kx = rng.integers(-3 * 64, (ws + 3) * 64 + 1, (h, w))
    ky = rng.integers(-3 * 64, (hs + 3) * 64 + 1, (h, w))
    return (kx / 64.0).astype(np.float32), (ky / 64.0).astype(np.float32), kx, ky


def identity_maps(w: int, h: int):
    r, c = np.mgrid[0:h, 0:w]
    return c.astype(np.float32), r.astype(np.float32)


def lens_maps(cam: dict, w: int, h: int):
    """The numpy model's maps of a camera scaled from 640 x 480 to w x h."""
    sx, sy = w / 640.0, h / 480.0
    new = cam["new_camera"]
    new = None if new is None else (new[0] * sx, new[1] * sy, new[2] * sx, new[3] * sy)
    return model_undistort_maps(cam["fx"] * sx, cam["fy"] * sy, cam["cx"] * sx, cam["cy"] * sy, cam["dist"], w, h, new)


NONFINITE = (np.nan, np.inf, -np.inf, 1e9, -1e9)


def small_cases(cn: int) -> dict:
    """name -> (map_x, map_y, raw): the cases of the CPU test, which the GPU test runs too."""
    ws, hs = 64, 40
    raw = noise_raw(ws, hs, cn, 100 + cn, pad=5)
    out = {}
    mx, my, _, _ = grid_maps(70, 37, ws, hs, 7)
    out["grid 70x37"] = (mx, my, raw)
    out["identity"] = identity_maps(ws, hs) + (raw,)
    ix, iy = identity_maps(ws, hs)
    out["last column"] = (np.full_like(ix, ws - 1), iy, raw)
    out["last row"] = (ix, np.full_like(iy, hs - 1), raw)
    bx, by = identity_maps(ws + 3, hs + 3)
    out["four borders"] = (bx - np.float32(1.25), by - np.float32(1.75), raw)       # taps -2 .. ws, -2 .. hs
    nx, ny = identity_maps(ws, hs)
    for k, v in enumerate(NONFINITE):
        nx[3 + k, 5] = v
        ny[20 + k, 9] = v
    out["non-finite"] = (nx, ny, raw)
    return out
