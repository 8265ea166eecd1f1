"""Test helpers of the corner detector: the plain-C restatement (tests/corner_detect_ref.c) built and loaded with ctypes,
an independent numpy model of the definition in include/pagk.h, and the test images."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SRC = os.path.join(HERE, "corner_detect_ref.c")
INFO_WORDS = 8
DEFAULTS = dict(quality_level=0.005, min_distance=20.0, harris_k=0.04, raw_cap=0)   # reference src/frame.cpp:181-184


def build_ref(out_dir: str):
    """gcc -O2 -ffp-contract=off (one rounding per operation, like the library) -> ctypes library."""
    so = os.path.join(str(out_dir), "corner_detect_ref.so")
    subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                    REF_SRC, "-lm"], check=True)
    lib = C.CDLL(so)
    vp, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    lib.cdr_response.restype = i32
    lib.cdr_response.argtypes = [vp, i32, i32, i64, f64, vp]
    lib.cdr_raw_bound.restype = i64
    lib.cdr_raw_bound.argtypes = [i32, i32]
    lib.cdr_detect.restype = i32
    lib.cdr_detect.argtypes = [vp, i32, i32, i64, vp, f64, f64, f64, i32, i32, i32, vp, vp, vp]
    return lib


def ref_response(lib, img, harris_k=0.04) -> np.ndarray:
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    R = np.zeros((h, w), np.float32)
    assert lib.cdr_response(img.ctypes.data, w, h, img.strides[0], harris_k, R.ctypes.data) == 0
    return R


def ref_detect(lib, img, mask, max_corners, cap=None, *, quality_level=0.005, min_distance=20.0, harris_k=0.04,
               raw_cap=0, with_response=False) -> dict:
    """The restatement's detector -> dict(corners (cap x 2, zero beyond the count), info, n, R when asked for)."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    cap = max(int(max_corners), 1) if cap is None else int(cap)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    assert m is None or m.shape == (h, w)
    corners = np.zeros((cap, 2), np.float32)
    info = np.zeros(INFO_WORDS, np.int32)
    R = np.zeros((h, w), np.float32) if with_response else None
    rc = lib.cdr_detect(img.ctypes.data, w, h, img.strides[0], None if m is None else m.ctypes.data, quality_level,
                        min_distance, harris_k, raw_cap, int(max_corners), cap, corners.ctypes.data, info.ctypes.data,
                        None if R is None else R.ctypes.data)
    assert rc == 0
    out = dict(corners=corners, info=info, n=int(info[0]))
    if R is not None:
        out["R"] = R
    return out


# ---- the numpy model: whole-array operations, written from the header's text alone ------------------------------------
def model_response(img, harris_k=0.04) -> np.ndarray:
    p = np.pad(np.asarray(img, np.uint8).astype(np.int64), 1, mode="reflect")   # numpy's "reflect" repeats no edge
    h, w = img.shape

    def win(dy, dx):
        return p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    gx = (win(-1, 1) + 2 * win(0, 1) + win(1, 1)) - (win(-1, -1) + 2 * win(0, -1) + win(1, -1))
    gy = (win(1, -1) + 2 * win(1, 0) + win(1, 1)) - (win(-1, -1) + 2 * win(-1, 0) + win(-1, 1))

    def block(prod):
        q = np.pad(prod, 1, mode="reflect")
        return sum(q[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    a, b, c = (block(v).astype(np.float64) for v in (gx * gx, gx * gy, gy * gy))
    tr = a + c
    return ((a * c - b * b) - np.float64(harris_k) * (tr * tr)).astype(np.float32)   # numpy never fuses


def raw_bound(w: int, h: int) -> int:
    return -(-(w - 2) // 2) * -(-(h - 2) // 2)


def model_detect(img, mask, max_corners, cap=None, *, quality_level=0.005, min_distance=20.0, harris_k=0.04,
                 raw_cap=0) -> dict:
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    cap = max(int(max_corners), 1) if cap is None else int(cap)
    R = model_response(img, harris_k)
    m = np.ones((h, w), bool) if mask is None else np.asarray(mask) != 0
    corners = np.zeros((cap, 2), np.float32)
    info = np.zeros(INFO_WORDS, np.int32)
    out = dict(corners=corners, info=info, R=R, n=0)
    if not m.any():
        return out
    rmax = R[m].max()
    if not rmax > 0:
        return out
    info[3] = np.array([rmax], np.float32).view(np.int32)[0]
    c = R[1:-1, 1:-1]
    ok = m[1:-1, 1:-1] & (c.astype(np.float64) > np.float64(quality_level) * np.float64(rmax))
    for dy, dx in ((-1, -1), (-1, 0), (-1, 1), (0, -1)):
        ok &= c >= R[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
    for dy, dx in ((0, 1), (1, -1), (1, 0), (1, 1)):
        ok &= c > R[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
    ys, xs = np.nonzero(ok)
    ys, xs = ys + 1, xs + 1
    info[1] = len(ys)
    rc = raw_cap if raw_cap > 0 else raw_bound(w, h)
    if len(ys) > rc:
        info[2] = 1
        return out
    keys = (R[ys, xs].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (ys * w + xs).astype(np.uint64)
    order = np.argsort(keys)[::-1]
    limit = min(cap, max(0, int(max_corners)))
    acc = np.zeros((limit + 1, 2), np.int64)
    n = visited = 0
    d2 = np.float64(min_distance) * np.float64(min_distance)
    for i in order:
        if n >= limit:
            break
        visited += 1
        x, y = int(xs[i]), int(ys[i])
        if min_distance >= 1 and n:
            dd = acc[:n] - (x, y)
            if ((dd * dd).sum(1).astype(np.float64) < d2).any():
                continue
        acc[n] = (x, y)
        n += 1
    corners[:n] = acc[:n]
    info[0], info[4] = n, visited
    out["n"] = n
    return out


# ---- images ------------------------------------------------------------------------------------------------------------
def texture_image(synth, w: int, h: int, seed: int) -> np.ndarray:
    tex = synth.Texture(synth.SplitMix64(seed))
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.clip(np.rint(tex(xx, yy)), 0, 255).astype(np.uint8)


def noise_image(w: int, h: int, seed: int = 5) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def planted_squares(w: int = 640, h: int = 480):
    """Value 40 with 24 x 24 squares every 64 pixels from (30, 30), each a different grey -> image, the corner pixels."""
    img = np.full((h, w), 40, np.uint8)
    pts, k = [], 0
    for y0 in range(30, h - 64, 64):        # 7 rows and 9 columns at 640 x 480: 63 squares, 252 corners
        for x0 in range(30, w - 64, 64):
            img[y0:y0 + 24, x0:x0 + 24] = 90 + 2 * k
            k += 1
            pts += [(x0, y0), (x0 + 23, y0), (x0, y0 + 23), (x0 + 23, y0 + 23)]
    return img, pts


def tie_bar() -> np.ndarray:
    """64 x 64 of value 30, a bar of value 200 over rows 10-39, columns 31-32: mirror-symmetric about x = 31.5."""
    img = np.full((64, 64), 30, np.uint8)
    img[10:40, 31:33] = 200
    return img


def holes_mask(w: int, h: int, n: int = 300, seed: int = 11) -> np.ndarray:
    """All ones with n 14 x 14 holes placed like the hand-over places them (clamped into the image)."""
    rng = np.random.default_rng(seed)
    m = np.ones((h, w), np.uint8)
    for x, y in zip(rng.integers(-5, w + 5, n), rng.integers(-5, h + 5, n)):
        x0, y0 = min(max(0, int(x) - 7), w - 14), min(max(0, int(y) - 7), h - 14)
        m[y0:y0 + 14, x0:x0 + 14] = 0
    return m


def same_detect(a: dict, b: dict) -> list:
    """Names of the arrays whose bytes differ."""
    return [k for k in ("corners", "info") if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()]
