"""Test helpers of the ORB descriptors and the matcher (include/pagk.h "ORB descriptors and matching"): the plain-C
restatement (tests/orb_ref.c) built and loaded with ctypes, an independent numpy model written from the definition (padded
convolutions, a disc mask, float32 scalars, unpacked bits), seeded sampling patterns and the test images."""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess

import numpy as np

import detect_ref_util as du

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SRC = os.path.join(HERE, "orb_ref.c")
INFO_WORDS = 8
EDGE = 19
DEFAULT_WEIGHTS = (54, 49, 34, 18)
UMAX = (15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3)
F = np.float32
FACTOR_PI = F(math.pi / float(F(180.0)))          # (float)(CV_PI / 180.f)


def build_ref(out_dir):
    so = os.path.join(str(out_dir), "orb_ref.so")
    subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                    REF_SRC, "-lm"], check=True)
    lib = C.CDLL(so)
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    lib.orb_ref_blur.restype = i32
    lib.orb_ref_blur.argtypes = [vp, i32, i32, i64, vp, vp]
    lib.orb_ref_fast_atan2.restype = f32
    lib.orb_ref_fast_atan2.argtypes = [f32, f32]
    lib.orb_ref_cos_sin.restype = None
    lib.orb_ref_cos_sin.argtypes = [f32, vp, vp]
    lib.orb_ref_moments.restype = None
    lib.orb_ref_moments.argtypes = [vp, i64, i32, i32, vp]
    lib.orb_ref_describe.restype = i32
    lib.orb_ref_describe.argtypes = [vp, i32, i32, i64, vp, vp, i32, i32, vp, vp, vp, vp, vp]
    lib.orb_ref_match.restype = i32
    lib.orb_ref_match.argtypes = [i32, i32, vp, i32, vp, i32, vp, vp, vp, vp]
    return lib


# ---- patterns and images -------------------------------------------------------------------------------------------------
def seeded_pattern(seed: int = 31) -> np.ndarray:
    """1024 int32 in [-13, 13]: 512 pseudo-random points (the reference's own table is not part of this repository)."""
    return np.random.default_rng(seed).integers(-13, 14, 1024).astype(np.int32)


def corner_pattern() -> np.ndarray:
    """The four corners (+-13, +-13) repeated: every tap at the largest reach the range allows."""
    return np.tile(np.array([13, 13, -13, 13, 13, -13, -13, -13], np.int32), 128)


def images(synth) -> dict:
    yy, xx = np.mgrid[0:80, 0:97]
    out = {"97x80 texture": du.texture_image(synth, 97, 80, 11), "160x120 texture": du.texture_image(synth, 160, 120, 12),
           "flat": np.full((80, 97), 130, np.uint8),
           "horizontal step": np.where(yy < 40, 30, 220).astype(np.uint8),       # the edge is a row: m10 = 0 at a centred point
           "vertical step": np.where(xx < 48, 30, 220).astype(np.uint8)}         # the edge is a column: m01 = 0
    for k in range(8):                                                           # a gradient in each octant
        t = math.radians(22.5 + 45.0 * k)
        g = 128.0 + 2.5 * ((xx - 48) * math.cos(t) + (yy - 40) * math.sin(t))
        out[f"gradient octant {k}"] = np.clip(np.rint(g), 0, 255).astype(np.uint8)
    return out


def grid_keypoints(w: int, h: int, step: int = 7) -> np.ndarray:
    """Keypoints all over the image, border and .5 coordinates included."""
    xs = np.arange(15.0, w - 14, step)
    ys = np.arange(15.0, h - 14, step)
    kp = np.array([(x, y) for y in ys for x in xs], np.float32)
    kp[1::3] += F(0.5)
    kp[2::5, 0] += F(0.25)
    return np.concatenate([kp, border_keypoints(w, h)])


def border_keypoints(w: int, h: int) -> np.ndarray:
    """The last valid centres (19, W - 20), the first flagged ones (18, W - 19), ties of the rounding (20.5 -> 20,
    21.5 -> 22, 18.5 -> 18 is flagged, W - 19.5 -> W - 20 or W - 19 by its parity), a NaN and a huge coordinate."""
    return np.array([(19, 19), (w - 20, h - 20), (19, h - 20), (w - 20, 19), (18, 30), (w - 19, 30), (30, 18), (30, h - 19),
                     (20.5, 21.5), (21.5, 20.5), (18.5, 30), (19.5, 30), (w - 19.5, 30), (30, h - 19.5), (-3, 30),
                     (np.nan, 30), (30, 1e30), (18.49, 19.49)], np.float32)


def many_keypoints(w: int, h: int, count: int, seed: int = 4) -> np.ndarray:
    """border_keypoints first, then seeded centres all over the image (some outside the border, a third on .5)."""
    rng = np.random.default_rng(seed)
    b = border_keypoints(w, h)
    kp = np.column_stack([rng.integers(16, w - 16, count), rng.integers(16, h - 16, count)]).astype(np.float32)
    kp[::3] += F(0.5)
    kp[:len(b)] = b
    return kp[:count]


# ---- the restatement -----------------------------------------------------------------------------------------------------
def ref_blur(lib, img, weights=DEFAULT_WEIGHTS) -> np.ndarray:
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    wt = np.array(weights, np.int32)
    out = np.zeros((h, w), np.uint8)
    assert lib.orb_ref_blur(img.ctypes.data, w, h, img.strides[0], wt.ctypes.data, out.ctypes.data) == 0
    return out


def ref_describe(lib, img, pattern, keypoints, weights=DEFAULT_WEIGHTS, cap=None, n=None) -> dict:
    """-> dict(angle (cap), desc (cap x 32), info, blurred); rows beyond the count are zero."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    kp = np.ascontiguousarray(keypoints, np.float32).reshape(-1, 2)
    n = kp.shape[0] if n is None else int(n)
    cap = max(kp.shape[0], 1) if cap is None else int(cap)
    buf = np.zeros((cap, 2), np.float32)
    buf[:kp.shape[0]] = kp
    wt, pat = np.array(weights, np.int32), np.ascontiguousarray(pattern, np.int32)
    ang, desc = np.full(cap, 7, np.float32), np.full((cap, 32), 7, np.uint8)
    info, bl = np.full(INFO_WORDS, 7, np.int32), np.zeros((h, w), np.uint8)
    rc = lib.orb_ref_describe(img.ctypes.data, w, h, img.strides[0], wt.ctypes.data, pat.ctypes.data, n, cap,
                              buf.ctypes.data, ang.ctypes.data, desc.ctypes.data, info.ctypes.data, bl.ctypes.data)
    assert rc == 0
    return dict(angle=ang, desc=desc, info=info, blurred=bl)


def ref_match(lib, desc_q, desc_t, match_floor=30, cap_q=None, nq=None, nt=None) -> dict:
    dq = np.ascontiguousarray(desc_q, np.uint8).reshape(-1, 32)
    dt = np.ascontiguousarray(desc_t, np.uint8).reshape(-1, 32)
    nq = dq.shape[0] if nq is None else int(nq)
    nt = dt.shape[0] if nt is None else int(nt)
    cap_q = max(dq.shape[0], 1) if cap_q is None else int(cap_q)
    idx, dist = np.full(cap_q, 7, np.int32), np.full(cap_q, 7, np.int32)
    keep, info = np.full(cap_q, 7, np.uint8), np.full(INFO_WORDS, 7, np.int32)
    qp = dq.ctypes.data if dq.size else None
    tp = dt.ctypes.data if dt.size else None
    assert lib.orb_ref_match(nq, cap_q, qp, nt, tp, match_floor, idx.ctypes.data, dist.ctypes.data, keep.ctypes.data,
                             info.ctypes.data) == 0
    return dict(train_idx=idx, distance=dist, keep=keep, info=info)


def same(a: dict, b: dict, keys) -> list:
    """Names of the arrays whose bytes differ."""
    return [k for k in keys if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()]


DESC_KEYS = ("angle", "desc", "info")
MATCH_KEYS = ("train_idx", "distance", "keep", "info")


# ---- the numpy model -----------------------------------------------------------------------------------------------------
def model_blur(img, weights=DEFAULT_WEIGHTS) -> np.ndarray:
    w7 = np.array([weights[abs(k)] for k in range(-3, 4)], np.int64)
    a = np.pad(np.asarray(img, np.int64), 3, mode="reflect")            # numpy's "reflect" is BORDER_REFLECT_101
    h, w = np.asarray(img).shape
    hor = sum(w7[k] * a[:, k:k + w] for k in range(7))                  # (h + 6) x w: rows still padded
    ver = sum(w7[k] * hor[k:k + h, :] for k in range(7))
    return ((ver + 32768) >> 16).astype(np.uint8)


def model_fast_atan2(y, x):
    """cv::fastAtan2's scalar form, every operation rounded to float32."""
    y, x = F(y), F(x)
    p1, p3 = F(0.9997878412794807) * F(180 / math.pi), F(-0.3258083974640975) * F(180 / math.pi)
    p5, p7 = F(0.1555786518463281) * F(180 / math.pi), F(-0.04432655554792128) * F(180 / math.pi)
    eps = F(2.220446049250313e-16)
    ax, ay = abs(x), abs(y)
    if ax >= ay:
        c = ay / (ax + eps)
        c2 = c * c
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    else:
        c = ax / (ay + eps)
        c2 = c * c
        a = F(90.0) - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    if x < 0:
        a = F(180.0) - a
    if y < 0:
        a = F(360.0) - a
    return F(a)


_S = (-1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04, 2.75573137070700676789e-06,
      -2.50507602534068634195e-08, 1.58969099521155010221e-10)
_C = (4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05, -2.75573143513906633035e-07,
      2.08757232129817482790e-09, -1.13596475577881948265e-11)


def model_cos_sin(r):
    """The steering pair by the algorithm stated in include/pagk.h, in Python floats (IEEE doubles, one rounding each)."""
    x = float(F(r))
    k = int(x * float.fromhex("0x1.45f306dc9c883p-1") + 0.5)
    t = (x - k * float.fromhex("0x1.921fb544p+0")) - k * float.fromhex("0x1.0b4611a626331p-34")
    z = t * t
    s = t + t * (z * (_S[0] + z * (_S[1] + z * (_S[2] + z * (_S[3] + z * (_S[4] + z * _S[5]))))))
    c = 1.0 - z * (0.5 - z * (_C[0] + z * (_C[1] + z * (_C[2] + z * (_C[3] + z * (_C[4] + z * _C[5]))))))
    co, si = ((c, s), (-s, c), (-c, -s), (s, -c))[k & 3]
    return F(co), F(si)


_DISC = np.array([[abs(u) <= UMAX[abs(v)] for u in range(-15, 16)] for v in range(-15, 16)])
_U = np.arange(-15, 16, dtype=np.int64)[None, :] * _DISC
_V = np.arange(-15, 16, dtype=np.int64)[:, None] * _DISC


def model_moments(img, cx: int, cy: int):
    p = np.asarray(img, np.int64)[cy - 15:cy + 16, cx - 15:cx + 16]
    return int((_U * p).sum()), int((_V * p).sum())


def model_describe(img, pattern, keypoints, weights=DEFAULT_WEIGHTS, cap=None, n=None) -> dict:
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    kp = np.asarray(keypoints, np.float32).reshape(-1, 2)
    n = kp.shape[0] if n is None else min(max(int(n), 0), kp.shape[0])
    cap = max(kp.shape[0], 1) if cap is None else int(cap)
    bl = model_blur(img, weights)
    pts = np.asarray(pattern, np.int32).reshape(512, 2).astype(np.float32)
    ang, desc, info = np.zeros(cap, np.float32), np.zeros((cap, 32), np.uint8), np.zeros(INFO_WORDS, np.int32)
    for k in range(n):
        fx, fy = np.rint(kp[k, 0]), np.rint(kp[k, 1])
        if not (EDGE <= fx < w - EDGE and EDGE <= fy < h - EDGE):
            ang[k] = -1.0
            info[1] += 1
            continue
        cx, cy = int(fx), int(fy)
        m10, m01 = model_moments(img, cx, cy)
        ang[k] = model_fast_atan2(F(m01), F(m10))
        a, b = model_cos_sin(ang[k] * FACTOR_PI)
        rows = cy + np.rint(pts[:, 0] * b + pts[:, 1] * a).astype(np.int64)      # float32 arrays: one rounding per operation
        cols = cx + np.rint(pts[:, 0] * a - pts[:, 1] * b).astype(np.int64)
        taps = bl[rows, cols]
        bits = (taps[0::2] < taps[1::2]).astype(np.uint8)                        # pair q: points 2q, 2q + 1
        desc[k] = np.packbits(bits.reshape(32, 8), axis=1, bitorder="little")[:, 0]
        info[0] += 1
    return dict(angle=ang, desc=desc, info=info, blurred=bl)


def model_match(desc_q, desc_t, match_floor=30, cap_q=None, nq=None, nt=None) -> dict:
    dq = np.asarray(desc_q, np.uint8).reshape(-1, 32)
    dt = np.asarray(desc_t, np.uint8).reshape(-1, 32)
    nq = dq.shape[0] if nq is None else int(nq)
    nt = dt.shape[0] if nt is None else int(nt)
    cap_q = max(dq.shape[0], 1) if cap_q is None else int(cap_q)
    idx, dist = np.full(cap_q, -1, np.int32), np.full(cap_q, 257, np.int32)
    keep, info = np.zeros(cap_q, np.uint8), np.zeros(INFO_WORDS, np.int32)
    matches = nq if nt > 0 else 0
    if matches:
        d = np.unpackbits(dq[:nq, None, :] ^ dt[None, :nt, :], axis=2).sum(axis=2)       # nq x nt
        idx[:nq] = d.argmin(axis=1)                                                      # the first minimum: the lowest index
        dist[:nq] = d.min(axis=1)
    mn, mx = (int(dist[:nq].min()), int(dist[:nq].max())) if matches else (0, 0)
    thr = max(2 * mn, match_floor)
    keep[:matches] = dist[:matches] <= thr
    info[:6] = (nq, matches, int(keep.sum()), mn, mx, thr)
    return dict(train_idx=idx, distance=dist, keep=keep, info=info)


def random_descriptors(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)


def flip_bits(row: np.ndarray, k: int, seed: int = 0) -> np.ndarray:
    """A copy of a 32-byte row with exactly k of its 256 bits flipped."""
    bits = np.unpackbits(row)
    pos = np.random.default_rng(seed).permutation(256)[:k]
    bits[pos] ^= 1
    return np.packbits(bits)
