"""Test helpers of pyramidal Lucas-Kanade (include/pagk.h "Pyramidal Lucas-Kanade"): the plain-C restatement
(tests/lk_ref.c) built and loaded with ctypes, an independent numpy model written from the definition (padded planes,
whole-image derivative planes with a zero frame, window slices, Python integers for the exact sums, float32 scalars for the
tail), the image pairs and feature sets of the shapes the tests use: shapes(), the first table, and edge_shapes() and
pyramid_shapes(), the edges of the kernels."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SRC = os.path.join(HERE, "lk_ref.c")
INFO_WORDS = 8
MAX_LEVELS = 8
# why a feature left a level (the record `why` of the restatement and of the model)
NOT_VISITED, TEMPLATE, MIN_EIG, RANGE, EPSILON, OSCILLATION, COUNT = range(7)
F = np.float32
DEFAULTS = dict(half_patch=10, max_level=2, max_count=30, epsilon=0.01, min_eig_threshold=1e-4, err_threshold=12.0)
KEYS = ("pt_out", "status_raw", "status", "err", "flow", "info")


def build_ref(out_dir):
    so = os.path.join(str(out_dir), "lk_ref.so")
    subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                    REF_SRC, "-lm"], check=True)
    lib = C.CDLL(so)
    vp, i32, i64, f32, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double
    lib.lk_ref_levels.restype = i32
    lib.lk_ref_levels.argtypes = [i32, i32, i32, i32]
    lib.lk_ref_pyrdown.restype = None
    lib.lk_ref_pyrdown.argtypes = [vp, i32, i32, i64, vp]
    lib.lk_ref_scharr.restype = None
    lib.lk_ref_scharr.argtypes = [vp, i32, i32, i64, vp, vp]
    lib.lk_ref_level.restype = i32
    lib.lk_ref_level.argtypes = [vp, i32, i32, i64, i32, i32, i32, vp]
    lib.lk_ref_track.restype = i32
    lib.lk_ref_track.argtypes = [vp, vp, i32, i32, i64, i64, i32, i32, i32, f64, f64, f32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    return lib


def params(**over) -> dict:
    p = dict(DEFAULTS)
    p.update(over)
    return p


# ---- the restatement -----------------------------------------------------------------------------------------------------
def ref_pyrdown(lib, img) -> np.ndarray:
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    out = np.zeros(((h + 1) // 2, (w + 1) // 2), np.uint8)
    lib.lk_ref_pyrdown(img.ctypes.data, w, h, img.strides[0], out.ctypes.data)
    return out


def ref_scharr(lib, img):
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    dx, dy = np.zeros((h, w), np.int16), np.zeros((h, w), np.int16)
    lib.lk_ref_scharr(img.ctypes.data, w, h, img.strides[0], dx.ctypes.data, dy.ctypes.data)
    return dx, dy


def ref_levels(lib, img, p: dict) -> list:
    """Levels 0 .. top of the image's pyramid."""
    img = np.asarray(img, np.uint8)
    top = lib.lk_ref_levels(img.shape[1], img.shape[0], p["half_patch"], p["max_level"])
    assert top >= 0
    out = [img]
    for _ in range(top):
        out.append(ref_pyrdown(lib, out[-1]))
    return out


def ref_track(lib, img_ref, img_cur, pts, p: dict, cap=None, n=None) -> dict:
    """-> dict(pt_out, status_raw, status, err, flow (cap rows), info, iters, why (cap x 8)); rows beyond the count are zero."""
    a, b = np.asarray(img_ref, np.uint8), np.asarray(img_cur, np.uint8)
    h, w = a.shape
    pt = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    n = pt.shape[0] if n is None else int(n)
    cap = max(pt.shape[0], 1) if cap is None else int(cap)
    buf = np.zeros((cap, 2), np.float32)
    buf[:pt.shape[0]] = pt
    out = dict(pt_out=np.full((cap, 2), 7, np.float32), status=np.full(cap, 7, np.uint8), status_raw=np.full(cap, 7, np.uint8),
               err=np.full(cap, 7, np.float32), flow=np.full((cap, 2), 7, np.float32), info=np.full(INFO_WORDS, 7, np.int32),
               iters=np.full(cap, 7, np.int32), why=np.full((cap, MAX_LEVELS), 7, np.uint8))
    rc = lib.lk_ref_track(a.ctypes.data, b.ctypes.data, w, h, a.strides[0], b.strides[0], p["half_patch"], p["max_level"],
                          p["max_count"], p["epsilon"], p["min_eig_threshold"], p["err_threshold"], n, cap, buf.ctypes.data,
                          out["pt_out"].ctypes.data, out["status"].ctypes.data, out["status_raw"].ctypes.data,
                          out["err"].ctypes.data, out["flow"].ctypes.data, out["info"].ctypes.data, out["iters"].ctypes.data,
                          out["why"].ctypes.data)
    assert rc == 0, rc
    return out


def same_array(a, b) -> bool:
    """np.array_equal on the bits: float arrays must have their NaNs in the same places and identical bits elsewhere."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))


def differing(a: dict, b: dict, keys=KEYS) -> list:
    """Names of the arrays that differ."""
    return [k for k in keys if not same_array(a[k], b[k])]


# ---- the numpy model -----------------------------------------------------------------------------------------------------
def model_levels(w: int, h: int, half_patch: int, max_level: int) -> int:
    win = 2 * half_patch + 1
    if not (w > win and h > win):
        return -1
    sizes = [(w, h)]
    for _ in range(max_level):
        w, h = (w + 1) // 2, (h + 1) // 2
        sizes.append((w, h))
    ok = [sw > win and sh > win for sw, sh in sizes]
    return next((l for l in range(1, len(ok)) if not ok[l]), len(ok)) - 1


_K5 = np.outer([1, 4, 6, 4, 1], [1, 4, 6, 4, 1]).astype(np.int64)


def model_pyrdown(img) -> np.ndarray:
    a = np.pad(np.asarray(img, np.int64), 2, mode="reflect")        # numpy's "reflect" is BORDER_REFLECT_101
    h, w = np.asarray(img).shape
    dh, dw = (h + 1) // 2, (w + 1) // 2
    a = np.pad(a, ((0, 2), (0, 2)), mode="edge")                     # (room for the strided slices; never read)
    acc = np.zeros((dh, dw), np.int64)
    for j in range(5):
        for i in range(5):
            acc += _K5[j, i] * a[j:j + 2 * dh:2, i:i + 2 * dw:2]
    return ((acc + 128) >> 8).astype(np.uint8)


def model_scharr(img):
    """The two derivative planes of a level (int64), the neighbours through the reflected index."""
    a = np.pad(np.asarray(img, np.int64), 1, mode="reflect")
    up, mid, dn = a[:-2, :], a[1:-1, :], a[2:, :]
    t0 = 3 * (up + dn) + 10 * mid                                    # h x (w + 2)
    t1 = dn - up
    dx = t0[:, 2:] - t0[:, :-2]
    dy = 3 * (t1[:, :-2] + t1[:, 2:]) + 10 * t1[:, 1:-1]
    return dx, dy


class _Level:
    """One pyramid level padded for the window reads: gray by reflection, derivatives by zeros, `win + 1` wide."""

    def __init__(self, img, win: int):
        self.h, self.w = img.shape
        self.pad = win + 1
        self.gray = np.pad(np.asarray(img, np.int64), self.pad, mode="reflect")
        dx, dy = model_scharr(img)
        self.dx, self.dy = np.pad(dx, self.pad), np.pad(dy, self.pad)

    def window(self, plane, x0: int, y0: int, win: int, iw):
        """sum over the four neighbours of plane * iw for the win x win pixels from (x0, y0)."""
        y, x = y0 + self.pad, x0 + self.pad
        p = plane[y:y + win + 1, x:x + win + 1]
        return p[:-1, :-1] * iw[0] + p[:-1, 1:] * iw[1] + p[1:, :-1] * iw[2] + p[1:, 1:] * iw[3]


def _weights(a, b):
    one, s = F(1.0), F(16384.0)
    iw00 = int(np.rint((one - a) * (one - b) * s))
    iw01 = int(np.rint(a * (one - b) * s))
    iw10 = int(np.rint((one - a) * b * s))
    return iw00, iw01, iw10, 16384 - iw00 - iw01 - iw10


def _outside(fx, fy, win, w, h) -> bool:
    if not (np.isfinite(fx) and np.isfinite(fy)):
        return True
    return bool(fx < -win or fx >= w or fy < -win or fy >= h)


def model_track(img_ref, img_cur, pts, p: dict, cap=None, n=None) -> dict:
    win = 2 * p["half_patch"] + 1
    h0, w0 = np.asarray(img_ref).shape
    top = model_levels(w0, h0, p["half_patch"], p["max_level"])
    assert top >= 0
    li, lj = [np.asarray(img_ref, np.uint8)], [np.asarray(img_cur, np.uint8)]
    for _ in range(top):
        li.append(model_pyrdown(li[-1]))
        lj.append(model_pyrdown(lj[-1]))
    LI, LJ = [_Level(m, win) for m in li], [_Level(m, win) for m in lj]
    pt = np.asarray(pts, np.float32).reshape(-1, 2)
    n = pt.shape[0] if n is None else min(max(int(n), 0), pt.shape[0])
    cap = max(pt.shape[0], 1) if cap is None else int(cap)
    n = min(n, cap)
    out = dict(pt_out=np.zeros((cap, 2), np.float32), status=np.zeros(cap, np.uint8), status_raw=np.zeros(cap, np.uint8),
               err=np.zeros(cap, np.float32), flow=np.zeros((cap, 2), np.float32), info=np.zeros(INFO_WORDS, np.int32),
               iters=np.zeros(cap, np.int32), why=np.zeros((cap, MAX_LEVELS), np.uint8))
    info, why = out["info"], out["why"]
    info[0], info[3] = n, top
    half = F(win - 1) * F(0.5)
    scale20 = F(2.0) ** F(-20)
    eps2 = float(p["epsilon"]) * float(p["epsilon"])
    with np.errstate(all="ignore"):
        for k in range(n):
            ref = pt[k]
            st, err = 1, F(0)
            nxt = np.zeros(2, np.float32)
            for l in range(top, -1, -1):
                I, J = LI[l], LJ[l]
                prev = ref * F(1.0 / (1 << l))
                nxt = prev.copy() if l == top else F(2.0) * nxt
                q = prev - half
                f = np.floor(q)
                if _outside(f[0], f[1], win, I.w, I.h):
                    if l == 0:
                        st, err = 0, F(0)
                        info[5] += 1
                    why[k, l] = TEMPLATE
                    continue
                ix0, iy0 = int(f[0]), int(f[1])
                iw = _weights(q[0] - f[0], q[1] - f[1])
                ival = (I.window(I.gray, ix0, iy0, win, iw) + 256) >> 9
                gx = (I.window(I.dx, ix0, iy0, win, iw) + 8192) >> 14
                gy = (I.window(I.dy, ix0, iy0, win, iw) + 8192) >> 14
                A11 = F(int((gx * gx).sum())) * scale20
                A12 = F(int((gx * gy).sum())) * scale20
                A22 = F(int((gy * gy).sum())) * scale20
                D = A11 * A22 - A12 * A12
                min_eig = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + F(4.0) * A12 * A12)) / F(2 * win * win)
                if float(min_eig) < p["min_eig_threshold"] or D < np.finfo(np.float32).eps:
                    if l == 0:
                        st = 0
                        info[4] += 1
                    why[k, l] = MIN_EIG
                    continue
                D = F(1.0) / D
                q = nxt - half
                pd = np.zeros(2, np.float32)
                why[k, l] = COUNT                                      # unless the loop is left early
                for j in range(p["max_count"]):
                    f = np.floor(q)
                    if _outside(f[0], f[1], win, J.w, J.h):
                        if l == 0:
                            st = 0
                            info[5] += 1
                        why[k, l] = RANGE
                        break
                    if l == 0:
                        out["iters"][k] = j + 1
                    iw = _weights(q[0] - f[0], q[1] - f[1])
                    diff = ((J.window(J.gray, int(f[0]), int(f[1]), win, iw) + 256) >> 9) - ival
                    b1 = F(int((diff * gx).sum())) * scale20
                    b2 = F(int((diff * gy).sum())) * scale20
                    d = np.array([(A12 * b2 - A22 * b1) * D, (A12 * b1 - A11 * b2) * D], np.float32)
                    q = q + d
                    nxt = q + half
                    if float(d[0]) * float(d[0]) + float(d[1]) * float(d[1]) <= eps2:
                        why[k, l] = EPSILON
                        break
                    if j > 0 and float(abs(d[0] + pd[0])) < 0.01 and float(abs(d[1] + pd[1])) < 0.01:
                        nxt = nxt - d * F(0.5)
                        why[k, l] = OSCILLATION
                        break
                    pd = d
                if l == 0 and st:
                    e = nxt - half
                    f = np.floor(e)
                    if _outside(f[0], f[1], win, J.w, J.h):
                        st = 0
                        info[5] += 1
                    else:
                        iw = _weights(e[0] - f[0], e[1] - f[1])
                        diff = ((J.window(J.gray, int(f[0]), int(f[1]), win, iw) + 256) >> 9) - ival
                        err = F(int(np.abs(diff).sum())) / F(32 * win * win)
            out["pt_out"][k] = nxt
            out["err"][k] = err
            out["status_raw"][k] = st
            out["status"][k] = 1 if (st and not err >= F(p["err_threshold"])) else 0
            out["flow"][k] = nxt - ref
            info[1] += st
            info[2] += int(out["status"][k])
    return out


# ---- image pairs and feature sets ----------------------------------------------------------------------------------------
def texture_pair(synth, w: int, h: int, seed: int, shift=(0.0, 0.0), gain: float = 1.0):
    """A synth texture and the same texture seen `shift` pixels further: a feature at p in the first image is at p + shift in
    the second."""
    tex = synth.Texture(synth.SplitMix64(seed))
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    a = np.clip(np.rint(tex(xx, yy)), 0, 255).astype(np.uint8)
    b = np.clip(np.rint(gain * tex(xx - shift[0], yy - shift[1])), 0, 255).astype(np.uint8)
    return a, b


def interior_points(w: int, h: int, count: int, margin: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(margin, w - 1 - margin, count), rng.uniform(margin, h - 1 - margin, count)]).astype(np.float32)


def border_points(w: int, h: int, win: int) -> np.ndarray:
    """Features on the borders; whose template's corner lies at -win and at W - 1 exactly, one step beyond either; a NaN
    and a 1e9 coordinate."""
    half = (win - 1) / 2
    return np.array([(0, 0), (w - 1, h - 1), (0, h - 1), (w - 1, 0), (0.5, h / 2), (w / 2, 0.25), (w - 1.5, h / 2),
                     (-win + half, h / 2), (-win + half - 0.5, h / 2), (w - 1 + half, h / 2), (w + half, h / 2),
                     (w / 2, -win + half), (w / 2, -win + half - 1), (w / 2, h - 1 + half), (w / 2, h + half),
                     (np.nan, h / 2), (w / 2, 1e9), (-1e9, np.nan)], np.float32)


def shapes(synth) -> dict:
    """The cases of the tests: name -> dict(ref, cur, pts, p, cap, n).  The smallest frames at which each rule can go wrong."""
    out = {}

    def add(name, w, h, hp, count, seed, shift, border=False, cap=None, n=None, spoil=False, **over):
        a, b = texture_pair(synth, w, h, seed, shift)
        if spoil:                                                        # a brighter left third: err >= 12 there (the filter)
            b[:, :w // 3] = np.clip(b[:, :w // 3].astype(np.int32) + 40 + 10 * (np.arange(h)[:, None] % 3), 0, 255)
        win = 2 * hp + 1
        pts = interior_points(w, h, count, min(hp, w // 4, h // 4), seed + 1)
        if border:
            bp = border_points(w, h, win)
            pts[:len(bp)] = bp
        pts[len(pts) // 2::7] = np.rint(pts[len(pts) // 2::7])          # some on integer coordinates (a = b = 0)
        out[name] = dict(ref=a, cur=b, pts=pts, p=params(half_patch=hp, **over), cap=cap, n=n)

    add("48x36 h2: three levels, borders, non-finite", 48, 36, 2, 64, 21, (1.3, -0.8), border=True)
    add("96x64 h10: top level cut to 1", 96, 64, 10, 64, 22, (-1.6, 1.1), spoil=True)
    add("40x24 h10: level 0 only", 40, 24, 10, 32, 23, (0.6, 0.4))
    add("33x31 h1: win 3, every parent odd", 33, 31, 1, 32, 24, (0.4, -0.3), border=True)
    add("160x120 h15: 961 pixels", 160, 120, 15, 64, 25, (2.2, -1.7))
    add("160x120 h5: cap 300, count 257", 160, 120, 5, 257, 26, (-2.4, 1.9), cap=300, n=257, spoil=True)
    return out


# ---- the edge table ------------------------------------------------------------------------------------------------------
NPIX_OF_WIN = {3: 1, 7: 1, 9: 2, 11: 2, 13: 4, 15: 4, 17: 8, 21: 8, 23: 16, 31: 16}   # both ends of every k_lk_track<NPIX>


def fine_pair(synth, w: int, h: int, seed: int, shift=(0.0, 0.0), zoom: float = 2.5):
    """texture_pair seen from `zoom` times further away: wavelengths from 6 / zoom px, so that a frame of a few pixels still
    has structure in both directions."""
    tex = synth.Texture(synth.SplitMix64(seed))
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    a = np.clip(np.rint(tex(zoom * xx, zoom * yy)), 0, 255).astype(np.uint8)
    b = np.clip(np.rint(tex(zoom * (xx - shift[0]), zoom * (yy - shift[1]))), 0, 255).astype(np.uint8)
    return a, b


def checkerboard(w: int, h: int, block: int = 4, dx: int = 0) -> np.ndarray:
    """0 / 255 in block x block squares, the pattern moved dx pixels to the right."""
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((xx - dx) // block + yy // block) & 1) * 255).astype(np.uint8)


def mixed_points(w: int, h: int, win: int, count: int, seed: int, nonfinite: bool) -> np.ndarray:
    """`count` features: the border points (with or without the three non-finite ones) first, the rest anywhere in the frame,
    every fourth of those on integer coordinates (a = b = 0)."""
    rng = np.random.default_rng(seed)
    pts = np.column_stack([rng.uniform(0, w - 1, count), rng.uniform(0, h - 1, count)]).astype(np.float32)
    bp = border_points(w, h, win)
    bp = bp if nonfinite else bp[:15]
    m = min(len(bp), count // 2)
    pts[:m] = bp[len(bp) - m:]                       # (the far end of the list: the non-finite ones, where asked for)
    pts[m::4] = np.rint(pts[m::4])
    return pts


# min_eig_threshold of the "about half" case, chosen on the CPU from the restatement's own minEig values on the frame
# "p7 96x80 defaults" below: 41 of its 48 features reach step 5 at level 0, and a scan of the threshold gave info[4] (lost to
# step 5 at level 0) = 4 at 0 and 1e-5 (D < FLT_EPSILON alone), 11 at 1e-4 .. 3e-3, 14 at 0.005, 16 at 0.007, 19 at 0.01,
# 20 at 0.012, 29 at 0.015, 36 at 0.02: the 20th smallest minEig lies between 0.01 and 0.012.
MIN_EIG_HALF = 0.012
ERR_NEVER = 256.0      # err = sum |diff| / (32 win^2) with |diff| <= 8160: at most 255


def edge_shapes(synth) -> dict:
    """The second table: name -> dict(ref, cur, pts, p, cap, n, npix, pitch, pyr, host, base).  pitch: None or the pitches of
    the (reference, current) slot; pyr: None or the parameters the pyramids are built with; host: the case also runs through
    the host form; base: None or the name of the default-parameter case on the same frame."""
    out = {}

    def put(name, a, b, pts, npix, pitch=None, pyr=None, host=False, base=None, **over):
        host = host or (npix == 4 and pitch is None and pyr is None)     # every k_lk_track<4> case the host form can express
        out[name] = dict(ref=a, cur=b, pts=pts, p=params(**over), cap=None, n=None, npix=npix, pitch=pitch, pyr=pyr,
                         host=host, base=base)

    # 1. every instantiation at both ends of its window range, on the smallest legal frame and on three levels
    shifts = [(1.0, -1.5), (-2.5, 1.0), (1.5, 2.0), (-1.0, -2.5), (2.5, -1.0)]
    for i, (win, npix) in enumerate(NPIX_OF_WIN.items()):
        hp = win // 2
        m = win + 1
        a, b = fine_pair(synth, m, m, 100 + win, (0.4, -0.3))
        put(f"win{win} npix{npix} minimal {m}x{m}", a, b, mixed_points(m, m, win, 40, 200 + win, nonfinite=(i % 2 == 0)),
            npix, host=True, half_patch=hp, max_level=0)
        w, h = min(4 * win + 9, 160), min(4 * win + 6, 128)
        a, b = texture_pair(synth, w, h, 300 + win, shifts[i % len(shifts)])
        put(f"win{win} npix{npix} three levels {w}x{h}", a, b, mixed_points(w, h, win, 48, 400 + win, nonfinite=(i % 2 == 1)),
            npix, half_patch=hp)

    # 2. parameters off their defaults, half patch 7 (k_lk_track<4>), top level 2
    w, h = 96, 80
    a, b = texture_pair(synth, w, h, 51, (1.7, -1.2))
    b[:, :w // 3] = np.clip(b[:, :w // 3].astype(np.int32) + 40 + 10 * (np.arange(h)[:, None] % 3), 0, 255)   # (the filter)
    # an almost flat field with a few pixels one or two gray levels up: minEig far below 1e-4 while D stays above FLT_EPSILON,
    # so that these features are lost to min_eig_threshold and to nothing else
    rng = np.random.default_rng(57)
    flat = (90 + (rng.random((30, 34)) < 0.08) * rng.integers(1, 3, (30, 34))).astype(np.uint8)
    a[28:58, 38:72] = flat
    b[28:58, 38:72] = flat
    pts = mixed_points(w, h, 15, 48, 52, nonfinite=True)
    pts[20:26] = [(52, 40), (55.5, 43.25), (57, 44), (53.75, 41.5), (56, 45), (54.25, 42.75)]
    base = "p7 96x80 defaults"
    put(base, a, b, pts, 4, half_patch=7)
    for key, val in (("max_count", 1), ("max_count", 2), ("epsilon", 0.0), ("epsilon", 1.0), ("min_eig_threshold", 0.0),
                     ("min_eig_threshold", MIN_EIG_HALF), ("err_threshold", 0.0), ("err_threshold", ERR_NEVER),
                     ("max_level", 0), ("max_level", 1)):
        put(f"p7 96x80 {key}={val:g}", a, b, pts, 4, base=base, half_patch=7, **{key: val})
    put("p7 96x80 pitches 29 and 3", a, b, pts, 4, pitch=(w + 29, w + 3), base=base, half_patch=7)
    put("p7 96x80 pitches 3 and 29", a, b, pts, 4, pitch=(w + 3, w + 29), base=base, half_patch=7)
    w, h = 160, 128
    a, b = texture_pair(synth, w, h, 53, (-2.3, 1.9))
    pts = mixed_points(w, h, 15, 48, 54, nonfinite=False)
    put("p7 160x128 max_level=7: top 3", a, b, pts, 4, half_patch=7, max_level=7)
    put("p7 160x128 max_level=1 over pyramids of 3", a, b, pts, 4, pyr=params(half_patch=7, max_level=3), half_patch=7,
        max_level=1)
    w, h = 136, 120
    a, b = texture_pair(synth, w, h, 55, (3.1, -2.6))
    put("p2 136x120 max_level=7: top 4", a, b, mixed_points(w, h, 5, 48, 56, nonfinite=True), 1, half_patch=2, max_level=7)

    # 3. extreme contrast: 0 / 255 squares of 4 x 4 against their inverse and against themselves one pixel further
    for hp, npix in ((7, 4), (15, 16)):
        w, h = (72, 68) if hp == 15 else (48, 44)
        a = checkerboard(w, h)
        pts = mixed_points(w, h, 2 * hp + 1, 32, 60 + hp, nonfinite=False)
        pts[1::2] = np.rint(pts[1::2])
        put(f"checker h{hp} inverse", a, 255 - a, pts, npix, half_patch=hp, max_level=1)
        put(f"checker h{hp} one pixel", a, checkerboard(w, h, dx=1), pts, npix, half_patch=hp, max_level=1)
        # with level 0 alone the first iteration of a feature on integer coordinates reads J where the template read I, with
        # a = b = 0: every diff is 32 (255 - 0) = 8160 or its negative (tests/test_lk_cpu.py asserts it)
        put(f"checker h{hp} inverse level 0", a, 255 - a, pts, npix, half_patch=hp, max_level=0)
    return out


def pyramid_shapes() -> dict:
    """Frames for the pyramid kernel's grid of 64 x 4 blocks, half patch 1, max_level 7: name -> image (seeded noise).  Level
    widths 63, 64, 65, 128 and 129; level heights of every residue modulo 4 from an even and from an odd parent; widths from
    even and odd parents."""
    sizes = [(257, 13), (130, 11), (127, 10), (256, 20), (126, 16), (125, 9), (258, 14)]
    rng = np.random.default_rng(70)
    return {f"{w}x{h}": rng.integers(0, 256, (h, w), dtype=np.uint8) for w, h in sizes}
