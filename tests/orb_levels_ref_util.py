"""Test helpers of ORB over a scale pyramid (include/pagk.h "ORB over a scale pyramid"): the plain-C restatement
(tests/orb_levels_ref.c, compiled together with the unchanged tests/fast_detect_ref.c and tests/orb_ref.c) loaded with ctypes,
independent numpy models of the level table (float32 scalars) and of the resize (whole-array arithmetic), and the packing."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import detect_ref_util as du
import fast_ref_util as fu
import orb_ref_util as ou

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCES = [os.path.join(HERE, f) for f in ("orb_levels_ref.c", "fast_detect_ref.c", "orb_ref.c")]
MAX_LEVELS = 8
INFO_WORDS = 32
F = np.float32
SET_KEYS = ("keypoints", "octave", "response", "angle", "desc", "info")
DETECT_KEYS = ("keypoints", "octave", "response", "info")


def build_ref(out_dir):
    so = os.path.join(str(out_dir), "orb_levels_ref.so")
    subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so, *SOURCES,
                    "-lm"], check=True)
    lib = C.CDLL(so)
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    lib.olr_levels.restype = i32
    lib.olr_levels.argtypes = [i32, f32, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.olr_resize.restype = i32
    lib.olr_resize.argtypes = [vp, i32, i32, i64, vp, i32, i32, i64]
    lib.olr_extract.restype = i32
    lib.olr_extract.argtypes = [vp, i32, i32, i64, i32, f32, i32, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.fdr_detect.restype = i32
    lib.fdr_detect.argtypes = [vp, i32, i32, i64, vp, i32, i32, i32, i32, vp, vp, vp, vp, i32]
    lib.fdr_bounds.restype = i32
    lib.fdr_bounds.argtypes = [i32, i32, i32, vp, vp]
    lib.orb_ref_describe.restype = i32
    lib.orb_ref_describe.argtypes = [vp, i32, i32, i64, vp, vp, i32, i32, vp, vp, vp, vp, vp]
    return lib


# ---- the restatement -----------------------------------------------------------------------------------------------------
def ref_levels(lib, n_features, scale_factor, n_levels, w, h):
    """The level table, or None where the definition refuses."""
    lw, lh = np.zeros(MAX_LEVELS, np.int32), np.zeros(MAX_LEVELS, np.int32)
    sc, quota, size = np.zeros(MAX_LEVELS, np.float32), np.zeros(MAX_LEVELS, np.int32), np.zeros(MAX_LEVELS, np.int32)
    ob = C.c_int32(0)
    if lib.olr_levels(n_features, scale_factor, n_levels, w, h, lw.ctypes.data, lh.ctypes.data, sc.ctypes.data,
                      quota.ctypes.data, size.ctypes.data, C.addressof(ob)):
        return None
    n = n_levels
    return dict(n_levels=n, width=lw[:n], height=lh[:n], scale=sc[:n], quota=quota[:n], size=size[:n], out_bound=int(ob.value))


def ref_resize(lib, src, dw, dh, dpitch=None) -> np.ndarray:
    """src may be a view with a row stride above its width; dpitch: the destination's."""
    src = np.asarray(src, np.uint8)
    assert src.strides[1] == 1
    sh, sw = src.shape
    dpitch = dw if dpitch is None else int(dpitch)
    dst = np.full((dh, dpitch), 0xA5, np.uint8)
    assert lib.olr_resize(src.ctypes.data, sw, sh, src.strides[0], dst.ctypes.data, dw, dh, dpitch) == 0
    assert (dst[:, dw:] == 0xA5).all()
    return dst[:, :dw]


def ref_extract(lib, img, ex, pattern=None, mask=None, weights=ou.DEFAULT_WEIGHTS, cap=None) -> dict:
    """olr_extract: operator() with a pattern, DetectFeatures without -> dict(n, keypoints, octave, response, angle, desc
    (cap rows, zero beyond the count), info, levels (the pyramid, a list of arrays), table)."""
    img = np.asarray(img, np.uint8)
    assert img.strides[1] == 1
    h, w = img.shape
    table = ref_levels(lib, ex.n_features, ex.scale_factor, ex.n_levels, w, h)
    assert table is not None
    cap = table["out_bound"] if cap is None else int(cap)
    kp, octave = np.full((cap, 2), 7, np.float32), np.full(cap, 7, np.int32)
    resp, ang, desc = np.full(cap, 7, np.float32), np.full(cap, 7, np.float32), np.full((cap, 32), 7, np.uint8)
    info = np.full(INFO_WORDS, 7, np.int32)
    sizes = [int(a) * int(b) for a, b in zip(table["width"], table["height"])]
    levels = np.zeros(sum(sizes), np.uint8)
    wt = np.array(weights, np.int32)
    pat = None if pattern is None else np.ascontiguousarray(pattern, np.int32)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    rc = lib.olr_extract(img.ctypes.data, w, h, img.strides[0], ex.n_features, ex.scale_factor, ex.n_levels, ex.ini_threshold,
                         ex.min_threshold, wt.ctypes.data, None if pat is None else pat.ctypes.data,
                         None if m is None else m.ctypes.data, cap, kp.ctypes.data, octave.ctypes.data, resp.ctypes.data,
                         None if pat is None else ang.ctypes.data, None if pat is None else desc.ctypes.data, info.ctypes.data,
                         levels.ctypes.data)
    assert rc == 0
    lv, off = [], 0
    for lw, lh, s in zip(table["width"], table["height"], sizes):
        lv.append(levels[off:off + s].reshape(int(lh), int(lw)))
        off += s
    out = dict(n=int(info[0]), keypoints=kp, octave=octave, response=resp, info=info, levels=lv, table=table, cap=cap)
    if pat is not None:
        out.update(angle=ang, desc=desc)
    return out


def same_set(got: dict, want: dict, keys=SET_KEYS) -> list:
    """Names of the arrays of a device set (capi's dict: full_* hold cap rows) whose bytes differ from the restatement's."""
    bad = []
    for k in keys:
        g = got["info"] if k == "info" else got["full_" + k]
        if np.asarray(g).tobytes() != np.asarray(want[k]).tobytes():
            bad.append(k)
    return bad


# ---- the numpy models ----------------------------------------------------------------------------------------------------
def model_levels(n_features, scale_factor, n_levels, w, h):
    """The level table in float32 scalars, written from the definition; None where it refuses."""
    sf = F(scale_factor)
    if not (1 <= n_levels <= MAX_LEVELS and F(1) < sf <= F(1.5) and 1 <= n_features <= 1 << 24):
        return None
    sc = [F(1)]
    for _ in range(1, n_levels):
        sc.append(F(sc[-1] * sf))
    inv = [F(F(1) / s) for s in sc]
    factor = F(F(1) / sf)
    p = 1.0
    for _ in range(n_levels):
        p *= float(factor)
    nd = F(F(F(n_features) * F(F(1) - factor)) / F(F(1) - F(p)))
    quota = []
    for _ in range(n_levels - 1):
        quota.append(int(np.rint(nd)))
        nd = F(nd * factor)
    quota.append(max(n_features - sum(quota), 0))
    lw = [int(np.rint(F(F(w) * i))) for i in inv]
    lh = [int(np.rint(F(F(h) * i))) for i in inv]
    bound = 0
    for a, b, q in zip(lw, lh, quota):
        if not (62 <= a <= 32767 and 62 <= b <= 32767):
            return None
        g = fu.model_grid(a, b)
        if g is None:
            return None
        bound += max(max(q, 1) + 2, 4 * g["n_ini"])
    return dict(n_levels=n_levels, width=np.array(lw, np.int32), height=np.array(lh, np.int32), scale=np.array(sc, np.float32),
                quota=np.array(quota, np.int32), size=np.array([int(F(F(31) * s)) for s in sc], np.int32), out_bound=bound)


def _axis(dst: int, src: int, clip_only: bool):
    """Source index, second index and the two Q11 coefficients per destination index of one axis."""
    scale = 1.0 / (float(dst) / float(src))
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    if clip_only:                                   # rows: both indices clipped, the fraction kept
        s0, s1 = np.clip(s, 0, src - 1), np.clip(s + 1, 0, src - 1)
        c0 = np.rint((F(1) - f) * F(2048)).astype(np.int64)
        c1 = np.rint(f * F(2048)).astype(np.int64)
        return s0, s1, c0, c1
    low = s < 0
    f, s = np.where(low, F(0), f), np.where(low, 0, s)
    single = s + 1 >= src
    last = s >= src - 1
    f, s = np.where(last, F(0), f), np.where(last, src - 1, s)
    c0 = np.rint((F(1) - f) * F(2048)).astype(np.int64)
    c1 = np.rint(f * F(2048)).astype(np.int64)
    c0, c1 = np.where(single, 2048, c0), np.where(single, 0, c1)      # a single tap: S = 2048 I[s]
    return s, np.minimum(s + 1, src - 1), c0, c1


def model_resize(src, dw, dh) -> np.ndarray:
    src = np.asarray(src, np.int64)
    sh, sw = src.shape
    x0, x1, a0, a1 = _axis(dw, sw, False)
    y0, y1, b0, b1 = _axis(dh, sh, True)
    hor = src[:, x0] * a0[None, :] + src[:, x1] * a1[None, :]          # sh x dw
    s0, s1 = hor[y0, :], hor[y1, :]
    v = (((b0[:, None] * (s0 >> 4)) >> 16) + ((b1[:, None] * (s1 >> 4)) >> 16) + 2) >> 2
    return (v & 255).astype(np.uint8)


def model_pyramid(img, table) -> list:
    lv = [np.ascontiguousarray(img, np.uint8)]
    for l in range(1, table["n_levels"]):
        lv.append(model_resize(lv[-1], int(table["width"][l]), int(table["height"][l])))
    return lv


def compose(fast_lib, orb_lib, levels, table, ex, pattern, weights=ou.DEFAULT_WEIGHTS) -> dict:
    """The packing written in Python on top of the one-level restatements: per level fdr_detect (N = max(quota, 1), no mask)
    and orb_ref_describe on the level image, coordinates scaled in float32, levels in ascending order."""
    kp, octave, resp, ang, desc, counts = [], [], [], [], [], []
    for l, img in enumerate(levels):
        n_l = max(int(table["quota"][l]), 1)
        d = fu.ref_detect(fast_lib, img, None, n_l, ini=ex.ini_threshold, mn=ex.min_threshold)
        n = d["n"]
        r = ou.ref_describe(orb_lib, img, pattern, d["keypoints"][:n], weights) if n else dict(angle=np.zeros(0, F),
                                                                                                 desc=np.zeros((0, 32), np.uint8))
        pts = d["keypoints"][:n].astype(np.float32)
        if l:
            pts = pts * table["scale"][l]
        kp.append(pts), octave.append(np.full(n, l, np.int32)), resp.append(d["response"][:n])
        ang.append(r["angle"][:n]), desc.append(r["desc"][:n]), counts.append(n)
    return dict(keypoints=np.concatenate(kp), octave=np.concatenate(octave), response=np.concatenate(resp),
                angle=np.concatenate(ang), desc=np.concatenate(desc), counts=counts)


# ---- images --------------------------------------------------------------------------------------------------------------
def texture(synth, w, h, seed=21):
    return du.texture_image(synth, w, h, seed)


def padded(img, pad=5, fill=0xEE):
    """The same pixels in rows of width + pad bytes (a view: a pitch above the width)."""
    img = np.asarray(img, np.uint8)
    buf = np.full((img.shape[0], img.shape[1] + pad), fill, np.uint8)
    buf[:, :img.shape[1]] = img
    return buf[:, :img.shape[1]]
