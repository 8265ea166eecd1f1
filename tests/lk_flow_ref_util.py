"""Test helpers of the flow form of pyramidal Lucas-Kanade (include/pagk.h, the addendum of "Pyramidal Lucas-Kanade"): the
plain-C restatement tests/lk_flow_ref.c built and loaded with ctypes, a numpy model of the same written on the padded planes
of tests/lk_ref_util.py, and flow_edge_shapes(), the flow edge table: every k_lk_flow<NPIX> at both ends of its window range
on the smallest legal frame of the window (and on three levels), initial points that are the reference point, a sub-pixel
step, a negative step, several windows away, infinite and NaN, a mix of status_in values, a count below the capacity, and
cameras with four and five coefficients and with dist_coef[0] == 0."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import lk_ref_util as lu

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SRC = os.path.join(HERE, "lk_flow_ref.c")
F = np.float32
KEYS = lu.KEYS + ("pt_out_dist",)
# offsets pt_init - pt_ref of the table, by feature index modulo len(OFFSETS); "far" is multiplied by the window
OFFSETS = ("zero", "sub-pixel", "negative", "far", "inf", "nan")
# fx fy cx cy | k1 k2 p1 p2 k3 | coefficients: the reference's D435i model, a five-coefficient model, and one with k1 == 0 (a
# copy whatever the other coefficients say); the principal point is moved into each frame by flow_edge_shapes()
CAMERAS = {
    "four": ((394.5643528049837, 395.2103902700227), (-0.0027697209770466296, -0.0007212258451583873, 0.00029903960869777114,
                                                      0.0003981049435158156, 0.0), 4),
    "five": ((61.5, 59.25), (-0.2834, 0.0739, 0.00019, 1.76e-05, -0.0112), 5),
    "copy": ((61.5, 59.25), (0.0, 0.0739, 0.00019, 1.76e-05, -0.0112), 5),
}


def build_ref(out_dir):
    so = os.path.join(str(out_dir), "lk_flow_ref.so")
    subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                    REF_SRC, "-lm"], check=True)
    lib = C.CDLL(so)
    vp, i32, i64, f32, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double
    lib.lk_flow_ref_track.restype = i32
    lib.lk_flow_ref_track.argtypes = [vp, vp, i32, i32, i64, i64, i32, i32, i32, f64, f64, f32, vp, i32, i32, i32] + [vp] * 12
    return lib


def camera_array(cam) -> np.ndarray | None:
    """cam: None or dict(fx, fy, cx, cy, dist (five values), n) -> the nine floats of the restatement."""
    if cam is None:
        return None
    return np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"], *cam["dist"]], np.float32)


def ref_flow(lib, img_ref, img_cur, pts, p: dict, cam=None, pt_init=None, status_in=None, cap=None, n=None) -> dict:
    """-> dict(pt_out, pt_out_dist (with a camera), status_raw, status, err, flow (cap rows), info, iters, why (cap x 8))."""
    a, b = np.asarray(img_ref, np.uint8), np.asarray(img_cur, np.uint8)
    h, w = a.shape
    pt = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    n = pt.shape[0] if n is None else int(n)
    cap = max(pt.shape[0], 1) if cap is None else int(cap)

    def rows(src, width, dtype, fill):
        if src is None:
            return None
        buf = np.full((cap, width) if width > 1 else (cap,), fill, dtype)
        src = np.asarray(src, dtype).reshape((-1, width) if width > 1 else (-1,))
        buf[:len(src)] = src
        return buf
    buf, init, live = rows(pt, 2, np.float32, 0), rows(pt_init, 2, np.float32, 0), rows(status_in, 1, np.uint8, 1)
    cam9 = camera_array(cam)
    out = dict(pt_out=np.full((cap, 2), 7, np.float32), status=np.full(cap, 7, np.uint8), status_raw=np.full(cap, 7, np.uint8),
               err=np.full(cap, 7, np.float32), flow=np.full((cap, 2), 7, np.float32), info=np.full(lu.INFO_WORDS, 7, np.int32),
               iters=np.full(cap, 7, np.int32), why=np.full((cap, lu.MAX_LEVELS), 7, np.uint8))
    if cam is not None:
        out["pt_out_dist"] = np.full((cap, 2), 7, np.float32)
    addr = lambda x: None if x is None else x.ctypes.data     # noqa: E731
    rc = lib.lk_flow_ref_track(a.ctypes.data, b.ctypes.data, w, h, a.strides[0], b.strides[0], p["half_patch"], p["max_level"],
                               p["max_count"], p["epsilon"], p["min_eig_threshold"], p["err_threshold"], addr(cam9),
                               cam["n"] if cam else 4, n, cap, buf.ctypes.data, addr(init), addr(live), out["pt_out"].ctypes.data,
                               addr(out.get("pt_out_dist")), out["status"].ctypes.data, out["status_raw"].ctypes.data,
                               out["err"].ctypes.data, out["flow"].ctypes.data, out["info"].ctypes.data,
                               out["iters"].ctypes.data, out["why"].ctypes.data)
    assert rc == 0, rc
    return out


# ---- the numpy model -----------------------------------------------------------------------------------------------------
def model_distort(pts, cam) -> np.ndarray:
    """DistortVecPoints (reference src/utils.cpp:49-76) in float32, one rounding per operation; a copy when k1 == 0."""
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    d = np.asarray(cam["dist"], np.float32)
    if d[0] == 0:
        return pts.copy()
    fx, fy, cx, cy = F(cam["fx"]), F(cam["fy"]), F(cam["cx"]), F(cam["cy"])
    fxi, fyi = F(1.0 / float(fx)), F(1.0 / float(fy))
    k1, k2, p1, p2 = d[0], d[1], d[2], d[3]
    k3 = d[4] if cam["n"] == 5 else F(0)
    one, two = F(1), F(2)
    with np.errstate(all="ignore"):
        x, y = (pts[:, 0] - cx) * fxi, (pts[:, 1] - cy) * fyi
        r2 = x * x + y * y
        r4 = r2 * r2
        r6 = r4 * r2
        rad = one + k1 * r2 + k2 * r4 + k3 * r6
        xd = x * rad + two * p1 * x * y + p2 * (r2 + two * x * x)
        yd = y * rad + p1 * (r2 + two * y * y) + two * p2 * x * y
        return np.column_stack([fx * xd + cx, fy * yd + cy]).astype(np.float32)


def model_flow(img_ref, img_cur, pts, p: dict, cam=None, pt_init=None, status_in=None, cap=None, n=None) -> dict:
    """The flow form from the definition: per live feature the level loop of the definition with the top level's next taken
    from pt_init; skipped and unused rows are zeros."""
    win = 2 * p["half_patch"] + 1
    h0, w0 = np.asarray(img_ref).shape
    top = lu.model_levels(w0, h0, p["half_patch"], p["max_level"])
    assert top >= 0
    li, lj = [np.asarray(img_ref, np.uint8)], [np.asarray(img_cur, np.uint8)]
    for _ in range(top):
        li.append(lu.model_pyrdown(li[-1]))
        lj.append(lu.model_pyrdown(lj[-1]))
    LI, LJ = [lu._Level(m, win) for m in li], [lu._Level(m, win) for m in lj]
    pt = np.asarray(pts, np.float32).reshape(-1, 2)
    start = pt if pt_init is None else np.asarray(pt_init, np.float32).reshape(-1, 2)
    live = np.ones(len(pt), np.uint8) if status_in is None else np.asarray(status_in, np.uint8)
    n = pt.shape[0] if n is None else min(max(int(n), 0), pt.shape[0])
    cap = max(pt.shape[0], 1) if cap is None else int(cap)
    n = min(n, cap)
    out = dict(pt_out=np.zeros((cap, 2), np.float32), status=np.zeros(cap, np.uint8), status_raw=np.zeros(cap, np.uint8),
               err=np.zeros(cap, np.float32), flow=np.zeros((cap, 2), np.float32), info=np.zeros(lu.INFO_WORDS, np.int32),
               iters=np.zeros(cap, np.int32), why=np.zeros((cap, lu.MAX_LEVELS), np.uint8))
    info, why = out["info"], out["why"]
    info[0], info[3] = n, top
    half = F(win - 1) * F(0.5)
    scale20 = F(2.0) ** F(-20)
    eps2 = float(p["epsilon"]) * float(p["epsilon"])
    tracked = np.zeros(cap, bool)
    with np.errstate(all="ignore"):
        for k in range(n):
            if not live[k]:
                info[6] += 1
                continue
            tracked[k] = True
            st, err = 1, F(0)
            nxt = np.zeros(2, np.float32)
            for l in range(top, -1, -1):
                I, J = LI[l], LJ[l]
                sc = F(1.0 / (1 << l))
                nxt = start[k] * sc if l == top else F(2.0) * nxt
                q = pt[k] * sc - half
                f = np.floor(q)
                if lu._outside(f[0], f[1], win, I.w, I.h):
                    if l == 0:
                        st, err = 0, F(0)
                        info[5] += 1
                    why[k, l] = lu.TEMPLATE
                    continue
                ix0, iy0 = int(f[0]), int(f[1])
                iw = lu._weights(q[0] - f[0], q[1] - f[1])
                ival = (I.window(I.gray, ix0, iy0, win, iw) + 256) >> 9
                gx = (I.window(I.dx, ix0, iy0, win, iw) + 8192) >> 14
                gy = (I.window(I.dy, ix0, iy0, win, iw) + 8192) >> 14
                A11, A12, A22 = (F(int(v.sum())) * scale20 for v in (gx * gx, gx * gy, gy * gy))
                D = A11 * A22 - A12 * A12
                min_eig = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + F(4.0) * A12 * A12)) / F(2 * win * win)
                if float(min_eig) < p["min_eig_threshold"] or D < np.finfo(np.float32).eps:
                    if l == 0:
                        st = 0
                        info[4] += 1
                    why[k, l] = lu.MIN_EIG
                    continue
                D = F(1.0) / D
                q = nxt - half
                pd = np.zeros(2, np.float32)
                why[k, l] = lu.COUNT
                for j in range(p["max_count"]):
                    f = np.floor(q)
                    if lu._outside(f[0], f[1], win, J.w, J.h):
                        if l == 0:
                            st = 0
                            info[5] += 1
                        why[k, l] = lu.RANGE
                        break
                    if l == 0:
                        out["iters"][k] = j + 1
                    iw = lu._weights(q[0] - f[0], q[1] - f[1])
                    diff = ((J.window(J.gray, int(f[0]), int(f[1]), win, iw) + 256) >> 9) - ival
                    b1 = F(int((diff * gx).sum())) * scale20
                    b2 = F(int((diff * gy).sum())) * scale20
                    d = np.array([(A12 * b2 - A22 * b1) * D, (A12 * b1 - A11 * b2) * D], np.float32)
                    q = q + d
                    nxt = q + half
                    if float(d[0]) * float(d[0]) + float(d[1]) * float(d[1]) <= eps2:
                        why[k, l] = lu.EPSILON
                        break
                    if j > 0 and float(abs(d[0] + pd[0])) < 0.01 and float(abs(d[1] + pd[1])) < 0.01:
                        nxt = nxt - d * F(0.5)
                        why[k, l] = lu.OSCILLATION
                        break
                    pd = d
                if l == 0 and st:
                    e = nxt - half
                    f = np.floor(e)
                    if lu._outside(f[0], f[1], win, J.w, J.h):
                        st = 0
                        info[5] += 1
                    else:
                        iw = lu._weights(e[0] - f[0], e[1] - f[1])
                        diff = ((J.window(J.gray, int(f[0]), int(f[1]), win, iw) + 256) >> 9) - ival
                        err = F(int(np.abs(diff).sum())) / F(32 * win * win)
            out["pt_out"][k] = nxt
            out["err"][k] = err
            out["status_raw"][k] = st
            out["status"][k] = 1 if (st and not err >= F(p["err_threshold"])) else 0
            out["flow"][k] = nxt - pt[k]
            info[1] += st
            info[2] += int(out["status"][k])
    if cam is not None:
        out["pt_out_dist"] = np.zeros((cap, 2), np.float32)
        out["pt_out_dist"][tracked] = model_distort(out["pt_out"][tracked], cam)
    return out


# ---- the flow edge table -------------------------------------------------------------------------------------------------
def offsets(count: int, win: int) -> np.ndarray:
    """pt_init - pt_ref per feature, the kinds of OFFSETS in turn."""
    kinds = {"zero": (0.0, 0.0), "sub-pixel": (0.3125, -0.4375), "negative": (-1.75, -2.5), "far": (3.0 * win + 0.5, 2.0 * win),
             "inf": (np.inf, 0.0), "nan": (0.0, np.nan)}
    return np.array([kinds[OFFSETS[k % len(OFFSETS)]] for k in range(count)], np.float32)


def flow_edge_shapes(synth) -> dict:
    """name -> dict(ref, cur, pts, init, live, p, cam, cap, n, npix, kind): per window of lk_ref_util.NPIX_OF_WIN the smallest
    legal frame (level 0 alone) and a frame of three levels.  n rows are handed in, of cap = n + 5 (the rest must come back
    zero); status_in switches off about a quarter of the rows; the cameras take turns."""
    out = {}
    shifts = [(1.0, -1.5), (-2.5, 1.0), (1.5, 2.0), (-1.0, -2.5), (2.5, -1.0)]
    cams = list(CAMERAS)
    for i, (win, npix) in enumerate(lu.NPIX_OF_WIN.items()):
        hp = win // 2
        m = win + 1
        w3, h3 = min(4 * win + 9, 160), min(4 * win + 6, 128)
        frames = (("minimal", m, m, lu.fine_pair(synth, m, m, 500 + win, (0.4, -0.3)), dict(half_patch=hp, max_level=0)),
                  ("three levels", w3, h3, lu.texture_pair(synth, w3, h3, 600 + win, shifts[i % len(shifts)]), dict(half_patch=hp)))
        for j, (kind, w, h, (a, b), over) in enumerate(frames):
            count = 42
            pts = lu.mixed_points(w, h, win, count, 700 + win + j, nonfinite=((i + j) % 2 == 0))
            # the border points come first: move them behind the interior points so that every kind of offset meets both
            pts = np.roll(pts, count // 2, axis=0)
            with np.errstate(invalid="ignore"):
                init = (pts + offsets(count, win)).astype(np.float32)
            rng = np.random.default_rng(800 + win + j)
            live = (rng.random(count) >= 0.25).astype(np.uint8)
            live[[1, 9, 17]] = (0, 1, 0)
            (fx, fy), dist, ncoef = CAMERAS[cams[(i + j) % len(cams)]]
            cam = dict(fx=fx, fy=fy, cx=w / 2.0 - 0.5, cy=h / 2.0 - 0.25, dist=dist, n=ncoef, name=cams[(i + j) % len(cams)])
            n = count - 2                                            # (the last two points are never handed in)
            out[f"win{win} npix{npix} {kind} {w}x{h} camera {cam['name']}"] = dict(
                ref=a, cur=b, pts=pts, init=init, live=live, p=lu.params(**over), cam=cam, cap=n + 5, n=n, npix=npix, kind=kind)
    return out


def run_case(fn, c, flow=True, **kw):
    """fn = a bound ref_flow / model_flow taking (ref, cur, pts, p, ...): the case in flow mode, or with flags = 0 (no initial
    point, every row live)."""
    extra = dict(pt_init=c["init"], status_in=c["live"]) if flow else {}
    return fn(c["ref"], c["cur"], c["pts"], c["p"], cam=c["cam"], cap=c["cap"], n=c["n"], **extra, **kw)
