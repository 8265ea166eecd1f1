"""Test helpers of the FAST-cells-and-quadtree detector: the plain-C restatement (tests/fast_detect_ref.c) built and loaded
with ctypes, an independent numpy model written from the definition in include/pagk.h (a whole-image m map, vectorised
suppression per cell, a list-of-lists tree), and the test images with the counts they were chosen by."""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess

import numpy as np

import detect_ref_util as du

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SRC = os.path.join(HERE, "fast_detect_ref.c")
INFO_WORDS = 8
INI_TH, MIN_TH = 20, 7          # both front-ends of the reference
BORDER = 16


def build_ref(out_dir: str):
    so = os.path.join(str(out_dir), "fast_detect_ref.so")
    subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                    REF_SRC, "-lm"], check=True)
    lib = C.CDLL(so)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    lib.fdr_bounds.restype = i32
    lib.fdr_bounds.argtypes = [i32, i32, i32, vp, vp]
    lib.fdr_cells.restype = i32
    lib.fdr_cells.argtypes = [vp, i32, i32, i64, i32, i32, vp, vp, vp]
    lib.fdr_detect.restype = i32
    lib.fdr_detect.argtypes = [vp, i32, i32, i64, vp, i32, i32, i32, i32, vp, vp, vp, vp, i32]
    return lib


def ref_bounds(lib, w, h, n):
    """(raw_bound, out_bound), or None where the definition excludes the size."""
    a, b = C.c_int32(0), C.c_int32(0)
    if lib.fdr_bounds(w, h, n, C.addressof(a), C.addressof(b)):
        return None
    return a.value, b.value


def ref_cells(lib, img, ini=INI_TH, mn=MIN_TH) -> dict:
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    rb, _ = ref_bounds(lib, w, h, 1)
    xy, sc, cnt = np.zeros((rb, 2), np.float32), np.zeros(rb, np.int32), np.zeros(4, np.int32)
    assert lib.fdr_cells(img.ctypes.data, w, h, img.strides[0], ini, mn, xy.ctypes.data, sc.ctypes.data, cnt.ctypes.data) == 0
    n = int(cnt[0])
    return dict(xy=xy[:n].copy(), score=sc[:n].copy(), n=n, first_empty=int(cnt[1]), empty=int(cnt[2]), cells=int(cnt[3]))


def ref_detect(lib, img, mask, n_features, cap=None, *, ini=INI_TH, mn=MIN_TH, reverse_tie=False) -> dict:
    """The restatement -> dict(keypoints (cap x 2, zero beyond the count), response (cap), info, n, stats)."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    cap = ref_bounds(lib, w, h, n_features)[1] if cap is None else int(cap)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    kp, resp = np.zeros((cap, 2), np.float32), np.zeros(cap, np.float32)
    info, stats = np.zeros(INFO_WORDS, np.int32), np.zeros(4, np.int32)
    rc = lib.fdr_detect(img.ctypes.data, w, h, img.strides[0], None if m is None else m.ctypes.data, ini, mn, n_features, cap,
                        kp.ctypes.data, resp.ctypes.data, info.ctypes.data, stats.ctypes.data, int(reverse_tie))
    assert rc == 0
    return dict(keypoints=kp, response=resp, info=info, n=int(info[0]),
                stats=dict(ties=int(stats[0]), inner=int(stats[1]), n_ini=int(stats[2]), longest=int(stats[3])))


def same_fast(a: dict, b: dict) -> list:
    """Names of the arrays whose bytes differ."""
    return [k for k in ("keypoints", "response", "info") if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()]


# ---- the numpy model ---------------------------------------------------------------------------------------------------
def model_grid(w, h):
    """The cell grid of the definition -> dict, or None where the definition excludes the size."""
    if w < 62 or h < 62 or w > 32767 or h > 32767:
        return None
    f = np.float32
    mbx, mby = w - BORDER, h - BORDER
    width, height = f(mbx - BORDER), f(mby - BORDER)
    nc, nr = int(width / f(30)), int(height / f(30))
    if nc < 1 or nr < 1:
        return None
    wc, hc = int(math.ceil(width / f(nc))), int(math.ceil(height / f(nr)))
    r = width / height
    n_ini = int(math.floor(float(r) + 0.5))      # positive: half away from zero is half up
    if n_ini < 1:
        return None
    cells = []
    for i in range(nr):
        y0 = BORDER + i * hc
        if y0 >= mby - 3:
            continue
        for j in range(nc):
            x0 = BORDER + j * wc
            if x0 >= mbx - 6:
                continue
            cells.append((i, j, x0, y0, min(x0 + wc + 6, mbx), min(y0 + hc + 6, mby)))
    return dict(n_cols=nc, n_rows=nr, w_cell=wc, h_cell=hc, max_bx=mbx, max_by=mby, n_ini=n_ini, hx=width / f(n_ini),
                cells=cells)


def model_bounds(w, h, n):
    g = model_grid(w, h)
    if g is None or n < 1:
        return None
    return g["n_rows"] * g["n_cols"] * -(-g["w_cell"] // 2) * -(-g["h_cell"] // 2), max(n + 2, 4 * g["n_ini"])


_RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0),
         (-3, 1), (-2, 2), (-1, 3)]


def model_m(img) -> np.ndarray:
    """m(p) for every pixel whose ring lies inside the image (elsewhere a value no threshold accepts).  The ring of a pixel
    of a cell's detection region lies inside the cell, so the whole-image map serves every cell."""
    I = np.asarray(img, np.uint8).astype(np.int32)
    h, w = I.shape
    c = I[3:h - 3, 3:w - 3]
    d = np.stack([I[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - c for dx, dy in _RING])
    best = np.full(c.shape, -1000, np.int32)
    for s in range(16):
        arc = d[[(s + k) % 16 for k in range(9)]]
        best = np.maximum(best, np.maximum(arc.min(0), (-arc).min(0)))
    m = np.full((h, w), -1000, np.int32)
    m[3:h - 3, 3:w - 3] = best
    return m


def model_cells(img, ini=INI_TH, mn=MIN_TH) -> dict:
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    g = model_grid(w, h)
    M = model_m(img)
    keys, first_empty, empty, per_cell = [], 0, 0, []
    for (i, j, x0, y0, x1, y1) in g["cells"]:
        sub = M[y0:y1, x0:x1]
        ch, cw = sub.shape
        found = []
        for which, t in enumerate((ini, mn)):
            S = np.zeros((ch + 2, cw + 2), np.int32)        # a ring of zeros: what lies outside the cell counts as 0
            if ch > 6 and cw > 6:
                inner = sub[3:ch - 3, 3:cw - 3]
                S[4:ch - 2, 4:cw - 2] = np.where(inner > t, inner - 1, 0)
            c = S[1:-1, 1:-1]
            keep = np.ones(c.shape, bool)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dx or dy:
                        keep &= c > S[1 + dy:1 + dy + ch, 1 + dx:1 + dx + cw]
            ys, xs = np.nonzero(keep)
            if len(ys):
                found = [(float(x + j * g["w_cell"]), float(y + i * g["h_cell"]), int(c[y, x])) for y, x in zip(ys, xs)]
                break
            if which == 0:
                first_empty += 1
        else:
            empty += 1
        keys += found
        per_cell.append(len(found))
    xy = np.array([(k[0], k[1]) for k in keys], np.float32).reshape(-1, 2)
    return dict(xy=xy, score=np.array([k[2] for k in keys], np.int32), n=len(keys), first_empty=first_empty, empty=empty,
                cells=len(g["cells"]), grid=g, per_cell=per_cell)


def _split(node):
    """DivideNode on (x0, y0, x1, y1, keys) -> the four children n1 .. n4 (keys in their order)."""
    x0, y0, x1, y1, keys = node
    mx, my = x0 + -(-(x1 - x0) // 2), y0 + -(-(y1 - y0) // 2)
    ch = [(x0, y0, mx, my, []), (mx, y0, x1, my, []), (x0, my, mx, y1, []), (mx, my, x1, y1, [])]
    for k in keys:
        ch[(0 if k[0] < mx else 1) + (0 if k[1] < my else 2)][4].append(k)
    return ch


def model_detect(img, mask, n_features, cap=None, *, ini=INI_TH, mn=MIN_TH, reverse_tie=False) -> dict:
    """The definition as list operations: the list is a Python list (front = index 0) of [node, creation number]."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    N = int(n_features)
    cells = model_cells(img, ini, mn)
    g = cells["grid"]
    cap = model_bounds(w, h, N)[1] if cap is None else int(cap)
    f = np.float32
    hx = g["hx"]
    keys = [(float(x), float(y), int(s), idx) for idx, ((x, y), s) in enumerate(zip(cells["xy"], cells["score"]))]
    seq = 0
    L = []
    buckets = [[] for _ in range(g["n_ini"])]
    for k in keys:
        buckets[int(f(k[0]) / hx)].append(k)
    for i in range(g["n_ini"]):
        L.append([(int(hx * f(i)), 0, int(hx * f(i + 1)), g["max_by"] - BORDER, buckets[i]), seq])
        seq += 1
    L = [e for e in L if e[0][4]]
    passes = inner = ties = broke = best_ties = 0
    longest = len(L)
    done = False

    def children_of(entry):
        nonlocal seq
        out = []
        for c in _split(entry[0]):
            if c[4]:
                out.append([c, seq])
                seq += 1
        return out

    while not done:
        passes += 1
        prev = len(L)
        front, rest, cand = [], [], []
        for e in L:
            if len(e[0][4]) == 1:
                rest.append(e)
                continue
            for c in children_of(e):
                front.insert(0, c)
                if len(c[0][4]) > 1:
                    cand.append(c)
        L = front + rest
        longest = max(longest, len(L))
        if len(L) >= N or len(L) == prev:
            done = True
        elif len(L) + 3 * len(cand) > N:
            while not done:
                passes += 1
                inner += 1
                prev = len(L)
                sizes = [len(c[0][4]) for c in cand]
                ties += len(sizes) - len(set(sizes))
                order = sorted(cand, key=lambda c: (len(c[0][4]), -c[1] if reverse_tie else c[1]))
                cand = []
                for left, e in zip(range(len(order) - 1, -1, -1), reversed(order)):
                    for c in children_of(e):
                        L.insert(0, c)
                        if len(c[0][4]) > 1:
                            cand.append(c)
                    L.remove(e)
                    longest = max(longest, len(L))
                    if len(L) >= N:
                        broke += left > 0     # the walk ends with candidates left (src/ORBextractor.cc:754)
                        break
                if len(L) >= N or len(L) == prev:
                    done = True
    kp, resp = np.zeros((cap, 2), np.float32), np.zeros(cap, np.float32)
    info = np.zeros(INFO_WORDS, np.int32)
    n = 0
    for e in L:
        ks = e[0][4]
        b = ks[0]
        for k in ks[1:]:
            if k[2] > b[2]:
                b = k
        best_ties += sum(k[2] == b[2] for k in ks) > 1      # the first of equal responses stays (:776)
        x, y = b[0] + BORDER, b[1] + BORDER
        if mask is not None and mask[int(y), int(x)] == 0:
            continue
        kp[n] = (x, y)
        resp[n] = b[2]
        n += 1
    info[:6] = (n, cells["n"], cells["first_empty"], cells["empty"], len(L), passes)
    return dict(keypoints=kp, response=resp, info=info, n=n, stats=dict(ties=ties, inner=inner, n_ini=g["n_ini"], longest=longest),
                cells=cells, branches=dict(broke=broke, best_ties=best_ties))


# ---- images ------------------------------------------------------------------------------------------------------------
def mixed_contrast(synth) -> np.ndarray:
    """The 640 x 480 texture (seed 7): columns 213-425 at 0.3 contrast about 127.5, columns 426-639 flat 90."""
    t = du.texture_image(synth, 640, 480, 7).astype(np.float64)
    mix = t.copy()
    mix[:, 213:426] = 127.5 + (t[:, 213:426] - 127.5) * 0.3
    mix[:, 426:] = 90
    return np.clip(np.rint(mix), 0, 255).astype(np.uint8)


def planted_pixels(w: int = 320, h: int = 240):
    """Background 40, single pixels 100 + (k % 150) on a 17 x 13 grid from (10, 10) -> image, {(x, y): value}."""
    img = np.full((h, w), 40, np.uint8)
    pts, k = {}, 0
    for y in range(10, h - 8, 13):
        for x in range(10, w - 8, 17):
            img[y, x] = 100 + (k % 150)
            pts[(x, y)] = 100 + (k % 150)
            k += 1
    return img, pts


def cases(synth) -> dict:
    """name -> (image, mask, N, expected).  expected: the figures the inputs were chosen by (include only what is known):
    cells, raw, nodes, returned, first_empty, empty, inner, n_ini, passes."""
    tex7 = du.texture_image(synth, 640, 480, 7)
    mix = mixed_contrast(synth)
    planted, pts = planted_pixels()
    return {
        "62x62 noise": (du.noise_image(62, 62, 3), None, 20, dict(cells=1, raw=56, nodes=22)),
        "97x80 noise": (du.noise_image(97, 80, 3), None, 50, dict(cells=2, raw=254, nodes=52)),
        "91x62 noise": (du.noise_image(91, 62, 3), None, 30, dict(cells=1, w_cell=59)),
        "320x240 texture": (du.texture_image(synth, 320, 240, 2), None, 100, dict(cells=54, raw=391, nodes=100)),
        "texture N=400": (tex7, None, 400, dict(cells=280, raw=2268, nodes=402, inner=1, min_ties=201)),
        "texture N=1000": (tex7, None, 1000, dict(nodes=1001, inner=2)),
        "texture N=1": (tex7, None, 1, dict(nodes=4)),
        "texture with holes": (tex7, du.holes_mask(640, 480), 400, dict(nodes=402, returned=328)),
        "640x480 noise": (du.noise_image(640, 480), None, 1000, dict(raw=27652)),
        "mixed N=400": (mix, None, 400, dict(first_empty=182, empty=91, raw=1036, nodes=400)),
        "mixed N=150": (mix, None, 150, dict(nodes=150)),
        "752x480 texture": (du.texture_image(synth, 752, 480, 1), None, 1000, dict(n_ini=2, cells=336, first_empty=9)),
        "641x479 texture": (du.texture_image(synth, 641, 479, 9), du.holes_mask(641, 479), 700, dict(nodes=701)),
        "planted pixels": (planted, None, len(pts) + 50, dict()),
        "flat 255": (np.full((240, 320), 255, np.uint8), None, 100, dict(raw=0, nodes=0, returned=0)),
        "all-zero mask": (tex7, np.zeros((480, 640), np.uint8), 400, dict(returned=0, nodes=402)),
    }


CASE_NAMES = ["62x62 noise", "97x80 noise", "91x62 noise", "320x240 texture", "texture N=400", "texture N=1000", "texture N=1",
              "texture with holes", "640x480 noise", "mixed N=400", "mixed N=150", "752x480 texture", "641x479 texture",
              "planted pixels", "flat 255", "all-zero mask"]
BIG = ("1920x1080 texture", 20000, dict(cells=2074, raw=12412, passes=12))   # host form only


def big_image(synth):
    return du.texture_image(synth, 1920, 1080, 3)


def check_expected(name, exp, info, stats, cells=None, w_cell=None):
    """Assert the figures of the issue's table against a result (info words, stats of a restatement or the model)."""
    got = dict(raw=int(info[1]), first_empty=int(info[2]), empty=int(info[3]), nodes=int(info[4]), returned=int(info[0]),
               passes=int(info[5]))
    if stats is not None:
        got.update(inner=stats["inner"], n_ini=stats["n_ini"])
    if cells is not None:
        got["cells"] = cells
    if w_cell is not None:
        got["w_cell"] = w_cell
    for k, v in exp.items():
        if k == "min_ties":
            assert stats is None or stats["ties"] >= v, (name, "ties", stats["ties"])
        elif k in got:
            assert got[k] == v, (name, k, got[k], v)
