"""Helpers of the association tests: the plain-C restatement (tests/associate_ref.c) through ctypes, an independent numpy model
of the count-and-compact formulation of include/pagk.h ("Track-to-detection association"), seeded neighbour lists with heavy
collisions, and the hand-built keypoint sets of the KLT arm."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SRC = os.path.join(HERE, "associate_ref.c")
INFO_WORDS = 8
STATS_WORDS = 8
F = np.float32
DEFAULTS = dict(th_ncc_high=0.6, th_ncc_low=0.3, th_ratio=0.75, use_ncc=1, min_matches=100, klt_max_distance=4.0, klt_ratio=0.7,
                klt_disparity_factor=1.5)
MATCH_KEYS = ("query", "train", "dist", "ncc", "flows", "info", "k")
KLT_KEYS = ("query", "train", "dist", "disparity", "stats", "info", "k")


def build_ref(out_dir):
    so = os.path.join(str(out_dir), "associate_ref.so")
    subprocess.run(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so, REF_SRC,
                    "-lm"], check=True)
    lib = C.CDLL(so)
    vp, i32, f32, f64 = C.c_void_p, C.c_int32, C.c_float, C.c_double
    lib.assoc_ref_match.restype = C.c_int
    lib.assoc_ref_match.argtypes = [i32, i32, i32, vp, vp, vp, vp, i32, f32, f32, f32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.assoc_ref_klt.restype = C.c_int
    lib.assoc_ref_klt.argtypes = [i32, i32, i32, vp, vp, vp, vp, f32, f64, f64, vp, vp, vp, vp, vp, vp]
    return lib


def same_array(a, b) -> bool:
    """Equality on the bits (NaNs in the same places)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))


def differing(a: dict, b: dict, keys) -> list:
    return [k for k in keys if not same_array(a[k], b[k])]


# ---- MatchFeatures -------------------------------------------------------------------------------------------------------
def ref_match(lib, count, idx, dist, ncc, m, use_ncc=True, th=(0.6, 0.3, 0.75), keys_cur_un=None, pt_pred=None) -> dict:
    """The literal sequential restatement -> dict(query, train, dist, ncc (n rows, -1 / 0 beyond the count), flows, info, k)."""
    n, cap = idx.shape
    nn = max(n, 1)
    q, t = np.full(nn, 7, np.int32), np.full(nn, 7, np.int32)
    d, c = np.full(nn, 7, F), np.full(nn, 7, F)
    flows = np.full((nn, 2), 7, F)
    info = np.full(INFO_WORDS, 7, np.int32)
    with_flows = keys_cur_un is not None
    k = lib.assoc_ref_match(n, m, cap, count.ctypes.data, idx.ctypes.data, dist.ctypes.data, ncc.ctypes.data, int(use_ncc),
                            th[0], th[1], th[2], keys_cur_un.ctypes.data if with_flows else None,
                            pt_pred.ctypes.data if with_flows else None, q.ctypes.data, t.ctypes.data, d.ctypes.data,
                            c.ctypes.data, flows.ctypes.data if with_flows else None, info.ctypes.data)
    assert k >= 0
    if not with_flows:
        flows[:] = 0
    return dict(query=q[:n], train=t[:n], dist=d[:n], ncc=c[:n], flows=flows[:n], info=info, k=np.int32(k))


def model_match(count, idx, dist, ncc, m, use_ncc=True, th=(0.6, 0.3, 0.75), keys_cur_un=None, pt_pred=None) -> dict:
    """Count and compact, in numpy: a choice per feature, the claims per current keypoint, the features whose choice has
    exactly one claim in increasing index."""
    n, cap = idx.shape
    hi, lo, ratio = F(th[0]), F(th[1]), F(th[2])
    c = count.astype(np.int64)
    over = c > cap
    n0, d0 = ncc[:, 0], dist[:, 0]
    n1 = ncc[:, 1] if cap > 1 else np.zeros(n, F)
    d1 = dist[:, 1] if cap > 1 else np.zeros(n, F)
    with np.errstate(invalid="ignore", over="ignore"):
        if use_ncc:
            take = (n0 > hi) | ((c > 1) & ~(n0 > hi) & ~(n0 < lo) & (n1 < (n0 * ratio).astype(F)))
        else:
            take = (c == 1) | ((c > 1) & (d0 < (d1 * ratio).astype(F)))
    take &= (c > 0) & ~over
    t = idx[:, 0].astype(np.int64)
    bad = take & ((t < 0) | (t >= m))
    chosen = take & ~bad
    claims = np.bincount(t[chosen], minlength=max(m, 1))
    keep = chosen.copy()
    keep[chosen] = claims[t[chosen]] == 1
    rows = np.flatnonzero(keep)
    k = len(rows)
    q, tr = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    d, cc = np.zeros(n, F), np.zeros(n, F)
    q[:k], tr[:k], d[:k], cc[:k] = rows, t[rows], d0[rows], n0[rows]
    flows = np.zeros((n, 2), F)
    if keys_cur_un is not None:
        flows[rows] = keys_cur_un[t[rows]] - pt_pred[rows]
    info = np.array([chosen.sum(), over.sum(), bad.sum(), (claims > 1).sum(), k, 0, 0, 0], np.int32)
    return dict(query=q, train=tr, dist=d, ncc=cc, flows=flows, info=info, k=np.int32(k))


def random_lists(seed, n, m, cap, special=True, overlong=False, bad_index=False, empty=False):
    """Seeded neighbour lists whose choices collide heavily: count, idx, dist, ncc (n x cap).  `special`: NaN and +-inf
    scores and distances among them."""
    rng = np.random.default_rng(seed)
    count = rng.integers(0, cap + 1, n).astype(np.int32)
    idx = rng.integers(0, max(m, 1), (n, cap)).astype(np.int32)
    ncc = np.sort(rng.uniform(0.0, 1.0, (n, cap)).astype(F), axis=1)[:, ::-1].copy()
    ncc[rng.random(n) < 0.3, 0] = F(0.9)                      # clear winners
    dist = np.sort(rng.uniform(0.0, 20.0, (n, cap)).astype(F), axis=1)
    dist[rng.random(n) < 0.3, 0] = F(0.01)
    if special and n:
        for v in (np.nan, np.inf, -np.inf):
            r = rng.integers(0, n, max(n // 8, 1))
            ncc[r, rng.integers(0, cap, len(r))] = v
            r = rng.integers(0, n, max(n // 8, 1))
            dist[r, rng.integers(0, cap, len(r))] = v
    if overlong and n:
        count[rng.integers(0, n, max(n // 10, 1))] = cap + 1 + rng.integers(0, 5)
    if bad_index and n:
        r = rng.integers(0, n, max(n // 10, 1))
        idx[r, 0] = np.where(rng.random(len(r)) < 0.5, -1 - rng.integers(0, 3, len(r)), m + rng.integers(0, 3, len(r)))
    if empty:
        count[:] = 0
    return count, idx, dist, ncc


# ---- the KLT arm ---------------------------------------------------------------------------------------------------------
def ref_klt(lib, cap, n, status, pt_lk, pt_ref, keys_cur, max_distance=4.0, ratio=0.7, factor=1.5) -> dict:
    keys_cur = np.ascontiguousarray(keys_cur, F).reshape(-1, 2)
    m = keys_cur.shape[0]
    q, t = np.full(cap, 7, np.int32), np.full(cap, 7, np.int32)
    d, disp = np.full(cap, 7, F), np.full(cap, 7, np.float64)
    stats, info = np.full(STATS_WORDS, 7, np.float64), np.full(INFO_WORDS, 7, np.int32)
    st, pl, pr = np.ascontiguousarray(status, np.uint8), np.ascontiguousarray(pt_lk, F), np.ascontiguousarray(pt_ref, F)
    assert len(st) >= cap and pl.shape[0] >= cap and pr.shape[0] >= cap
    k = lib.assoc_ref_klt(cap, n, m, st.ctypes.data, pl.ctypes.data, pr.ctypes.data, keys_cur.ctypes.data if m else None,
                          max_distance, ratio, factor, q.ctypes.data, t.ctypes.data, d.ctypes.data, disp.ctypes.data,
                          stats.ctypes.data, info.ctypes.data)
    assert k >= 0
    return dict(query=q, train=t, dist=d, disparity=disp, stats=stats, info=info, k=np.int32(k))


def _dist(q, keys):
    """d of the definition for one query against every keypoint: f32, one rounding per operation."""
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = (q[0] - keys[:, 0]).astype(F), (q[1] - keys[:, 1]).astype(F)
        return np.sqrt(((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F)).astype(F)


def model_klt(cap, n, status, pt_lk, pt_ref, keys_cur, max_distance=4.0, ratio=0.7, factor=1.5) -> dict:
    """Top two per query, the minimum claiming index per keypoint, two compactions around a sequential f64 sum."""
    keys_cur = np.ascontiguousarray(keys_cur, F).reshape(-1, 2)
    m = keys_cur.shape[0]
    n = min(max(int(n), 0), cap)
    info = np.zeros(INFO_WORDS, np.int32)
    choice, d0s = np.full(cap, -1, np.int64), np.zeros(cap, F)
    for i in range(n):
        if not status[i]:
            continue
        info[0] += 1
        d = _dist(pt_lk[i], keys_cur) if m else np.zeros(0, F)
        with np.errstate(invalid="ignore"):
            near = np.flatnonzero(d <= F(max_distance))
        info[1 + min(len(near), 2)] += 1
        if len(near) == 0:
            continue
        order = near[np.argsort(d[near], kind="stable")]
        if len(near) > 1:
            with np.errstate(invalid="ignore", divide="ignore"):
                r = np.float64(F(d[order[0]]) / F(d[order[1]]))
            if not r < ratio:
                info[4] += 1
                continue
        choice[i], d0s[i] = order[0], d[order[0]]
    owner = np.full(max(m, 1), np.iinfo(np.int32).max, np.int64)
    has = np.flatnonzero(choice >= 0)
    np.minimum.at(owner, choice[has], has)
    win = has[owner[choice[has]] == has]
    info[5] = len(has) - len(win)
    t = choice[win]
    with np.errstate(invalid="ignore", over="ignore"):
        ex, ey = (pt_ref[win, 0] - keys_cur[t, 0]).astype(F), (pt_ref[win, 1] - keys_cur[t, 1]).astype(F)
        disp = np.sqrt(((ex * ex).astype(F) + (ey * ey).astype(F)).astype(F)).astype(F).astype(np.float64)

    def ordered(v):
        s, top = np.float64(0.0), np.float64(0.0)
        for x in v:
            s = s + x
            top = x if x > top else top
        return s, top
    with np.errstate(invalid="ignore", divide="ignore"):
        sum1, max1 = ordered(disp)
        avg1 = sum1 / np.float64(len(win))
        th = avg1 * np.float64(factor)
        keep = ~(disp > th)
        sum2, max2 = ordered(disp[keep])
        avg2 = sum2 / np.float64(keep.sum())
    k = int(keep.sum())
    q, tr = np.full(cap, -1, np.int32), np.full(cap, -1, np.int32)
    d, dd = np.zeros(cap, F), np.zeros(cap, np.float64)
    q[:k], tr[:k], d[:k], dd[:k] = win[keep], t[keep], d0s[win[keep]], disp[keep]
    info[6], info[7] = len(win) - k, k
    stats = np.array([avg1, avg2, max1, max2, th, sum1, sum2, 0.0], np.float64)
    return dict(query=q, train=tr, dist=d, disparity=dd, stats=stats, info=info, k=np.int32(k))


def place(q, target, sx=1, sy=1):
    """A keypoint t (f32 pair) whose distance from the query q, computed as the definition computes it, is exactly the f32
    `target`: the x offset is the largest representable one not beyond the target, the y offset is scanned in steps of one
    ulp of q.y until the rounded distance is the target."""
    q = np.asarray(q, F)
    target = F(target)
    if target == 0:
        return q.copy()
    tx = F(q[0] - F(sx) * target)
    for _ in range(64):                                             # walk back until |dx| <= target
        if abs(F(q[0] - tx)) <= target:
            break
        tx = np.nextafter(tx, q[0], dtype=F)
    dx = F(q[0] - tx)
    u = np.spacing(max(abs(q[1]), F(1.0))).astype(F)
    ks = np.arange(0, 200000, dtype=np.float64)
    ty = (np.float64(q[1]) - sy * ks * np.float64(u)).astype(F)
    dy = (q[1] - ty).astype(F)
    d = np.sqrt(((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F)).astype(F)
    hit = np.flatnonzero(d == target)
    assert len(hit), (q, target)
    t = np.array([tx, ty[hit[0]]], F)
    assert _dist(q, t[None])[0] == target
    return t


R_BELOW = np.nextafter(F(0.7), F(0), dtype=F) if np.float64(F(0.7)) >= 0.7 else F(0.7)    # the largest f32 below 0.7 ...
R_ABOVE = np.nextafter(R_BELOW, F(1), dtype=F)                                            # ... and the next one up
assert np.float64(R_BELOW) < 0.7 <= np.float64(R_ABOVE)

SCENARIOS = ("none", "at 4", "beyond 4", "inside 4", "equal pair", "two at 0", "ratio below", "ratio above", "three")


def isolated(pt_lk, status, n, gap=9.0):
    """Indices of live queries that lie more than `gap` pixels from every other live query, in index order."""
    live = [i for i in range(n) if status[i] and np.isfinite(pt_lk[i]).all()]
    out = []
    for i in live:
        d = [np.hypot(*(pt_lk[i].astype(np.float64) - pt_lk[j].astype(np.float64))) for j in live if j != i]
        if not d or min(d) > gap:
            out.append(i)
    return out


def cluster(pt_lk, status, n):
    """Three consecutive live queries within a pixel and a half of each other, and far from every other live query."""
    for i in range(n - 2):
        tri = (i, i + 1, i + 2)
        if all(status[j] for j in tri) and all(np.hypot(*(pt_lk[a].astype(np.float64) - pt_lk[b].astype(np.float64))) < 1.5
                                               for a in tri for b in tri):
            rest = [j for j in range(n) if status[j] and j not in tri and np.isfinite(pt_lk[j]).all()]
            if all(np.hypot(*(pt_lk[i].astype(np.float64) - pt_lk[j].astype(np.float64))) > 11 for j in rest):
                return tri
    return None


def branch_keypoints(pt_lk, status, pt_ref, n):
    """The hand-built set: one scenario of SCENARIOS per isolated live query, in order, and `three` on the cluster ->
    (keys_cur, {scenario: query index or triple}).  Scenarios for which no query is left are missing from the dict.  The
    keypoint at exactly 4 px lies on the far side of its query from the reference point: the largest disparity of the set."""
    iso, tri = isolated(pt_lk, status, n), cluster(pt_lk, status, n)
    keys, used = [], {}
    for name, i in zip(SCENARIOS[:-1], iso):
        q = pt_lk[i]
        used[name] = i
        if name == "at 4":
            keys.append(place(q, 4.0, -1 if q[0] >= pt_ref[i][0] else 1, 1))
        elif name == "beyond 4":
            keys.append(place(q, np.nextafter(F(4), F(5), dtype=F), -1, 1))
        elif name == "inside 4":
            keys.append(place(q, np.nextafter(F(4), F(0), dtype=F), 1, -1))
        elif name == "equal pair":
            keys += [place(q, 1.5, 1, 1), place(q, 1.5, -1, -1)]
        elif name == "two at 0":
            keys += [q.copy(), q.copy()]
        elif name in ("ratio below", "ratio above"):
            r = R_BELOW if name == "ratio below" else R_ABOVE
            keys += [place(q, 2.0, -1, 1), place(q, F(2) * r)]         # d0 / 2 is exact: the quotient is r
    if tri is not None:
        used["three"] = tri
        keys.append(pt_lk[tri[1]].copy())
    # a neighbour of nothing, so that the set is never empty
    keys.append(np.array([-100.0, -100.0], F))
    return np.array(keys, F).reshape(-1, 2), used


def klt_sets(pt_lk, status, pt_ref, n) -> dict:
    """Keypoint sets built from Lucas-Kanade's outputs: name -> keys_cur (m x 2)."""
    live = [i for i in range(n) if status[i] and np.isfinite(pt_lk[i]).all()]
    out = {"branches": branch_keypoints(pt_lk, status, pt_ref, n)[0]}
    out["exact"] = pt_lk[live].copy() if live else np.zeros((0, 2), F)        # every live query meets its own point
    out["empty"] = np.zeros((0, 2), F)
    iso = isolated(pt_lk, status, n)
    if len(iso) >= 2:   # two matches, the second keypoint 4 px further along its query's flow: all but one survive the filter
        a, b = iso[0], iso[1]
        flow = pt_lk[b].astype(np.float64) - pt_ref[b].astype(np.float64)
        sx = -1 if flow[0] >= 0 else 1                                         # t.x = q.x - sx * dx
        # (the first keypoint is its query's reference point where that is a neighbour: disparity 0)
        first = pt_ref[a] if _dist(pt_lk[a], pt_ref[a][None])[0] < F(3.9) else pt_lk[a]
        out["two"] = np.array([first, place(pt_lk[b], 4.0, sx, 1)], F)
    return out


def synthetic_queries():
    """Queries for the hand-built set with nothing left to chance: isolated points on a 20 px grid with fractional
    coordinates, a cluster of three, a dead row and a NaN row -> (status, pt_lk, pt_ref, n, cap)."""
    rng = np.random.default_rng(77)
    grid = np.array([(30 + 20 * (k % 4), 25 + 20 * (k // 4)) for k in range(8)], np.float64) + rng.uniform(0, 1, (8, 2))
    tri = np.array([(150.25, 40.5), (150.75, 40.5), (150.25, 41.0)])
    pt_lk = np.concatenate([grid[:3], [[np.nan, 5.0]], grid[3:], tri, [[200.0, 200.0]], [[0, 0]]]).astype(F)
    n, cap = len(pt_lk) - 1, len(pt_lk) + 2
    status = np.ones(cap, np.uint8)
    status[3] = 0            # the NaN row is dead, as Lucas-Kanade leaves it
    status[n - 1] = 0        # a dead row with a finite point
    status[n:] = 1           # rows at or beyond the count are not live whatever their status
    pl = np.zeros((cap, 2), F)
    pl[:len(pt_lk)] = pt_lk
    pr = (pl.astype(np.float64) - np.array([1.25, -0.5])).astype(F)
    return status, pl, pr, n, cap


KLT_CASE_NAMES = ("160x120 h5: cap 300, count 257", "160x120 h15: 961 pixels")


def klt_cases(synth) -> dict:
    """Two of lk_ref_util's small shapes with a device count well below the capacity (so that isolated queries exist) and
    three reference points moved next to each other: name -> dict(ref, cur, pts, p, cap, n)."""
    import lk_ref_util as lu
    shapes = lu.shapes(synth)
    out = {}
    for name, n in zip(KLT_CASE_NAMES, (40, 40)):
        c = dict(shapes[name])
        pts = c["pts"].copy()
        h, w = c["ref"].shape
        live = pts[:n].astype(np.float64)
        centre = np.array([w / 2, h / 2])
        # the point that is furthest from every other one among those well inside the frame becomes the cluster's first
        gaps = [min(np.hypot(*(live[i] - live[j])) for j in range(n) if j != i) if np.abs(live[i] - centre).max() < min(w, h) / 4
                else 0.0 for i in range(n - 2)]
        b = int(np.argmax(gaps))
        far = pts[b].astype(np.float64)
        pts[b + 1] = (far + (0.5, 0.0)).astype(F)
        pts[b + 2] = (far + (0.0, 0.5)).astype(F)
        c.update(pts=pts, n=n, cap=c["cap"] or len(pts))
        out[name] = c
    return out
