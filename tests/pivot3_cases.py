"""The 4th Cholesky pivot of the path's normal equations: a float64 restatement of the reference's LLT and solve
(oracle/pagk_oracle.c: llt4_inplace, llt4_solve_norm) that also says WHERE the factorisation stopped, and the systems
the pivot-3 tests share.  The restatement decides nothing about results -- those always come from the oracle -- it only
classifies a system as "pivot 3 rejected" or "every pivot accepted", so that a test can show both sides of the device's
branch ran (csrc/pagk_device.h: Pivot3Known)."""
import functools

import numpy as np

F = np.float64
ALT_LOWER_SEQ, ALT_UPPER_TREE, ALT_NORM_SEQ, ALT_LLT_RECIP, ALT_PIVOT_TREE = 1, 2, 4, 8, 32
ALL_SOLVER_BITS = 1 | 2 | 4 | 8 | 32
PATCH_SIZES = (289, 361, 441)   # (2h + 1)^2 for h = 8, 9, 10: the two-round bodies of the 4-wave kernel


def restate(H, b, alt=0):
    """-> x[4], norm, stopped_at (0..3: the pivot at which the LLT returned, 4: all accepted), sums (the amounts
    subtracted from H11, H22, H33 as far as the factorisation got).  One IEEE operation per line of the C."""
    M = [[F(H[r][c]) for c in range(4)] for r in range(4)]
    b = [F(v) for v in b]
    stopped, sums = 4, {}
    with np.errstate(all="ignore"):
        for k in range(4):
            x = M[k][k]
            if k > 0:
                s = M[k][0] * M[k][0]
                if k == 3 and (alt & ALT_PIVOT_TREE):
                    s = s + (M[k][1] * M[k][1] + M[k][2] * M[k][2])
                else:
                    for j in range(1, k):
                        s = s + M[k][j] * M[k][j]
                sums[k] = s
                x = x - s
            if x <= 0.0:
                stopped = k
                break
            x = np.sqrt(x)
            M[k][k] = x
            rx = F(1.0) / x
            for i in range(k + 1, 4):
                if k > 0:
                    s = M[i][0] * M[k][0]
                    for j in range(1, k):
                        s = s + M[i][j] * M[k][j]
                    M[i][k] = M[i][k] - s
                M[i][k] = M[i][k] * rx if (alt & ALT_LLT_RECIP) else M[i][k] / x
        r0, r1, r2, r3 = b
        r0 = r0 / M[0][0]
        r1 = r1 - M[1][0] * r0
        r1 = r1 / M[1][1]
        r2 = r2 - (M[2][0] * r0 + M[2][1] * r1)
        r2 = r2 / M[2][2]
        if alt & ALT_LOWER_SEQ:
            r3 = r3 - ((M[3][0] * r0 + M[3][1] * r1) + M[3][2] * r2)
        else:
            r3 = r3 - (M[3][0] * r0 + (M[3][1] * r1 + M[3][2] * r2))
        r3 = r3 / M[3][3]
        r3 = r3 / M[3][3]
        r2 = r2 - M[3][2] * r3
        r2 = r2 / M[2][2]
        r1 = r1 - (M[2][1] * r2 + M[3][1] * r3)
        r1 = r1 / M[1][1]
        if alt & ALT_UPPER_TREE:
            r0 = r0 - (M[1][0] * r1 + (M[2][0] * r2 + M[3][0] * r3))
        else:
            r0 = r0 - ((M[1][0] * r1 + M[2][0] * r2) + M[3][0] * r3)
        r0 = r0 / M[0][0]
        if alt & ALT_NORM_SEQ:
            nrm = np.sqrt(((r0 * r0 + r1 * r1) + r2 * r2) + r3 * r3)
        else:
            nrm = np.sqrt((r0 * r0 + r2 * r2) + (r1 * r1 + r3 * r3))
    return np.array([r0, r1, r2, r3]), nrm, stopped, sums


def classify(H, alt=0):
    """per system: the pivot at which the reference's LLT returned (4: none)"""
    zero = np.zeros(4)
    return np.array([restate(Hi, zero, alt)[2] for Hi in H])


@functools.lru_cache(maxsize=None)
def structured(P, n=4096, seed=0x9170):
    """Normal equations summed the way the kernels sum them: P pixels in order, each entry the ordered float64 sum of
    exact products of float32 (Ix, Iy, c, 1), c constant over the patch -- column 3 is column 2 / c, H is singular and
    the 4th pivot is what rounding left of zero."""
    rng = np.random.default_rng(seed + P)
    J = np.empty((n, P, 4))
    J[:, :, 0] = rng.normal(0, 8, (n, P)).astype(np.float32)
    J[:, :, 1] = rng.normal(0, 8, (n, P)).astype(np.float32)
    J[:, :, 2] = (-rng.uniform(1, 255, n)).astype(np.float32)[:, None]   # c = -I1(pt), a bilinear sample of u8 pixels
    J[:, :, 3] = 1.0
    e = rng.normal(0, 5, (n, P)).astype(np.float32).astype(np.float64)
    H = np.empty((n, 4, 4))
    b = np.empty((n, 4))
    for r in range(4):
        for c in range(4):
            H[:, r, c] = np.cumsum(J[:, :, r] * J[:, :, c], axis=1)[:, -1]   # cumsum: strictly sequential
        b[:, r] = np.cumsum(-J[:, :, r] * e, axis=1)[:, -1]
    H.setflags(write=False)
    b.setflags(write=False)
    return H, b


def _diag(h33, a=0.0, h22=4.0, h11=4.0, h00=4.0):
    """diag(4, 4, 4, h33) with H30 = 2a: every root and quotient is exact, so x3 = h33 - a * a to the bit"""
    H = np.diag([h00, h11, h22, h33]).astype(np.float64)
    H[3, 0] = H[0, 3] = 2.0 * a
    return H, np.array([1.0, -2.0, 3.0, 5.0])


@functools.lru_cache(maxsize=None)
def edges():
    """Case (b): the edges of the branch.  -> names, H, b, expected pivot at which the reference stops (3: the 4th pivot
    is rejected, 4: accepted)."""
    tiny = np.ldexp(1.0, -400)
    out = [
        ("x3 = +0", *_diag(1.0, a=1.0), 3),
        ("x3 = -0", *_diag(-0.0), 3),
        ("x3 = smallest positive normal (out of range: redo)", *_diag(np.ldexp(1.0, -1022)), 4),
        ("x3 = 2^-400 (first value in range)", *_diag(tiny), 4),
        ("x3 = below 2^-400 (last value out of range)", *_diag(np.nextafter(tiny, 0.0)), 4),
        ("x3 = 2^401 (first value out of range above)", *_diag(np.ldexp(1.0, 401)), 4),
        ("x3 = below 2^401 (last value in range)", *_diag(np.nextafter(np.ldexp(1.0, 401), 0.0)), 4),
        ("x3 = NaN (not rejected: the root is taken)", *_diag(np.nan), 4),
        ("x3 = -3", *_diag(1.0, a=2.0), 3),
        ("x3 = -inf", *_diag(-np.inf), 3),
        ("x3 = +inf", *_diag(np.inf), 4),
        ("rejected with H33 out of range (2^-500)", *_diag(np.ldexp(1.0, -500), a=1.0), 3),
        ("x3 = inf - inf = NaN (accepted)", *_diag(np.inf, a=np.inf), 4),
    ]
    # ... and on the path's own systems, H33 moved onto and around the sum it is compared with
    Hs, bs = structured(441)
    for i in range(8):
        s3 = restate(Hs[i], bs[i])[3][3]
        for name, h33, stop in (("x3 = +0 (H33 = the sum)", s3, 3),
                                ("x3 = -1 ulp", np.nextafter(s3, 0.0), 3),
                                ("x3 = +1 ulp", np.nextafter(s3, np.inf), 4),
                                ("x3 = 1: comfortably accepted", s3 + 1.0, 4),
                                ("x3 = -1: comfortably rejected", s3 - 1.0, 3)):
            H = Hs[i].copy()
            H[3, 3] = h33
            out.append((f"structured {i}: {name}", H, bs[i].copy(), stop))
    names = [o[0] for o in out]
    return names, np.array([o[1] for o in out]), np.array([o[2] for o in out]), np.array([o[3] for o in out])


@functools.lru_cache(maxsize=None)
def early_pivots():
    """Case (c): pivot 0, 1 or 2 zero, negative, NaN or outside [2^-400, 2^401): the lean form must hand the solve to the
    plain divisions, whatever the 4th pivot then does.  -> names, H, b."""
    out = []
    Hs, bs = structured(441)
    for i in range(8, 16):
        H0, b0 = Hs[i], bs[i]
        sums = restate(H0, b0)[3]

        def put(name, r, c, v, scale=1.0):
            H = H0.copy() * scale
            H[r, c] = v
            out.append((f"structured {i}: {name}", H, b0.copy() * scale))
        put("H scaled by 2^410 (x0 too large)", 0, 0, H0[0, 0] * np.ldexp(1.0, 410), np.ldexp(1.0, 410))
        put("H scaled by 2^-420 (x0 too small)", 0, 0, H0[0, 0] * np.ldexp(1.0, -420), np.ldexp(1.0, -420))
        put("H00 = 0", 0, 0, 0.0)
        put("H00 = -1", 0, 0, -1.0)
        put("H00 = NaN", 0, 0, np.nan)
        put("H00 = inf", 0, 0, np.inf)
        put("x1 = +0", 1, 1, sums[1])
        put("x1 = -1", 1, 1, sums[1] - 1.0)
        put("x1 = NaN", 1, 1, np.nan)
        put("x2 = +0", 2, 2, sums[2])
        put("x2 = -1", 2, 2, sums[2] - 1.0)
        put("x2 = inf", 2, 2, np.inf)
    for name, kw in (("x0 = 2^-500", dict(h00=np.ldexp(1.0, -500))), ("x1 = 2^-500", dict(h11=np.ldexp(1.0, -500))),
                     ("x2 = 2^-500", dict(h22=np.ldexp(1.0, -500))), ("x2 = 2^-1074", dict(h22=5e-324)),
                     ("x1 = 2^401", dict(h11=np.ldexp(1.0, 401))), ("x2 = 2^500", dict(h22=np.ldexp(1.0, 500)))):
        for h33, a in ((1.0, 1.0), (2.0, 1.0), (1.0, 2.0)):   # three different 4th pivots behind it
            H, b = _diag(h33, a=a, **kw)
            out.append((f"diagonal: {name}, H33 = {h33}, H30 = {2 * a}", H, b))
    return [o[0] for o in out], np.array([o[1] for o in out]), np.array([o[2] for o in out])
