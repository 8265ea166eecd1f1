"""The case table of the compiled-reference pin, for both binaries (the tracker's part, oracle/_ref/ref_tracker, is the second
half of this file): what oracle/_ref/ref_patchmatch -- the reference's own
src/patch_match.cpp and src/utils.cpp, compiled unchanged against the stand-ins of oracle/ref_shim -- is run on, and the
helpers that run it.  tests/test_reference_build_cpu.py holds the oracle to the binary on these cases,
tests/golden/make_ref_shim.py writes the binary's outputs to tests/golden/ref_shim/<case>.npz, and
tests/test_reference_build_gpu.py holds the HIP path to those files.

Small, seeded and deterministic (synth.SplitMix64).  Every case carries rows pinned to the borders -- (0, 0), (W-1, H-1),
(W-0.5, H-0.5), (W-0.25, H/2), (W/2, H-0.25), negative coordinates, points up to 3 px outside -- and about 5 % of rows with
status_in == 0.  A frame pair is an analytic texture and the same texture shifted by a known amount; the initial points are the
reference points plus that shift plus noise of sigma = 2 px.

Conditions (asserted in test_reference_build_cpu.py from the REFERENCE's outputs): on every frame with image content the
reference ends at least half of the rows with status 1 and at least one row with status 0.

EXCLUDED names, per case, the rows left out of a comparison because the reference reads memory there that the stand-in cannot
make defined -- each with its reason, never more than 5 % of a case.  It is empty: with two zero rows, 16 zero bytes and zero
row padding behind every image of the stand-in, every tap of the member sampler and of the free sampler (x == cols: the next
row's first pixel on a continuous image, as in the oracle; y == rows: a zero row, the oracle's 0) is defined."""
import dataclasses
import math
import os
import struct
import subprocess
import sys

import numpy as np

from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("PAGK_REFERENCE", "/root/reference")
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "ref_patchmatch")
REF_BIN_SAN = os.path.join(ROOT, "oracle", "_ref", "ref_patchmatch_san")
FIXTURE_DIR = os.path.join(ROOT, "tests", "golden", "ref_shim")
OUTPUTS = ("status", "pt_un", "pt_dist", "pix_err", "dist_pred", "ncc")
MAX_EXCLUDED_SHARE = 0.05
SHIFT = (1.37, -0.83)       # the true motion between the two frames, px
NOISE_SIGMA = 2.0           # of the initial points around reference + shift, px

sys.path.insert(0, os.path.join(ROOT, "tools", "ref_dump"))
import export_cases   # noqa: E402  (the kit's writer and reader of the binary's file formats)
import import_ref     # noqa: E402


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    width: int
    height: int
    n: int
    half_patch: int
    iterations: int
    pyramids: int
    what: str
    has_gyro: bool = True
    illumination: bool = True
    affine: bool = True
    penalty: bool = False
    ncc: bool = False
    dist: tuple = (0.0, 0.0, 0.0, 0.0)   # k1 k2 p1 p2 [k3]: five entries make mDistCoef.total() == 5
    step: int = 0                        # bytes per image row; 0 = continuous
    content: str = "texture"             # "gray": both frames constant 128
    init: str = "shifted"                # "equal": pt_init == pt_ref in every third row (such a row ends with status 0)
    committed: bool = True               # False: too large for a fixture, CPU only
    seed: int = 0


def _flag_cases():
    out = []
    for k, (a, i, p) in enumerate([(a, i, p) for a in (0, 1) for i in (0, 1) for p in (0, 1)]):
        # all flags off (the gyro initial too), then on; NCC on the all-on row and, without the warp, on a0_i1_p0
        out.append(Case(f"flags_a{a}_i{i}_p{p}", 160, 120, 256, 5, 10, 3, "a flag pattern of tests/golden/flags_* with rows at the borders",
                        has_gyro=(a, i, p) != (0, 0, 0), affine=bool(a), illumination=bool(i), penalty=bool(p),
                        ncc=(a, i, p) in ((1, 1, 1), (0, 1, 0)),
                        seed=0x5E510000 + k))
    return out


CASES = tuple(_flag_cases()) + (
    Case("odd_161x121", 161, 121, 256, 5, 10, 3, "odd parents; penalty and NCC on", penalty=True, ncc=True,
         dist=synth.D435I.dist, seed=0x5E510010),
    Case("odd_33x31_L5", 33, 31, 64, 5, 10, 5, "every parent odd, 2x1 top", seed=0x5E510011),
    Case("square_64_L7", 64, 64, 64, 10, 30, 7, "1x1 top; penalty; no affine", penalty=True, affine=False, seed=0x5E510012),
    Case("small_40x24_L4", 40, 24, 64, 7, 5, 4, "levels smaller than the patch", seed=0x5E510013),
    Case("h1_nogyro_ncc", 97, 81, 128, 1, 10, 4, "no gyro initial, NCC", has_gyro=False, ncc=True, seed=0x5E510014),
    Case("h15_noillum_k1", 97, 81, 128, 15, 30, 2, "no illumination, k1 = -0.2", illumination=False,
         dist=(-0.2, 0.0, 0.0, 0.0), seed=0x5E510015),
    Case("deep_256x192_L8", 256, 192, 200, 2, 1, 8, "PAGK_MAX_PYRAMIDS levels, one iteration", seed=0x5E510016),
    Case("step_176", 160, 120, 128, 5, 10, 3, "padded rows: row step 176", step=176, ncc=True, dist=synth.D435I.dist,
         seed=0x5E510017),
    Case("dist5_k3", 160, 120, 128, 5, 10, 3, "five distortion coefficients with k3 != 0",
         dist=(-0.28, 0.07, 0.0002, -0.0003, 0.05), seed=0x5E510018),
    Case("constant_gray", 160, 120, 64, 5, 10, 3, "constant gray: every H singular, the NaN-update exit", content="gray",
         seed=0x5E510019),
    Case("penalty_d0", 160, 120, 64, 5, 10, 3, "penalty with pt_init == pt_ref: d == 0, 0/0 in the Jacobian", penalty=True,
         init="equal", seed=0x5E51001A),
    Case("cfg1_752x480", 752, 480, 1000, 10, 30, 3, "config-1 workload of synth.py; the sensitivity check", committed=False,
         seed=0x5EED0001),
)

# case name -> {row: reason}: rows left out of a comparison (module docstring).  Empty.
EXCLUDED = {}


def case(name):
    return next(c for c in CASES if c.name == name)


def committed_cases():
    return [c.name for c in CASES if c.committed]


def border_points(width, height):
    """Reference points on, across and up to 3 px outside every border."""
    w, h = float(width), float(height)
    return np.array([(0, 0), (w - 1, h - 1), (w - 0.5, h - 0.5), (w - 0.25, h / 2), (w / 2, h - 0.25), (-1.5, -0.75),
                     (-3, h / 2), (w / 2, -2.25), (w, h), (w + 3, h + 3), (w + 1.5, h / 3), (w / 3, h + 2), (0.25, h - 1),
                     (w - 1, 0.5)], np.float64)


def _normal(rng, n):
    u = rng.uniform(2 * n)   # Box-Muller
    return np.sqrt(-2.0 * np.log(1.0 - u[0::2])) * np.cos(2 * math.pi * u[1::2])


def _padded(img, step):
    if not step or step == img.shape[1]:
        return np.ascontiguousarray(img)
    buf = np.zeros((img.shape[0], step), np.uint8)   # padding bytes are defined as 0
    buf[:, :img.shape[1]] = img
    return buf[:, :img.shape[1]]


def camera_of(c):
    return dataclasses.replace(synth.generic_camera(c.width, c.height), dist=tuple(float(v) for v in c.dist))


def params_of(c, solver_variant=0):
    return capi.make_params(half_patch=c.half_patch, iterations=c.iterations, pyramids=c.pyramids, has_gyro=c.has_gyro,
                            illumination=c.illumination, affine=c.affine, penalty=c.penalty, ncc=c.ncc, camera=camera_of(c),
                            solver_variant=solver_variant)


def _stamp(c, rng, pt_ref, pt_init, status_in):
    """The rows every case has: the border points in front, a status_in == 0 row every 20 rows."""
    b = border_points(c.width, c.height)
    k = min(len(b), c.n // 2)
    pt_ref[:k] = b[:k]
    pt_init[:k] = b[:k] + np.array(SHIFT) + NOISE_SIGMA * np.c_[_normal(rng, k), _normal(rng, k)]
    if c.init == "equal":
        pt_init[0::3] = pt_ref[0::3]
    status_in[:] = 1
    status_in[17::20] = 0
    status_in[3] = 0   # ... one of them on a border row


def make_inputs(c):
    """-> dict(img_ref, img_cur, pt_ref, pt_init, affine, status_in); the images are views of `step`-wide rows."""
    if c.name == "cfg1_752x480":
        w = synth.config(1, seed=c.seed)
        rng = synth.SplitMix64(c.seed ^ 0xB0BDE5)
        pt_ref, pt_init, status_in = w.pt_ref.astype(np.float64), w.pt_init.astype(np.float64), w.status_in.copy()
        _stamp(c, rng, pt_ref, pt_init, status_in)
        return dict(img_ref=w.img_ref, img_cur=w.img_cur, pt_ref=pt_ref.astype(np.float32), pt_init=pt_init.astype(np.float32),
                    affine=w.affine, status_in=status_in)
    rng = synth.SplitMix64(c.seed)
    if c.content == "gray":
        img_ref = np.full((c.height, c.width), 128, np.uint8)
        img_cur = img_ref.copy()
    else:
        tex = synth.Texture(rng)
        yy, xx = np.mgrid[0:c.height, 0:c.width].astype(np.float64)
        img_ref = synth._to_u8(tex(xx, yy))
        img_cur = synth._to_u8(1.05 * tex(xx - SHIFT[0], yy - SHIFT[1]) + 4.0)
    u = rng.uniform(2 * c.n)
    pt_ref = np.c_[u[0::2] * (c.width - 1), u[1::2] * (c.height - 1)]   # anywhere in the frame, margins included
    pt_init = pt_ref + np.array(SHIFT) + NOISE_SIGMA * np.c_[_normal(rng, c.n), _normal(rng, c.n)]
    status_in = np.ones(c.n, np.uint8)
    _stamp(c, rng, pt_ref, pt_init, status_in)
    affine = np.array([1.0, 0.0, 0.0, 1.0]) + 0.03 * np.c_[_normal(rng, c.n), _normal(rng, c.n), _normal(rng, c.n), _normal(rng, c.n)]
    return dict(img_ref=_padded(img_ref, c.step), img_cur=_padded(img_cur, c.step), pt_ref=pt_ref.astype(np.float32),
                pt_init=pt_init.astype(np.float32), affine=np.ascontiguousarray(affine, np.float32), status_in=status_in)


def cfg_of(params):
    return [params.half_patch, params.iterations, params.pyramids, params.has_gyro_predict_initial, params.consider_illumination,
            params.consider_affine, params.regularization_penalty, params.calculate_ncc]


def camera_row(params):
    return [params.fx, params.fy, params.cx, params.cy] + [params.dist_coef[k] for k in range(5)]


def run_reference(params, inp, workdir, name="case", binary=REF_BIN):
    """The compiled reference on one case -> (its six outputs and pyramid levels, the finished process)."""
    fin, fout = os.path.join(str(workdir), name + ".in"), os.path.join(str(workdir), name + ".ref")
    export_cases.write_in(fin, inp["img_ref"], inp["img_cur"], cfg_of(params), camera_row(params), inp["pt_ref"], inp["pt_init"],
                          inp["affine"], inp["status_in"], n_dist_coef=params.n_dist_coef, step=inp["img_ref"].strides[0])
    if os.path.exists(fout):
        os.remove(fout)
    proc = subprocess.run([binary, fin, fout], capture_output=True, text=True)
    out = import_ref.read_ref(fout) if proc.returncode == 0 else None
    return out, proc


def differing_rows(got, ref, n, keys=OUTPUTS):
    """Rows in which any of the outputs differs in any bit (NaN equals NaN of the same payload class: array_equal's rule)."""
    bad = np.zeros(n, bool)
    for k in keys:
        a, b = np.asarray(got[k][:n]), np.asarray(ref[k][:n])
        same = (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else a == b
        bad |= ~(same.reshape(n, -1).all(axis=1))
    return np.flatnonzero(bad)


# ---- the free NCC overloads of src/utils.cpp ------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class NccCase:
    name: str
    width: int
    height: int
    half_patch: int
    use_affine: bool
    step: int = 0
    seed: int = 0


NCC_CASES = (
    NccCase("ncc_plain", 160, 120, 5, False, seed=0x5E510100),
    NccCase("ncc_warp", 160, 120, 5, True, seed=0x5E510101),
    NccCase("ncc_warp_step_176", 160, 120, 5, True, step=176, seed=0x5E510102),
    NccCase("ncc_plain_odd_h2", 97, 81, 2, False, seed=0x5E510103),
)


def ncc_case(name):
    return next(c for c in NCC_CASES if c.name == name)


def make_ncc_inputs(c):
    """Point pairs for NCC(half, ref, cur, pt_ref, pt_cur, warp): the border set -- integer coordinates whose patches reach
    column `cols` and row `rows` exactly (the free sampler's `>` clamp) among them -- and interior points."""
    rng = synth.SplitMix64(c.seed)
    tex = synth.Texture(rng)
    yy, xx = np.mgrid[0:c.height, 0:c.width].astype(np.float64)
    img_ref = synth._to_u8(tex(xx, yy))
    img_cur = synth._to_u8(1.05 * tex(xx - SHIFT[0], yy - SHIFT[1]) + 4.0)
    w, h, hp = float(c.width), float(c.height), float(c.half_patch)
    exact = np.array([(w - hp, h / 2), (w / 2, h - hp), (w - hp, h - hp), (hp - 0.5, hp - 0.5), (w - hp - 1, h - hp - 1),
                      (w - hp + 1, h - hp + 1)], np.float64)
    b = np.concatenate([exact, border_points(c.width, c.height)])
    n = 64
    u = rng.uniform(2 * n)
    pt_ref = np.c_[u[0::2] * (w - 1), u[1::2] * (h - 1)]
    pt_ref[:len(b)] = b
    pt_cur = pt_ref + np.array(SHIFT) + 0.5 * np.c_[_normal(rng, n), _normal(rng, n)]
    pt_cur[:len(exact)] = exact[::-1]   # ... and current points whose patches end on the edge exactly
    affine = np.array([1.0, 0.0, 0.0, 1.0]) + 0.03 * np.c_[_normal(rng, n), _normal(rng, n), _normal(rng, n), _normal(rng, n)]
    affine[:len(exact)] = (1.0, 0.0, 0.0, 1.0)   # an identity warp keeps those taps on the edge
    return dict(img_ref=_padded(img_ref, c.step), img_cur=_padded(img_cur, c.step), pt_ref=pt_ref.astype(np.float32),
                pt_cur=pt_cur.astype(np.float32), affine=np.ascontiguousarray(affine, np.float32))


def run_reference_ncc(c, inp, workdir, binary=REF_BIN):
    """The compiled reference's two free NCC overloads on one case -> (by_images, by_values, the finished process)."""
    fin, fout = os.path.join(str(workdir), c.name + ".ncc"), os.path.join(str(workdir), c.name + ".out")
    n = int(inp["pt_ref"].shape[0])
    with open(fin, "wb") as f:
        f.write(b"PAGKNC1\0")
        f.write(struct.pack("<6i", c.width, c.height, n, c.half_patch, inp["img_ref"].strides[0], int(c.use_affine)))
        f.write(np.ascontiguousarray(inp["img_ref"]).tobytes())
        f.write(np.ascontiguousarray(inp["img_cur"]).tobytes())
        for k in ("pt_ref", "pt_cur", "affine"):
            f.write(np.ascontiguousarray(inp[k], np.float32).tobytes())
    if os.path.exists(fout):
        os.remove(fout)
    proc = subprocess.run([binary, "--ncc", fin, fout], capture_output=True, text=True)
    if proc.returncode != 0:
        return None, None, proc
    raw = open(fout, "rb").read()
    assert raw[:8] == b"PAGKNCR1" and struct.unpack_from("<i", raw, 8)[0] == n
    return np.frombuffer(raw, np.float32, n, 12).copy(), np.frombuffer(raw, np.float32, n, 12 + 4 * n).copy(), proc


# ---- fixtures: tests/golden/ref_shim/<case>.npz ----------------------------------------------------------------------------
def load_fixture(name):
    """-> (params, inputs, the reference's outputs, built_with) of a PatchMatch case, the row step restored."""
    z = np.load(os.path.join(FIXTURE_DIR, name + ".npz"), allow_pickle=False)
    cfg, cam = [int(v) for v in z["cfg"]], [float(v) for v in z["camera"]]
    n_dist = int(z["n_dist_coef"])
    camera = synth.Camera(cam[0], cam[1], cam[2], cam[3], tuple(cam[4:4 + n_dist]))
    params = capi.make_params(half_patch=cfg[0], iterations=cfg[1], pyramids=cfg[2], has_gyro=bool(cfg[3]), illumination=bool(cfg[4]),
                              affine=bool(cfg[5]), penalty=bool(cfg[6]), ncc=bool(cfg[7]), camera=camera)
    step = int(z["row_step"])
    inp = dict(img_ref=_padded(z["img_ref"], step), img_cur=_padded(z["img_cur"], step), pt_ref=z["pt_ref"], pt_init=z["pt_init"],
               affine=z["affine"], status_in=z["status_in"])
    return params, inp, {k: z["out_" + k] for k in OUTPUTS}, str(z["built_with"])


def load_ncc_fixture(name):
    z = np.load(os.path.join(FIXTURE_DIR, name + ".npz"), allow_pickle=False)
    step = int(z["row_step"])
    inp = dict(img_ref=_padded(z["img_ref"], step), img_cur=_padded(z["img_cur"], step), pt_ref=z["pt_ref"], pt_cur=z["pt_cur"],
               affine=z["affine"])
    return inp, z["out_by_images"], z["out_by_values"], str(z["built_with"])


# ==== the tracker: oracle/_ref/ref_tracker, the reference's own src/gyro_aided_tracker.cpp compiled unchanged ================
# One row per statement of the reference that branches (the `what` of every row says which).  Four modes, as ref_tracker.cpp
# lists them; third-party algorithms (the RANSAC fits, Lucas-Kanade) are inputs of a case.  tests/test_reference_tracker_cpu.py
# holds the project's CPU side to the binary on this table, tests/golden/make_ref_shim.py writes the binary's outputs to
# tests/golden/ref_shim/tracker/<case>.npz, tests/test_reference_tracker_gpu.py holds the device entry points to those files.
TRK_BIN = os.path.join(ROOT, "oracle", "_ref", "ref_tracker")
TRK_BIN_SAN = os.path.join(ROOT, "oracle", "_ref", "ref_tracker_san")
TRK_FIXTURE_DIR = os.path.join(FIXTURE_DIR, "tracker")
TRK_MAX_EXCLUDED_SHARE = 0.10
_DTYPES = (np.uint8, np.int32, np.float32, np.float64)
T_REF, T_CUR = 100.0, 100.05
EXACT_CAMERA = (128.0, 128.0, 80.0, 60.0)   # K * K^-1 is the identity in f32: with a zero rotation a prediction IS its reference point
RBC_TILTED = synth.rodrigues(np.array([0.3, -0.2, 0.5])).astype(np.float32)


def write_arrays(path, arrays):
    """The array container ref_tracker reads and writes (oracle/ref_shim/ref_tracker.cpp)."""
    with open(path, "wb") as f:
        f.write(b"PAGKARR1" + struct.pack("<i", len(arrays)))
        for name, a in arrays.items():
            a = np.ascontiguousarray(a)
            code = next(k for k, t in enumerate(_DTYPES) if a.dtype == t)
            dims = list(a.shape) + [1] * (3 - a.ndim)
            f.write(name.encode().ljust(24, b"\0") + struct.pack("<5i", code, a.ndim, *dims) + a.tobytes())


def read_arrays(path):
    raw = open(path, "rb").read()
    assert raw[:8] == b"PAGKARR1"
    count, pos, out = struct.unpack_from("<i", raw, 8)[0], 12, {}
    for _ in range(count):
        name = raw[pos:pos + 24].rstrip(b"\0").decode()
        code, ndim, d0, d1, d2 = struct.unpack_from("<5i", raw, pos + 24)
        shape = (d0, d1, d2)[:ndim]
        size = int(np.prod(shape, dtype=np.int64)) * np.dtype(_DTYPES[code]).itemsize
        out[name] = np.frombuffer(raw, _DTYPES[code], int(np.prod(shape, dtype=np.int64)), pos + 44).reshape(shape).copy()
        pos += 44 + size
    assert pos == len(raw)
    return out


def run_tracker(mode, inputs, workdir, name, binary=TRK_BIN):
    """The compiled reference tracker on one case -> (its outputs or None, the finished process).  Its log files
    (trackFeatures.txt, timeCost.txt) go to a scratch directory under workdir, never into the tree."""
    fin, fout = os.path.join(str(workdir), name + ".trk"), os.path.join(str(workdir), name + ".out")
    scratch = os.path.join(str(workdir), name + ".scratch") + "/"
    write_arrays(fin, inputs)
    if os.path.exists(fout):
        os.remove(fout)
    proc = subprocess.run([binary, "--" + mode, fin, fout, scratch], capture_output=True, text=True)
    return (read_arrays(fout) if proc.returncode == 0 else None), proc


@dataclasses.dataclass(frozen=True)
class TrackerCase:
    name: str
    mode: str          # track | validate | search | klt
    what: str          # the statements of src/gyro_aided_tracker.cpp the row exists for
    make: str          # the builder below
    args: dict = dataclasses.field(default_factory=dict)
    branches: dict = dataclasses.field(default_factory=dict)   # branch counts seen in the compiled reference's outputs


def _window(kind, rng, rate=0.6):
    """Sample times and rates between T_REF and T_CUR.  `exact`: the first and last sample ON the frame times (tini = tend = 0)."""
    n = int(kind[1])
    lo, hi = (T_REF, T_CUR) if kind.endswith("exact") else (T_REF - 0.0013, T_CUR + 0.0021)
    t = np.linspace(lo, hi, n)
    w = ((rng.uniform(3 * n).reshape(n, 3) - 0.5) * 2 * rate).astype(np.float32)
    if "small" in kind:   # the step between samples 1 and 2 turns by d just below / just above 1e-4 (:579)
        d = 0.99e-4 if "below" in kind else 1.01e-4
        w[1] = w[2] = np.float32(d / (t[2] - t[1])) * np.array([0.6, 0.0, 0.8], np.float32)
    if kind.startswith("z"):
        w[:] = 0
    return t, w


def _frames(width, height, rng, content="texture"):
    if content == "gray":
        img = np.full((height, width), 128, np.uint8)
        return img, img.copy()
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    if content == "period8":   # both frames the same image of period 8 in x and y: patches 8 px apart are equal, NCC and all
        cell = (rng.uniform(64).reshape(8, 8) * 200 + 20).astype(np.uint8)
        img = cell[(yy.astype(int) % 8), (xx.astype(int) % 8)]
        return img, img.copy()
    tex = synth.Texture(rng)
    ref = synth._to_u8(tex(xx, yy))
    if content == "same":
        return ref, ref.copy()
    return ref, synth._to_u8(1.05 * tex(xx - SHIFT[0], yy - SHIFT[1]) + 4.0)


def _base(width, height, seed, keys_ref, keys_cur=None, *, type_=4, method=1, half=5, ncc=1, dist=(0.0, 0.0, 0.0, 0.0),
          camera=None, window="w5_offset", rbc=None, bias=(0.0, 0.0, 0.0), content="texture", rate=0.6):
    rng = synth.SplitMix64(seed)
    img_ref, img_cur = _frames(width, height, rng, content)
    cam = camera if camera is not None else (0.6 * width, 0.6 * width, width / 2.0 - 0.5, height / 2.0 - 0.5)
    t, w = _window(window, rng, rate)
    keys_ref = np.ascontiguousarray(keys_ref, np.float32).reshape(-1, 2)
    keys_cur = np.zeros((0, 2), np.float32) if keys_cur is None else np.ascontiguousarray(keys_cur, np.float32).reshape(-1, 2)
    return dict(img_ref=img_ref, img_cur=img_cur, cam=np.array(list(cam) + list(dist) + [0.0] * (5 - len(dist)), np.float32),
                cfg=np.array([len(dist), half, type_, method, ncc], np.int32), times=np.array([T_REF, T_CUR]), imu_t=t, imu_w=w,
                bias=np.array(bias, np.float32), rbc=np.ascontiguousarray(np.eye(3) if rbc is None else rbc, np.float32).reshape(9),
                keys_ref=keys_ref, keys_ref_un=keys_ref.copy(), keys_cur=keys_cur, keys_cur_un=keys_cur.copy())


def _spread(width, height, n, rng, margin=0.0):
    u = rng.uniform(2 * n)
    return np.c_[margin + u[0::2] * (width - 1 - 2 * margin), margin + u[1::2] * (height - 1 - 2 * margin)]


def make_track(width=160, height=120, n=64, seed=0, borders=True, **kw):
    """TrackFeatures(): features anywhere in the frame, the border set of the PatchMatch table in front."""
    rng = synth.SplitMix64(seed ^ 0x7AC)
    pts = _spread(width, height, n, rng)
    if borders:
        b = border_points(width, height)
        pts[:len(b)] = b
    return _base(width, height, seed, pts, **kw)


def make_track_exact(seed=0, **kw):
    """A zero rotation under EXACT_CAMERA and no distortion: the predicted and the distorted point equal the reference point,
    so the border tests of :131 and :134 see exactly 0, the last float below width / height, width / height and beyond."""
    w, h = 160.0, 120.0
    below_w, below_h = float(np.nextafter(np.float32(w), np.float32(0))), float(np.nextafter(np.float32(h), np.float32(0)))
    pts = [(0, 0), (0, 50), (50, 0), (below_w, 50), (50, below_h), (below_w, below_h), (w, 50), (50, h), (w, h), (-0.0, 30),
           (float(-np.finfo(np.float32).tiny), 30), (30, -0.25), (w + 1, 50), (50, h + 2), (80, 60), (159, 119), (159.5, 60), (80, 119.5)]
    return _base(160, 120, seed, np.array(pts, np.float64), camera=EXACT_CAMERA, window="z2_exact", **kw)


def make_validate(n=64, seed=0, scene="plane", active="all", h21="true", f21="true", noise=0.3, outliers=6, span=10.0):
    """GeometryValidation(): correspondences of a plane (a homography moves them) or of a sideways translation (the epipolar
    lines are the image rows; the disparities spread over `span` px, and h21 = "shift" is the translation by their middle); H21 and F21 -- what the RANSAC fits would return -- are the case's inputs."""
    rng = synth.SplitMix64(seed)
    p1 = _spread(160, 120, n, rng)
    H = np.array([[1.02, 0.01, 2.0], [-0.015, 0.99, -1.5], [1e-4, -5e-5, 1.0]])
    F = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])   # x2 = x1 + (d, 0): y2 == y1
    if scene == "plane":
        q = np.c_[p1, np.ones(n)] @ H.T
        p2 = q[:, :2] / q[:, 2:]
    else:
        p2 = p1 + np.c_[2.0 + span * rng.uniform(n), np.zeros(n)]
    p2 = p2 + noise * np.c_[_normal(rng, n), _normal(rng, n)]
    p2[:outliers] += 25.0 * (rng.uniform(2 * outliers).reshape(-1, 2) - 0.5)
    status = np.ones(n, np.uint8)
    if active != "all":       # `active` rows on, spread over the table with inactive rows between them (:434-440)
        status[:] = 0
        status[np.linspace(0, n - 1, int(active)).round().astype(int)] = 1
        assert int(status.sum()) == int(active)
    h_of = dict(true=H, identity=np.eye(3), shift=np.array([[1.0, 0, 2.0 + span / 2], [0, 1.0, 0], [0, 0, 1.0]]), far=np.array([[1.0, 0, 300.0], [0, 1.0, 300.0], [0, 0, 1.0]]),
                singular=np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 0.0]]), rank1=np.outer([1.0, 2.0, 0.5], [0.5, -1.0, 2.0]))
    f_of = dict(true=F, zero=np.zeros((3, 3)), far=np.array([[0.0, 0, 0], [0, 0, 0], [0, 0, 1.0]]) + 1e-9 * np.eye(3),
                tilted=np.array([[0.0, 0.0, 0.02], [0.0, 0.0, -1.0], [-0.02, 1.0, 0.0]]))
    inp = _base(160, 120, seed, p1, window="w2_exact")
    inp.update(status=status, pt_predict_un=p2.astype(np.float32), H21=np.ascontiguousarray(h_of[h21]).reshape(9),
               F21=np.ascontiguousarray(f_of[f21]).reshape(9))
    return inp


def make_search_lists(seed=0, ncc=1):
    """SearchByGyroPredict() under EXACT_CAMERA with a zero rotation (a prediction is its reference point) on a frame of period
    8 that both images share: detections 8 px from a query see the query's own patch, so NCC values tie exactly, and so do
    distances.  Lists of 0, 1, 2 and many neighbours; two and three queries that claim one detection (:993-1007); queries whose
    neighbours come only with level 2 (:921-925) next to lists found at level 1, which level 2 must leave alone (:793)."""
    q, d = [], []
    def add(query, dets):
        q.append(query), d.extend(dets)
    add((20, 20), [])                                            # no neighbour at either level
    add((60, 20), [(60, 20)])                                    # one neighbour, the query's own patch
    add((100, 20), [(100, 20), (104, 23)])                       # two
    add((140, 20), [(148, 20), (132, 20), (140, 28), (140, 12), (140, 20), (143, 22), (137, 19)])   # many; four tie in NCC and distance
    add((20, 60), [(35, 60)])                                    # level 2 only (|dx| = 15 > 10)
    add((60, 60), [(60, 60), (76, 60)])                          # found at level 1; (76, 60) is in reach of level 2 and must not join
    add((100, 60), [(108, 60)])                                  # claimed by this query and the next one: erased (:997-1007)
    add((116, 60), [])
    add((20, 100), [(28, 100)])                                  # claimed by three: the third finds the set entry and erases nothing
    add((36, 100), [])
    add((28, 92), [])
    add((80, 100), [(83, 101), (78, 97)])                        # two neighbours of other patches: the ratio and the low-NCC rules
    add((120, 100), [(123, 103)])                                # one neighbour of another patch: rejected unless NCC > TH_NCC_HIGH (:973)
    add((5, 117), [(5, 117), (2, 119)])                                # within half a patch of the border: the free sampler's `>` clamp
    add((157, 117), [(157, 117), (159, 119)])
    return _base(160, 120, seed, np.array(q, np.float64), np.array(d, np.float64), type_=1, camera=EXACT_CAMERA, window="z2_exact",
                 content="period8", ncc=ncc)


def make_search_texture(n=64, seed=0, ncc=1, type_=1, spacing=None, **kw):
    """SearchByGyroPredict() on a textured pair with a gyro window: detections scattered around the true motion of every
    feature, so NCC values and distances of every size meet the rules of MatchFeatures (:959-989).  With `spacing` the features
    lie on a grid wider than the level-1 radius with one detection each on the same image: every feature matches."""
    rng = synth.SplitMix64(seed ^ 0x5EA)
    if spacing:
        gx, gy = np.meshgrid(np.arange(6, 160 - 5, spacing), np.arange(6, 120 - 5, spacing))
        pts = np.c_[gx.ravel(), gy.ravel()][:n].astype(np.float64)
        det = pts.copy()
        det[-6:] += (15.0, 0.0)   # out of reach of level 1, in reach of level 2 -- which must not run (:921)
        return _base(160, 120, seed, pts, det, type_=type_, camera=EXACT_CAMERA, window="z2_exact", content="same", ncc=ncc, **kw)
    pts = _spread(160, 120, n, rng)
    pts[:8] = [(3, 3), (157, 4), (2, 116), (158, 117), (5, 60), (155, 60), (80, 4), (80, 116)]   # within half a patch of the border
    k = np.array([1, 2, 3, 1, 2, 0, 1, 5] * (n // 8 + 1))[:n]
    det = np.concatenate([pts[i] + np.array(SHIFT) + 6.0 * np.c_[_normal(rng, k[i]), _normal(rng, k[i])] for i in range(n) if k[i]])
    det[::5] = np.round(det[::5])
    return _base(160, 120, seed, pts, det, type_=type_, ncc=ncc, rate=0.15, **kw)


def make_klt(n=48, seed=0):
    """TrackFeatures() type 0 and SearchByOpencvKLT() with Lucas-Kanade's result as an input: errors on both sides of 12 and
    exactly 12 (>= at :372, < at :1048), status 0 rows, detections 0, 1, 2 and more within the radius of 4 px, distance ratios on
    both sides of 0.7, a detection two tracks claim (:1089), and disparities beyond 1.5 times the average (:1119)."""
    rng = synth.SplitMix64(seed ^ 0x417)
    pts = _spread(160, 120, n, rng, margin=6.0)
    lk = pts + np.array(SHIFT) + 0.4 * np.c_[_normal(rng, n), _normal(rng, n)]
    lk[5] = lk[4] + (0.5, 0.0)                # two tracks end next to each other: both claim the detection at lk[4]
    lk[40:44] += (14.0, 9.0)                  # large disparities
    status = np.ones(n, np.uint8)
    status[7::11] = 0
    err = (rng.uniform(n) * 11.0).astype(np.float32)
    err[3], err[9], err[13] = 12.0, 12.5, np.float32(np.nextafter(np.float32(12.0), np.float32(0)))
    k = np.array([1, 2, 1, 0, 1, 0, 3, 1] * (n // 8 + 1))[:n]
    det = [lk[i] + 0.8 * np.c_[_normal(rng, k[i]), _normal(rng, k[i])] for i in range(n) if k[i]]
    det += [lk[16:20] + (2.0, 0.0), lk[16:20] + (-2.5, 0.0), lk[20:24] + (0.0, 1.0), lk[20:24] + (0.0, -3.9), lk[24:26] + (4.0, 0.0),
            lk[26:28] + (2.0, 0.0), lk[26:28] + (-2.0, 0.0)]   # ratios 0.8, 0.26, distance exactly 4, equal distances
    inp = _base(160, 120, seed, pts, np.concatenate(det), type_=0, window="w3_offset", dist=synth.D435I.dist)
    lk32 = lk.astype(np.float32)
    inp.update(lk_pt=lk32, lk_status=status, lk_err=err, lk2_pt=lk32, lk2_status=status, lk2_err=err)
    return inp


TRACKER_CASES = (
    # ---- integration windows (:521-587) with the prediction (:118-256) and, for types 2-6, PatchMatch and Step 3 (:289-341)
    TrackerCase("track_t4_w5_offset", "track", "five samples off the frame times: first, middle and last branch of :530-555, tini and tend "
                "non-zero; tilted Rbc, bias; type 4", "make_track",
                dict(seed=0x7AC00001, type_=4, window="w5_offset", rbc=RBC_TILTED, bias=(0.01, -0.02, 0.005), dist=synth.D435I.dist)),
    TrackerCase("track_t1_exact_borders", "track", "type 1; predictions exactly on 0, the last float below width / height, on them "
                "and outside (:131, :134); two samples on the frame times: the i == 0 && i == n-1 branch, tini = tend = 0",
                "make_track_exact", dict(seed=0x7AC00002, type_=1)),
    TrackerCase("track_t1_m2_k1pos_h7", "track", "SINGLE_HOMOGRAPHY (:235-255); k1 = +0.3 pushes distorted points over the border "
                "where the undistorted one is inside (:134); three samples off the frame times: first and last branch only; half "
                "patch 7", "make_track", dict(seed=0x7AC00003, type_=1, method=2, half=7, window="w3_offset", dist=(0.3, 0.0, 0.0, 0.0))),
    TrackerCase("track_t2_w2_offset_odd", "track", "type 2 (no illumination, no affine); two samples off the frame times; 161 x 121",
                "make_track", dict(width=161, height=121, seed=0x7AC00004, type_=2, window="w2_offset", dist=synth.D435I.dist)),
    TrackerCase("track_t3_w3_exact_k3", "track", "type 3; three samples on the frame times; five distortion coefficients (:70)",
                "make_track", dict(seed=0x7AC00005, type_=3, window="w3_exact", dist=(-0.28, 0.07, 0.0002, -0.0003, 0.05), rbc=RBC_TILTED)),
    TrackerCase("track_t5_nogyro_odd", "track", "type 5: no prediction, the identity affine and copied points of :263-271; 97 x 81",
                "make_track", dict(width=97, height=81, seed=0x7AC00006, type_=5, window="w5_exact", dist=synth.D435I.dist)),
    TrackerCase("track_t6_small_below", "track", "type 6 (penalty); one step with d just below 1e-4: deltaR = I + W (:579-580)",
                "make_track", dict(seed=0x7AC00007, type_=6, window="w5_small_below_offset", bias=(0.002, 0.0, -0.001))),
    TrackerCase("track_t4_m2_small_above", "track", "type 4 with SINGLE_HOMOGRAPHY; the same step with d just above 1e-4 (:583)",
                "make_track", dict(seed=0x7AC00008, type_=4, method=2, window="w5_small_above_offset", bias=(0.002, 0.0, -0.001))),
    TrackerCase("track_t4_none_survive", "track", "constant frames: no feature survives PatchMatch, cnt == 0, the 0/0 average, the "
                "threshold falls back to the half patch (:305-308)", "make_track",
                dict(seed=0x7AC00009, type_=4, content="gray", n=32), dict(pm_survivors=0, kept=0)),
    TrackerCase("track_t4_h1_filters", "track", "half patch 1 under a rotation the images do not follow: rows fail the status, the pixel-"
                "error and the distance condition of :322", "make_track", dict(seed=0x7AC0000A, type_=4, half=1, rate=2.5, window="w5_offset"),
                dict(pm_survivors=51, fail_pix_err=1, fail_dist=22, kept=28)),
    # ---- geometry validation (:429-508, :589-768)
    TrackerCase("val_8_active", "validate", "8 active rows among 64: skipped, status untouched, returns 0 (:445)", "make_validate",
                dict(seed=0x7AC00101, active=8, outliers=0)),
    TrackerCase("val_9_active", "validate", "9 active rows among 64: runs; compaction and vIndeces (:434-440, :473-481)", "make_validate",
                dict(seed=0x7AC00102, active=9, outliers=0)),
    TrackerCase("val_select_h", "validate", "a plane with the true H21 and an F21 that fits nothing: RH > 0.45, H's inliers kept", "make_validate",
                dict(seed=0x7AC00103, scene="plane", f21="tilted", active=40), dict(model="H")),
    TrackerCase("val_select_f", "validate", "a sideways translation with the true F21 and the identity as H21: RH <= 0.45, F's inliers kept",
                "make_validate", dict(seed=0x7AC00104, scene="sideways", h21="identity"), dict(model="F")),
    TrackerCase("val_rh_above", "validate", "disparities within 3.4 px and the translation by their middle as H21: RH = 0.4525 > 0.45 (:463), "
                "H's inliers kept -- one row fewer than F's", "make_validate",
                dict(seed=0x7AC00105, scene="sideways", h21="shift", span=3.4), dict(model="H")),
    TrackerCase("val_rh_below", "validate", "the same scene with the disparities within 3.5 px: RH = 0.4498, F's inliers kept", "make_validate",
                dict(seed=0x7AC00105, scene="sideways", h21="shift", span=3.5), dict(model="F")),
    TrackerCase("val_both_zero", "validate", "no row within either threshold: both scores 0, RH = 0/0, F chosen, every row an outlier",
                "make_validate", dict(seed=0x7AC00107, h21="far", f21="far", n=32), dict(model="F")),
    TrackerCase("val_zero_f", "validate", "F21 = 0: 0/0 distances, NaN score, no row fails a NaN comparison (:731-739)", "make_validate",
                dict(seed=0x7AC00108, f21="zero", n=32)),
    TrackerCase("val_singular_h", "validate", "H21 with a zero last row: H12 = 0, 1/0 and 0 * inf in the transfer errors (:641-662)",
                "make_validate", dict(seed=0x7AC00109, h21="singular", n=32)),
    TrackerCase("val_rank1_h", "validate", "H21 of rank 1: the inverse's zero-determinant rule", "make_validate",
                dict(seed=0x7AC0010A, h21="rank1", n=32)),
    # ---- SearchByGyroPredict (:859-1009)
    TrackerCase("search_lists_ncc", "search", "lists of 0, 1, 2 and many neighbours with tied NCC values and distances: the two-stack "
                "order (:826-842); two and three claims of one detection; level 2 after under 100 matches", "make_search_lists",
                dict(seed=0x7AC00201, ncc=1)),
    TrackerCase("search_lists_dist", "search", "the same lists ordered and matched by distance (mbNCC false, :831-836, :977-989)",
                "make_search_lists", dict(seed=0x7AC00202, ncc=0)),
    TrackerCase("search_texture_ncc", "search", "every branch of the NCC rule (:961-974) on scattered detections; border patches", "make_search_texture",
                dict(seed=0x7AC00203, ncc=1, rbc=RBC_TILTED)),
    TrackerCase("search_texture_dist", "search", "every branch of the distance rule (:978-988)", "make_search_texture",
                dict(seed=0x7AC00204, ncc=0)),
    TrackerCase("search_t4_texture", "search", "type 4: the lists are searched around the PatchMatch result with the predicted affine",
                "make_search_texture", dict(seed=0x7AC00205, ncc=1, type_=4, n=48)),
    TrackerCase("search_128_matches", "search", "128 features, 122 matches at level 1: at least 100, level 2 does not run (:921)",
                "make_search_texture", dict(seed=0x7AC00206, n=128, spacing=11)),
    # ---- TrackFeatures type 0 and SearchByOpencvKLT (:353-380, :1017-1136)
    TrackerCase("klt_basic", "klt", "Lucas-Kanade's result as an input: the error filters, radiusMatch lists of 0, 1, 2 and more, the "
                "ratio test, a detection claimed twice, the disparity filter", "make_klt", dict(seed=0x7AC00301)),
)


def tracker_case(name):
    return next(c for c in TRACKER_CASES if c.name == name)


def make_tracker_inputs(c):
    return globals()[c.make](**c.args)


def load_tracker_fixture(name):
    """-> (inputs, the compiled reference's outputs) of tests/golden/ref_shim/tracker/<name>.npz"""
    z = np.load(os.path.join(TRK_FIXTURE_DIR, name + ".npz"), allow_pickle=False)
    return ({k[3:]: z[k] for k in z.files if k.startswith("in_")}, {k[4:]: z[k] for k in z.files if k.startswith("out_")})


# ==== the ORB extractor: oracle/_ref/ref_orb, the reference's own src/ORBextractor.cc compiled unchanged ======================
# One row per branch of ComputeKeyPointsOctTree, DistributeOctTree / DivideNode, the constructor, ComputePyramid, DetectFeatures'
# mask test, IC_Angle and computeOrbDescriptor (the `what` of every row says which), at the smallest size that reaches it.
# tests/test_reference_orb_cpu.py holds the restatements and numpy models to the binary on this table and asserts that every
# branch named is reached, tests/golden/make_ref_shim.py writes the binary's outputs to tests/golden/ref_shim/orb/<case>.npz,
# tests/test_reference_orb_gpu.py holds the device entry points to those files.  The sampling pattern is an input of a case
# (the tests' seeded patterns and corner_pattern()): the reference's own table is in no file of this repository.
ORB_BIN = os.path.join(ROOT, "oracle", "_ref", "ref_orb")
ORB_BIN_SAN = os.path.join(ROOT, "oracle", "_ref", "ref_orb_san")
ORB_FIXTURE_DIR = os.path.join(FIXTURE_DIR, "orb")


@dataclasses.dataclass(frozen=True)
class OrbCase:
    name: str
    what: str          # the statements of src/ORBextractor.cc the row exists for
    image: str         # a key of orb_image()
    n_features: int
    n_levels: int = 1
    scale: float = 1.2
    mode: str = "detect"       # detect: DetectFeatures(); extract: operator()
    pattern: str = ""          # extract: "seed<k>" (orb_ref_util.seeded_pattern(k)) or "corner" (corner_pattern())
    mask: str = ""             # detect: a key of orb_mask()
    ini: int = 20
    mn: int = 7
    committed: bool = True     # False: too large for a fixture, CPU only


def _planted(w, h, pixels, background=40):
    img = np.full((h, w), background, np.uint8)
    for x, y, v in pixels:
        img[y, x] = v
    return img


def _patch(w, h, seed):
    """A texture in the left half of a flat frame: level images that compress (a fixture's size)."""
    import detect_ref_util as du
    t = du.texture_image(synth, w, h, seed)
    t[:, w // 2:] = 90
    return t


def _mixed(w, h, seed):
    """A texture whose middle third has 0.3 of the contrast (cells whose first FAST pass is empty and whose second is not) and
    whose right third is flat (cells empty after both)."""
    import detect_ref_util as du
    t = du.texture_image(synth, w, h, seed).astype(np.float64)
    a, b = w // 3, 2 * w // 3
    t[:, a:b] = 127.5 + (t[:, a:b] - 127.5) * 0.3
    t[:, b:] = 90
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


# single bright pixels on a flat background: a keypoint each, score value - 41; (45, 30) lies on node 0's right edge of a
# 91 x 62 frame (x - 16 == int(hX) == 29 with hX = 29.5); (60, 25) and (61, 25) have equal scores and are neighbours: both
# dropped; no other pixel within 15 of (30, 40): its disc has m10 = m01 = 0
PLANTED_91x62 = ((45, 30, 200), (60, 25, 150), (61, 25, 150), (70, 40, 120), (74, 44, 120), (30, 40, 180), (24, 22, 90), (66, 19, 99))


def orb_image(name):
    import detect_ref_util as du
    import fast_ref_util as fu
    if name == "planted pixels":
        return fu.planted_pixels()[0]
    if name == "flat 255":
        return np.full((240, 320), 255, np.uint8)
    kind, _, rest = name.partition(" ")
    w, h = (int(v) for v in kind.split("x")) if "x" in kind and kind[0].isdigit() else (0, 0)
    if rest.startswith("noise"):
        return du.noise_image(w, h, int(rest[5:] or 3))
    if rest.startswith("texture"):
        return du.texture_image(synth, w, h, int(rest[7:] or 2))
    if rest.startswith("patch"):
        return _patch(w, h, int(rest[5:] or 7))
    if rest.startswith("mixed"):
        return _mixed(w, h, int(rest[5:] or 7))
    if rest == "planted":
        return _planted(w, h, PLANTED_91x62)
    if rest == "pixels":
        return fu.planted_pixels(w, h)[0]
    raise KeyError(name)


def orb_mask(name, w, h):
    import detect_ref_util as du
    if name == "holes":
        return du.holes_mask(w, h)
    if name == "right half":   # zero where x >= W / 2
        m = np.ones((h, w), np.uint8)
        m[:, w // 2:] = 0
        return m
    raise KeyError(name)


def orb_pattern(name):
    import orb_ref_util as ou
    return ou.corner_pattern() if name == "corner" else ou.seeded_pattern(int(name[4:]))


def make_orb_inputs(c, descending=False, border_a5=False, own_table=False):
    img = np.ascontiguousarray(orb_image(c.image))
    inp = dict(img=img, cfg=np.array([c.n_features, c.n_levels, c.ini, c.mn, int(c.mode == "extract"), int(descending), int(border_a5),
                                      int(own_table)], np.int32), scale=np.array([c.scale], np.float32))
    if c.mask:
        inp["mask"] = np.ascontiguousarray(orb_mask(c.mask, img.shape[1], img.shape[0]))
    if c.mode == "extract" and not own_table:
        inp["pattern"] = np.ascontiguousarray(orb_pattern(c.pattern), np.int32)
    return inp


def run_orb(inputs, workdir, name, binary=ORB_BIN):
    """The compiled reference extractor on one case -> (its outputs or None, the finished process)."""
    fin, fout = os.path.join(str(workdir), name + ".orb"), os.path.join(str(workdir), name + ".out")
    write_arrays(fin, inputs)
    if os.path.exists(fout):
        os.remove(fout)
    proc = subprocess.run([binary, fin, fout], capture_output=True, text=True)
    return (read_arrays(fout) if proc.returncode == 0 else None), proc


def orb_case(name):
    return next(c for c in ORB_CASES if c.name == name)


def load_orb_fixture(name):
    """-> (inputs, the compiled reference's outputs) of tests/golden/ref_shim/orb/<name>.npz"""
    z = np.load(os.path.join(ORB_FIXTURE_DIR, name + ".npz"), allow_pickle=False)
    inp, out = {k[3:]: z[k] for k in z.files if k.startswith("in_")}, {k[4:]: z[k] for k in z.files if k.startswith("out_")}
    out["level_0"] = inp["img"]   # ComputePyramid's level 0 is the image: stored once
    return inp, out


ORB_CASES = (
    # ---- the cells of ComputeKeyPointsOctTree (:797-852)
    OrbCase("one_cell_62x62", "one cell (:808-811); the inner loop entered (:697) and left mid-walk (:754); 22 nodes for N = 20", "62x62 noise3", 20),
    OrbCase("nini2_boundary_key", "nIni = 2 with hX = 29.5 (:567-569): a key at x = 29 = int(hX) falls to node 0 (:593); two neighbours of "
            "equal score, both dropped by cv::FAST; isolated pixels: m10 = m01 = 0 in IC_Angle; "
            " ends by size == prevSize (:693)", "91x62 planted", 30, mode="extract", pattern="seed31"),
    OrbCase("nini2_ties_91x62", "nIni = 2; nodes of equal size in the sort of :708; equal responses in a node: the first stays (:776)", "91x62 noise3", 30),
    OrbCase("round_2p5_107x62", "round() half away from zero (:567): 75 / 30 = 2.5 -> nIni = 3", "107x62 noise3", 30),
    OrbCase("round_0p5_62x92", "round() half away from zero (:567): 30 / 60 = 0.5 -> nIni = 1", "62x92 noise3", 30),
    OrbCase("column_skip_813x62", "26 columns of 31: the last starts at maxBorderX - 6 and is skipped (:827)", "813x62 texture2", 200),
    OrbCase("row_skip_468x903", "29 rows of 31: the last starts at maxBorderY - 3 and is skipped (:818); 468 wide keeps nIni at 1",
            "468x903 pixels", 300),
    OrbCase("fallback_152x92", "cells whose first pass is empty and whose second is not, and cells empty after both (:836-842)",
            "152x92 mixed7", 60),
    # ---- DistributeOctTree and DivideNode (:505-787)
    OrbCase("prev_size_planted", "every node ends with one key: size == prevSize below N (:693)", "planted pixels", 400),
    OrbCase("inner_320x240", "the inner loop (:700-761) with 53 sort ties, left mid-walk; 15 nodes whose best response is shared", "320x240 texture2", 100),
    OrbCase("n1_160x120", "N = 1: done after the first round by size >= N (:693)", "160x120 texture12", 1),
    OrbCase("flat_255", "no keypoint at all: every cell empty after both passes, an empty list", "flat 255", 100),
    # ---- the constructor (:434-470), ComputePyramid (:1207-1230), the packing and the mask (:1066-1205)
    OrbCase("levels8_240x224", "8 levels at 1.2, the last 67 x 63; odd parents in resize; half of the frame flat (the fixture's size)", "240x224 patch21", 300, 8, 1.2, "extract", "seed31"),
    OrbCase("levels2_1p5_corner", "2 levels at 1.5; corner_pattern(): taps reach 18", "160x120 texture12", 120, 2, 1.5, "extract", "corner"),
    OrbCase("quota_tie_1p4", "nDesiredFeaturesPerScale = 94.5: cvRound gives 94 (:466)", "120x100 noise3", 162, 2, 1.4, "extract", "seed7"),
    OrbCase("quota_zero_last", "quotas 1, 1, 0: the last level runs with N = 0 (:470, :693)", "120x100 noise3", 2, 3, 1.2),
    OrbCase("size_tie_75x75", "75 * (1 / 1.2f) = 62.5 in float: cvRound gives 62 (:1212); on level 1 keypoints 19 from every border; "
            "angles in every octant", "75x75 noise3", 1000, 2, 1.2, "extract", "seed31"),
    OrbCase("masked_levels4", "DetectFeatures with a mask: keypoints of levels >= 1 dropped at mask[int(y s), int(x s)] (:1199-1203)",
            "240x224 patch21", 300, 4, 1.2, mask="holes"),
    # ---- too large for a fixture: CPU only
    OrbCase("texture_640x480_n400", "280 cells, 201 sort ties", "640x480 texture7", 400, committed=False),
    OrbCase("texture_752x480_n1000", "nIni = 2 on 336 cells; 4 levels", "752x480 texture1", 1000, 4, 1.2, "extract", "seed31", committed=False),
)
