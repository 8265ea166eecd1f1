"""The case table of the compiled-reference pin: what oracle/_ref/ref_patchmatch -- the reference's own
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
