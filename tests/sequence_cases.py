"""The table of the frame loop's edge shapes (tests/test_sequence_model_cpu.py runs the CPU model over it,
tests/test_sequence_shapes_gpu.py the library): odd sizes, a cap that is no multiple of 64, cap == target_n, a deep pyramid
on a small frame, the smallest frame, more than one round of 2048 rows, both switches off, every detector under every arm,
the scene of the older loop tests, the sensor form.

Every row is hu.rotating_sequence(synth, NF, W, H, 0x5EED0A10, step); candidate lists come per frame from
np.random.default_rng(7).uniform((1, 1), (W - 2, H - 2), (n_cand, 2)) in float32; the fits use seed 0x5EED0F17 with 512 + 256
hypotheses; new_point_threshold = 0.8 * target_n; ten iterations.  cand_cap is the length of the lists (the longest list
the row hands in) unless the row says otherwise.  No size had to be moved to the nearest one the library accepts:
pagk_sequence_params_check (which covers pagk_lk_levels) passes every row as written, and the FAST detector takes 161 x 121.
The state words of every row and frame are printed by both test modules; the FAST rows keep 24 keys, skip the detector in
frame 1 (20 or 21 of 24 survive, above the threshold of 19.2) and run it in every later frame."""
from __future__ import annotations

import functools

import numpy as np

import fit_ref_util as ftu
import gyro_integrate_ref_util as gu
import handover_ref_util as hu
import lk_ref_util as lu
import sequence_model as sm
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, synth

SEED = 0x5EED0A10
FAST_STEP, MID_STEP, SLOW_STEP = (0.035, -0.045, 0.03), (0.01, -0.012, 0.01), (0.004, -0.005, 0.003)
FIT = dict(seed=0x5EED0F17, iters_H=512, iters_F=256)
RATIO = 0.8
T0, DT = 100.0, 1.0 / 30.0


def _row(width, height, h, levels, cap, target, arm="patchmatch", detector=0, n_cand=200, step=FAST_STEP, nf=7, gyro=1,
         validate=1, gray=None, cand_cap=None, superpoint=False, raw=None):
    return dict(width=width, height=height, half_patch=h, levels=levels, cap=cap, target_n=target, arm=arm, detector=detector,
                n_cand=n_cand, step=step, nf=nf, gyro=gyro, validate=validate, gray=gray,
                cand_cap=n_cand if cand_cap is None else cand_cap, superpoint=superpoint, raw=raw)


_SMALL = dict(width=160, height=120, h=5, levels=3, cap=70, target=64)
_ODD = dict(width=161, height=121, h=5, levels=3, cap=40, target=24)
TABLE = {
    "base": _row(**_SMALL),
    "nogyro-novalidate": _row(**_SMALL, gyro=0, validate=0, step=SLOW_STEP),
    "nogyro": _row(**_SMALL, gyro=0, step=SLOW_STEP),
    "novalidate": _row(**_SMALL, validate=0, step=SLOW_STEP),
    "odd-gray3": _row(161, 121, 5, 3, 70, 64, gray=3),
    "deep-small": _row(97, 81, 3, 4, 33, 32, n_cand=100, step=MID_STEP),
    "cap-is-target": _row(160, 120, 5, 2, 12, 12, step=MID_STEP),
    "smallest": _row(14, 14, 1, 1, 4, 4, n_cand=8),
    "two-rounds-pm": _row(320, 240, 5, 3, 2200, 2100, n_cand=3000, cand_cap=4096, nf=4),
    "two-rounds-lk-gyro": _row(320, 240, 5, 3, 2200, 2100, arm="lk-gyro", n_cand=3000, cand_cap=4096, nf=4),
    "lk": _row(**_SMALL, arm="lk"),
    "lk-gyro": _row(**_SMALL, arm="lk-gyro"),
    "lk-gyro-harris": _row(**_ODD, arm="lk-gyro", detector=1),
    "lk-harris": _row(**_ODD, arm="lk", detector=1),
    "pm-harris": _row(**_ODD, detector=1),
    "lk-gyro-fast": _row(**_ODD, arm="lk-gyro", detector=2),
    "pm-fast": _row(**_ODD, detector=2),
    "default-scene-pm": _row(640, 480, 5, 3, 448, 400, superpoint=True, cand_cap=1024, nf=9),
    "default-scene-lk": _row(640, 480, 5, 3, 448, 400, arm="lk", superpoint=True, cand_cap=1024, nf=9),
    "default-scene-lk-gyro": _row(640, 480, 5, 3, 448, 400, arm="lk-gyro", superpoint=True, cand_cap=1024, nf=9),
    # raw 173 x 131 x 3 through maps of 161 x 121: the raw frame is the scene at the raw size in three channels (shifted,
    # inverted), the maps a shift by (6.25, 5.5) raw pixels, so every rectified pixel interpolates
    "sensor": _row(**_ODD, arm="lk-gyro", raw=(173, 131, 3)),
}
ROWS = list(TABLE)
PLAIN = [name for name in ROWS if TABLE[name]["raw"] is None]


def _colour(img):
    return np.ascontiguousarray(np.stack([img, np.roll(img, 1, axis=1), 255 - np.roll(img, 2, axis=0)], axis=2))


def candidates(width, height, n_cand, nf):
    rng = np.random.default_rng(7)
    return [np.ascontiguousarray(rng.uniform((1, 1), (width - 2, height - 2), (n_cand, 2)).astype(np.float32)) for _ in range(nf)]


@functools.lru_cache(maxsize=None)
def _rendered(nf, width, height, step):
    cam, imgs, _, _, rot9, _ = hu.rotating_sequence(synth, nf, width, height, SEED, step)
    return cam, tuple(imgs), tuple(rot9)


def scene(name: str) -> dict:
    """The inputs of a row and the model's configuration (tests/sequence_model.py); nothing here needs a device."""
    r = TABLE[name]
    W, H, nf = r["width"], r["height"], r["nf"]
    sw, sh = (W, H) if r["raw"] is None else r["raw"][:2]
    cam, imgs, rot9 = _rendered(nf, sw, sh, r["step"])
    imgs = list(imgs)
    if r["gray"] is not None:
        imgs[r["gray"]] = np.full((sh, sw), 128, np.uint8)
    if r["superpoint"]:
        lists = hu.seq_candidates()
        cands = [lists[k % 4] for k in range(nf)]
    else:
        cands = candidates(W, H, r["n_cand"], nf)
    p = capi.make_params(half_patch=r["half_patch"], iterations=10, pyramids=r["levels"], has_gyro=bool(r["gyro"]), camera=cam)
    cfg = dict(arm=r["arm"], p=p, width=W, height=H, cap=r["cap"], target_n=r["target_n"], threshold=RATIO * r["target_n"],
               detector=r["detector"], validate=r["validate"], sigma=1.0, fit=ftu.params(**FIT),
               lk=lu.params(half_patch=r["half_patch"]))
    out = dict(name=name, row=r, cfg=cfg, cam=cam, imgs=imgs, rot9=rot9, cands=cands)
    if r["raw"] is not None:
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        times = [T0 + k * DT for k in range(nf)]
        out.update(raws=[_colour(im) for im in imgs], map_x=xx + np.float32(6.25), map_y=yy + np.float32(5.5), times=times,
                   windows=[None] + [dict(gu.constant_rate_window(r["step"], times[k - 1], times[k]), camera=(p.fx, p.fy, p.cx, p.cy))
                                     for k in range(1, nf)])
    return out


def sequence_params(sc: dict) -> "capi.SequenceParams":
    """The row as the library takes it (pagk_sequence_params; the detectors' defaults)."""
    r, cfg = sc["row"], sc["cfg"]
    tracker, flow = {"patchmatch": (capi.SEQ_PATCHMATCH, 0), "lk": (capi.SEQ_LK, 0), "lk-gyro": (capi.SEQ_LK, 1)}[r["arm"]]
    return capi.sequence_params_default(track=cfg["p"], lk=capi.lk_params_default(**cfg["lk"]), fit=capi.fit_params_default(**FIT),
                                        tracker=tracker, lk_initial_flow=flow, width=r["width"], height=r["height"], cap=r["cap"],
                                        target_n=r["target_n"], new_point_threshold=cfg["threshold"], detector=r["detector"],
                                        cand_cap=r["cand_cap"], validate=r["validate"], sigma=1.0)


def sensor_params(sc: dict) -> "capi.SequenceSensor":
    ws, hs, cn = sc["row"]["raw"]
    return capi.sequence_sensor_default(rectify=capi.rectify_params_default(channels=cn), raw=1, src_width=ws, src_height=hs)


def model(refs, sc: dict) -> list:
    """The CPU model's frames of a scene (refs: sequence_model.build_refs)."""
    if sc["row"]["raw"] is not None:
        return sm.run_sensor(refs, sc["cfg"], sc["raws"], sc["map_x"], sc["map_y"], sc["windows"], sc["times"], sc["cands"])
    return sm.run(refs, sc["cfg"], sc["imgs"], sc["rot9"], sc["cands"])


def words(frames) -> list:
    """[total, reach, survivors, added, rejected] per frame."""
    return [[int(v) for v in f["state"][:5]] for f in frames]
