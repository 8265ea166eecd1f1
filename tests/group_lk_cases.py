"""The rigs of the Lucas-Kanade sequence group (pagk_sequence_group_create_lk): tests/test_sequence_group_lk_cpu.py runs the
CPU model over those whose raggedness the GPU tests rely on, tests/test_sequence_group_lk_gpu.py the library over all of them.
Nothing here needs a device.

A plain rig is a scene of tests/sequence_cases.py (hu.rotating_sequence through sequence_cases._rendered, the candidate lists
of sequence_cases.candidates) and, per camera, one of the feeds of tests/test_sequence_group_gpu.py ("full", "sparse",
"gray3", "shifted").  A sensor rig is a rig of tests/group_sensor_cases.py with the arm changed to "lk-gyro": its cameras,
maps, windows and Rbc are taken as they are.  The tracking parameters of the PatchMatch block (half patch 5, `levels` levels)
only size the frame slots here; Lucas-Kanade has its own half patch and max_level."""
from __future__ import annotations

import numpy as np

import fit_ref_util as ftu
import group_sensor_cases as gc
import lk_ref_util as lu
import sequence_cases as sc
import sequence_model as sm
import test_sequence_group_gpu as tg
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi

RIG = ("full", "sparse", "gray3")


def plain_rig(name, kinds, width, height, lk_half, max_level, cap, target, arm="lk-gyro", validate=1, nf=7, n_cand=200,
              cand_cap=None, levels=3, step=sc.FAST_STEP) -> dict:
    cam, imgs, rot9 = sc._rendered(nf, width, height, step)
    lists = sc.candidates(width, height, n_cand, nf)
    scene = dict(imgs=list(imgs), cands=lists, gray=np.full((height, width), 128, np.uint8))
    p = capi.make_params(half_patch=min(5, lk_half), iterations=10, pyramids=levels, has_gyro=True, camera=cam)
    cfg = dict(arm=arm, p=p, width=width, height=height, cap=cap, target_n=target, threshold=sc.RATIO * target, detector=0,
               validate=validate, sigma=1.0, fit=ftu.params(**sc.FIT), lk=lu.params(half_patch=lk_half, max_level=max_level))
    cams = [dict(kind=kind, feed=tg._feed(scene, kind, nf)) for kind in kinds]
    return dict(name=name, cfg=cfg, cameras=cams, rot9=list(rot9), nf=nf, k=len(kinds),
                cand_cap=n_cand if cand_cap is None else cand_cap, sensor=False)


def ragged(arm: str, validate: int) -> dict:
    """Row 1: 160 x 120, three cameras that differ in what they are fed."""
    return plain_rig(f"ragged-{arm}-{validate}", RIG, 160, 120, 5, 2, 70, 64, arm=arm, validate=validate)


def sensor_rig(detector: int, raw: int = 1) -> dict:
    """Row 5: rig A of tests/group_sensor_cases.py (raw 173 x 131 x 3 through maps of 161 x 121, every camera its own Rbc,
    camera 2 with a constant-gray frame 3) under the arm "lk-gyro"; detector 0 hands in the lists of the row "sensor".
    raw = 0: rig C's gray frames at 161 x 121 (the level-0 copy path of sensor members), two cameras."""
    rig = gc.rig_a() if raw else gc.rig_c()
    cfg = dict(rig["cfg"], arm="lk-gyro", detector=detector, lk=lu.params(half_patch=5))
    cams = [dict(c) for c in rig["cameras"]]
    if detector == 0:
        lists = sc.candidates(cfg["width"], cfg["height"], 200, gc.NF)
        for j, c in enumerate(cams):
            c["cands"] = [lists[(k + j) % gc.NF] for k in range(gc.NF)]
    return dict(rig, name=f"lk-sensor-{detector}-{raw}", cfg=cfg, cameras=cams, cand_cap=200 if detector == 0 else 0, sensor=True,
                nf=gc.NF)


def sequence_params(rig: dict) -> "capi.SequenceParams":
    cfg = rig["cfg"]
    return capi.sequence_params_default(track=cfg["p"], lk=capi.lk_params_default(**cfg["lk"]), fit=capi.fit_params_default(**sc.FIT),
                                        tracker=capi.SEQ_LK, lk_initial_flow=1 if cfg["arm"] == "lk-gyro" else 0,
                                        width=cfg["width"], height=cfg["height"], cap=cfg["cap"], target_n=cfg["target_n"],
                                        new_point_threshold=cfg["threshold"], detector=cfg["detector"], cand_cap=rig["cand_cap"],
                                        validate=cfg["validate"], sigma=1.0)


def model(refs, rig: dict, j: int) -> list:
    """The CPU model's frames of camera j."""
    if rig["sensor"]:
        return gc.model(refs, rig, j)
    feed = rig["cameras"][j]["feed"]
    return sm.run(refs, rig["cfg"], [f[0] for f in feed], rig["rot9"], [f[1] for f in feed])
