"""The rigs of the sensor form of the sequence group (tests/test_sequence_group_sensor_cpu.py runs the CPU model over them,
tests/test_sequence_group_sensor_gpu.py the library).  Nothing here needs a device.

A rig is a list of cameras; a camera is what ONE sensor sequence is fed: its maps, its Rbc, its raw frames, its windows, its
time stamps and (detector 0) its candidate lists.  The cameras of a rig share pagk_sequence_params and everything of
pagk_sequence_sensor but Rbc.  All of it is built from the helpers of the older tables: hu.rotating_sequence (through
sequence_cases._rendered), gu.constant_rate_window, sequence_cases._colour, FIT and RATIO.

  rig A  FAST on raw colour frames: maps of 161 x 121 from raw 173 x 131 x 3, h = 5, three levels, cap 40, target 24,
         threshold 19.2, 7 frames (the sizes of the rows "pm-fast" and "sensor" of tests/sequence_cases.py).  Three cameras
         that differ in what a table record carries: camera 0 maps shifted by (6.25, 5.5), Rbc = I, the scene; camera 1 maps
         shifted by (3.5, 8.25), Rbc a rotation about z (its window's rates are those of Rbc * step, so that its Rcl and rot9
         are the scene's), the scene rolled by (3, 5) pixels -- in frame 1 it keeps 16 of 24 keys, below the threshold, and tops up
         while cameras 0 and 2 keep 23 and skip the detector; camera 2 as camera 0 with frame 3 a constant gray.
  rig B  lists on gray raw frames: 160 x 120 from a 1-channel 172 x 130 frame (the W % 4 == 0 store path of the rectify
         kernel, where A takes the tail path), detector 0 with 400 candidates, cap 300, target 280: two blocks of
         k_flow_velocity and of the key arrays.  Two cameras: full lists, and 40 candidates on alternate frames.
  rig C  rig A's configuration with raw = 0 (gray frames at 161 x 121, the IMU half alone) and flow_velocity = 0, k = 2."""
from __future__ import annotations

import numpy as np

import fit_ref_util as ftu
import gyro_integrate_ref_util as gu
import lk_ref_util as lu
import sequence_cases as sc
import sequence_model as sm
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi

NF = 7
T0, DT = sc.T0, sc.DT
STEP = sc.FAST_STEP
RBC_Z = gu.rodrigues64((0.0, 0.0, 0.3)).astype(np.float32)          # camera 1 of rig A: rolled about the optical axis
EYE = np.eye(3, dtype=np.float32)


def _shift_maps(width, height, dx, dy):
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float32)
    return xx + np.float32(dx), yy + np.float32(dy)


def _windows(p, rbc, times, step=STEP):
    """Per frame the window whose Rcl is the scene's step rotation under `rbc`: Rcl = Rbc^T dR^T Rbc = rodrigues(step) when
    dR^T = rodrigues(Rbc step), so the constant rate is that of the step turned into the body frame."""
    body = np.asarray(rbc, np.float64).reshape(3, 3) @ np.asarray(step, np.float64)
    out = [None]
    for k in range(1, len(times)):
        w = dict(gu.constant_rate_window(body, times[k - 1], times[k]), camera=(p.fx, p.fy, p.cx, p.cy))
        w["Rbc"] = np.ascontiguousarray(rbc, np.float32).reshape(3, 3)
        out.append(w)
    return out


def _camera(p, maps, rbc, frames, cands, t0=T0):
    times = [t0 + k * DT for k in range(len(frames))]
    return dict(maps=maps, rbc=np.ascontiguousarray(rbc, np.float32).reshape(3, 3), frames=frames, cands=cands, times=times,
                windows=_windows(p, rbc, times))


def _cfg(p, width, height, cap, target, detector, validate):
    return dict(arm="patchmatch", p=p, width=width, height=height, cap=cap, target_n=target, threshold=sc.RATIO * target,
                detector=detector, validate=validate, sigma=1.0, fit=ftu.params(**sc.FIT), lk=lu.params(half_patch=5))


def _rig(name, cfg, cameras, raw, flow_velocity=1):
    return dict(name=name, cfg=cfg, cameras=cameras, raw=raw, flow_velocity=flow_velocity, k=len(cameras))


def rig_a() -> dict:
    W, H, ws, hs = 161, 121, 173, 131
    cam, imgs, _ = sc._rendered(NF, ws, hs, STEP)
    p = capi.make_params(half_patch=5, iterations=10, pyramids=3, has_gyro=True, camera=cam)
    scene = [sc._colour(im) for im in imgs]
    rolled = [sc._colour(np.roll(im, (5, 3), axis=(0, 1))) for im in imgs]
    gray3 = list(scene)
    gray3[3] = np.full((hs, ws, 3), 128, np.uint8)
    none = [None] * NF
    cams = [_camera(p, _shift_maps(W, H, 6.25, 5.5), EYE, scene, none),
            _camera(p, _shift_maps(W, H, 3.5, 8.25), RBC_Z, rolled, none),
            _camera(p, _shift_maps(W, H, 6.25, 5.5), EYE, gray3, none)]
    return _rig("A", _cfg(p, W, H, 40, 24, 2, 1), cams, (ws, hs, 3))


def rig_b(switches: int) -> dict:
    """switches 0: validate = 0 and has_gyro_predict_initial = 0; 1: both on."""
    W, H, ws, hs, n_cand = 160, 120, 172, 130, 400
    step = STEP if switches else sc.SLOW_STEP                       # (without the prediction only a slow scene is tracked)
    cam, imgs, _ = sc._rendered(NF, ws, hs, step)
    p = capi.make_params(half_patch=5, iterations=10, pyramids=3, has_gyro=bool(switches), camera=cam)
    frames = [np.ascontiguousarray(im) for im in imgs]
    lists = sc.candidates(W, H, n_cand, NF)
    sparse = [lists[k][:40] if k % 2 == 0 else lists[k][:0] for k in range(NF)]
    maps = _shift_maps(W, H, 6.25, 5.5)
    cams = [_camera(p, maps, EYE, frames, lists), _camera(p, maps, EYE, frames, sparse)]
    for c in cams:
        c["windows"] = _windows(p, EYE, c["times"], step)
    rig = _rig("B%d" % switches, _cfg(p, W, H, 300, 280, 0, switches), cams, (ws, hs, 1))
    rig["cand_cap"] = n_cand
    return rig


def rig_c() -> dict:
    W, H = 161, 121
    cam, imgs, _ = sc._rendered(NF, W, H, STEP)
    p = capi.make_params(half_patch=5, iterations=10, pyramids=3, has_gyro=True, camera=cam)
    frames = [np.ascontiguousarray(im) for im in imgs]
    rolled = [np.ascontiguousarray(np.roll(im, (2, 3), axis=(0, 1))) for im in imgs]
    none = [None] * NF
    cams = [_camera(p, None, EYE, frames, none), _camera(p, None, RBC_Z, rolled, none)]
    return _rig("C", _cfg(p, W, H, 40, 24, 2, 1), cams, None, flow_velocity=0)


def rolled_camera(rig: dict, shift: int) -> dict:
    """Camera 0 of the rig with every frame rolled by `shift` columns: one more camera of the same configuration."""
    c = dict(rig["cameras"][0])
    c["frames"] = [np.ascontiguousarray(np.roll(f, shift, axis=1)) for f in c["frames"]]
    return c


def sequence_params(rig: dict) -> "capi.SequenceParams":
    cfg = rig["cfg"]
    return capi.sequence_params_default(track=cfg["p"], fit=capi.fit_params_default(**sc.FIT), tracker=capi.SEQ_PATCHMATCH,
                                        width=cfg["width"], height=cfg["height"], cap=cfg["cap"], target_n=cfg["target_n"],
                                        new_point_threshold=cfg["threshold"], detector=cfg["detector"],
                                        cand_cap=rig.get("cand_cap", 0 if cfg["detector"] else 1), validate=cfg["validate"],
                                        sigma=1.0)


def sensor_params(rig: dict, **overrides) -> "capi.SequenceSensor":
    """The sensor block the cameras share (Rbc is each camera's own: camera["rbc"])."""
    kw = dict(flow_velocity=rig["flow_velocity"])
    if rig["raw"] is not None:
        ws, hs, cn = rig["raw"]
        kw.update(rectify=capi.rectify_params_default(channels=cn), raw=1, src_width=ws, src_height=hs)
    kw.update(overrides)
    return capi.sequence_sensor_default(**kw)


def window(w: dict):
    """(capi.ImuWindow, keep) of a window of a camera."""
    return capi.imu_window(w["t_ref"], w["t_cur"], w["t"], w["w"], w["bias"])


def model(refs, rig: dict, j: int) -> list:
    """The CPU model's frames of camera j (tests/sequence_model.run_sensor; raw = 0: the frames are the rectified ones)."""
    c = rig["cameras"][j]
    if rig["raw"] is None:
        rot9 = [gu.ref_integrate(refs.gyro, w)[1] for w in c["windows"][1:]]
        return sm.run(refs, rig["cfg"], c["frames"], rot9, c["cands"])
    return sm.run_sensor(refs, rig["cfg"], c["frames"], c["maps"][0], c["maps"][1], c["windows"], c["times"], c["cands"])


def top_up_runs(frames, cfg) -> list:
    """Per frame k >= 1: does the top-up rule (src/frame.cpp:164-169) let the detector run?  From the state words alone:
    survivors below the threshold or the reach flag of the frame before unset, and room for new points."""
    out = [None]
    for k in range(1, len(frames)):
        m, reach = int(frames[k]["state"][2]), int(frames[k - 1]["state"][1])
        out.append((m < cfg["threshold"] or not reach) and cfg["target_n"] - m > 0)
    return out
