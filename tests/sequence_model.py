"""The frame loop of include/pagk.h, section "The sequence the context owns", as a pure CPU composition of the restatements
the per-kernel tests already use as expected values: no call into libpagk_hip.so, no torch, no runtime.  One function per
arm (run_patchmatch, run_lk; the gyro-started Lucas-Kanade is run_lk(flow=True)), the sensor form around them (run_sensor),
and the two-pass compositions that define the detecting hand-overs (restated_handover_detect, restated_handover_fast).

A configuration is a plain dict (tests/sequence_cases.py builds it): p (a capi.Params, a ctypes struct), width, height, cap,
target_n, threshold, detector (0 the candidate lists, 1 Harris, 2 FAST), validate, sigma, fit (fit_ref_util.params) and, for
Lucas-Kanade, lk (lk_ref_util.params).  Every run returns one dict per frame: the hand-over's arrays keys, keys_un,
keys_normal, index_in_last, live (cap rows), state, info, and from frame 1 on "pair": what the pair handed over --
n (the live count the pair started from), status (after the validation), pt_predict, pt_predict_un, err (n rows each),
defined (the rows whose points the header defines: every row for Lucas-Kanade, Step 3's survivors for PatchMatch, whose
other entries are "left untouched"), entering (status-true rows in front of the validation) and cleared (by it)."""
from __future__ import annotations

import types

import numpy as np

import detect_ref_util as du
import fast_ref_util as fau
import fit_ref_util as ftu
import gyro_integrate_ref_util as gu
import handover_ref_util as hu
import lk_flow_ref_util as fu
import rectify_ref_util as ru
from oracle import pagk_oracle as orc

SET = ("keys", "keys_un", "keys_normal", "index_in_last", "live")
NONE = (np.zeros(0, np.uint8), np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32))


def build_refs(out_dir) -> types.SimpleNamespace:
    """Every restatement the loop is made of, compiled once into out_dir."""
    d = str(out_dir)
    return types.SimpleNamespace(handover=hu.build_ref(d), fit=ftu.build_ref(d), flow=fu.build_ref(d), detect=du.build_ref(d),
                                 fast=fau.build_ref(d), rectify=ru.build_ref(d), gyro=gu.build_ref(d))


# ---- the detecting hand-overs: two passes of the restated hand-over around the restated detector ---------------------------
def restated_handover_detect(href, dref, p, img, cap, target_n, thr, status, pp, ppu, state, **det):
    """The composition that defines the fused call, made of the two restatements."""
    h, w = img.shape
    cam = hu.camera_of(p)
    none = np.zeros((0, 2), np.float32)
    state = np.zeros(8, np.int32) if state is None else np.asarray(state, np.int32)
    first = hu.ref_handover(href, cam, w, h, cap, target_n, thr, status, pp, ppu, none, state=state)   # its mask, its survivors
    m, reach = int(first["state"][2]), int(state[1])
    n_new = target_n - m
    if (m < thr or not reach) and n_new > 0:
        d = du.ref_detect(dref, img, first["mask"], n_new, cap=cap, **det)
    else:
        d = dict(corners=np.zeros((cap, 2), np.float32), info=np.zeros(8, np.int32), n=0)
    out = hu.ref_handover(href, cam, w, h, cap, target_n, thr, status, pp, ppu, d["corners"][:d["n"]], state=state)
    out["info"] = d["info"]
    return out


def restated_handover_fast(href, fref, p, img, cap, target_n, thr, status, pp, ppu, state, n_features=0):
    """The composition that defines the fused call, made of the two restatements: the detector without a mask, then the
    hand-over on its list."""
    h, w = img.shape
    cam = hu.camera_of(p)
    none = np.zeros((0, 2), np.float32)
    state = np.zeros(8, np.int32) if state is None else np.asarray(state, np.int32)
    first = hu.ref_handover(href, cam, w, h, cap, target_n, thr, status, pp, ppu, none, state=state)   # its survivors
    m, reach = int(first["state"][2]), int(state[1])
    if (m < thr or not reach) and target_n - m > 0:
        d = fau.ref_detect(fref, img, None, n_features or target_n)
        cand, info = d["keypoints"][:d["n"]], d["info"]
    else:
        cand, info = none, np.zeros(8, np.int32)
    out = hu.ref_handover(href, cam, w, h, cap, target_n, thr, status, pp, ppu, cand, state=state)
    out["info"] = info
    return out


# ---- the stages ----------------------------------------------------------------------------------------------------------
def handover(refs, cfg, img, status, pp, ppu, cand, state):
    """The hand-over of the configured detector; the frame's mask is dropped (the sequence does not hand it out)."""
    a = (cfg["p"], img, cfg["cap"], cfg["target_n"], cfg["threshold"], status, pp, ppu, state)
    if cfg["detector"] == 1:
        out = restated_handover_detect(refs.handover, refs.detect, *a, **cfg.get("harris", {}))
    elif cfg["detector"] == 2:
        out = restated_handover_fast(refs.handover, refs.fast, *a)
    else:
        out = hu.ref_handover(refs.handover, hu.camera_of(cfg["p"]), cfg["width"], cfg["height"], cfg["cap"], cfg["target_n"],
                              cfg["threshold"], status, pp, ppu, cand, state=state)
        out["info"] = np.zeros(8, np.int32)
    out.pop("mask")
    return out


def validation(refs, cfg, keys_un, ppu, status):
    """pagk_geometry_validation_device as its header text defines it -> (status, cleared rows).  Nothing changes when at
    most 8 points take part or neither model could be fitted; a model that could not be fitted scores 0 with no inliers,
    the choice is pagk_geometry_select's, and the chosen model's outliers are cleared."""
    st = np.array(status, np.uint8, copy=True)
    if int(st.sum()) <= 8:
        return st, 0
    f = ftu.ref_fit(refs.fit, cfg["fit"], keys_un, ppu, st)
    has_H, has_F = f["H"]["status"] == 1, f["F"]["status"] == 1
    if has_H and has_F:
        _, out, _ = orc.geometry_validation(f["H21"], f["H12"], f["F21"], keys_un, ppu, st, cfg["sigma"])
    elif not has_H and not has_F:
        return st, 0
    else:
        rows = np.nonzero(st)[0]
        p1, p2 = np.ascontiguousarray(keys_un[rows]), np.ascontiguousarray(ppu[rows])
        none = np.zeros(len(rows), np.uint8)
        inl_H, sc_H = orc.check_homography(f["H21"], f["H12"], p1, p2, cfg["sigma"]) if has_H else (none, np.float32(0))
        inl_F, sc_F = orc.check_fundamental(f["F21"], p1, p2, cfg["sigma"]) if has_F else (none, np.float32(0))
        inl = inl_H if orc.geometry_select(sc_H, sc_F) else inl_F
        out = st.copy()
        out[rows[np.asarray(inl) == 0]] = 0
    return out, int(st.sum()) - int(out.sum())


def _rot(rot9):
    """(K R K^-1 with its unread third row zero, the third row of R) of the nine floats a step is handed."""
    r = np.asarray(rot9, np.float32).reshape(9)
    return np.concatenate([r[:6], np.zeros(3, np.float32)]).reshape(3, 3), r[6:9].copy()


def _loop(refs, cfg, imgs, cands, track):
    """The loop around `track(k, n, keys_un) -> (status, pt_predict, pt_predict_un, err, defined)` of the live rows."""
    lists = cands if cfg["detector"] == 0 else [None] * len(imgs)
    frames = [handover(refs, cfg, imgs[0], *NONE, lists[0], np.zeros(8, np.int32))]
    for k in range(1, len(imgs)):
        prev = frames[-1]
        n = int(prev["state"][0])
        keys_un = np.ascontiguousarray(prev["keys_un"][:n])
        if n == 0:      # nothing to track, nothing to validate: the hand-over runs on an all-zero status
            st1, pp, ppu = NONE
            err, defined = np.zeros(0, np.float32), np.zeros(0, bool)
        else:
            st1, pp, ppu, err, defined = track(k, n, keys_un)
        st2, cleared = validation(refs, cfg, keys_un, ppu, st1) if (cfg["validate"] and n) else (st1, 0)
        f = handover(refs, cfg, imgs[k], st2, pp, ppu, lists[k], prev["state"])
        f["pair"] = dict(n=n, status=st2, pt_predict=pp, pt_predict_un=ppu, err=err, defined=defined, entering=int(st1.sum()),
                         cleared=cleared)
        frames.append(f)
    return frames


def run_patchmatch(refs, cfg, imgs, rot9, cands):
    """The PatchMatch arm: the prediction (or, without it, pt_init = keys_un, every live row's status_in 1, the identity
    affine), orc.track, Step 3, the validation, the hand-over."""
    p = cfg["p"]

    def track(k, n, keys_un):
        if p.has_gyro_predict_initial:
            KRK, r3 = _rot(rot9[k - 1])
            pu, _, st, A = orc.gyro_predict(p, cfg["width"], cfg["height"], p.half_patch, KRK, r3, keys_un)
        else:
            pu, st, A = keys_un, np.ones(n, np.uint8), np.tile(np.float32([1, 0, 0, 1]), (n, 1))
        o = orc.track(p, imgs[k - 1], imgs[k], keys_un, np.ascontiguousarray(pu), np.ascontiguousarray(A), st)
        _, st1, pp, ppu = orc.post_filter(p.half_patch, o["status"][:n], o["pix_err"][:n], o["dist_pred"][:n], o["pt_dist"][:n],
                                          o["pt_un"][:n])
        return st1, pp, ppu, np.zeros(n, np.float32), st1.astype(bool)
    return _loop(refs, cfg, imgs, cands, track)


def run_lk(refs, cfg, imgs, rot9, cands, flow: bool):
    """Lucas-Kanade with flags 0, or (flow) started from the prediction, whose status is the flow form's status_in."""
    p = cfg["p"]
    camd = dict(fx=p.fx, fy=p.fy, cx=p.cx, cy=p.cy, dist=[p.dist_coef[i] for i in range(5)], n=p.n_dist_coef)

    def track(k, n, keys_un):
        extra = {}
        if flow:
            KRK, r3 = _rot(rot9[k - 1])
            pu, _, st, _ = orc.gyro_predict(p, cfg["width"], cfg["height"], p.half_patch, KRK, r3, keys_un)
            extra = dict(pt_init=pu, status_in=st)
        r = fu.ref_flow(refs.flow, imgs[k - 1], imgs[k], keys_un, cfg["lk"], cam=camd, **extra)
        return r["status"][:n], r["pt_out_dist"][:n], r["pt_out"][:n], r["err"][:n], np.ones(n, bool)
    return _loop(refs, cfg, imgs, cands, track)


def run(refs, cfg, imgs, rot9, cands):
    """The arm named by cfg["arm"]: "patchmatch", "lk" or "lk-gyro"."""
    if cfg["arm"] == "patchmatch":
        return run_patchmatch(refs, cfg, imgs, rot9, cands)
    return run_lk(refs, cfg, imgs, rot9, cands, flow=(cfg["arm"] == "lk-gyro"))


def run_sensor(refs, cfg, raws, map_x, map_y, windows, times, cands):
    """The sensor form around the model: restated rectified frames and the restated rot9 of every window go through the
    arm; "velocity" (cap x 2) per frame is the header's flow velocity, zero for the first frame."""
    imgs = [ru.ref_rectify(refs.rectify, map_x, map_y, r) for r in raws]
    rot9 = [gu.ref_integrate(refs.gyro, w)[1] for w in windows[1:]]
    frames = run(refs, cfg, imgs, rot9, cands)
    frames[0]["velocity"] = np.zeros((cfg["cap"], 2), np.float32)
    for k in range(1, len(frames)):
        f, last = frames[k], frames[k - 1]
        f["velocity"] = gu.model_flow_velocity(cfg["cap"], int(f["state"][0]), f["keys_normal"], last["keys_normal"],
                                               f["index_in_last"], times[k], times[k - 1])
    return frames
