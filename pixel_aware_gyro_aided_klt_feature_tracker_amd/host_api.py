"""ctypes access to the C++ API shell (libpagk_tracker.so: the reference's GyroAidedTracker /
PatchMatch classes over the C ABI).  Used by the tests to drive TrackFeatures() end to end."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import capi

LIB_PATH = os.path.join(capi.PKG_DIR, "libpagk_tracker.so")
_lib = None


def load():
    global _lib
    if _lib is None:
        capi.load()  # libpagk_hip.so first (RTLD_GLOBAL), the shell links against it
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run __graft_entry__.build()")
        lib = C.CDLL(LIB_PATH)
        vp, i = C.c_void_p, C.c_int
        lib.pagk_tracker_track_features.restype = C.c_int
        lib.pagk_tracker_track_features.argtypes = [vp, vp, i, i, C.c_long, i, vp, vp, vp, i, i, i, i, vp, vp, i,
                                                    C.c_double, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp]
        if hasattr(lib, "pagk_tracker_track_features_ex"):   # (absent from an older shell loaded for an A/B run)
            lib.pagk_tracker_track_features_ex.restype = C.c_int
            lib.pagk_tracker_track_features_ex.argtypes = lib.pagk_tracker_track_features.argtypes + [vp, vp]
        lib.pagk_tracker_geometry_validation.restype = C.c_int
        lib.pagk_tracker_geometry_validation.argtypes = [i, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_float)]
        lib.pagk_tracker_geometry_validation_fit.restype = C.c_int
        lib.pagk_tracker_geometry_validation_fit.argtypes = [i, vp, vp, vp, C.c_ulonglong, C.POINTER(C.c_float)]
        lib.pagk_seq_load_keypoints.restype = C.c_int
        lib.pagk_seq_load_keypoints.argtypes = [C.c_char_p, vp, i]
        lib.pagk_seq_load_correspondences.restype = C.c_int
        lib.pagk_seq_load_correspondences.argtypes = [C.c_char_p, vp, vp, i, i]
        lib.pagk_seq_find_time.restype = C.c_int
        lib.pagk_seq_find_time.argtypes = [vp, i, C.c_double]
        lib.pagk_seq_parse_image_line.restype = C.c_int
        lib.pagk_seq_parse_image_line.argtypes = [C.c_char_p, C.POINTER(C.c_double)]
        lib.pagk_seq_load_imu.restype = C.c_int
        lib.pagk_seq_load_imu.argtypes = [C.c_char_p, vp, i]
        lib.pagk_seq_imu_windows.restype = C.c_int
        lib.pagk_seq_imu_windows.argtypes = [C.c_char_p, vp, i, vp, vp]
        lib.pagk_tracker_last_error.restype = C.c_char_p
        lib.pagk_tracker_release.restype = None
        _lib = lib
    return _lib


def track_features(img_ref, img_cur, keys_ref, K, dist, *, type=4, half_patch=5, iterations=10, pyramids=3,
                   Rcl=None, imu=None, t_ref=0.0, t_cur=0.0):
    """GyroAidedTracker(ctor #1) -> TrackFeatures() (reference Examples/Demo/RealSenseD435i.cpp:244-251).  type 0 (pyramidal
    Lucas-Kanade, src/gyro_aided_tracker.cpp:353-380) fills status, pt_predict_un, pt_predict, error (mvError) and
    flows_predict_un (mvFlowsPredictUn) and returns the number of kept features."""
    lib = load()
    n = int(keys_ref.shape[0])
    nn = max(n, 1)
    K = np.ascontiguousarray(K, np.float32)
    dist = np.ascontiguousarray(dist, np.float32)
    keys_ref = np.ascontiguousarray(keys_ref, np.float32)
    R = None if Rcl is None else np.ascontiguousarray(Rcl, np.float32)
    imu_a = None if imu is None else np.ascontiguousarray(imu, np.float64)
    out = dict(status=np.zeros(nn, np.uint8), pt_predict_un=np.zeros((nn, 2), np.float32),
               pt_predict=np.zeros((nn, 2), np.float32), status_pm=np.zeros(nn, np.uint8),
               pt_pm_un=np.zeros((nn, 2), np.float32), pix_err=np.zeros(nn, np.float64),
               dist_pred=np.zeros(nn, np.float64), affine=np.zeros((nn, 4), np.float32),
               error=np.zeros(nn, np.float32), flows_predict_un=np.zeros((nn, 2), np.float32))
    args = [img_ref.ctypes.data, img_cur.ctypes.data, img_ref.shape[1], img_ref.shape[0], img_ref.strides[0], n,
            keys_ref.ctypes.data, K.ctypes.data, dist.ctypes.data, type, half_patch, iterations, pyramids,
            None if R is None else R.ctypes.data, None if imu_a is None else imu_a.ctypes.data,
            0 if imu_a is None else int(imu_a.shape[0]), t_ref, t_cur,
            out["status"].ctypes.data, out["pt_predict_un"].ctypes.data, out["pt_predict"].ctypes.data,
            out["status_pm"].ctypes.data, out["pt_pm_un"].ctypes.data, out["pix_err"].ctypes.data,
            out["dist_pred"].ctypes.data, out["affine"].ctypes.data]
    if hasattr(lib, "pagk_tracker_track_features_ex"):
        ret = lib.pagk_tracker_track_features_ex(*args, out["error"].ctypes.data, out["flows_predict_un"].ctypes.data)
    else:   # an older shell: no type 0, error and flows_predict_un stay zero
        ret = lib.pagk_tracker_track_features(*args)
    if ret == -100:
        raise RuntimeError("GyroAidedTracker: " + lib.pagk_tracker_last_error().decode())
    return ret, {k: v[:n] for k, v in out.items()}


def geometry_validation(keys_ref_un, pt_predict_un, status, H21, H12, F21):
    """GyroAidedTracker::GeometryValidation() with an installed model fitter (reference
    src/gyro_aided_tracker.cpp:429-480) -> (cnt_inlier, status, track_score)."""
    lib = load()
    k = np.ascontiguousarray(keys_ref_un, np.float32).reshape(-1, 2)
    q = np.ascontiguousarray(pt_predict_un, np.float32).reshape(-1, 2)
    st = np.array(status, np.uint8, copy=True)
    H21, H12, F21 = (np.ascontiguousarray(M, np.float64) for M in (H21, H12, F21))
    ts = C.c_float(0)
    ret = lib.pagk_tracker_geometry_validation(int(st.shape[0]), k.ctypes.data, q.ctypes.data, st.ctypes.data,
                                               H21.ctypes.data, H12.ctypes.data, F21.ctypes.data, C.byref(ts))
    if ret == -100:
        raise RuntimeError("GyroAidedTracker: " + lib.pagk_tracker_last_error().decode())
    return ret, st, np.float32(ts.value)


# ---- sequence formats of the reference's demo (csrc/host/sequence_io.h) ----
def geometry_validation_fit(keys_ref_un, pt_predict_un, status, seed=None):
    """GyroAidedTracker::GeometryValidation() with no fitter installed: the device fits (reference
    src/gyro_aided_tracker.cpp:429-480, 589-768) -> (cnt_inlier, status, track_score).  seed None = the shell's default."""
    lib = load()
    k = np.ascontiguousarray(keys_ref_un, np.float32).reshape(-1, 2)
    q = np.ascontiguousarray(pt_predict_un, np.float32).reshape(-1, 2)
    st = np.array(status, np.uint8, copy=True)
    ts = C.c_float(0)
    ret = lib.pagk_tracker_geometry_validation_fit(int(st.shape[0]), k.ctypes.data, q.ctypes.data, st.ctypes.data,
                                                   DEFAULT_FIT_SEED if seed is None else int(seed), C.byref(ts))
    if ret == -100:
        raise RuntimeError("GyroAidedTracker: " + lib.pagk_tracker_last_error().decode())
    return ret, st, np.float32(ts.value)


DEFAULT_FIT_SEED = 0x5EED0F17   # GyroAidedTracker::kDefaultFitSeed


def load_keypoints(path: str) -> np.ndarray:
    """SuperPoint keypoint list "idx, x, y" (reference src/frame.cpp:222-240) -> n x 2 float32."""
    lib = load()
    n = lib.pagk_seq_load_keypoints(path.encode(), None, 0)
    if n < 0:
        raise FileNotFoundError(path)
    xy = np.zeros((max(n, 1), 2), np.float32)
    lib.pagk_seq_load_keypoints(path.encode(), xy.ctypes.data, n)
    return xy[:n]


def load_correspondences(path: str):
    """corresponds.txt "<t_seconds>, <stamp>" (reference Examples/Demo/RealSenseD435i.cpp:167-182)."""
    lib = load()
    n = lib.pagk_seq_load_correspondences(path.encode(), None, None, 64, 0)
    if n < 0:
        raise FileNotFoundError(path)
    times = np.zeros(max(n, 1), np.float64)
    names = C.create_string_buffer(64 * max(n, 1))
    lib.pagk_seq_load_correspondences(path.encode(), times.ctypes.data, C.addressof(names), 64, n)
    raw = names.raw
    return times[:n], [raw[64 * k:64 * k + 64].split(b"\0", 1)[0].decode() for k in range(n)]


def find_time(times: np.ndarray, t: float) -> int:
    """findTimeCorrespondenIndex (reference include/common.h:105-114)."""
    times = np.ascontiguousarray(times, np.float64)
    return load().pagk_seq_find_time(times.ctypes.data, int(times.shape[0]), float(t))


def parse_image_line(line: str):
    """One line of image_file_list.txt -> time in seconds, or None (reference RealSenseD435i.cpp:89-94)."""
    t = C.c_double(0)
    return t.value if load().pagk_seq_parse_image_line(line.encode(), C.byref(t)) else None


def load_imu(path: str) -> np.ndarray:
    """imu.txt "<stamp_ns> ax ay az wx wy wz" (reference RealSenseD435i.cpp:102-141) -> n x 7 (ax..wz, t)."""
    lib = load()
    n = lib.pagk_seq_load_imu(path.encode(), None, 0)
    if n < 0:
        raise FileNotFoundError(path)
    out = np.zeros((max(n, 1), 7), np.float64)
    lib.pagk_seq_load_imu(path.encode(), out.ctypes.data, n)
    return out[:n]


def imu_windows(imu_path: str, frame_times):
    """The demo's streaming IMU window per frame pair (reference RealSenseD435i.cpp:196-218) ->
    (first_index, count) per frame."""
    ft = np.ascontiguousarray(frame_times, np.float64)
    first = np.zeros(max(len(ft), 1), np.int32)
    counts = np.zeros(max(len(ft), 1), np.int32)
    n = load().pagk_seq_imu_windows(imu_path.encode(), ft.ctypes.data, len(ft), first.ctypes.data, counts.ctypes.data)
    if n < 0:
        raise FileNotFoundError(imu_path)
    return first[:len(ft)], counts[:len(ft)]


# ---- Step 3 and the frame hand-over on the device (include/pagk.h), for hosts that hold numpy arrays ----
def _device_context(ctx):
    """A caller's capi.Context, or one this module keeps for its own calls."""
    global _ctx
    if ctx is not None:
        return ctx
    if _ctx is None:
        _ctx = capi.Context(0)
    return _ctx


_ctx = None


def post_filter_device(half_patch: int, status_pm, pix_err, dist_pred, pt_pm, pt_pm_un, ctx=None):
    """pagk_post_filter_device on host arrays (copied up, filtered on the device, copied back) ->
    (kept, status, pt_predict, pt_predict_un, (th_pix, th_dist)); bit-identical to capi.post_filter."""
    import torch
    c = _device_context(ctx)
    st = np.ascontiguousarray(status_pm, np.uint8)
    n = int(st.shape[0])
    arrays = (st, np.ascontiguousarray(pix_err, np.float64), np.ascontiguousarray(dist_pred, np.float64),
              np.ascontiguousarray(pt_pm, np.float32).reshape(-1, 2), np.ascontiguousarray(pt_pm_un, np.float32).reshape(-1, 2))
    if any(a.shape[0] != n for a in arrays):
        raise ValueError("the five input arrays differ in length")
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(a if n else np.zeros((1,) + a.shape[1:], a.dtype)).to(dev) for a in arrays]
    d_out = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
    d_pp, d_ppu = torch.zeros((max(n, 1), 2), device=dev), torch.zeros((max(n, 1), 2), device=dev)
    d_kept, d_th = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    c.post_filter_device(n, half_patch, d[0], d[1], d[2], d[3], d[4], d_out, d_pp, d_ppu, d_kept, d_th)
    c.sync()
    th = d_th.cpu().numpy()
    return int(d_kept.cpu()[0]), d_out.cpu().numpy()[:n], d_pp.cpu().numpy()[:n], d_ppu.cpu().numpy()[:n], (th[0], th[1])


def frame_handover(params, width, height, cap, target_n, new_point_threshold, status, pt_predict, pt_predict_un,
                   candidates, state=None, ctx=None) -> dict:
    """pagk_frame_handover (host buffers): the survivors of a pair and the accepted candidates as the next pair's
    keypoints -> dict(keys, keys_un, keys_normal, index_in_last, live, mask, state)."""
    return _device_context(ctx).frame_handover(params, width, height, cap, target_n, new_point_threshold, status,
                                               pt_predict, pt_predict_un, candidates, state=state)


def frame_handover_device(ctx, *args):
    """pagk_frame_handover_device on device arrays: capi.Context.frame_handover_device."""
    return ctx.frame_handover_device(*args)


def gyro_predict_device_live(ctx, *args):
    """pagk_gyro_predict_device_live on device arrays: capi.Context.gyro_predict_device_live."""
    return ctx.gyro_predict_device_live(*args)


# ---- the corner detector (reference src/frame.cpp:156-218), array in, array out ----
def detect_corners(img, mask=None, max_corners: int = 1000, det=None, ctx=None) -> dict:
    """pagk_detect_corners (host buffers): the reference's goodFeaturesToTrack call with the Harris response on an 8-bit
    image -> dict(corners (n x 2 float32, strongest first), info and its words by name)."""
    return _device_context(ctx).detect_corners(np.ascontiguousarray(img, np.uint8), mask, max_corners, det)


def frame_handover_detect(params, img, cap, target_n, new_point_threshold, status, pt_predict, pt_predict_un, det=None,
                          state=None, ctx=None) -> dict:
    """pagk_frame_handover_detect (host buffers): the hand-over with the top-up detected on `img` under the mask the call
    builds -> dict(keys, keys_un, keys_normal, index_in_last, live, mask, state, info)."""
    return _device_context(ctx).frame_handover_detect(params, np.ascontiguousarray(img, np.uint8), cap, target_n,
                                                      new_point_threshold, status, pt_predict, pt_predict_un, det=det,
                                                      state=state)


def corner_response(img, ctx=None) -> np.ndarray:
    """pagk_selftest_corner_response: the detector's response map of an image (float32, harris_k = 0.04)."""
    return _device_context(ctx).selftest_corner_response(np.ascontiguousarray(img, np.uint8))


# ---- the detector of the reference's front-ends (src/ORBextractor.cc:1148-1205), array in, array out ----
def detect_fast(img, mask=None, n_features: int = 1000, fast=None, ctx=None) -> dict:
    """pagk_detect_fast (host buffers): FAST-9/16 in cells of about 30 pixels with the fall-back threshold, the quadtree
    down to n_features nodes, the mask test -> dict(keypoints (n x 2 float32, list order), response (n), info and its
    words by name)."""
    return _device_context(ctx).detect_fast(np.ascontiguousarray(img, np.uint8), mask, n_features, fast)


def frame_handover_fast(params, img, cap, target_n, new_point_threshold, status, pt_predict, pt_predict_un, fast=None,
                        state=None, ctx=None) -> dict:
    """pagk_frame_handover_fast (host buffers): the hand-over with the candidates = detect_fast(img, no mask) ->
    dict(keys, keys_un, keys_normal, index_in_last, live, mask, state, info)."""
    return _device_context(ctx).frame_handover_fast(params, np.ascontiguousarray(img, np.uint8), cap, target_n,
                                                    new_point_threshold, status, pt_predict, pt_predict_un, fast=fast,
                                                    state=state)


# ---- the ORB baseline of the reference's front-ends for one level (src/ORBextractor.cc:1066-1145, ----
# ---- src/ORBDetectAndDespMatcher.cpp:55-91), array in, array out ----
def orb_extract(img, n_features: int, pattern, fast=None, orb=None, ctx=None) -> dict:
    """ORBextractor::operator() with one level: detect_fast with no mask, then pagk_orb_describe on its keypoints ->
    dict(keypoints (n x 2 float32), response (n), angle (n), desc (n x 32 uint8), detect_info, describe_info).  `pattern`
    is the host's sampling table (1024 integers); it is uploaded to the context on every call."""
    c = _device_context(ctx)
    img = np.ascontiguousarray(img, np.uint8)
    c.orb_set_pattern(pattern)
    det = c.detect_fast(img, None, n_features, fast)
    d = c.orb_describe(img, det["keypoints"], orb)
    return dict(keypoints=det["keypoints"], response=det["response"], angle=d["angle"], desc=d["desc"],
                detect_info=det["info"], describe_info=d["info"])


def orb_match_pair(img_ref, img_cur, n_features: int, pattern, fast=None, orb=None, ctx=None) -> dict:
    """ORBDetectAndDespMatcher::FindFeatureMatches: orb_extract on both images, then pagk_orb_match with the reference
    image's descriptors as the query rows -> dict(ref, cur (the two orb_extract results), train_idx, distance, keep, info
    and its words by name: nq, matches, kept -- the three counts the reference logs --, min_dist, max_dist, threshold)."""
    c = _device_context(ctx)
    ref = orb_extract(img_ref, n_features, pattern, fast, orb, c)
    cur = orb_extract(img_cur, n_features, pattern, fast, orb, c)
    out = c.orb_match(ref["desc"], cur["desc"], orb)
    out.update(ref=ref, cur=cur)
    return out


# ---- ORB over a scale pyramid (src/ORBextractor.cc:434-470, 789-875, 1066-1232), array in, array out ----
def orb_extract_levels(img, extractor, pattern, orb=None, ctx=None) -> dict:
    """ORBextractor::operator() with extractor.n_levels levels (pagk_orb_extract_levels) -> dict(n, keypoints (n x 2
    float32, original-image coordinates), octave (n), response (n), angle (n), desc (n x 32 uint8), info and its words by
    name).  `pattern` is the host's sampling table (1024 integers); it is uploaded to the context on every call."""
    c = _device_context(ctx)
    c.orb_set_pattern(pattern)
    return c.orb_extract_levels(np.ascontiguousarray(img, np.uint8), extractor, orb)


def orb_detect_levels(img, extractor, mask=None, ctx=None) -> dict:
    """ORBextractor::DetectFeatures with extractor.n_levels levels (pagk_orb_detect_levels) -> dict(n, keypoints, octave,
    response, info): the candidate list of the hand-over, in the reference's order."""
    return _device_context(ctx).orb_detect_levels(np.ascontiguousarray(img, np.uint8), extractor, mask)


def orb_match_pair_levels(img_ref, img_cur, extractor, pattern, orb=None, ctx=None) -> dict:
    """ORBDetectAndDespMatcher::FindFeatureMatches with extractor.n_levels levels, as one chain on the device: both images
    into frame slots 0 and 1, pagk_orb_extract_slot on each, pagk_orb_match_slots with the reference image as the query ->
    dict(ref, cur (the two sets), train_idx, distance, keep (nq rows), info and its words by name)."""
    c = _device_context(ctx)
    c.orb_set_pattern(pattern)
    ref_img, cur_img = np.ascontiguousarray(img_ref, np.uint8), np.ascontiguousarray(img_cur, np.uint8)
    c.frame_upload(0, ref_img, 1)
    c.frame_upload(1, cur_img, 1)
    c.orb_extract_slot(extractor, 0, orb)
    c.orb_extract_slot(extractor, 1, orb)
    c.orb_match_slots(0, 1, orb)
    cap_r = capi.orb_extractor_levels(extractor, ref_img.shape[1], ref_img.shape[0])["out_bound"]
    cap_c = capi.orb_extractor_levels(extractor, cur_img.shape[1], cur_img.shape[0])["out_bound"]
    ref, cur = c.orb_slot_read(0, cap_r), c.orb_slot_read(1, cap_c)
    out = c.orb_match_slots_read(0, cap_r)
    nq = ref["n"]
    out.update(train_idx=out["train_idx"][:nq], distance=out["distance"][:nq], keep=out["keep"][:nq], ref=ref, cur=cur)
    return out


# ---- the two-view pose of a frame pair (src/ORBDetectAndDespMatcher.cpp:84-108), array in, array out ----
def _focal_and_centre(K):
    """(mfx + mfy) / 2 and (mcx, mcy) of a 3 x 3 camera matrix, as PoseEstimation2d2d passes them (:97, :105)."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    return (K[0, 0] + K[1, 1]) / 2.0, float(K[0, 2]), float(K[1, 2])


def pose_estimation_2d2d(pts1, pts2, K, status=None, params=None, ctx=None) -> dict:
    """ORBDetectAndDespMatcher::PoseEstimation2d2d by the library's definition (pagk_pose_2d2d): H21, H12, F21 as
    pagk_geometry_fit fits them, the essential matrix by the deterministic five-point RANSAC, R and t by the cheirality test
    -> dict(H21, H12, F21, E, R, t, mask_H, mask_F, mask_E, mask_pose, fit_info, pose_info, info: the pose words by name)."""
    f, cx, cy = _focal_and_centre(K)
    return _device_context(ctx).pose_2d2d(pts1, pts2, f, cx, cy, status, params)


def orb_pose_pair(img_ref, img_cur, n_features: int, pattern, K, fast=None, orb=None, params=None, ctx=None) -> dict:
    """FindFeatureMatches followed by PoseEstimation2d2d, the two calls both front-ends make per frame pair: orb_match_pair,
    then pose_estimation_2d2d on points1[q] = ref keypoint q, points2[q] = cur keypoint train_idx[q] with status = keep
    (:86-91) -> the result of orb_match_pair plus `pose` (the dict of pose_estimation_2d2d), pts1, pts2 and status."""
    c = _device_context(ctx)
    out = orb_match_pair(img_ref, img_cur, n_features, pattern, fast, orb, c)
    kp1, kp2 = out["ref"]["keypoints"], out["cur"]["keypoints"]
    tr = np.asarray(out["train_idx"], np.int64)
    st = (np.asarray(out["keep"]) != 0) & (tr >= 0) & (tr < len(kp2))
    pts2 = np.zeros_like(kp1)
    pts2[st] = kp2[tr[st]]
    out.update(pose=pose_estimation_2d2d(kp1, pts2, K, st.astype(np.uint8), params, c), pts1=kp1, pts2=pts2,
               status=st.astype(np.uint8))
    return out


# ---- pyramidal Lucas-Kanade, the image-only baseline of the comparison (src/gyro_aided_tracker.cpp:353-380), ----
# ---- array in, array out ----
def lk_track(img_ref, img_cur, pts, lk=None, ctx=None) -> dict:
    """cv::calcOpticalFlowPyrLK and the error filter of TrackFeatures' type 0 by the library's definition (pagk_lk_track) ->
    dict(pt_out (n x 2 float32), status (n, after the filter), status_raw (n), err (n), flow (n x 2), info and its words by
    name: n, raw, kept, top_level, lost_min_eig, lost_out_of_range)."""
    return _device_context(ctx).lk_track(np.ascontiguousarray(img_ref, np.uint8), np.ascontiguousarray(img_cur, np.uint8),
                                         pts, lk)


def lk_track_flow(img_ref, img_cur, pts, lk=None, cam=None, pt_init=None, status_in=None, ctx=None) -> dict:
    """Lucas-Kanade started from an initial point (OPTFLOW_USE_INITIAL_FLOW, the reference's open experiment at
    src/gyro_aided_tracker.cpp:364-365) by the library's definition (pagk_lk_track_flow): rows with status_in == 0 are left
    out, pt_out_dist = DistortVecPoints(pt_out) with the camera of `cam` (a capi.Params) -> the dict of lk_track plus
    pt_out_dist and `skipped`."""
    return _device_context(ctx).lk_track_flow(np.ascontiguousarray(img_ref, np.uint8), np.ascontiguousarray(img_cur, np.uint8),
                                              pts, lk, cam, pt_init, status_in)


# ---- track-to-detection association (src/gyro_aided_tracker.cpp:859-939, :1017-1136), array in, array out ----
def search_by_gyro_predict(img_ref, img_cur, half_patch, keys_ref, pt_predict_un, status, affine, keys_cur, keys_cur_un,
                           assoc=None, radius_unit=None, cap=64, ctx=None) -> dict:
    """Steps 2 and 3 of GyroAidedTracker::SearchByGyroPredict behind a finished prediction (pagk_search_gyro_predict): the
    neighbour search, MatchFeatures, the wider search when fewer than min_matches came out, the flow error -> dict(rc,
    n_matches, query, train, dist, ncc, flows_err (n x 2), count, idx, dist_lists, ncc_lists, info and its words by name)."""
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)     # noqa: E731
    return _device_context(ctx).search_gyro_predict(img_ref, img_cur, int(half_patch), f32(keys_ref).reshape(-1, 2),
                                                    f32(pt_predict_un).reshape(-1, 2), np.ascontiguousarray(status, np.uint8),
                                                    f32(affine), f32(keys_cur).reshape(-1, 2), f32(keys_cur_un).reshape(-1, 2),
                                                    assoc, radius_unit, cap)


def search_by_klt(img_ref, img_cur, keys_ref, keys_cur, lk=None, assoc=None, ctx=None) -> dict:
    """GyroAidedTracker::SearchByOpencvKLT by the library's definition (pagk_search_klt): pyramidal Lucas-Kanade, the err
    filter, the radius match against the detected keypoints, ratio test, first-come uniqueness, the mean-disparity filter ->
    dict(n_matches, query, train, dist, disparity, pt_out, status, err, stats, info, lk_info and their fields by name)."""
    return _device_context(ctx).search_klt(np.ascontiguousarray(img_ref, np.uint8), np.ascontiguousarray(img_cur, np.uint8),
                                           keys_ref, keys_cur, lk, assoc)


# ---- gyro integration (src/gyro_aided_tracker.cpp:511-587), array in, array out ----
def gyro_integrate(Rbc, K, t_ref: float, t_cur: float, t, w, bias=(0.0, 0.0, 0.0), ctx=None) -> dict:
    """GyroAidedTracker::IntegrateGyroMeasurements and SetRcl by the library's definition (pagk_gyro_integrate, include/pagk.h
    "Gyro integration"): the samples (t: n time stamps, w: n x 3 rates in rad/s) between the frames at t_ref and t_cur ->
    dict(Rcl (3 x 3), rot9 (rows 0 and 1 of K Rcl K^-1, then the third row of Rcl: what the sequence's prediction reads))."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    cam = capi.make_params()
    cam.fx, cam.fy, cam.cx, cam.cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    win, keep = capi.imu_window(t_ref, t_cur, t, w, bias)
    rcl, rot9 = _device_context(ctx).gyro_integrate(Rbc, cam, win)
    del keep
    return dict(Rcl=rcl, rot9=rot9)
