"""Every entry point of include/pagk.h that takes a device pointer, one row each: for every pointer argument its element
type, its documented length as an expression of the call's scalars, its role and the kind of guard fill it gets
(tests/arena.py).  Plain data: nothing here imports the package or touches a device.  test_arena_cpu.py holds the table
against the header (every declared device entry point is a row or an entry of EXEMPT, every `d_` parameter is in its
row); test_device_bounds_gpu.py runs the rows on guarded arrays.

Lengths are the header's text, not the kernels': `where` names the sentence.  They count ELEMENTS of `dtype`.  Names an
expression may use: the function's own scalar parameters, `channels`, `iters_H` / `iters_F` / `iters_E` (fields of the
parameter structs), the *_WORDS constants and image_length(width, height, step) = (height - 1) * step + width.
`W`, `H` are the size of level 0 of the frame slot the call reads.

role: "in", "out", "inout"; `optional`: the header allows NULL.
tail: what the header says about entries at and beyond the count the call reports -- None (no count: every entry is
written), "untouched", or the value they are set to (0, -1, 257)."""
import dataclasses

DETECT_INFO_WORDS = 8
ORB_INFO_WORDS = 8
LK_INFO_WORDS = 8
FIT_INFO_WORDS = 12
POSE_INFO_WORDS = 16
ASSOC_INFO_WORDS = 8
ASSOC_STATS_WORDS = 8
HANDOVER_STATE_WORDS = 8

IMAGE_RULE = "Conventions: 'an image ... is (height - 1) * step + width bytes long'"


def image_length(width, height, step):
    return (height - 1) * step + width if width > 0 and height > 0 else 0


@dataclasses.dataclass(frozen=True)
class Arr:
    name: str            # the parameter; "d_out.pt_un" is field pt_un of the pagk_outputs that d_out points to
    dtype: str           # "f32", "f64", "u8", "i32"
    length: str          # elements, an expression of the call's scalars
    role: str            # "in", "out", "inout"
    kind: str            # arena fill kind: "float", "byte", "index"
    optional: bool = False
    tail: object = None
    where: str = ""      # the header sentence the length comes from, where it is not the parameter's own comment


@dataclasses.dataclass(frozen=True)
class Form:
    function: str
    arrays: tuple
    per_stream: bool = False   # batch forms: every array is a host array of k device pointers, one set per stream / frame


def _in(name, dtype, length, kind, optional=False, where=""):
    return Arr(name, dtype, length, "in", kind, optional, None, where)


def _out(name, dtype, length, kind, optional=False, tail=None, where=""):
    return Arr(name, dtype, length, "out", kind, optional, tail, where)


def _io(name, dtype, length, kind, optional=False, tail=None, where=""):
    return Arr(name, dtype, length, "inout", kind, optional, tail, where)


_TRACK_IN = (
    _in("d_pt_ref_un", "f32", "2 * n", "float", where="Conventions: points are interleaved (x, y) float32 pairs, n of them"),
    _in("d_pt_init_un", "f32", "2 * n", "float", optional=True),
    _in("d_affine", "f32", "4 * n", "float", optional=True, where="Conventions: affine is n x 4 float32"),
    _in("d_status_in", "u8", "n", "byte"),
)
# pagk_outputs: "Any pointer except pt_un/status may be NULL"; n = 0 writes nothing
_TRACK_OUT = (
    _out("d_out.pt_un", "f32", "2 * n", "float"),
    _out("d_out.pt_dist", "f32", "2 * n", "float", optional=True),
    _out("d_out.status", "u8", "n", "byte"),
    _out("d_out.pix_err", "f64", "n", "float", optional=True),
    _out("d_out.dist_pred", "f64", "n", "float", optional=True),
    _out("d_out.ncc", "f32", "n", "float", optional=True),
    _out("d_out.iters", "i32", "n", "index", optional=True),
)
_IMAGE = "image_length(width, height, step)"

_PREDICT_OUT = (
    _out("d_pt_predict_un", "f32", "2 * n", "float"),
    _out("d_pt_predict", "f32", "2 * n", "float"),
    _out("d_status", "u8", "n", "byte"),
    # "affine untouched" where a prediction leaves the image (or d_live[i] == 0): rows the call may not write
    _io("d_affine", "f32", "4 * n", "float", optional=True),
)

_HANDOVER_IN = (
    _in("d_status", "u8", "cap", "byte", where="survivors: 'd_status[i] != 0 (cap entries)'"),
    _in("d_pt_predict", "f32", "2 * cap", "float"),
    _in("d_pt_predict_un", "f32", "2 * cap", "float"),
)
_HANDOVER_OUT = (
    _out("d_keys", "f32", "2 * cap", "float", tail=0, where="outputs: 'entries of the key arrays at and beyond total are zeroed'"),
    _out("d_keys_un", "f32", "2 * cap", "float", tail=0),
    _out("d_keys_normal", "f32", "2 * cap", "float", optional=True, tail=0),
    _out("d_index_in_last", "i32", "cap", "index", tail=-1, where="outputs: '(index_in_last: -1)'"),
    _out("d_live", "u8", "cap", "byte", where="outputs: 'd_live[i] = i < total for all cap entries'"),
    _out("d_mask", "u8", "width * height", "byte", optional=True),
    _io("d_state", "i32", "HANDOVER_STATE_WORDS", "index"),
)
_INFO = _out("d_info", "i32", "DETECT_INFO_WORDS", "index")

_FIT_OUT = (
    _out("d_models", "f64", "27", "float"),
)
_NBR_IN = (
    _in("d_keys_ref", "f32", "2 * n", "float"),
    _in("d_pt_predict_un", "f32", "2 * n", "float"),
    _in("d_status", "u8", "n", "byte"),
    _in("d_affine", "f32", "4 * n", "float", optional=True),
    _in("d_keys_cur", "f32", "2 * m", "float"),
    _in("d_keys_cur_un", "f32", "2 * m", "float"),
)
_MATCH_OUT = (
    _out("d_match_query", "i32", "n", "index", tail=-1, where="outputs: 'rows at or beyond the count: -1, -1, 0, 0'"),
    _out("d_match_train", "i32", "n", "index", tail=-1),
    _out("d_match_dist", "f32", "n", "float", optional=True, tail=0),
    _out("d_match_ncc", "f32", "n", "float", optional=True, tail=0),
    _out("d_n_matches", "i32", "1", "index"),
)

FORMS = (
    Form("pagk_frame_set_device", (_in("d_data", "u8", _IMAGE, "byte", where=IMAGE_RULE),)),
    Form("pagk_frame_set_device_batch", (_in("d_data", "u8", _IMAGE, "byte", where=IMAGE_RULE),), per_stream=True),
    Form("pagk_track_device", _TRACK_IN + _TRACK_OUT),
    Form("pagk_track_device_fused", _TRACK_IN + _TRACK_OUT + (_in("d_next", "u8", _IMAGE, "byte", where=IMAGE_RULE),)),
    Form("pagk_track_device_batch", _TRACK_IN + _TRACK_OUT, per_stream=True),
    Form("pagk_gyro_predict_device", (_in("d_pt_ref_un", "f32", "2 * n", "float"),) + _PREDICT_OUT),
    Form("pagk_gyro_predict_device_rot",
         (_in("d_rot", "f32", "9", "float"), _in("d_pt_ref_un", "f32", "2 * n", "float")) + _PREDICT_OUT),
    Form("pagk_gyro_predict_device_live",
         (_in("d_rot", "f32", "9", "float"), _in("d_pt_ref_un", "f32", "2 * n", "float"), _in("d_live", "u8", "n", "byte"))
         + _PREDICT_OUT),
    Form("pagk_post_filter_device", (
        _in("d_status_pm", "u8", "n", "byte"), _in("d_pix_err", "f64", "n", "float"), _in("d_dist_pred", "f64", "n", "float"),
        _in("d_pt_pm", "f32", "2 * n", "float", optional=True), _in("d_pt_pm_un", "f32", "2 * n", "float", optional=True),
        _out("d_status_out", "u8", "n", "byte"),
        # "Survivors' points are copied, other entries of d_pt_predict(_un) are left untouched"
        _io("d_pt_predict", "f32", "2 * n", "float", optional=True), _io("d_pt_predict_un", "f32", "2 * n", "float", optional=True),
        _out("d_kept", "i32", "1", "index"), _out("d_thresholds", "f64", "2", "float", optional=True))),
    Form("pagk_frame_handover_device", _HANDOVER_IN + (
        _in("d_n_cand", "i32", "1", "index"),
        _in("d_cand_un", "f32", "2 * cand_cap", "float", where="top-up: 'Candidates j = 0 .. *d_n_cand - 1 (clamped to [0, cand_cap])'"),
    ) + _HANDOVER_OUT),
    Form("pagk_detect_corners_device", (
        _in("d_mask", "u8", "W * H", "byte", optional=True), _in("d_max_corners", "i32", "1", "index", optional=True),
        _out("d_corners", "f32", "2 * cap", "float", tail=0, where="output: 'entries beyond the number are zeroed'"), _INFO)),
    Form("pagk_frame_handover_detect_device", _HANDOVER_IN + _HANDOVER_OUT + (_INFO,)),
    Form("pagk_detect_fast_device", (
        _in("d_mask", "u8", "W * H", "byte", optional=True),
        _out("d_keypoints", "f32", "2 * cap", "float", tail=0, where="result: 'entries beyond the count are zeroed'"),
        _out("d_response", "f32", "cap", "float", optional=True, tail=0), _INFO)),
    Form("pagk_frame_handover_fast_device", _HANDOVER_IN + _HANDOVER_OUT + (_INFO,)),
    Form("pagk_frame_rectify_device", (
        _in("d_raw", "u8", "(src_height - 1) * src_step + src_width * channels", "byte", where=IMAGE_RULE),)),
    Form("pagk_orb_describe_device", (
        _in("d_keypoints", "f32", "2 * cap", "float"), _in("d_n", "i32", "1", "index"),
        _out("d_angle", "f32", "cap", "float", optional=True, tail=0, where="'Rows at or beyond the count are zeroed'"),
        _out("d_desc", "u8", "32 * cap", "byte", tail=0), _out("d_info", "i32", "ORB_INFO_WORDS", "index"))),
    Form("pagk_orb_match_device", (
        _in("d_desc_q", "u8", "32 * cap_q", "byte"), _in("d_nq", "i32", "1", "index"),
        _in("d_desc_t", "u8", "32 * cap_t", "byte"), _in("d_nt", "i32", "1", "index"),
        _out("d_train_idx", "i32", "cap_q", "index", tail=-1, where="'Rows at or beyond nq get -1 / 257 / 0'"),
        _out("d_distance", "i32", "cap_q", "index", tail=257), _out("d_keep", "u8", "cap_q", "byte", tail=0),
        _out("d_info", "i32", "ORB_INFO_WORDS", "index"))),
    Form("pagk_lk_pyramid_device", ()),   # no caller array: reads a slot, writes a buffer of the context
    Form("pagk_lk_track_device", (
        _in("d_pt_ref", "f32", "2 * cap", "float"), _in("d_n", "i32", "1", "index", optional=True),
        _out("d_pt_out", "f32", "2 * cap", "float", tail=0, where="'Rows at or beyond the count are zeroed'"),
        _out("d_status", "u8", "cap", "byte", tail=0), _out("d_status_raw", "u8", "cap", "byte", optional=True, tail=0),
        _out("d_err", "f32", "cap", "float", tail=0), _out("d_flow", "f32", "2 * cap", "float", optional=True, tail=0),
        _out("d_info", "i32", "LK_INFO_WORDS", "index"))),
    Form("pagk_geometry_scores_device", (
        _in("d_pts1", "f32", "2 * n", "float"), _in("d_pts2", "f32", "2 * n", "float"),
        _out("d_inliers_H", "u8", "n", "byte"), _out("d_inliers_F", "u8", "n", "byte"), _out("d_scores", "f32", "2", "float"))),
    Form("pagk_geometry_fit_device", (
        _in("d_pts1", "f32", "2 * n", "float"), _in("d_pts2", "f32", "2 * n", "float"), _in("d_status", "u8", "n", "byte", optional=True))
        + _FIT_OUT + (
        _out("d_mask_H", "u8", "n", "byte", optional=True), _out("d_mask_F", "u8", "n", "byte", optional=True),
        _out("d_info", "i32", "FIT_INFO_WORDS", "index"), _out("d_hyp_counts", "i32", "iters_H + iters_F", "index", optional=True))),
    Form("pagk_geometry_validation_device", (
        _in("d_pt_ref_un", "f32", "2 * n", "float"), _in("d_pt_predict_un", "f32", "2 * n", "float"),
        _io("d_status", "u8", "n", "byte"), _out("d_cnt", "i32", "1", "index"), _out("d_score", "f32", "1", "float"))),
    Form("pagk_pose_2d2d_device", (
        _in("d_pts1", "f32", "2 * n", "float"), _in("d_pts2", "f32", "2 * n", "float"), _in("d_status", "u8", "n", "byte", optional=True))
        + _FIT_OUT + (
        _out("d_pose", "f64", "21", "float"),
        _out("d_mask_H", "u8", "n", "byte", optional=True), _out("d_mask_F", "u8", "n", "byte", optional=True),
        _out("d_mask_E", "u8", "n", "byte", optional=True), _out("d_mask_pose", "u8", "n", "byte", optional=True),
        _out("d_fit_info", "i32", "FIT_INFO_WORDS", "index"), _out("d_pose_info", "i32", "POSE_INFO_WORDS", "index"),
        _out("d_cand_counts", "i32", "10 * iters_E", "index", optional=True))),
    Form("pagk_pose_from_matches_device", (
        _in("d_kp_ref", "f32", "2 * cap_q", "float"), _in("d_nq", "i32", "1", "index"),
        _in("d_kp_cur", "f32", "2 * cap_t", "float"), _in("d_nt", "i32", "1", "index"),
        _in("d_train_idx", "i32", "cap_q", "index"), _in("d_keep", "u8", "cap_q", "byte"))
        + _FIT_OUT + (
        _out("d_pose", "f64", "21", "float"),
        _out("d_mask_H", "u8", "cap_q", "byte", optional=True), _out("d_mask_F", "u8", "cap_q", "byte", optional=True),
        _out("d_mask_E", "u8", "cap_q", "byte", optional=True), _out("d_mask_pose", "u8", "cap_q", "byte", optional=True),
        _out("d_fit_info", "i32", "FIT_INFO_WORDS", "index"), _out("d_pose_info", "i32", "POSE_INFO_WORDS", "index"))),
    Form("pagk_near_neighbors_device", _NBR_IN + (
        # count is IN/OUT; a list's entries beyond its count keep the caller's content
        _io("d_count", "i32", "n", "index"), _io("d_nbr_idx", "i32", "n * cap", "index", tail="untouched"),
        _io("d_nbr_dist", "f32", "n * cap", "float", tail="untouched"), _io("d_nbr_ncc", "f32", "n * cap", "float", tail="untouched"))),
    Form("pagk_match_features_device", (
        _in("d_count", "i32", "n", "index"), _in("d_nbr_idx", "i32", "n * cap", "index"),
        _in("d_nbr_dist", "f32", "n * cap", "float"), _in("d_nbr_ncc", "f32", "n * cap", "float"))
        + _MATCH_OUT + (_out("d_info", "i32", "ASSOC_INFO_WORDS", "index"),)),
    Form("pagk_search_gyro_predict_device", _NBR_IN + (
        _in("d_m", "i32", "1", "index", optional=True),
        _out("d_count", "i32", "n", "index", where="'The call zeroes d_count'"),
        _out("d_nbr_idx", "i32", "n * cap", "index", tail="untouched"), _out("d_nbr_dist", "f32", "n * cap", "float", tail="untouched"),
        _out("d_nbr_ncc", "f32", "n * cap", "float", tail="untouched"))
        + _MATCH_OUT + (
        _out("d_flows_err", "f32", "2 * n", "float", optional=True), _out("d_info", "i32", "ASSOC_INFO_WORDS", "index"))),
    Form("pagk_search_klt_device", (
        _in("d_keys_ref", "f32", "2 * cap", "float"), _in("d_n", "i32", "1", "index", optional=True),
        _in("d_keys_cur", "f32", "2 * m", "float"), _in("d_m", "i32", "1", "index", optional=True),
        _out("d_pt_out", "f32", "2 * cap", "float", tail=0), _out("d_status", "u8", "cap", "byte", tail=0),
        _out("d_err", "f32", "cap", "float", tail=0),
        _out("d_match_query", "i32", "cap", "index", tail=-1), _out("d_match_train", "i32", "cap", "index", tail=-1),
        _out("d_match_dist", "f32", "cap", "float", optional=True, tail=0), _out("d_disparity", "f64", "cap", "float", tail=0),
        _out("d_n_matches", "i32", "1", "index"), _out("d_stats", "f64", "ASSOC_STATS_WORDS", "float"),
        _out("d_info", "i32", "ASSOC_INFO_WORDS", "index"), _out("d_lk_info", "i32", "LK_INFO_WORDS", "index"))),
)

# Entry points the GPU test cannot run, each with its reason.
EXEMPT = {
    "pagk_multi_allgather": "needs RCCL and a group of devices: the exchange of the sharded path (test_multi_gpu.py)",
    "pagk_track_sharded": "needs a group of devices; its arrays are host buffers, the device slices are the library's own",
}


def form(function):
    return next(f for f in FORMS if f.function == function)


def length(arr, scalars):
    """Elements of `arr` for the call's scalars (a dict)."""
    names = dict(globals())
    names.update(scalars)
    return int(eval(arr.length, {"__builtins__": {}}, names))   # noqa: S307 -- the expressions are this file's own
