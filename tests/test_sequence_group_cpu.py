"""CPU tests of the sequence group (pagk_sequence_group_*): the ranges pagk_sequence_group_check accepts, every call on a NULL
lead or a NULL list, the header rules of the six declarations (no d_ parameter, no "device pointer" in a comment, the
reference's lines), the sentences of the older sections that stay as they were, and the shape of the batched kernels' header."""
import ctypes as C
import os
import re

import numpy as np

from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pagk_sequence_group_check", "pagk_sequence_group_create", "pagk_sequence_group_destroy",
                "pagk_sequence_group_start", "pagk_sequence_group_step", "pagk_sequence_group_status")
CSRC = os.path.join(ROOT, "pixel_aware_gyro_aided_klt_feature_tracker_amd", "csrc")


def test_group_check_ranges(built):
    ok = capi.sequence_params_default
    gyro_off, gyro_on = capi.make_params(has_gyro=False), capi.make_params(has_gyro=True)
    for kw in (dict(), dict(validate=0), dict(validate=1), dict(track=gyro_off), dict(track=gyro_on), dict(validate=0, track=gyro_off),
               dict(cap=400), dict(cand_cap=1), dict(width=14, height=14)):
        p = ok(**kw)
        assert capi.sequence_params_check(p) == capi.PAGK_OK and capi.sequence_group_check(p) == capi.PAGK_OK, kw
    # what a plain sequence accepts and the group refuses: Lucas-Kanade, both detectors
    for kw in (dict(tracker=capi.SEQ_LK), dict(tracker=capi.SEQ_LK, lk_initial_flow=1), dict(detector=1), dict(detector=2, cand_cap=0),
               dict(detector=1, cand_cap=0), dict(tracker=capi.SEQ_LK, detector=2)):
        p = ok(**kw)
        assert capi.sequence_params_check(p) == capi.PAGK_OK and capi.sequence_group_check(p) == capi.PAGK_E_ARG, kw
    # what no sequence accepts
    for kw in (dict(tracker=2), dict(validate=2), dict(detector=3), dict(width=13), dict(cap=399), dict(cand_cap=0),
               dict(sigma=0.0), dict(new_point_threshold=float("nan"))):
        assert capi.sequence_group_check(ok(**kw)) == capi.PAGK_E_ARG, kw
    assert capi.sequence_group_check(ok(track=capi.make_params(half_patch=0))) == capi.PAGK_E_ARG
    assert capi.sequence_group_check(ok(fast=capi.fast_params_default(n_levels=8))) == capi.PAGK_E_UNSUPPORTED   # the nested check's code
    assert capi.load().pagk_sequence_group_check(None) == capi.PAGK_E_ARG


def test_every_call_refuses_a_null_lead_or_list(built):
    lib = capi.load()
    E = capi.PAGK_E_ARG
    a = np.zeros(4096, np.float32).ctypes.data
    imgs = (capi.Image * 2)(capi.image_view(np.zeros((480, 640), np.uint8)), capi.image_view(np.zeros((480, 640), np.uint8)))
    lists = (C.c_void_p * 2)(a, a)
    counts = (C.c_int32 * 2)(4, 4)
    none = (C.c_void_p * 2)(None, None)
    assert lib.pagk_sequence_group_create(None, 2) == E
    assert lib.pagk_sequence_group_create(none, 2) == E          # a list without a lead
    assert lib.pagk_sequence_group_create(none, 0) == E
    assert lib.pagk_sequence_group_destroy(None) == E
    assert lib.pagk_sequence_group_start(None, imgs, lists, counts) == E
    assert lib.pagk_sequence_group_step(None, imgs, a, lists, counts, capi.SEQ_DIRECT) == E
    assert lib.pagk_sequence_group_status(None, a) == E


def test_header_rules_of_the_new_declarations(built):
    hdr = open(os.path.join(ROOT, "include", "pagk.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = capi.load()
    assert "#define PAGK_VERSION 303" in hdr
    for name in ENTRY_POINTS:
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name) and getattr(lib, name).argtypes, name
        m = re.search(r"\b(?:int|void) " + name + r"\s*\((.*?)\);", code, flags=re.S)
        assert m, name
        params = [p.split()[-1].lstrip("*") for p in m.group(1).split(",")]
        assert not any(p.startswith("d_") for p in params), (name, params)
        decl = re.search(r"\b(?:int|void) " + name + r"\(", hdr).start()
        comment = hdr[:decl].rsplit("/*", 1)[1]
        assert comment.rstrip().endswith("*/") and "Examples/Demo/RealSenseD435i.cpp:" in comment, name
        assert not re.search(r"device\s+pointer", comment), name
    assert len(lib.pagk_sequence_group_step.argtypes) == 6 and len(lib.pagk_sequence_group_start.argtypes) == 4
    # the section stands behind the sensor form and says what it lifts and what it leaves out
    assert hdr.index("The sensor form of the sequence: raw frames") < hdr.index("The sequence group: k cameras stepped together")
    section = hdr[hdr.index("The sequence group: k cameras stepped together"):hdr.index("int pagk_sequence_group_check")]
    flat = " ".join(section.replace(" * ", " ").split())
    for word in ("Examples/Demo/RealSenseD435i.cpp:199-321", "it lifts the first item", "k cameras batched", "byte for byte",
                 "pagk_frame_set_device_batch", "pagk_track_device_batch", "one linear chain", "Out of scope of the group: Lucas-Kanade",
                 "the Harris and FAST detectors", "sensor sequences", "member by member"):
        assert word in flat, word
    for meth in ("start", "step", "read", "read_pair", "close"):
        assert callable(getattr(runtime.DeviceSequenceGroup, meth)), meth
    for meth in ("start", "step", "status", "destroy"):
        assert callable(getattr(capi.SequenceGroup, meth)), meth


def test_the_pinned_sentences_of_the_older_sections_stand(built):
    hdr = open(os.path.join(ROOT, "include", "pagk.h")).read()
    plain = hdr[hdr.index("The sequence the context owns"):hdr.index("typedef struct pagk_sequence_params")]
    scope = " ".join(plain[plain.index("Out of scope:"):].replace(" * ", " ").split())
    assert "in both forms: k cameras batched, sharding, tracker type GYRO_PREDICT, the C++ shell classes." in scope
    assert "Out of scope: raw-frame rectification" in plain and "One sequence per context." in plain
    sensor = hdr[hdr.index("The sensor form of the sequence: raw frames"):hdr.index("typedef struct pagk_sequence_sensor")]
    assert "PAGK_E_ARG on a sensor sequence" in sensor and "bit for bit" in sensor


def test_batched_kernels_take_the_camera_from_the_grid():
    src = open(os.path.join(CSRC, "pagk_group_kernel.h")).read()
    kernels = re.findall(r"__global__ void __launch_bounds__\((\d+)\) (k_group_\w+)\(const GroupRec \*__restrict__ table\)\n\{(.*?)\n\}", src, flags=re.S)
    assert sorted(k[1] for k in kernels) == sorted(
        ["k_group_gyro_predict", "k_group_post_filter", "k_group_fit_compact", "k_group_fit_hyp", "k_group_fit_refit",
         "k_group_scores_fit", "k_group_fit_select", "k_group_handover_fill", "k_group_handover_holes", "k_group_handover_keys"])
    for bound, name, body in kernels:
        assert "blockIdx.y" in body or "group_fit_args(table)" in body, name     # the camera is the grid's second dimension
        assert "_body(" in body and "__syncthreads" not in body and "return" not in body, name   # nothing but its camera's own body
    host = open(os.path.join(CSRC, "pagk_hip.hip")).read()
    for bound, name, _ in kernels:
        single = {"k_group_scores_fit": "k_geometry_scores_fit"}.get(name, name.replace("k_group_", "k_"))
        block = re.search(r"hipLaunchKernelGGL\(" + single + r", dim3\(.*?\), dim3\((\d+)\)", host)
        assert block and block.group(1) == bound, name                              # the workgroup of the camera's own launch
        assert re.search(r"hipLaunchKernelGGL\(" + name + r", dim3\([^;]*?, kk\), dim3\(" + bound + r"\)", host), name
    assert 'reserve(lead, lead->buf[pagk_ctx::GROUP]' in host                       # the table is a library buffer like every other
