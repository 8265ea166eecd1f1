"""CPU tests of the sensor form of the sequence group (pagk_sequence_group_*_sensor): the ranges
pagk_sequence_group_sensor_check accepts, every new call on a NULL lead or a NULL list, the header rules of the four
declarations and the place and the words of their section, the shape of the batched kernels' header
(csrc/pagk_group_sensor_kernel.h), and -- from the CPU model alone, with no call into the library -- that the rigs of
tests/group_sensor_cases.py show what the GPU tests need them to show."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import group_sensor_cases as gc
import sequence_cases as sc
import sequence_model as sm
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pixel_aware_gyro_aided_klt_feature_tracker_amd", "csrc")
ENTRY_POINTS = ("pagk_sequence_group_sensor_check", "pagk_sequence_group_create_sensor", "pagk_sequence_group_start_sensor",
                "pagk_sequence_group_step_sensor")
E = capi.PAGK_E_ARG


# ---- check and exports -------------------------------------------------------------------------------------------------------
def test_group_sensor_check_ranges(built):
    ok, sensor = capi.sequence_params_default, capi.sequence_sensor_default
    rgb = dict(rectify=capi.rectify_params_default(channels=3), raw=1, src_width=173, src_height=131)
    for detector in (0, 2):
        for validate in (0, 1):
            for gyro in (False, True):
                for raw in (0, 1):
                    for flow in (0, 1):
                        p = ok(detector=detector, validate=validate, track=capi.make_params(has_gyro=gyro))
                        s = sensor(flow_velocity=flow, **(rgb if raw else {}))
                        assert capi.sequence_group_sensor_check(p, s) == capi.PAGK_OK, (detector, validate, gyro, raw, flow)
    s = sensor()
    # what a sensor sequence accepts and the sensor group refuses: the Harris detector, Lucas-Kanade
    for kw in (dict(detector=1), dict(tracker=capi.SEQ_LK), dict(tracker=capi.SEQ_LK, lk_initial_flow=1),
               dict(tracker=capi.SEQ_LK, detector=2)):
        p = ok(**kw)
        assert capi.sequence_params_check(p) == capi.PAGK_OK and capi.sequence_group_sensor_check(p, s) == E, kw
    # a bad sensor block, a bad parameter block, the nested check's code, NULL
    for kw in (dict(raw=2), dict(flow_velocity=2), dict(imu_cap=0), dict(imu_cap=capi.IMU_MAX_SAMPLES + 1), dict(raw=1),
               dict(rectify=capi.rectify_params_default(channels=3)), dict(Rbc=[float("nan")] * 9)):
        assert capi.sequence_group_sensor_check(ok(), sensor(**kw)) == E, kw
    for kw in (dict(detector=3), dict(validate=2), dict(width=13), dict(cand_cap=0)):
        assert capi.sequence_group_sensor_check(ok(**kw), s) == E, kw
    assert capi.sequence_group_sensor_check(ok(fast=capi.fast_params_default(n_levels=8)), s) == capi.PAGK_E_UNSUPPORTED
    lib = capi.load()
    assert lib.pagk_sequence_group_sensor_check(None, C.byref(s)) == E
    assert lib.pagk_sequence_group_sensor_check(C.byref(ok()), None) == E
    # the plain group's check stays what it was
    assert capi.sequence_group_check(ok(detector=2, cand_cap=0)) == E and capi.sequence_group_check(ok(tracker=capi.SEQ_LK)) == E
    assert capi.sequence_group_check(ok()) == capi.PAGK_OK


def test_every_new_call_refuses_a_null_lead_or_list(built):
    lib = capi.load()
    a = np.zeros(4096, np.float32).ctypes.data
    imgs = (capi.Image * 2)(capi.image_view(np.zeros((480, 640), np.uint8)), capi.image_view(np.zeros((480, 640), np.uint8)))
    wins = (capi.ImuWindow * 2)()
    times = (C.c_double * 2)(0.0, 0.0)
    lists = (C.c_void_p * 2)(a, a)
    counts = (C.c_int32 * 2)(4, 4)
    none = (C.c_void_p * 2)(None, None)
    assert lib.pagk_sequence_group_create_sensor(None, 2) == E
    assert lib.pagk_sequence_group_create_sensor(none, 2) == E          # a list without a lead
    assert lib.pagk_sequence_group_create_sensor(none, 0) == E
    assert lib.pagk_sequence_group_start_sensor(None, imgs, times, lists, counts) == E
    assert lib.pagk_sequence_group_step_sensor(None, imgs, wins, lists, counts, capi.SEQ_DIRECT) == E


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
    assert len(lib.pagk_sequence_group_step_sensor.argtypes) == 6 and len(lib.pagk_sequence_group_start_sensor.argtypes) == 5
    assert len(lib.pagk_sequence_group_sensor_check.argtypes) == 2
    # the section stands behind the plain group's and says what it lifts and what stays out
    title = "The sensor form of the sequence group: k raw frames and k IMU windows in"
    assert hdr.index("int pagk_sequence_group_status(") < hdr.index(title) < hdr.index("int pagk_sequence_group_sensor_check(")
    section = hdr[hdr.index(title):hdr.index("int pagk_sequence_group_sensor_check(")]
    flat = " ".join(section.replace(" * ", " ").split())
    for word in ("Examples/Demo/RealSenseD435i.cpp:202", "src/frame.cpp:81-87", "src/gyro_aided_tracker.cpp:511-587",
                 "src/frame.cpp:172-179", "it lifts two items", "sensor sequences and the FAST detector", "byte for byte",
                 "pagk_sequence_read_velocity", "its own skip word", "pagk_frame_set_device_batch", "pagk_track_device_batch",
                 "always, also when nothing predicts", "member by member", "one linear chain",
                 "What stays out: the Harris detector, Lucas-Kanade, cameras whose parameters differ"):
        assert word in flat, word
    # the plain group's section and check are what they were
    plain = hdr[hdr.index("The sequence group: k cameras stepped together"):hdr.index("int pagk_sequence_group_check")]
    assert "Out of scope of the group: Lucas-Kanade, the Harris and FAST detectors, sensor" in " ".join(plain.replace(" * ", " ").split())
    for meth in ("start", "step", "read", "read_pair", "read_velocity", "close"):
        assert callable(getattr(runtime.DeviceSequenceGroup, meth)), meth
    for meth in ("start_sensor", "step_sensor", "status", "destroy"):
        assert callable(getattr(capi.SequenceGroup, meth)), meth
    assert callable(capi.sequence_group_sensor_check)


# ---- kernel shape -------------------------------------------------------------------------------------------------------------
RIG_KERNELS = {   # batched kernel -> (the single-camera kernel, its body)
    "k_rig_rectify": ("k_rectify", "rectify_body"), "k_rig_gyro_integrate": ("k_gyro_integrate", "gyro_integrate_body"),
    "k_rig_handover_plan": ("k_handover_plan", "handover_plan_body"), "k_rig_fast_cells": ("k_fast_cells", "fast_cells_body"),
    "k_rig_fast_offsets": ("k_fast_offsets", "fast_offsets_body"), "k_rig_fast_gather": ("k_fast_gather", "fast_gather_body"),
    "k_rig_fast_tree": ("k_fast_tree", "fast_tree_body"), "k_rig_flow_velocity": ("k_flow_velocity", "flow_velocity_body"),
}


def test_batched_kernels_take_the_camera_from_the_grid():
    src = open(os.path.join(CSRC, "pagk_group_sensor_kernel.h")).read()
    kernels = re.findall(r"__global__ void __launch_bounds__\((\d+)\) (k_\w+)\(const RigRec \*__restrict__ table\)\n\{(.*?)\n\}", src,
                         flags=re.S)
    assert sorted(k[1] for k in kernels) == sorted(RIG_KERNELS) and src.count("__global__") == len(RIG_KERNELS)
    assert not re.search(r"\bk_group_\w+", re.sub(r"//.*", "", src)) and "struct RigRec" in src   # a prefix and a record of their own
    host = open(os.path.join(CSRC, "pagk_hip.hip")).read()
    every = "".join(open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith(".h"))
    for bound, name, body in kernels:
        single, fn = RIG_KERNELS[name]
        assert "group_global(table)[blockIdx.y]" in body, name                      # the camera is the grid's second dimension
        assert body.count("_body") == 1 and fn in body, name                        # nothing but its camera's own body
        assert "__syncthreads" not in body and "blockIdx.x" not in body and not re.search(r"\b(return|if|for|while)\b", body), name
        # the single-camera kernel is the body's other caller, with the same workgroup
        assert re.search(r"__launch_bounds__\(" + bound + r"\)\s+(?:void )?" + single + r"\([^)]*\)\s*\{\s*" + fn + r"\b[^}]*\}", every), name
        if name == "k_rig_rectify":
            assert re.search(r"hipLaunchKernelGGL\(\(k_rectify<1, true>\), grd, blk,", host) and "blk(256)" in host
            assert host.count("k_rig_rectify<") == 6 and re.search(r"const dim3 grd\(\(unsigned\)\(\(threads \+ 255\) / 256\), kk\), blk\(256\);", host)
            continue
        block = re.search(r"hipLaunchKernelGGL\(" + single + r", dim3\(.*?\), dim3\((\d+)\)", host)
        assert block and block.group(1) == bound, name
        assert re.search(r"hipLaunchKernelGGL\(" + name + r", dim3\([^;]*?, kk\), dim3\(" + bound + r"\)", host), name
    # the ten kernels of the plain group are reused as they are, the second table is a library buffer like every other
    group = open(os.path.join(CSRC, "pagk_group_kernel.h")).read()
    assert len(re.findall(r"__global__ void __launch_bounds__\(\d+\) k_group_\w+\(const GroupRec \*__restrict__ table\)", group)) == 10
    assert "reserve(lead, lead->buf[pagk_ctx::GROUP_SENSOR]" in host and "pagk_ctx::GROUP_SENSOR})" in host


# ---- non-vacuity, from the CPU model alone -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    return sm.build_refs(tmp_path_factory.mktemp("group_sensor_refs"))


def test_rig_a_is_ragged(refs):
    rig = gc.rig_a()
    frames = [gc.model(refs, rig, j) for j in range(rig["k"])]
    words = [sc.words(f) for f in frames]
    runs = [gc.top_up_runs(f, rig["cfg"]) for f in frames]
    print("state words per camera and frame:", words)
    print("info[0] per camera and frame:", [[int(f["info"][0]) for f in fr] for fr in frames])
    print("the top-up runs:", runs)
    # one frame in which the top-up runs for one camera and is skipped for another
    assert any(len({r[k] for r in runs}) == 2 for k in range(1, gc.NF))
    for j in (0, 1):   # every camera that is not gray gains FAST keys: the detector's list reaches the hand-over
        assert any(w[3] > 0 and int(f["info"][0]) > 0 for w, f in zip(words[j][1:], frames[j][1:])), j
    # camera 2 loses everything at its gray frame, where FAST finds nothing, and is refilled by the next one
    assert words[2][3][0] == 0 and words[2][3][2] == 0 and int(frames[2][3]["info"][0]) == 0
    assert words[2][4][2] == 0 and words[2][4][3] > 0 and words[2][4][0] == rig["cfg"]["target_n"]
    # camera 1 differs from camera 0 in what its record carries, and in its results
    assert not np.array_equal(rig["cameras"][0]["rbc"], rig["cameras"][1]["rbc"])
    assert frames[0][1]["keys"].tobytes() != frames[1][1]["keys"].tobytes()
    assert any(f["velocity"].any() for f in frames[1][1:])


@pytest.mark.parametrize("switches", [0, 1])
def test_rig_b_has_a_sparse_camera_and_two_blocks(refs, switches):
    rig = gc.rig_b(switches)
    full, sparse = (sc.words(gc.model(refs, rig, j)) for j in range(2))
    print("state words:", full, sparse)
    assert rig["cfg"]["cap"] > 256 and full[0][0] > 256                             # rows in the second block of 256 are live
    assert all(f[0] != s[0] for f, s in zip(full[1:], sparse[1:]))
    assert all(f[2] > 8 for f in full[1:]), "the full camera tracks"
