"""CPU tests of the result ring of a sequence (include/pagk.h "The result ring of a sequence"): the layout of a record, the
ranges and NULL arguments of every new entry point that needs no device, the header rules of the four declarations, the numpy
model of the track ids (tests/results_model.py) against a hand-written example and against the plain-C restatement
(tests/results_ref.c), that restatement and the layout function under AddressSanitizer and UBSan in a stand-alone program, and
-- from the CPU model alone -- that the rows of tests/results_cases.py show what the GPU tests need them to show."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import results_cases as rcs
import results_model as rm
import sequence_cases as sc
import sequence_model as sm
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pixel_aware_gyro_aided_klt_feature_tracker_amd", "csrc")
ENTRY_POINTS = ("pagk_sequence_results_layout", "pagk_sequence_results_create", "pagk_sequence_fetch", "pagk_sequence_poll")
E = capi.PAGK_E_ARG
# part -> bytes per row (None: a fixed part of 256 bytes), in the documented order
PARTS = (("header", None), ("state", None), ("info", None), ("keys", 8), ("keys_un", 8), ("keys_normal", 8), ("index_in_last", 4),
         ("live", 1), ("track_id", 8), ("age", 4), ("velocity", 8), ("status", 1), ("pt_predict", 8), ("pt_predict_un", 8), ("err", 4))


# ---- the layout ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", rcs.LAYOUT_CAPS)
def test_layout(built, cap):
    assert tuple(name for name, _ in PARTS) == capi.RESULTS_PARTS
    plain, sensor = capi.sequence_results_layout(cap, 0), capi.sequence_results_layout(cap, 1)
    end = 0
    for name, row in PARTS:
        off = getattr(plain, name)
        assert off == end and off % 256 == 0, name                  # in the documented order, disjoint, aligned
        assert getattr(sensor, name) == off, name                   # the sensor flag moves nothing
        size = 32 if row is None else cap * row
        end = off + (size + 255) // 256 * 256
    assert plain.bytes == sensor.bytes == end                       # the last offset plus the last part, rounded up
    assert (plain.cap, plain.sensor, sensor.sensor) == (cap, 0, 1)


def test_layout_ranges_and_null(built):
    lib = capi.load()
    lay = capi.ResultsLayout()
    for cap in (0, -1, (1 << 24) + 1):
        assert lib.pagk_sequence_results_layout(cap, 0, C.byref(lay)) == E, cap
    for sensor in (-1, 2):
        assert lib.pagk_sequence_results_layout(4, sensor, C.byref(lay)) == E, sensor
    assert lib.pagk_sequence_results_layout(4, 0, None) == E
    assert lib.pagk_sequence_results_layout(1 << 24, 1, C.byref(lay)) == capi.PAGK_OK
    assert lay.bytes == (1 << 24) * sum(row or 0 for _, row in PARTS) + 3 * 256          # 70 bytes per row and the three fixed parts
    with pytest.raises(ValueError):
        capi.sequence_results_layout(0)


def test_every_new_call_refuses_a_null_context(built):
    lib = capi.load()
    r = capi.SequenceResult()
    assert lib.pagk_sequence_results_create(None, 4) == E
    assert lib.pagk_sequence_fetch(None, 0, C.byref(r)) == E
    assert lib.pagk_sequence_poll(None, 0) == E


def test_struct_layout_matches_a_c_probe(built, tmp_path):
    fields = {"pagk_results_layout": capi.ResultsLayout, "pagk_sequence_result": capi.SequenceResult}
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pagk.h"\nint main(void) {\n' + "".join(
        f'    printf("%zu\\n", sizeof({t}));\n' + "".join(f'    printf("%zu\\n", offsetof({t}, {f}));\n' for f, _ in cls._fields_)
        for t, cls in fields.items()) + "    return 0;\n}\n")
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    lines = iter(subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split())
    for t, cls in fields.items():
        assert int(next(lines)) == C.sizeof(cls), t
        for f, _ in cls._fields_:
            assert int(next(lines)) == getattr(cls, f).offset, (t, f)


# ---- the header ---------------------------------------------------------------------------------------------------------------
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
        # the reference's lines, or the plain statement that it has none
        assert comment.rstrip().endswith("*/") and "no counterpart" in comment and "Examples/Demo/RealSenseD435i.cpp:" in comment, name
        assert not re.search(r"device\s+pointer", comment), name
    assert [len(getattr(lib, n).argtypes) for n in ENTRY_POINTS] == [3, 2, 3, 2]
    # the section stands behind the sensor group's and carries the definition of the ids
    title = "The result ring of a sequence"
    assert hdr.index("int pagk_sequence_group_step_sensor(") < hdr.index(title) < hdr.index("typedef struct pagk_results_layout")
    section = hdr[hdr.index(title):hdr.index("typedef struct pagk_results_layout")]
    flat = " ".join(section.replace(" * ", " ").split())
    for word in ("no counterpart", "mvPtIndexInLastFrame", "src/frame.cpp:135,192", "include/frame.h:80", "At a start next_id = 0",
                 "track_id = -1, age = 0", "track_id = track_id_last[i], age = age_last[i] + 1", "next_id += n_new",
                 "new rows need not follow the survivors", "begins at 0 again and empties the ring", "Opt-in", "f % depth",
                 "byte for byte", "all zero for frame 0", "a third table the lead owns", "Out of scope: one contiguous record"):
        assert word in flat, word
    fetch = hdr[:hdr.index("int pagk_sequence_fetch(")].rsplit("/*", 1)[1]
    assert "stay valid until the call that hands in frame `frame + depth`" in " ".join(fetch.replace(" * ", " ").split())
    status = hdr[:hdr.index("int pagk_sequence_status(")].rsplit("/*", 1)[1]
    assert "[3] the depth of the result" in status
    for meth in ("sequence_results_create", "sequence_fetch", "sequence_poll"):
        assert callable(getattr(capi.Context, meth)), meth
    for cls in (runtime.DeviceSequence, runtime.DeviceSequenceGroup):
        assert callable(cls.fetch) and callable(cls.poll)


def test_the_pack_is_one_body_with_two_callers():
    src = open(os.path.join(CSRC, "pagk_results_kernel.h")).read()
    assert re.search(r"__device__ __forceinline__ void results_pack_body\(const ResultsArgs &a\)", src)
    kernels = re.findall(r"__global__ void __launch_bounds__\((\d+)\) (k_\w+)\(", src)
    assert kernels == [("1024", "k_results_pack"), ("1024", "k_group_results_pack")] and src.count("results_pack_body(a);") == 2
    body = src[src.index("void results_pack_body("):src.index("__global__")]
    assert "return" not in body                                          # no exit but the whole workgroup's, at the end
    assert "atomic" not in src and "while" not in body                  # no workgroup waits for another
    assert "group_global(table)[blockIdx.y]" in src
    host = open(os.path.join(CSRC, "pagk_hip.hip")).read()
    assert re.search(r"hipLaunchKernelGGL\(k_results_pack, dim3\(results_blocks\(q\.p\.cap\)\), dim3\(1024\)", host)
    assert re.search(r"hipLaunchKernelGGL\(k_group_results_pack, dim3\(results_blocks\(p\.cap\), kk\), dim3\(1024\)", host)
    assert "reserve(ctx, b, lay.total, NOT_IN_CAPTURE_NOR_UNDER_GRAPH, \"the result ring's block\"" in host
    assert "reserve(lead, lead->buf[pagk_ctx::GROUP_RESULTS]" in host
    assert "pagk_ctx::RESULTS, pagk_ctx::GROUP_RESULTS" in host[host.index("ctx->buf[pagk_ctx::FEAT].mirrored = true;"):][:400]   # state


# ---- the id rule --------------------------------------------------------------------------------------------------------------
EXAMPLE_LIVE = [3, 4, 2, 0, 5]
EXAMPLE_INDEX = [[-1] * 6,
                 [0, -1, 2, -1, -1, -1],          # a new row between two survivors, and one behind them
                 [-1] * 6,                        # no survivor
                 [-1] * 6,                        # no live row
                 [-1] * 6]
EXAMPLE_ID = [[0, 1, 2, -1, -1, -1], [0, 3, 2, 4, -1, -1], [5, 6, -1, -1, -1, -1], [-1] * 6, [7, 8, 9, 10, 11, -1]]
EXAMPLE_AGE = [[0] * 6, [1, 0, 1, 0, 0, 0], [0] * 6, [0] * 6, [0] * 6]
EXAMPLE_NEW, EXAMPLE_NEXT = [3, 2, 2, 0, 5], [3, 5, 7, 7, 12]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return rm.build_ref(tmp_path_factory.mktemp("results_ref"))


def _same_ids(a, b, what):
    for f, (x, y) in enumerate(zip(a, b)):
        assert x["track_id"].dtype == y["track_id"].dtype == np.int64 and x["age"].dtype == y["age"].dtype == np.int32
        assert x["track_id"].tobytes() == y["track_id"].tobytes() and x["age"].tobytes() == y["age"].tobytes(), (what, f)
        assert (x["n_new"], x["next_id"]) == (y["n_new"], y["next_id"]), (what, f)


def test_model_on_the_hand_written_example(ref):
    got = rm.ids(EXAMPLE_INDEX, EXAMPLE_LIVE)
    for f, g in enumerate(got):
        assert g["track_id"].tolist() == EXAMPLE_ID[f] and g["age"].tolist() == EXAMPLE_AGE[f], f
        assert (g["n_new"], g["next_id"]) == (EXAMPLE_NEW[f], EXAMPLE_NEXT[f]), f
    _same_ids(got, rm.ref_ids(ref, EXAMPLE_INDEX, EXAMPLE_LIVE), "example")
    # an age beyond one: a track that survives twice, through a row that moves
    got = rm.ids([[-1, -1, -1], [1, 0, -1], [-1, 1, 0]], [2, 3, 3])
    assert [g["track_id"].tolist() for g in got] == [[0, 1, -1], [1, 0, 2], [3, 0, 1]]
    assert [g["age"].tolist() for g in got] == [[0, 0, 0], [1, 1, 0], [0, 2, 2]]


def test_model_equals_the_restatement_on_seeded_runs(ref):
    rng = np.random.default_rng(0x5EED)
    for cap in (1, 4, 33, 70, 1025, 2200):
        nf = 6
        live = rng.integers(0, cap + 1, nf)
        live[3] = 0
        idx = np.full((nf, cap), -1, np.int32)
        for f in range(1, nf):
            if live[f - 1]:
                keep = rng.random(cap) < 0.7
                keep[live[f]:] = False
                idx[f, keep] = rng.integers(0, live[f - 1], int(keep.sum()))
        _same_ids(rm.ids(idx, live), rm.ref_ids(ref, idx, live), cap)


def test_restatement_and_layout_run_clean_under_the_sanitizers(built, tmp_path):
    """A stand-alone program (tests/results_sanitize.c: its own main, compiled together with tests/results_ref.c, linked against
    the library for pagk_sequence_results_layout, which needs no device) under AddressSanitizer and UBSan."""
    exe = str(tmp_path / "results_sanitize")
    pkg = capi.PKG_DIR
    subprocess.run(["gcc", "-std=c99", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "results_sanitize.c"), os.path.join(ROOT, "tests", "results_ref.c"), "-o", exe,
                    "-L", pkg, "-l:libpagk_hip.so", f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "6 runs clean" in r.stdout, r.stdout


# ---- non-vacuity, from the CPU model alone ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    return sm.build_refs(tmp_path_factory.mktemp("results_refs"))


def test_odd_gray3_loses_every_track_and_issues_larger_ids(refs, ref):
    scene = rcs.scene("odd-gray3")
    frames = sc.model(refs, scene)
    got = rm.ids_of_frames(frames)
    _same_ids(got, rm.ref_ids(ref, np.stack([f["index_in_last"] for f in frames]), [int(f["state"][0]) for f in frames]), "odd-gray3")
    print("state words:", sc.words(frames), "next_id:", [g["next_id"] for g in got])
    gray = scene["row"]["gray"]
    assert int(frames[gray]["state"][2]) == 0 and not (got[gray]["age"] > 0).any()        # no survivor at the gray frame
    before = max(int(g["track_id"].max()) for g in got[:gray])
    later = np.concatenate([g["track_id"][g["track_id"] >= 0] for g in got[gray:]])
    assert before >= 0 and later.size and int(later.min()) > before
    assert any((g["age"] > 1).any() for g in got[:gray])                                  # tracks that live for several frames


def test_three_chunks_refill_issues_ids_in_several_chunks(refs):
    scene = rcs.scene("three-chunks-refill")
    row = scene["row"]
    assert (row["width"], row["height"], row["half_patch"], row["levels"], row["cap"], row["target_n"], row["n_cand"], row["nf"],
            row["gray"]) == (320, 240, 5, 3, 2200, 2100, 3000, 4, 2)
    assert "three-chunks-refill" not in sc.TABLE
    frames = sc.model(refs, scene)
    got = rm.ids_of_frames(frames)
    print("state words:", sc.words(frames), "n_new:", [g["n_new"] for g in got], "next_id:", [g["next_id"] for g in got])
    hit = []
    for f in range(1, len(frames)):
        n = int(frames[f]["state"][0])
        fresh = np.nonzero(frames[f]["index_in_last"][:n] < 0)[0]
        if got[f - 1]["next_id"] > 0 and len(set((fresh // rcs.CHUNK).tolist())) >= 2:
            hit.append(f)
    assert hit, "no frame with next_id > 0 in front of it and new rows in two chunks of 1024 rows"
    # ... and a frame in which survivors and new rows share the key set, in front of it
    assert any(0 < g["n_new"] < int(f["state"][0]) for g, f in zip(got[1:], frames[1:]))
