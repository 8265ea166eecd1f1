"""csrc/pagk_layout.h: the block carver and the level workspace give the offsets the host code spelled out by hand
before the header existed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pixel_aware_gyro_aided_klt_feature_tracker_amd", "csrc")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("layout") / "layout_probe.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-o", so,
                    os.path.join(HERE, "layout_probe.cpp")], check=True)
    lib = C.CDLL(so)
    lib.layout_probe.restype = C.c_uint64
    lib.layout_probe.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.levels_probe.restype = None
    lib.levels_probe.argtypes = [C.c_uint64, C.c_uint64, C.c_int32, C.c_void_p]
    return lib


def up(v):
    return (v + 255) // 256 * 256


@pytest.mark.parametrize("sizes", [[0], [1], [255], [256], [257], [0, 1, 255, 256, 257, (1 << 32) + 5, 0, 3],
                                   [(1 << 32) + 257, 1], [257, 0, 0, 1], list(range(250, 266))])
def test_carver_matches_the_hand_written_loop(probe, sizes):
    want, total = [], 0
    for size in sizes:                      # the loop every carving site used to carry
        want.append(total)
        total = (total + size + 255) // 256 * 256
    off = np.zeros(len(sizes), np.uint64)
    got = probe.layout_probe(np.asarray(sizes, np.uint64).ctypes.data, len(sizes), off.ctypes.data)
    assert off.tolist() == want and got == total
    assert all(o % 256 == 0 for o in want)
    # ... and its other spelling, `off = total; total += align_up(size)`
    assert want == [sum(up(s) for s in sizes[:k]) for k in range(len(sizes))] and total == sum(up(s) for s in sizes)


@pytest.mark.parametrize("n, nq, pyramids", [(1, 1, 2), (67, 17, 3), (16000, 4000, 5)])
def test_levels_layout_matches_the_byte_arithmetic_of_the_launches(probe, n, nq, pyramids):
    # launch_track / pagk_track_device_batch before the header: 32768 B of counters, ready lists, a 256 B hand-over count,
    # the list, then 16 B of float state and a 32 B SuspState per feature, unpadded
    ready_bytes = up((pyramids - 1) * 8 * ((nq + 7) // 8) * 4)
    susp_zero = 256 + up(n * 4)
    sb = 32768 + ready_bytes
    want = [32768, sb, sb + 256, sb + susp_zero, sb + susp_zero + n * 16, sb + susp_zero + n * 16 + n * 32]
    got = np.zeros(6, np.uint64)
    probe.levels_probe(n, nq, pyramids, got.ctypes.data)
    assert got.tolist() == want
