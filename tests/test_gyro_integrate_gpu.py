"""GPU tests of pagk_gyro_integrate (kernel k_gyro_integrate, include/pagk.h "Gyro integration") against the plain-C
restatement tests/gyro_integrate_ref.c, byte for byte, on the whole edge table of tests/gyro_integrate_ref_util.py: Rcl and
rot9; independence of what the context's workspaces held; the refusals, none of which reaches the device."""
import numpy as np
import pytest

import gyro_integrate_ref_util as gu
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, host_api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return gu.build_ref(tmp_path_factory.mktemp("gyro_integrate_ref"))


@pytest.fixture(scope="module")
def table():
    return gu.edge_table()


@pytest.fixture(scope="module")
def restated(ref, table):
    return {name: gu.ref_integrate(ref, c) for name, c in table.items()}


def _device(c, case):
    cam = capi.make_params()
    cam.fx, cam.fy, cam.cx, cam.cy = case["camera"]
    win, keep = capi.imu_window(case["t_ref"], case["t_cur"], case["t"], case["w"], case["bias"])
    return c.gyro_integrate(case["Rbc"], cam, win)


def test_kernel_equals_the_restatement_on_the_edge_table(ctx, table, restated):
    for name, case in table.items():
        rcl, rot9 = _device(ctx, case)
        assert rcl.tobytes() == restated[name][0].tobytes(), (name, rcl, restated[name][0])
        assert rot9.tobytes() == restated[name][1].tobytes(), (name, rot9, restated[name][1])


def test_result_does_not_depend_on_what_the_workspaces_held(table, restated):
    for word in (0x00000001, 0xffc0ffc0):
        c = capi.Context(0)
        try:
            c.selftest_fill_workspaces(word, True)
            for name in ("64 samples", "Rbc not I, bias, 64", "2 samples", "0 samples", "d below 1e-4"):
                rcl, rot9 = _device(c, table[name])
                assert rcl.tobytes() == restated[name][0].tobytes() and rot9.tobytes() == restated[name][1].tobytes(), (word, name)
        finally:
            c.close()


def test_host_api_and_refusals(ctx, table, restated):
    case = table["Rbc not I"]
    fx, fy, cx, cy = case["camera"]
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    out = host_api.gyro_integrate(case["Rbc"], K, case["t_ref"], case["t_cur"], case["t"], case["w"], case["bias"], ctx=ctx)
    assert out["Rcl"].tobytes() == restated["Rbc not I"][0].tobytes() and out["rot9"].tobytes() == restated["Rbc not I"][1].tobytes()
    for name, (bad, cap) in gu.refused_windows().items():
        if cap != 64:
            continue                                             # (the host form's imu_cap is PAGK_IMU_MAX_SAMPLES)
        with pytest.raises(capi.PagkError) as e:
            _device(ctx, bad)
        assert e.value.code == capi.PAGK_E_ARG, name
    rcl, rot9 = _device(ctx, case)                               # ... and the context works on
    assert rcl.tobytes() == restated["Rbc not I"][0].tobytes()
