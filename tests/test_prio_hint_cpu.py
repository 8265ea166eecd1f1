"""The hint of csrc/pagk_prio.h without a GPU: the fluid model's hint mode on a case small enough to work out by hand, and the parsing of
PAGK_PRIO_HINT."""

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import prio_fluid_model as fm  # noqa: E402


HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pixel_aware_gyro_aided_klt_feature_tracker_amd", "csrc")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """csrc/pagk_prio_env.h compiled by itself (the parser the library applies to PAGK_PRIO_HINT in pagk_create)."""
    so = str(tmp_path_factory.mktemp("prio_hint") / "prio_hint_probe.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-o", so,
                    os.path.join(HERE, "prio_hint_probe.cpp")], check=True)
    lib = C.CDLL(so)
    lib.prio_hint_parse_probe.restype = C.c_int
    lib.prio_hint_parse_probe.argtypes = [C.c_char_p, C.c_int]
    lib.prio_hint_default_probe.restype = C.c_int
    return lib


def test_fluid_model_hint_mode_on_eight_workgroups():
    # Two CUs, four slots each, one pyramid level: workgroup i runs on CU i mod 2.  CU 0 holds workgroup 0 with 12 iterations and three
    # with 2; CU 1 holds four with 2.  In the model's units a workgroup needs SETUP + iterations * LONE cycles of its own, runs them at
    # full speed while it has U = SHARE / LONE of the CU's VALU, and four equals get a quarter each: speed 0.25 / U.
    it = np.array([[12], [2], [2], [2], [2], [2], [2], [2]])
    hint = it.sum(1)
    us = lambda cycles: cycles / (fm.GHZ * 1e3)   # noqa: E731
    short, long_ = fm.SETUP + 2 * fm.LONE, fm.SETUP + 12 * fm.LONE
    # no hint (K = 4 is never reached before the short ones end: 3 > 4 is false): everybody crawls until the short ones are done, after
    # which workgroup 0 -- as far along as they were -- runs its other ten iterations alone
    crowded = short / (0.25 / fm.U)
    want_off = us(crowded + 10 * fm.LONE)
    # hinted: workgroup 0 outranks its three mates from the start and is never slowed down
    want_on = us(long_)
    step = us(100.0)   # the model's time step
    off = fm.simulate(it, fm.behind(4), slots=4, ncu=2)
    assert abs(off - want_off) <= 3 * step, (off, want_off)
    on = fm.simulate(it, fm.behind(4), slots=4, ncu=2, hint=hint, T=4)
    assert abs(on - want_on) <= 3 * step, (on, want_on)
    assert on < off - 3.0
    # a threshold nobody exceeds, and the switch: the K rule alone
    assert fm.simulate(it, fm.behind(4), slots=4, ncu=2, hint=hint, T=12) == off
    assert fm.simulate(it, fm.behind(4), slots=4, ncu=2, hint=hint, T=0) == off
    # everybody boosted is nobody boosted
    assert fm.simulate(it, fm.behind(4), slots=4, ncu=2, hint=hint, T=1) == off
    # a wrong hint: a short mate of the straggler is boosted instead and ends sooner, the other three share what it leaves.  The CU
    # hands out the same VALU time in total, so the three short ones are through at the same moment as without a hint and the
    # straggler ends where it ended then: nothing gained, nothing lost
    wrong = np.array([2, 2, 12, 2, 2, 2, 2, 2])
    assert abs(fm.simulate(it, fm.behind(4), slots=4, ncu=2, hint=wrong, T=4) - off) <= 3 * step
    assert fm.boosted_per_cu(hint, 4, slots=4, ncu=2) == (0.5, 0)
    assert fm.boosted_per_cu(hint, 1, slots=4, ncu=2) == (4.0, 2)
    assert fm.boosted_per_cu(hint, 0, slots=4, ncu=2) == (0.0, 0)
    assert fm.flagged_share(wrong, hint, 4, share=0.125) == 0.0 and fm.flagged_share(hint, hint, 4, share=0.125) == 1.0


@pytest.mark.parametrize("text,want", [("0", 0), ("1", 1), ("14", 14), ("007", 7), ("1000000", 1000000),
                                       ("", -5), ("-1", -5), ("+3", -5), (" 3", -5), ("3 ", -5), ("auto", -5), ("1e3", -5), ("12x", -5),
                                       ("1000001", -5), ("99999999999999999999", -5)])
def test_the_environment_knob_parses_whole_numbers_only(probe, text, want):
    # a mistyped PAGK_PRIO_HINT leaves the default (here: the fallback -5) in place instead of switching the hint off
    assert probe.prio_hint_parse_probe(text.encode(), -5) == want


def test_the_default_threshold_is_the_models_choice(probe):
    # profiles/prio_hint/fluid_model.log, DESIGN.md section 4.4
    assert probe.prio_hint_default_probe() == 14
