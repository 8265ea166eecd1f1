"""The dispatch order of the 4-wave kernels without a GPU (csrc/pagk_order.h): the ordering rule the device build and
pagk_dispatch_order_get promise, restated here in numpy, and the conservative rule by which a launch is handed the array."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pixel_aware_gyro_aided_klt_feature_tracker_amd", "csrc")

INT32_MAX, INT32_MIN = 2**31 - 1, -2**31


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("dispatch_order") / "dispatch_order_probe.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, "-o", so,
                    os.path.join(HERE, "dispatch_order_probe.cpp")], check=True)
    lib = C.CDLL(so)
    lib.order_serves_probe.argtypes = [C.c_longlong, C.c_int]
    lib.order_reference_probe.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    lib.order_reference_probe.restype = None
    lib.order_state_probe.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    lib.order_state_probe.restype = None
    return lib


def reference(lib, hints):
    h = np.ascontiguousarray(hints, np.int32)
    out = np.full(h.shape[0], -1, np.int32)
    lib.order_reference_probe(h.shape[0], h.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out


def restated(hints, key_max):
    """The rule in one line: sort by clamped key, descending, stable."""
    keys = np.clip(np.asarray(hints, np.int64), 0, key_max)
    return np.argsort(-keys, kind="stable").astype(np.int32)


def test_keys_are_clamped_into_a_fixed_range(probe):
    kmax = probe.order_key_max_probe()
    assert kmax == 127   # 30 iterations on each of four levels (120) is still its own class
    for hint, want in ((0, 0), (1, 1), (26, 26), (kmax, kmax), (kmax + 1, kmax), (1000, kmax), (INT32_MAX, kmax), (-1, 0), (INT32_MIN, 0)):
        assert probe.order_key_probe(hint) == want, hint


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 300, 700, 1000, 4097])
def test_stable_descending_order(probe, n):
    kmax = probe.order_key_max_probe()
    rng = np.random.default_rng(n)
    sets = {
        "zero": np.zeros(n, np.int32),                       # no forecast: the identity
        "equal": np.full(n, 17, np.int32),
        "iteration counts": rng.integers(0, 91, n).astype(np.int32),
        "few classes": rng.integers(9, 12, n).astype(np.int32),   # long runs of ties
        "any int32": rng.integers(INT32_MIN, INT32_MAX, n, endpoint=True).astype(np.int32),
        "ascending": np.arange(n, dtype=np.int32) % (kmax + 1),
    }
    sets["any int32"][::7] = INT32_MAX
    sets["any int32"][3::11] = -5
    for what, hints in sets.items():
        got = reference(probe, hints)
        assert np.array_equal(np.sort(got), np.arange(n)), f"{what}: not a permutation of [0, {n})"
        assert np.array_equal(got, restated(hints, kmax)), what
    assert np.array_equal(reference(probe, sets["zero"]), np.arange(n))
    assert np.array_equal(reference(probe, sets["equal"]), np.arange(n))


def test_ties_keep_index_order_and_clamped_keys_tie(probe):
    hints = np.array([5, 9, 5, 200, 9, -3, 0, INT32_MAX, 127, 128, 5], np.int32)
    # 200, INT32_MAX, 127 and 128 all clamp to 127 and keep their index order; -3 and 0 tie at the end
    assert reference(probe, hints).tolist() == [3, 7, 8, 9, 1, 4, 0, 2, 10, 5, 6]
    assert reference(probe, np.array([4], np.int32)).tolist() == [0]


def test_which_launches_the_order_serves(probe):
    top = probe.order_max_n_probe()
    assert top >= 6000   # the 4-wave kernels are selected up to ~6000 features
    for n, want in ((0, 0), (1, 0), (256, 0), (257, 1), (1000, 1), (top, 1), (top + 1, 0)):
        assert probe.order_serves_probe(n, 256) == want, n
    assert probe.order_serves_probe(300, 304) == 0 and probe.order_serves_probe(305, 304) == 1


BUILD, BUILD_GRAPH, BUILD_FOREIGN, LAUNCH, CLEAR, SET, IDLE, GRAPHS_GONE, USABLE, SWITCH, CAPTURE_END, REPLAY, REPLACED = range(13)
BIG = 1 << 20   # both arrays hold this many slots


def run(lib, script):
    s = np.ascontiguousarray(script, np.int32).reshape(-1, 4)
    out = np.zeros(s.shape[0], np.int32)
    lib.order_state_probe(s.shape[0], s.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out.tolist()


def test_a_launch_gets_the_order_only_behind_a_build_for_its_n_on_its_stream(probe):
    A, B = 0, 1
    # nothing is built before a hinted launch has said how many features there are; then pyramid -> track, step after step
    assert run(probe, [(BUILD, 0, A, BIG), (LAUNCH, 1000, A, 0), (BUILD, 0, A, BIG), (LAUNCH, 1000, A, 0),
                       (LAUNCH, 1000, A, 0),                       # two launches, one build: the second reads fresher hints than the order
                       (BUILD, 0, A, BIG), (LAUNCH, 1000, A, 0)]) == [0, 0, 1000, 1, 0, 1000, 1]
    # another n than the build's: identity, and the next build is for the new n
    assert run(probe, [(LAUNCH, 1000, A, 0), (BUILD, 0, A, BIG), (LAUNCH, 700, A, 0), (BUILD, 0, A, BIG), (LAUNCH, 700, A, 0)]) \
        == [0, 1000, 0, 700, 1]
    # a workgroup per CU or fewer, or more than the builder holds: never
    top = probe.order_max_n_probe()
    assert run(probe, [(LAUNCH, 256, A, 0), (BUILD, 0, A, BIG), (LAUNCH, 256, A, 0)]) == [0, 0, 0]
    assert run(probe, [(LAUNCH, top + 1, A, 0), (BUILD, 0, A, BIG), (LAUNCH, top + 1, A, 0)]) == [0, 0, 0]
    # an array that could not grow (under a live graph): no build, identity
    assert run(probe, [(LAUNCH, 1000, A, 0), (BUILD, 0, A, 999), (LAUNCH, 1000, A, 0)]) == [0, 0, 0]
    # a build on another stream than the launch's (a prefetched pyramid): identity
    assert run(probe, [(LAUNCH, 1000, A, 0), (BUILD, 0, B, BIG), (LAUNCH, 1000, A, 0)]) == [0, 1000, 0]
    # the switch
    assert run(probe, [(SWITCH, 0, 0, 0), (LAUNCH, 1000, A, 0), (BUILD, 0, A, BIG), (LAUNCH, 1000, A, 0)]) == [0, 0, 0, 0]


def test_clearing_or_writing_the_hints_retires_the_build(probe):
    A = 0
    # cleared behind the build (new features; a host-buffer call): identity, and nothing to sort until a launch has run again
    assert run(probe, [(LAUNCH, 1000, A, 0), (BUILD, 0, A, BIG), (CLEAR, 0, 0, 0), (USABLE, 1000, A, 0), (LAUNCH, 1000, A, 0),
                       (CLEAR, 0, 0, 0), (BUILD, 0, A, BIG), (LAUNCH, 1000, A, 0), (BUILD, 0, A, BIG), (LAUNCH, 1000, A, 0)]) \
        == [0, 1000, 0, 0, 0, 0, 0, 0, 1000, 1]
    # hints installed by the caller: the old build is history, the next pyramid launch sorts the new ones
    assert run(probe, [(LAUNCH, 1000, A, 0), (BUILD, 0, A, BIG), (SET, 700, 0, 0), (USABLE, 1000, A, 0), (USABLE, 700, A, 0),
                       (BUILD, 0, A, BIG), (USABLE, 700, A, 0), (LAUNCH, 700, A, 0)]) == [0, 1000, 0, 0, 0, 700, 1, 1]


def test_the_array_is_bound_to_one_stream_until_the_host_has_waited_for_it(probe):
    A, B = 0, 1
    head = [(LAUNCH, 1000, A, 0), (BUILD, 0, A, BIG), (LAUNCH, 1000, A, 0)]   # the last launch on A reads the array
    assert run(probe, head + [(BUILD, 0, B, BIG)]) == [0, 1000, 1, 0]         # ... so a pyramid on B does not rebuild it
    assert run(probe, head + [(BUILD, 0, A, BIG)]) == [0, 1000, 1, 1000]      # on A, stream order separates them
    assert run(probe, head + [(IDLE, 0, B, 0), (BUILD, 0, B, BIG)]) == [0, 1000, 1, 0, 0]
    assert run(probe, head + [(IDLE, 0, A, 0), (BUILD, 0, B, BIG), (LAUNCH, 1000, B, 0)]) == [0, 1000, 1, 0, 1000, 1]   # the host waited for A
    # a BUILD binds the array too: one enqueued on B (and, say, stalled behind an event) keeps A from building and from reading, so it
    # cannot land under a launch on A; waiting for A changes nothing, waiting for B frees the array
    stalled = [(LAUNCH, 1000, A, 0), (BUILD, 0, B, BIG)]
    assert run(probe, stalled + [(BUILD, 0, A, BIG), (LAUNCH, 1000, A, 0)]) == [0, 1000, 0, 0]
    assert run(probe, stalled + [(IDLE, 0, A, 0), (BUILD, 0, A, BIG), (LAUNCH, 1000, A, 0)]) == [0, 1000, 0, 0, 0]
    assert run(probe, stalled + [(IDLE, 0, B, 0), (BUILD, 0, A, BIG), (LAUNCH, 1000, A, 0)]) == [0, 1000, 0, 1000, 1]
    # a new buffer holds nothing built
    assert run(probe, [(LAUNCH, 1000, A, 0), (BUILD, 0, A, BIG), (REPLACED, 0, 0, 0), (LAUNCH, 1000, A, 0)]) == [0, 1000, 0, 0]


def test_a_replayed_graph_binds_the_array_to_the_stream_it_runs_on(probe):
    A, B = 0, 1
    # captured [pyramid + build -> launch] on A: recording binds nothing and leaves no build behind ...
    cap = [(LAUNCH, 1000, A, 0), (BUILD_GRAPH, 0, A, BIG), (LAUNCH, 1000, A, 1), (CAPTURE_END, 0, 0, 0)]
    assert run(probe, cap) == [0, 1000, 1, 1]
    assert run(probe, cap + [(USABLE, 1000, A, 0), (BUILD, 0, B, BIG)]) == [0, 1000, 1, 1, 0, 1000]
    # ... the replay does: the host waits for A (a sync), replays on A, switches to B and builds a pyramid there -- no order workgroup,
    # the replay's tracking node may be reading the array
    seq = cap + [(IDLE, 0, A, 0), (REPLAY, 0, A, 0), (BUILD, 0, B, BIG), (LAUNCH, 1000, B, 0)]
    assert run(probe, seq) == [0, 1000, 1, 1, 0, 0, 0, 0]
    # after waiting for A it may
    assert run(probe, seq + [(IDLE, 0, A, 0), (BUILD, 0, B, BIG), (LAUNCH, 1000, B, 0)]) == [0, 1000, 1, 1, 0, 0, 0, 0, 0, 1000, 1]
    # a replay on another stream than the one the array is bound to must wait for the device first, and rebinds it
    assert run(probe, cap + [(REPLAY, 0, A, 0), (REPLAY, 0, A, 0), (REPLAY, 0, B, 0), (REPLAY, 0, B, 0), (BUILD, 0, A, BIG)]) \
        == [0, 1000, 1, 1, 0, 0, 1, 0, 0]
    assert run(probe, [(LAUNCH, 1000, A, 0), (BUILD, 0, A, BIG), (LAUNCH, 1000, A, 1), (CAPTURE_END, 0, 0, 0), (REPLAY, 0, B, 0)]) \
        == [0, 1000, 1, 1, 1]   # (a direct build on A, a captured reader, replayed on B)
    # a build that was only recorded has not run: the direct launch behind the capture runs in index order
    assert run(probe, [(LAUNCH, 1000, A, 0), (BUILD_GRAPH, 0, A, BIG), (CAPTURE_END, 0, 0, 0), (LAUNCH, 1000, A, 0)]) == [0, 1000, 1, 0]
    # a capture that recorded neither says so
    assert run(probe, [(LAUNCH, 200, A, 1), (CAPTURE_END, 0, 0, 0)]) == [0, 0]


def test_a_live_graph_freezes_the_n_the_array_is_built_for(probe):
    A = 0
    # captured [pyramid + build -> launch] for 1000 features; afterwards direct launches of 700
    cap = [(LAUNCH, 1000, A, 0), (BUILD_GRAPH, 0, A, BIG), (LAUNCH, 1000, A, 1), (CAPTURE_END, 0, 0, 0)]
    assert run(probe, cap + [(LAUNCH, 700, A, 0), (BUILD, 0, A, BIG), (LAUNCH, 700, A, 0)]) == [0, 1000, 1, 1, 0, 0, 0]
    # ... 1000 again is fine; and once the graphs are gone, so is any n
    assert run(probe, cap + [(LAUNCH, 1000, A, 0), (BUILD, 0, A, BIG), (LAUNCH, 1000, A, 0)]) == [0, 1000, 1, 1, 0, 1000, 1]
    assert run(probe, cap + [(GRAPHS_GONE, 0, 0, 0), (LAUNCH, 700, A, 0), (BUILD, 0, A, BIG), (LAUNCH, 700, A, 0)]) \
        == [0, 1000, 1, 1, 0, 0, 700, 1]
    # a capture that is not the context's own: nobody reports its graph's replays or its end, so it neither builds nor reads
    assert run(probe, [(LAUNCH, 1000, A, 0), (BUILD_FOREIGN, 0, A, BIG), (LAUNCH, 1000, A, 2)]) == [0, 0, 0]
    assert run(probe, [(LAUNCH, 1000, A, 0), (BUILD, 0, A, BIG), (LAUNCH, 1000, A, 2)]) == [0, 1000, 0]
