"""The guard check checked, and the table of device entry points complete.  No GPU: Arena("cpu") through every kind of
planted error on the smallest arrays, and tests/device_forms.py against the declarations of include/pagk.h."""
import os
import re

import numpy as np
import pytest
import torch

import arena as ar
import device_forms as df

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pagk.h")
DT = {"f32": torch.float32, "f64": torch.float64, "u8": torch.uint8, "i32": torch.int32}


# ---- the arena ---------------------------------------------------------------------------------------------------------------
def _small(which="A"):
    a = ar.Arena("cpu", capacity=1 << 18, which=which)
    a.inp("pts", np.arange(6, dtype=np.float32).reshape(3, 2), "float")
    a.inp("flags", np.array([1, 0, 1], np.uint8), "byte")
    a.inp("count", np.array([3], np.int32), "index")
    a.out("res", torch.float64, (3,), "float")
    a.out("idx", torch.int32, (3,), "index")
    a.inout("state", np.array([0, 1, 0, 0], np.int32), "index")
    return a


def _poke(a, name, offset, value):
    """One byte at `offset` relative to array `name`."""
    e = a.entries[name]
    a.raw[a.base + e.off + offset] = value


@pytest.mark.parametrize("which", ["A", "B"])
def test_layout(which):
    a = _small(which)
    for name, e in a.entries.items():
        v = a.view(name)
        assert v.data_ptr() % 256 == 0, name
        assert v.numel() * v.element_size() == e.nbytes, name
        assert e.guard == 4096
    assert ar.guard_width(4097) == 8192 and ar.guard_width(0) == 4096 and ar.guard_width(4096) == 4096
    # no array's guard overlaps another array or its guards
    spans = sorted((e.off - e.guard, e.off + e.nbytes + e.guard) for e in a.entries.values())
    assert all(hi <= lo for (_, hi), (lo, _) in zip(spans, spans[1:]))
    assert a.damaged() == {} and a.inputs_unchanged() == []
    assert np.array_equal(a.payload("pts"), np.arange(6, dtype=np.float32).reshape(3, 2))
    assert a.payload("state").tolist() == [0, 1, 0, 0]


def test_empty_array_has_an_address():
    a = ar.Arena("cpu", capacity=1 << 16)
    v = a.out("none", torch.float32, (0, 2), "float")
    assert v.numel() == 0 and a.payload("none").shape == (0, 2)
    e = a.entries["none"]
    assert a.arg("none").data_ptr() == a.raw.data_ptr() + a.base + e.off and a.arg("none").data_ptr() % 256 == 0
    _poke(a, "none", 0, 1)
    _poke(a, "none", -1, 1)
    assert a.damaged() == {"none": [-1, 0]}


def test_fills():
    a = _small("A")
    assert np.isnan(a.payload("res")).all() and a.payload("res").tobytes() == b"\xff" * 24
    assert a.payload("idx").tolist() == [0, 0, 0]
    e = a.entries["pts"]
    assert bytes(a.raw[a.base + e.off - 4:a.base + e.off].tolist()) == b"\xff" * 4
    a.refill("B")
    a.reset_outputs()
    assert a.payload("res").tolist() == [7.0, 7.0, 7.0] and a.payload("idx").tolist() == [1, 1, 1]
    assert a.payload("state").tolist() == [0, 1, 0, 0]
    for name, want in (("pts", np.float32(7.0).tobytes()), ("flags", b"\xff"), ("count", np.int32(1).tobytes())):
        e = a.entries[name]
        k = len(want)
        assert bytes(a.raw[a.base + e.off - k:a.base + e.off].tolist()) == want, name
        assert bytes(a.raw[a.base + e.off + e.nbytes:a.base + e.off + e.nbytes + k].tolist()) == want, name
    assert a.damaged() == {}
    assert a.sentinel("idx").tolist() == [1, 1, 1] and a.sentinel("idx", "A").tolist() == [0, 0, 0]


PLANTED = [  # (array, byte offset relative to the array, reported)
    ("res", -1, True),            # one byte just before
    ("res", 24, True),            # one byte just after
    ("res", -4096, True),         # the far end of the front guard
    ("res", 24 + 4095, True),     # the far end of the rear guard
    ("flags", 3, True),           # just after an array of odd length
    ("idx", 12, True),
    ("pts", 0, False),            # inside the payload: no damage
    ("res", 23, False),
]


@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("name,offset,reported", PLANTED)
def test_planted_byte(which, name, offset, reported):
    a = _small(which)
    _poke(a, name, offset, 0x5A)
    assert a.damaged() == ({name: [offset]} if reported else {})
    if not reported and a.entries[name].role == "in":
        assert a.inputs_unchanged() == [name]


def test_stray_row():
    """A whole row written at index n of a 3 x 2 array: eight bytes, at the offsets of row 3."""
    a = _small()
    e = a.entries["pts"]
    a.raw[a.base + e.off + 24:a.base + e.off + 32] = torch.tensor([1.5, 2.5], dtype=torch.float32).view(torch.uint8)
    assert a.damaged() == {"pts": list(range(24, 32))}
    # a row written with the value the guard holds is the one thing a fill cannot see: the other fill does
    b = _small("B")
    e = b.entries["pts"]
    b.raw[b.base + e.off + 24:b.base + e.off + 32] = 0xFF
    assert b.damaged() == {"pts": list(range(24, 32))}


def test_refill_makes_the_old_fill_damage():
    a = _small("A")
    e = a.entries["flags"]
    a.refill("B")
    assert a.damaged() == {}
    _poke(a, "flags", -1, 0x00)                       # fill A of a byte array
    a.raw[a.base + a.entries["count"].off + 4] = 0    # fill A of an index array (B is 1: low byte first)
    assert a.damaged() == {"flags": [-1], "count": [4]}
    a.refill("A")
    assert a.damaged() == {}
    assert e.initial.tolist() == [1, 0, 1] and a.inputs_unchanged() == []


def test_image_padding_is_guard():
    img = np.arange(12, dtype=np.uint8).reshape(3, 4) + 1
    a = ar.Arena("cpu", capacity=1 << 16)
    v = a.image("img", img, 7)
    assert v.numel() == ar.image_length(4, 3, 7) == 18
    assert v.tolist() == [1, 2, 3, 4, 0, 0, 0, 5, 6, 7, 8, 0, 0, 0, 9, 10, 11, 12]
    assert a.damaged() == {}
    _poke(a, "img", 5, 9)        # row padding
    _poke(a, "img", 18, 9)       # the padding of the last row lies outside the array
    assert a.damaged() == {"img": [5, 18]}
    a.refill("B")
    assert a.view("img").tolist()[4:7] == [255, 255, 255] and a.damaged() == {} and a.inputs_unchanged() == []


# ---- the table against the header -------------------------------------------------------------------------------------------
def _declarations():
    """{function: (parameter names that are pointers, the comment directly in front of the declaration)}."""
    text = open(HEADER).read()
    out = {}
    pattern = re.compile(r"(/\*(?:(?!\*/).)*\*/\s*)?^(?:int|void|int32_t|size_t|float|const char \*|pagk_ctx \*)\s*\**(pagk_\w+)\(([^;{]*)\);",
                         re.S | re.M)
    for m in pattern.finditer(text):
        comment, name, params = m.group(1) or "", m.group(2), m.group(3)
        comment = re.sub(r"\s*\n\s*\*\s*", " ", comment)   # one line, without the frame
        params = re.sub(r"/\*.*?\*/", "", params, flags=re.S)
        pointers = []
        for p in params.split(","):
            p = p.strip()
            if "*" in p or "[" in p:
                pointers.append(re.sub(r"\[.*\]", "", p).split("*")[-1].split()[-1])
        out[name] = (pointers, comment)
    return out


def test_header_is_parsed():
    d = _declarations()
    assert len(d) > 100
    assert d["pagk_track_device"][0] == ["ctx", "params", "d_pt_ref_un", "d_pt_init_un", "d_affine", "d_status_in", "d_out"]
    assert "d_thresholds" in d["pagk_post_filter_device"][0] and "d_keys_normal" in d["pagk_frame_handover_device"][0]
    assert "device pointers" in d["pagk_track_device"][1]


def test_every_device_entry_point_has_a_row():
    rows = {f.function for f in df.FORMS}
    assert len(rows) == len(df.FORMS), "a function has two rows"
    decl = _declarations()
    for name, (pointers, comment) in decl.items():
        # (a comment can only call a PARAMETER a device pointer: the context does not count)
        device = any(p.startswith("d_") for p in pointers) or (
            re.search(r"device\s+pointer", comment) and any(p != "ctx" for p in pointers))
        if device:
            assert (name in rows) != (name in df.EXEMPT), f"{name} takes device pointers: one row in FORMS, or an entry of EXEMPT"
    for name in list(rows) + list(df.EXEMPT):
        assert name in decl, f"{name} is not declared in include/pagk.h"
    assert set(df.EXEMPT) == {"pagk_multi_allgather", "pagk_track_sharded"}, "only the multi-device calls are exempt"


@pytest.mark.parametrize("f", df.FORMS, ids=lambda f: f.function)
def test_row_names_every_device_parameter(f):
    pointers = [p for p in _declarations()[f.function][0] if p.startswith("d_")]
    named = [a.name.split(".")[0] for a in f.arrays]
    assert sorted(set(named)) == sorted(pointers), f"{f.function}: the row and the declaration differ"
    names = [a.name for a in f.arrays]
    assert len(set(names)) == len(names)
    for a in f.arrays:
        assert a.dtype in DT and a.role in ("in", "out", "inout") and a.kind in ar.KINDS
        assert a.kind == {"f32": "float", "f64": "float", "u8": "byte", "i32": "index"}[a.dtype], a.name
        assert a.tail is None or a.role != "in"


def test_lengths_evaluate():
    s = dict(n=67, cap=80, cap_q=70, cap_t=65, m=65, cand_cap=65, width=97, height=80, step=128, W=97, H=80, src_width=97,
             src_height=80, src_step=300, channels=3, iters_H=96, iters_F=48, iters_E=32)
    for f in df.FORMS:
        for a in f.arrays:
            assert df.length(a, s) >= 1, (f.function, a.name)
    assert df.length(df.form("pagk_frame_set_device").arrays[0], s) == 79 * 128 + 97
    assert df.length(df.form("pagk_frame_rectify_device").arrays[0], s) == 79 * 300 + 291
    assert df.length(df.form("pagk_geometry_fit_device").arrays[-1], s) == 144


def test_every_row_has_a_gpu_case():
    """Every function of the table is called through its capi.Context method by a scenario of tests/device_plans.py, and
    tests/test_device_bounds_gpu.py runs that scenario (the sources are the record)."""
    here = os.path.dirname(os.path.abspath(__file__))
    plans = open(os.path.join(here, "device_plans.py")).read()
    test = open(os.path.join(here, "test_device_bounds_gpu.py")).read()
    scenarios = re.split(r"^def ", plans, flags=re.M)[1:]
    for f in df.FORMS:
        short = f.function[len("pagk_"):]
        users = [s.split("(")[0] for s in scenarios if re.search(r"\.%s\b" % short, s)]
        assert users, f"{f.function} has a row and no scenario"
        assert any(re.search(r"check\(dp\.%s\(" % u, test) for u in users), f"{f.function}: no case runs its scenario"
