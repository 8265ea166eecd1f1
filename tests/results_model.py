"""The track ids of include/pagk.h ("The result ring of a sequence") in numpy: per frame, from index_in_last and the live count
alone, track_id, age, n_new and next_id -- with a cumulative sum where tests/results_ref.c (the same rule in plain C) keeps a
running counter.  ids_of_frames derives them from the frames tests/sequence_model.py yields.  No call into the library."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def ids(index_in_last, n_live) -> list:
    """index_in_last: nf x cap int32, n_live: nf counts -> one dict(track_id int64[cap], age int32[cap], n_new, next_id) per
    frame; a start: next_id = 0."""
    out, next_id = [], 0
    last_id = last_age = None
    for idx, n in zip(np.asarray(index_in_last, np.int32), n_live):
        cap = idx.shape[0]
        n = min(max(int(n), 0), cap)
        live = np.arange(cap) < n
        fresh = live & (idx < 0)
        rank = np.cumsum(fresh) - fresh                     # new rows in front of each row, in row order
        track_id = np.full(cap, -1, np.int64)
        age = np.zeros(cap, np.int32)
        track_id[fresh] = next_id + rank[fresh]
        kept = live & (idx >= 0)
        if kept.any():
            track_id[kept] = last_id[idx[kept]]
            age[kept] = last_age[idx[kept]] + 1
        n_new = int(fresh.sum())
        next_id += n_new
        out.append(dict(track_id=track_id, age=age, n_new=n_new, next_id=next_id))
        last_id, last_age = track_id, age
    return out


def ids_of_frames(frames) -> list:
    """... of the frames a run of tests/sequence_model.py returns."""
    return ids(np.stack([f["index_in_last"] for f in frames]), [int(f["state"][0]) for f in frames])


def build_ref(out_dir) -> C.CDLL:
    """tests/results_ref.c as a shared library (no sanitizer: it is loaded into this process)."""
    so = os.path.join(str(out_dir), "libresults_ref.so")
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(HERE, "results_ref.c"), "-o", so],
                   check=True)
    lib = C.CDLL(so)
    lib.results_ref_run.restype = None
    lib.results_ref_run.argtypes = [C.c_int32, C.c_int32] + [C.c_void_p] * 6
    return lib


def ref_ids(lib, index_in_last, n_live) -> list:
    """The same list as ids(), by the plain-C restatement."""
    idx = np.ascontiguousarray(index_in_last, np.int32)
    nf, cap = idx.shape
    live = np.ascontiguousarray(n_live, np.int32)
    track_id, age = np.zeros((nf, cap), np.int64), np.zeros((nf, cap), np.int32)
    n_new, next_id = np.zeros(nf, np.int32), np.zeros(nf, np.int64)
    lib.results_ref_run(nf, cap, *(a.ctypes.data for a in (live, idx, track_id, age, n_new, next_id)))
    return [dict(track_id=track_id[f], age=age[f], n_new=int(n_new[f]), next_id=int(next_id[f])) for f in range(nf)]
