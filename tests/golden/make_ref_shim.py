"""Generates tests/golden/ref_shim/<case>.npz: one file per committed case of tests/reference_cases.py with the inputs, the
parameters and the six outputs that oracle/_ref/ref_patchmatch wrote -- the reference's own src/patch_match.cpp and
src/utils.cpp, compiled unchanged against the project's stand-ins (oracle/ref_shim), with the oracle's llt / resize / log
(the `built_with` string of every file says so).  Data the reference's program wrote while running; no program text.

tests/golden/ref_shim/tracker/<case>.npz holds the same for oracle/_ref/ref_tracker -- the reference's own
src/gyro_aided_tracker.cpp, compiled unchanged under its own header -- over reference_cases.TRACKER_CASES: every input array as
in_<name>, every array the binary wrote as out_<name> (oracle/ref_shim/ref_tracker.cpp lists them).  Arrays only.

tests/golden/ref_shim/orb/<case>.npz holds the same for oracle/_ref/ref_orb -- the reference's own src/ORBextractor.cc, compiled
unchanged under its own header -- over the committed rows of reference_cases.ORB_CASES (oracle/ref_shim/ref_orb.cpp lists the
arrays).  level_0 is the input image and is left out.  Arrays only; the sampling pattern in them is the tests' own.

Kept apart from tests/golden/ref/, which stays reserved for a real OpenCV + Eigen build (tools/ref_dump/).

Needs the binary (`make -C oracle ref` where the reference's sources are).  The files are written with fixed zip timestamps:
regenerating reproduces them byte for byte.   python tests/golden/make_ref_shim.py"""
import io
import os
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
import reference_cases as rc  # noqa: E402


def save_npz(path, **arrays):
    """np.savez_compressed without the wall clock in the archive."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def built_with(raw_tail):
    return np.array(bytes(raw_tail).decode().strip())


def patchmatch_arrays(c, workdir):
    params, inp = rc.params_of(c), rc.make_inputs(c)
    out, proc = rc.run_reference(params, inp, workdir, c.name)
    if out is None:
        raise RuntimeError(f"{c.name}: ref_patchmatch exited with {proc.returncode}: {proc.stderr}")
    return dict(img_ref=np.ascontiguousarray(inp["img_ref"]), img_cur=np.ascontiguousarray(inp["img_cur"]),
                row_step=np.int32(inp["img_ref"].strides[0]), pt_ref=inp["pt_ref"], pt_init=inp["pt_init"], affine=inp["affine"],
                status_in=inp["status_in"], cfg=np.array(rc.cfg_of(params), np.int32),
                camera=np.array(rc.camera_row(params), np.float64), n_dist_coef=np.int32(params.n_dist_coef),
                built_with=built_with(out["built_with"]), **{"out_" + k: out[k] for k in rc.OUTPUTS})


def ncc_arrays(c, workdir):
    inp = rc.make_ncc_inputs(c)
    by_images, by_values, proc = rc.run_reference_ncc(c, inp, workdir)
    if by_images is None:
        raise RuntimeError(f"{c.name}: ref_patchmatch --ncc exited with {proc.returncode}: {proc.stderr}")
    text = ("reference src/utils.cpp:110-148 and :166-202 over include/utils.h:32-46, compiled unchanged (g++ -O3 -std=c++14 "
            "-ffp-contract=off, no -march); project stand-ins for OpenCV (oracle/ref_shim)")
    return dict(img_ref=np.ascontiguousarray(inp["img_ref"]), img_cur=np.ascontiguousarray(inp["img_cur"]),
                row_step=np.int32(inp["img_ref"].strides[0]), pt_ref=inp["pt_ref"], pt_cur=inp["pt_cur"], affine=inp["affine"],
                half_patch=np.int32(c.half_patch), use_affine=np.int32(c.use_affine), built_with=np.array(text),
                out_by_images=by_images, out_by_values=by_values)


def tracker_arrays(c, workdir, binary=None):
    inp = rc.make_tracker_inputs(c)
    out, proc = rc.run_tracker(c.mode, inp, workdir, c.name, **({"binary": binary} if binary else {}))
    if out is None:
        raise RuntimeError(f"{c.name}: ref_tracker --{c.mode} exited with {proc.returncode}: {proc.stderr}")
    return {**{"in_" + k: v for k, v in inp.items()}, **{"out_" + k: v for k, v in out.items()}}


def orb_arrays(c, workdir, binary=None):
    inp = rc.make_orb_inputs(c)
    out, proc = rc.run_orb(inp, workdir, c.name, **({"binary": binary} if binary else {}))
    if out is None:
        raise RuntimeError(f"{c.name}: ref_orb exited with {proc.returncode}: {proc.stderr}")
    assert np.array_equal(out["level_0"], inp["img"])
    return {**{"in_" + k: v for k, v in inp.items()}, **{"out_" + k: v for k, v in out.items() if k != "level_0"}}


def main():
    if not os.path.exists(rc.REF_BIN) or not os.path.exists(rc.TRK_BIN) or not os.path.exists(rc.ORB_BIN):
        sys.exit(f"{rc.REF_BIN}, {rc.TRK_BIN} or {rc.ORB_BIN} is missing: make -C oracle ref (needs the reference's sources)")
    os.makedirs(rc.TRK_FIXTURE_DIR, exist_ok=True)
    os.makedirs(rc.ORB_FIXTURE_DIR, exist_ok=True)
    with tempfile.TemporaryDirectory() as workdir:
        for name in rc.committed_cases():
            a = patchmatch_arrays(rc.case(name), workdir)
            path = os.path.join(rc.FIXTURE_DIR, name + ".npz")
            save_npz(path, **a)
            print(f"{name}: n={a['status_in'].shape[0]} status 1 in {int(a['out_status'].sum())} rows, {os.path.getsize(path)} bytes")
        for c in rc.NCC_CASES:
            a = ncc_arrays(c, workdir)
            path = os.path.join(rc.FIXTURE_DIR, c.name + ".npz")
            save_npz(path, **a)
            print(f"{c.name}: n={a['pt_ref'].shape[0]}, {os.path.getsize(path)} bytes")
        for c in rc.TRACKER_CASES:
            path = os.path.join(rc.TRK_FIXTURE_DIR, c.name + ".npz")
            save_npz(path, **tracker_arrays(c, workdir))
            print(f"tracker/{c.name}: {os.path.getsize(path)} bytes")
        for c in rc.ORB_CASES:
            if c.committed:
                path = os.path.join(rc.ORB_FIXTURE_DIR, c.name + ".npz")
                save_npz(path, **orb_arrays(c, workdir))
                print(f"orb/{c.name}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
