"""Pinning kit, step 1: tests/golden/*.npz -> <outdir>/<case>.in, the raw layout tools/ref_dump/dump_patchmatch.cpp and
oracle/ref_shim/ref_patchmatch.cpp read (documented at the top of those files).  Needs numpy only.
python tools/ref_dump/export_cases.py <outdir>

Version 1 ("PAGKIN1") is what dump_patchmatch.cpp reads: four distortion coefficients, continuous images.  Version 2
("PAGKIN2", read by ref_patchmatch.cpp) adds mDistCoef.total() (4 or 5), the fifth coefficient and the images' row step."""
import glob
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def write_in(out_path, img_ref, img_cur, cfg, camera, pt_ref, pt_init, affine, status_in, n_dist_coef=4, step=None):
    """cfg: half_patch iterations pyramids has_gyro illumination affine penalty ncc; camera: fx fy cx cy k1 k2 p1 p2 [k3].
    Writes version 1 unless a fifth coefficient or a row step other than the width asks for version 2.  The images are
    written with their rows packed (a strided view is fine); `step` travels as a number."""
    height, width = img_ref.shape
    step = width if step is None else int(step)
    v2 = n_dist_coef != 4 or step != width
    cam = [float(v) for v in camera] + [0.0] * 9
    with open(out_path, "wb") as f:
        f.write(b"PAGKIN2\0" if v2 else b"PAGKIN1\0")
        f.write(struct.pack("<11i", width, height, int(pt_ref.shape[0]), *[int(v) for v in cfg[:8]]))
        if v2:
            f.write(struct.pack("<2i", int(n_dist_coef), step))
        f.write(np.asarray(cam[:9 if v2 else 8], np.float32).tobytes())
        f.write(np.ascontiguousarray(img_ref, np.uint8).tobytes())
        f.write(np.ascontiguousarray(img_cur, np.uint8).tobytes())
        for a, dt in ((pt_ref, np.float32), (pt_init, np.float32), (affine, np.float32), (status_in, np.uint8)):
            f.write(np.ascontiguousarray(a, dt).tobytes())


def export_case(npz_path: str, out_path: str) -> None:
    z = np.load(npz_path, allow_pickle=False)
    cfg = [int(v) for v in z["cfg"]]          # half_patch iterations pyramids has_gyro illumination affine penalty [ncc]
    cfg = cfg + [0] * (8 - len(cfg))
    write_in(out_path, z["img_ref"], z["img_cur"], cfg, z["camera"][:8], z["pt_ref"], z["pt_init"], z["affine"], z["status_in"])


def main():
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    for p in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz"))):
        name = os.path.splitext(os.path.basename(p))[0]
        export_case(p, os.path.join(out, name + ".in"))
        print("wrote", os.path.join(out, name + ".in"))


if __name__ == "__main__":
    main()
