"""Times of the FAST-cells-and-quadtree detector (include/pagk.h: pagk_detect_fast_device) beside the Harris detector
(pagk_detect_corners_device) on one image in a frame slot.  Not part of bench.py.

  python tools/fast_time.py WIDTH HEIGHT N [CALLS]

The image is the synth.Texture of the tests (seed 7 at 640 wide, 1 otherwise), the mask all ones; the FAST detector runs
with n_features = N, the Harris detector with max_corners = N.  Each detector is timed twice, alternating, with a host
clock around CALLS calls that end in a synchronisation (ms per call).  For the per-kernel table run it under
`rocprofv3 --kernel-trace --stats -- python tools/fast_time.py ...`, a run of its own without counters."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import detect_ref_util as du  # noqa: E402
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, synth  # noqa: E402


def main():
    W, H, N = (int(v) for v in sys.argv[1:4])
    calls = int(sys.argv[4]) if len(sys.argv) > 4 else 200
    img = du.texture_image(synth, W, H, 7 if W == 640 else 1)
    c = capi.Context(0)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        c.set_stream(stream.cuda_stream)
        c.frame_upload(1, img, 1)
        ob = capi.detect_fast_bounds(W, H, N)[1]
        d_k = torch.zeros((max(ob, N), 2), device="cuda:0")
        d_r = torch.zeros(max(ob, N), device="cuda:0")
        d_i = torch.zeros(8, dtype=torch.int32, device="cuda:0")
        fp, dp = capi.fast_params_default(n_features=N), capi.detect_params_default()
        fns = dict(fast=lambda: c.detect_fast_device(fp, 1, None, ob, d_k, d_r, d_i),
                   harris=lambda: c.detect_corners_device(dp, 1, None, N, None, d_k, d_i))
        ms, info = dict(fast=[], harris=[]), {}
        for name in ("fast", "harris", "fast", "harris"):
            for _ in range(5):
                fns[name]()
            c.sync()
            t0 = time.perf_counter()
            for _ in range(calls):
                fns[name]()
            c.sync()
            ms[name].append((time.perf_counter() - t0) / calls * 1e3)
            info[name] = d_i.cpu().numpy().tolist()
        print(f"RESULT {W}x{H} N={N}: fast {ms['fast'][0]:.3f} / {ms['fast'][1]:.3f} ms per call (info {info['fast'][:6]}), "
              f"harris {ms['harris'][0]:.3f} / {ms['harris'][1]:.3f} ms per call (info {info['harris'][:5]})", flush=True)
    c.set_stream(None)
    c.close()


if __name__ == "__main__":
    main()
