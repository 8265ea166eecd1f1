"""Times of the device rectification (include/pagk.h: pagk_frame_rectify_device) at the shapes of BASELINE configs[1]
(752x480) and configs[3] (1920x1080), one and three channels.  Not part of bench.py.  One JSON line per figure.

  --mode kernels  `--reps` calls of pagk_frame_rectify_device (rectification + pyramid) per shape and channel count, timed
                  with events; every line carries the byte floor of k_rectify: W*H*(8 + 1) for the map entries and the
                  result, plus the source bytes once (Ws*Hs*cn).  Run it under `rocprofv3 --kernel-trace --stats -- python
                  tools/rectify_time.py --mode kernels --configs N` (one run per shape, no counters) for the kernel's
                  own time.
  --mode loop     runtime.SequenceTracker in graph mode (with the detector, so no list comes from outside), frame time in
                  windows that end in a synchronisation:
                  --rectify on   fed raw frames of --loop-channels channels (rectify=...)
                  --rectify off  the same loop fed the same frames rectified beforehand
                  Alternate the two in processes of one session; the difference is what rectification costs in the graph.
                  With one channel both loops move the same bytes from the host, and the difference is the kernel; with
                  three the raw frame's larger host-to-device copy is part of it.
  --mode host     what the device path replaces: the plain-C restatement (tests/rectify_ref.c, gcc -O2, one core)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, synth  # noqa: E402

LOOP_N = {1: 500, 3: 3000}
ENTRY_BYTES = 8


def emit(**kw):
    print(json.dumps(kw), flush=True)


def lens(idx):
    """The maps of a lens with k1 = -0.28 scaled to the config's image, seen through the same camera."""
    w = synth.config(idx, n=8)
    h, wd = w.img_ref.shape
    f = 0.62 * wd
    mx, my = capi.undistort_maps(f, f, wd / 2 + 3.3, h / 2 - 1.7, [-0.28, 0.07, 0.0002, -0.0001, 0.0], wd, h)
    return w, mx, my


def colour(img, cn):
    if cn == 1:
        return img
    planes = [img, np.roll(img, 1, axis=1), 255 - np.roll(img, 2, axis=0), img][:cn]
    return np.ascontiguousarray(np.stack(planes, axis=2))


def floor_bytes(wd, h, ws, hs, cn):
    return wd * h * (ENTRY_BYTES + 1) + ws * hs * cn


def run_kernels(idx, reps, channels):
    w, mx, my = lens(idx)
    h, wd = w.img_ref.shape
    stream = torch.cuda.Stream()
    c = capi.Context(0)
    try:
        with torch.cuda.stream(stream):
            c.set_stream(stream.cuda_stream)
            c.rectify_set_maps(mx, my)
            for cn in channels:
                rp = capi.rectify_params_default(channels=cn)
                d_raw = torch.from_numpy(colour(w.img_ref, cn).reshape(h, wd * cn)).to("cuda:0")
                for _ in range(3):
                    c.frame_rectify_device(0, rp, d_raw.data_ptr(), wd, h, wd * cn, w.pyramids)
                stream.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(reps):
                    c.frame_rectify_device(0, rp, d_raw.data_ptr(), wd, h, wd * cn, w.pyramids)
                e1.record(stream)
                stream.synchronize()
                emit(mode="kernels", config=idx, width=wd, height=h, channels=cn, reps=reps,
                     rectify_and_pyramid_ms_per_call=e0.elapsed_time(e1) / reps, floor_bytes=floor_bytes(wd, h, wd, h, cn))
    finally:
        c.set_stream(None)
        c.close()


def run_loop(idx, rectify, cn, n, frames, windows, warmup):
    from pixel_aware_gyro_aided_klt_feature_tracker_amd import runtime
    import frame_loop_time as flt
    _, mx, my = lens(idx)
    w, p, imgs, rots, _ = flt.workload(idx)
    h, wd = w.img_ref.shape
    rp = capi.rectify_params_default(channels=cn)
    raws = [colour(im, cn) for im in imgs]
    if not rectify:   # the same frames, rectified beforehand
        c = capi.Context(0)
        c.rectify_set_maps(mx, my)
        raws = [c.rectify(rp, r) for r in raws]
        c.close()
    det = capi.detect_params_default()
    sq = runtime.SequenceTracker(p, wd, h, n, n, 1.0, None, detector=det, rectify=(mx, my, rp, (h, wd)) if rectify else None)
    try:
        sq.start(raws[0], snapshot=False)
        k = 1
        for _ in range(warmup):
            sq.step(raws[k & 1], rots[k & 1], snapshot=False)
            k += 1
        sq.synchronize()
        assert sq.mode_used == "graph"
        for wnd in range(windows):
            sq.synchronize()
            t0 = time.perf_counter()
            for _ in range(frames):
                res = sq.step(raws[k & 1], rots[k & 1], snapshot=False)
                k += 1
            sq.synchronize()
            dt = time.perf_counter() - t0
            st = res.to_numpy()
            emit(mode="loop", rectify=bool(rectify), channels=cn, config=idx, width=wd, height=h, n=n, window=wnd, frames=frames,
                 ms_per_frame=dt * 1e3 / frames, last_total=st["total"], last_survivors=st["survivors"])
    finally:
        sq.close()


def run_host(idx, reps, channels):
    import tempfile
    import rectify_ref_util as ru
    w, mx, my = lens(idx)
    h, wd = w.img_ref.shape
    lib = ru.build_ref(tempfile.mkdtemp(prefix="rectify_ref_"))
    for cn in channels:
        raw = colour(w.img_ref, cn)
        ru.ref_rectify(lib, mx, my, raw)
        t0 = time.perf_counter()
        for _ in range(reps):
            ru.ref_rectify(lib, mx, my, raw)
        emit(mode="host", config=idx, width=wd, height=h, channels=cn, reps=reps,
             restatement_ms=(time.perf_counter() - t0) * 1e3 / reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("kernels", "loop", "host"), required=True)
    ap.add_argument("--configs", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--channels", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--rectify", choices=("on", "off"), default="on")
    ap.add_argument("--loop-channels", type=int, default=1)
    ap.add_argument("--n", type=int, default=0, help="loop mode: features per frame (default 500 at configs[1], 3000 at configs[3])")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--frames", type=int, default=0, help="frames per window (default: 300 at configs[1], 100 at configs[3])")
    ap.add_argument("--windows", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=12)
    a = ap.parse_args()
    if a.mode != "host" and not torch.cuda.is_available():
        raise SystemExit("rectify_time.py needs a HIP device")
    for idx in a.configs:
        if a.mode == "kernels":
            run_kernels(idx, a.reps, a.channels)
        elif a.mode == "host":
            run_host(idx, a.reps, a.channels)
        else:
            run_loop(idx, a.rectify == "on", a.loop_channels, a.n or LOOP_N[idx], a.frames or {1: 300, 3: 100}[idx], a.windows, a.warmup)


if __name__ == "__main__":
    main()
