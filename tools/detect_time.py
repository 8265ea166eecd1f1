"""Times of the device corner detector (include/pagk.h: pagk_detect_corners_device, pagk_frame_handover_detect_device) on
the images of BASELINE configs[1] (752x480) and configs[3] (1920x1080).  Not part of bench.py.  One JSON line per figure.

  --mode kernels  full detections (max_corners 1000 / 20000) and top-ups of 50 under a mask with holes, device arrays, timed
                  with events around `--reps` calls.  Run it under `rocprofv3 --kernel-trace --stats -- python
                  tools/detect_time.py --mode kernels` (a run of its own, no counters) for the per-kernel table.
  --mode loop     runtime.SequenceTracker in graph mode, frame time in windows that end in a synchronisation:
                  --detector on   the hand-over detects its own top-up (detector=...)
                  --detector off  the same loop fed a ready-made candidate list (the detector's corners of the two images,
                                  computed once in front of the loop)
                  Both track `--n` features (default 500 / 3000: what a minimum distance of 20 lets the images hold) with
                  ratio 1, so every frame is topped up.  Alternate the two in processes of one session; the difference is
                  what detection costs inside the graph.
  --mode host     what the device detector replaces: the plain-C restatement (tests/corner_detect_ref.c, gcc -O2, one
                  core) on the same image and mask, plus the copies the host shape needs -- image and mask down, list up."""
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
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, synth  # noqa: E402

FULL = {1: 1000, 3: 20000}
LOOP_N = {1: 500, 3: 3000}


def emit(**kw):
    print(json.dumps(kw), flush=True)


def run_kernels(idx, reps):
    from detect_ref_util import holes_mask
    w = synth.config(idx)
    img = w.img_ref
    h, wd = img.shape
    det = capi.detect_params_default()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream()
    c = capi.Context(0)
    try:
        with torch.cuda.stream(stream):
            c.set_stream(stream.cuda_stream)
            d_img = torch.from_numpy(img).to(dev)
            c.frame_set_device(0, d_img.data_ptr(), wd, h, wd, w.pyramids)
            cap = FULL[idx]
            d_c = torch.zeros((cap, 2), device=dev)
            d_i = torch.zeros(capi.DETECT_INFO_WORDS, dtype=torch.int32, device=dev)
            d_mask = torch.from_numpy(holes_mask(wd, h, cap * 3 // 10)).to(dev)
            for what, mask, mc in (("full", None, cap), ("top-up 50", d_mask, 50)):
                d_max = torch.tensor([mc], dtype=torch.int32, device=dev)
                for _ in range(3):
                    c.detect_corners_device(det, 0, mask, cap, d_max, d_c, d_i)
                stream.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(reps):
                    c.detect_corners_device(det, 0, mask, cap, d_max, d_c, d_i)
                e1.record(stream)
                stream.synchronize()
                info = d_i.cpu().numpy()
                emit(mode="kernels", config=idx, width=wd, height=h, what=what, max_corners=mc, reps=reps,
                     ms_per_call=e0.elapsed_time(e1) / reps, corners=int(info[0]), raw=int(info[1]), visited=int(info[4]))
    finally:
        c.set_stream(None)
        c.close()


def run_loop(idx, detector, n, frames, windows, warmup):
    from pixel_aware_gyro_aided_klt_feature_tracker_amd import runtime
    import frame_loop_time as flt
    w, p, imgs, rots, _ = flt.workload(idx)
    h, wd = w.img_ref.shape
    det = capi.detect_params_default()
    lists = None
    if not detector:   # the ready-made list: the same detector's corners, once, in front of the loop
        c = capi.Context(0)
        lists = [c.detect_corners(im, None, 4 * n, det)["corners"].copy() for im in imgs]
        c.close()
    sq = runtime.SequenceTracker(p, wd, h, n, n, 1.0, None, cand_cap=4 * n, detector=det if detector else None)
    try:
        sq.start(imgs[0], None if detector else lists[0], snapshot=False)
        k = 1
        for _ in range(warmup):
            sq.step(imgs[k & 1], rots[k & 1], None if detector else lists[k & 1], snapshot=False)
            k += 1
        sq.synchronize()
        assert sq.mode_used == "graph"
        for wnd in range(windows):
            sq.synchronize()
            t0 = time.perf_counter()
            for _ in range(frames):
                res = sq.step(imgs[k & 1], rots[k & 1], None if detector else lists[k & 1], snapshot=False)
                k += 1
            sq.synchronize()
            dt = time.perf_counter() - t0
            st = res.to_numpy()
            emit(mode="loop", detector=bool(detector), config=idx, width=wd, height=h, n=n, window=wnd, frames=frames,
                 ms_per_frame=dt * 1e3 / frames, last_total=st["total"], last_survivors=st["survivors"], last_added=st["added"])
    finally:
        sq.close()


def run_host(idx, reps):
    import tempfile
    import detect_ref_util as du
    holes_mask = du.holes_mask
    w = synth.config(idx)
    img = w.img_ref
    h, wd = img.shape
    lib = du.build_ref(tempfile.mkdtemp(prefix="detect_ref_"))
    cap = FULL[idx]
    mask = holes_mask(wd, h, cap * 3 // 10)
    dev = torch.device("cuda", 0)
    d_img, d_mask = torch.zeros((h, wd), dtype=torch.uint8, device=dev), torch.zeros((h, wd), dtype=torch.uint8, device=dev)
    pin_img, pin_mask = torch.from_numpy(img.copy()).pin_memory(), torch.from_numpy(mask).pin_memory()
    for what, m, mc in (("full", None, cap), ("top-up 50", mask, 50)):
        du.ref_detect(lib, img, m, mc)
        t0 = time.perf_counter()
        for _ in range(reps):
            r = du.ref_detect(lib, img, m, mc)
        cpu_ms = (time.perf_counter() - t0) * 1e3 / reps
        d_list = torch.zeros((max(r["n"], 1), 2), device=dev)
        pin_list = torch.from_numpy(r["corners"][:max(r["n"], 1)].copy()).pin_memory()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):   # the host shape: image and mask come down, the list goes up
            pin_img.copy_(d_img), pin_mask.copy_(d_mask)
            torch.cuda.synchronize()
            d_list.copy_(pin_list)
            torch.cuda.synchronize()
        copy_ms = (time.perf_counter() - t0) * 1e3 / reps
        emit(mode="host", config=idx, width=wd, height=h, what=what, max_corners=mc, reps=reps, restatement_ms=cpu_ms,
             copies_ms=copy_ms, corners=r["n"], raw=int(r["info"][1]), visited=int(r["info"][4]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("kernels", "loop", "host"), required=True)
    ap.add_argument("--configs", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--detector", choices=("on", "off"), default="on")
    ap.add_argument("--n", type=int, default=0, help="loop mode: features per frame (default 500 at configs[1], 3000 at configs[3])")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=0, help="frames per window (default: 300 at configs[1], 100 at configs[3])")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=12)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("detect_time.py needs a HIP device")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    for idx in a.configs:
        if a.mode == "kernels":
            run_kernels(idx, a.reps)
        elif a.mode == "host":
            run_host(idx, a.reps)
        else:
            run_loop(idx, a.detector == "on", a.n or LOOP_N[idx], a.frames or {1: 300, 3: 100}[idx], a.windows, a.warmup)


if __name__ == "__main__":
    main()
