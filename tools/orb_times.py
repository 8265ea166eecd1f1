"""Device time of pagk_orb_describe_device (blur included) and pagk_orb_match_device at the workload's shape: a 752 x 480
frame pair, 1000 keypoints asked per frame, 1000 x 1000 descriptor rows.  Stream events around the calls on the context
stream; the keypoints come from pagk_detect_fast_device, the sampling pattern is seeded.  GPU box only.
    python tools/orb_times.py [--width 752 --height 480 --features 1000 --calls 4000 --repeats 7]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, synth


def texture(w, h, seed):
    tex = synth.Texture(synth.SplitMix64(seed))
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.clip(np.rint(tex(xx, yy)), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=752)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=4000, help="back-to-back calls per timed window")
    ap.add_argument("--repeats", type=int, default=7, help="timed windows per figure")
    a = ap.parse_args()
    dev = "cuda:0"
    w, h, nf = a.width, a.height, a.features
    cap = capi.detect_fast_bounds(w, h, nf)[1]
    ctx = capi.Context(0)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx.set_stream(stream.cuda_stream)
        ctx.orb_set_pattern(np.random.default_rng(31).integers(-13, 14, 1024).astype(np.int32))
        fast, orb = capi.fast_params_default(n_features=nf), capi.orb_params_default()
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        d_k, d_n = [z((cap, 2), torch.float32) for _ in range(2)], [z(8, torch.int32) for _ in range(2)]
        d_a, d_d = [z(cap, torch.float32) for _ in range(2)], [z((cap, 32), torch.uint8) for _ in range(2)]
        d_oi, d_mi = [z(8, torch.int32) for _ in range(2)], z(8, torch.int32)
        d_idx, d_dist, d_keep = z(cap, torch.int32), z(cap, torch.int32), z(cap, torch.uint8)
        for s in range(2):
            ctx.frame_upload(s, texture(w, h, 7 + s), 1)
            ctx.detect_fast_device(fast, s, None, cap, d_k[s], None, d_n[s])

        def describe():
            ctx.orb_describe_device(orb, 0, cap, d_k[0], d_n[0], d_a[0], d_d[0], d_oi[0])

        def match():
            ctx.orb_match_device(orb, cap, d_d[0], d_n[0], cap, d_d[1], d_n[1], d_idx, d_dist, d_keep, d_mi)

        ctx.orb_describe_device(orb, 1, cap, d_k[1], d_n[1], d_a[1], d_d[1], d_oi[1])
        describe()
        match()
        stream.synchronize()
        counts = [int(t.cpu()[0]) for t in d_n]
        print(f"shape {w} x {h}, n_features {nf}, cap {cap}: keypoints {counts}, describe info {d_oi[0].cpu().tolist()[:2]}, "
              f"match info {d_mi.cpu().tolist()[:6]}", flush=True)

        def timed(fn, calls):
            for _ in range(20):
                fn()
            out = []
            for _ in range(a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(calls):
                    fn()
                e1.record(stream)
                e1.synchronize()
                out.append(e0.elapsed_time(e1) * 1e3 / calls)
            return out

        for name, fn in (("describe (blur + orientation + descriptors)", describe), ("match (best + filter)", match)):
            many, one = timed(fn, a.calls), timed(fn, 1)
            print(f"{name}: {a.calls} back-to-back calls {statistics.median(many):8.1f} us per call (min {min(many):.1f}, "
                  f"max {max(many):.1f} over {a.repeats} windows); one call between two events {statistics.median(one):8.1f} us "
                  f"(min {min(one):.1f}, max {max(one):.1f})", flush=True)
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
