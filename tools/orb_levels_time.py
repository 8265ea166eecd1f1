"""Device time of one pagk_orb_extract_slot as a replayed graph for 1, 4 and 8 levels, beside the one-level chain
pagk_detect_fast_device + pagk_orb_describe_device as a replayed graph, in the same process and in alternating blocks; shape
752 x 480, 1000 features, a seeded sampling pattern.  Stream events around blocks of replays.  GPU box only.
    python tools/orb_levels_time.py [--width 752 --height 480 --features 1000 --replays 300 --rounds 7]
    python tools/orb_levels_time.py --profile 50     # 50 direct calls of each and nothing else: the run rocprofv3 traces"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, synth

LEVELS = (1, 4, 8)


def texture(w, h, seed):
    tex = synth.Texture(synth.SplitMix64(seed))
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.clip(np.rint(tex(xx, yy)), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=752)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--replays", type=int, default=300, help="graph replays per timed block")
    ap.add_argument("--rounds", type=int, default=7, help="rounds of alternating blocks")
    ap.add_argument("--profile", type=int, default=0, help="direct calls of each form, no timing")
    a = ap.parse_args()
    dev = "cuda:0"
    w, h, nf = a.width, a.height, a.features
    cap1 = capi.detect_fast_bounds(w, h, nf)[1]
    ctx = capi.Context(0)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx.set_stream(stream.cuda_stream)
        ctx.orb_set_pattern(np.random.default_rng(31).integers(-13, 14, 1024).astype(np.int32))
        fast, orb = capi.fast_params_default(n_features=nf), capi.orb_params_default()
        ex = {nl: capi.orb_extractor_default(n_features=nf, n_levels=nl) for nl in LEVELS}
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        d_k, d_n, d_a, d_d, d_oi = z((cap1, 2), torch.float32), z(8, torch.int32), z(cap1, torch.float32), z((cap1, 32), torch.uint8), z(8, torch.int32)
        img = texture(w, h, 7)
        for s in range(4):
            ctx.frame_upload(s, img, 1)
        slot = {nl: k for k, nl in enumerate(LEVELS)}

        def chain():
            ctx.detect_fast_device(fast, 3, None, cap1, d_k, None, d_n)
            ctx.orb_describe_device(orb, 3, cap1, d_k, d_n, d_a, d_d, d_oi)

        work = {f"{nl} level{'s' if nl > 1 else ''}": (lambda nl=nl: ctx.orb_extract_slot(ex[nl], slot[nl], orb)) for nl in LEVELS}
        work["one-level chain"] = chain
        for fn in work.values():          # direct once: every buffer reaches its size before anything is captured
            fn()
        stream.synchronize()
        for nl in LEVELS:
            t = capi.orb_extractor_levels(ex[nl], w, h)
            r = ctx.orb_slot_read(slot[nl], t["out_bound"])
            print(f"{nl} levels: sizes {list(zip(t['width'].tolist(), t['height'].tolist()))}, quotas {t['quota'].tolist()}, "
                  f"keypoints {r['level_counts'][:nl].tolist()} = {r['n']}, raw {r['level_raw'][:nl].tolist()}", flush=True)
        print(f"one-level chain: keypoints {int(d_n.cpu()[0])}, describe info {d_oi.cpu().tolist()[:2]}", flush=True)
        if a.profile:
            for _ in range(a.profile):
                for fn in work.values():
                    fn()
            stream.synchronize()
        else:
            gid = {}
            for name, fn in work.items():
                ctx.graph_begin()
                try:
                    fn()
                finally:
                    gid[name] = ctx.graph_end()
            for g in gid.values():
                for _ in range(20):
                    ctx.graph_launch(g)
            stream.synchronize()
            times = {name: [] for name in gid}
            for _ in range(a.rounds):     # alternating blocks: every form meets the same neighbours on the device
                for name, g in gid.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for _ in range(a.replays):
                        ctx.graph_launch(g)
                    e1.record(stream)
                    e1.synchronize()
                    times[name].append(e0.elapsed_time(e1) * 1e3 / a.replays)
            for name, t in times.items():
                print(f"RESULT {w}x{h} N={nf} {name}: {statistics.median(t):8.1f} us per replay (min {min(t):.1f}, max {max(t):.1f} "
                      f"over {a.rounds} blocks of {a.replays})", flush=True)
            for g in gid.values():
                ctx.graph_destroy(g)
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
