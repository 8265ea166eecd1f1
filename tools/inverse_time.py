"""Launch time of the template-Jacobian mode (pagk_params::inverse == PAGK_INVERSE_TEMPLATE) beside the forward mode
(automatic variant) on the BASELINE shapes, in one process, the two arms alternating:

    python tools/inverse_time.py [--out profiles/inverse_time.json] [--blocks 12] [--per-block 20] [--configs 1,3,4]

Per workload (synth.config(1) with 1000 features, config(3) with 20000, config(4) with 4000): both frames resident, the
per-feature arrays on the device, pagk_track_device of each arm captured as a graph after a direct run (if a capture is
refused both arms run as direct launches) and replayed in blocks of `per-block` launches between two device events; `blocks`
blocks per arm (at least 200 launches), forward and inverse block by block in turn, after a warm-up block of each.  Reported
per arm: the median, the smallest and the largest block's time per launch, the variant, and the iterations per live feature.
The yardstick is the forward arm of the same run."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, distributed, synth

CONFIGS = {1: 1000, 3: 20000, 4: 4000}


def measure(cfg: int, n: int, blocks: int, per_block: int) -> dict:
    w = synth.config(cfg, n=n)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream()
    c = capi.Context(0)
    arms = {"forward": 0, "inverse": capi.PAGK_INVERSE_TEMPLATE}
    res = {"config": cfg, "name": w.name, "features": w.n, "half_patch": w.half_patch, "pyramids": w.pyramids,
           "iterations": w.iterations, "blocks": blocks, "launches_per_block": per_block}
    try:
        with torch.cuda.stream(stream):
            c.set_stream(stream.cuda_stream)
            c.frame_upload(0, w.img_ref, w.pyramids)
            c.frame_upload(1, w.img_cur, w.pyramids)
            d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (w.pt_ref, w.pt_init, w.affine, w.status_in)]
            live = w.status_in[:w.n] > 0
            params, outs, graphs, info = {}, {}, {}, {}
            for arm, inverse in arms.items():
                params[arm] = capi.make_params(half_patch=w.half_patch, iterations=w.iterations, pyramids=w.pyramids,
                                               has_gyro=w.has_gyro, camera=w.camera, inverse=inverse)
                outs[arm] = distributed.alloc_device_outputs(w.n, dev)
                c.track_device(params[arm], 0, 1, w.n, d[0], d[1], d[2], d[3], outs[arm])   # direct: sizes every workspace
                stream.synchronize()
                c.check_launch()
                got = {k: outs[arm][k].cpu().numpy()[:w.n] for k in ("status", "iters", "pt_un")}
                err = np.linalg.norm(got["pt_un"][live].astype(np.float64) - w.pt_true[:w.n][live], axis=1)
                info[arm] = {"variant": c.last_variant(), "live": int(live.sum()), "tracked": int(got["status"][live].sum()),
                             "iters_per_live_feature": float(got["iters"][live].mean()),
                             "median_error_px": float(np.median(err))}
            mode = "graph"
            try:
                for arm in arms:
                    c.graph_begin()
                    try:
                        c.track_device(params[arm], 0, 1, w.n, d[0], d[1], d[2], d[3], outs[arm])
                    finally:
                        graphs[arm] = c.graph_end()
            except capi.PagkError as e:
                print(f"config {cfg}: capture refused ({e}); both arms run as direct launches", file=sys.stderr)
                for gid in graphs.values():
                    c.graph_destroy(gid)
                graphs, mode = {}, "direct"

            def block(arm):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                for _ in range(per_block):
                    if mode == "graph":
                        c.graph_launch(graphs[arm])
                    else:
                        c.track_device(params[arm], 0, 1, w.n, d[0], d[1], d[2], d[3], outs[arm])
                b.record(stream)
                b.synchronize()
                return a.elapsed_time(b) * 1e3 / per_block   # us per launch

            times = {arm: [] for arm in arms}
            for arm in arms:
                block(arm)                                   # warm-up
            for _ in range(blocks):
                for arm in arms:
                    times[arm].append(block(arm))
            c.check_launch()
            for gid in graphs.values():
                c.graph_destroy(gid)
            res["mode"] = mode
            for arm in arms:
                t = np.array(times[arm])
                res[arm] = dict(info[arm], us_per_launch_median=float(np.median(t)), us_per_launch_min=float(t.min()),
                                us_per_launch_max=float(t.max()), launches=blocks * per_block)
            res["inverse_over_forward"] = res["inverse"]["us_per_launch_median"] / res["forward"]["us_per_launch_median"]
    finally:
        c.set_stream(None)
        c.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--blocks", type=int, default=12)
    ap.add_argument("--per-block", type=int, default=20)
    ap.add_argument("--configs", default="1,3,4")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("inverse_time.py measures on the GPU: no HIP device here")
    rows = []
    for cfg in (int(v) for v in a.configs.split(",")):
        r = measure(cfg, CONFIGS[cfg], a.blocks, a.per_block)
        rows.append(r)
        f, i = r["forward"], r["inverse"]
        print(f"config {cfg} ({r['features']} features, h = {r['half_patch']}, {r['mode']}): "
              f"forward variant {f['variant']} {f['us_per_launch_median']:.1f} us [{f['us_per_launch_min']:.1f}, {f['us_per_launch_max']:.1f}], "
              f"{f['iters_per_live_feature']:.2f} iterations | inverse {i['us_per_launch_median']:.1f} us "
              f"[{i['us_per_launch_min']:.1f}, {i['us_per_launch_max']:.1f}], {i['iters_per_live_feature']:.2f} iterations | "
              f"ratio {r['inverse_over_forward']:.3f}", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/inverse_time.py", "device": torch.cuda.get_device_name(0), "workloads": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
