"""Device time of pyramidal Lucas-Kanade (tracker type 0) next to the PatchMatch step (tracker type 4) on the same input:
synth.config(1), a 752 x 480 frame pair with 1000 keypoints, half patch 10.  Each step is captured once and timed as a
replayed graph between two stream events, the two trackers' windows alternating:
    LK          pagk_lk_pyramid_device of the current frame + pagk_lk_track_device (and each of the two alone)
    PatchMatch  pagk_frame_set_device of the current frame (its pyramid) + pagk_track_device (and the tracking alone)
The Lucas-Kanade result is compared with the restatement (tests/lk_ref.c) before any time is reported.  GPU box only.
    python tools/lk_times.py [--replays 2000 --repeats 7]"""
import argparse
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import lk_ref_util as lu
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, synth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=2000, help="graph replays per timed window (0.6 s for the slowest step, 0.15 s for the fastest tracker step)")
    ap.add_argument("--repeats", type=int, default=7, help="timed windows per figure")
    a = ap.parse_args()
    dev = "cuda:0"
    wl = synth.config(1)
    h, w = wl.img_ref.shape
    n = wl.n
    lk_p = lu.params(half_patch=wl.half_patch)
    lk = capi.lk_params_default(**lk_p)
    pm = capi.make_params(half_patch=wl.half_patch, iterations=wl.iterations, pyramids=wl.pyramids, has_gyro=wl.has_gyro,
                          camera=wl.camera)
    want = lu.ref_track(lu.build_ref(tempfile.mkdtemp(prefix="lk_ref_")), wl.img_ref, wl.img_cur, wl.pt_ref, lk_p)
    ctx = capi.Context(0)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ctx.set_stream(stream.cuda_stream)
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)     # noqa: E731
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)       # noqa: E731
        d_img = [up(wl.img_ref), up(wl.img_cur)]
        d_ref, d_init, d_aff, d_st = up(wl.pt_ref), up(wl.pt_init), up(wl.affine), up(wl.status_in)
        lk_out = dict(pt_out=z((n, 2), torch.float32), status=z(n, torch.uint8), status_raw=z(n, torch.uint8),
                      err=z(n, torch.float32), flow=z((n, 2), torch.float32), info=z(capi.LK_INFO_WORDS, torch.int32))
        pm_out = dict(pt_un=z((n, 2), torch.float32), pt_dist=z((n, 2), torch.float32), status=z(n, torch.uint8),
                      pix_err=z(n, torch.float64), dist_pred=z(n, torch.float64), ncc=z(n, torch.float32))

        def set_frame(s):
            ctx.frame_set_device(s, d_img[s].data_ptr(), w, h, w, wl.pyramids)

        def lk_pyramid():
            ctx.lk_pyramid_device(lk, 1)

        def lk_track():
            ctx.lk_track_device(lk, 0, 1, n, d_ref, None, lk_out["pt_out"], lk_out["status"], lk_out["status_raw"], lk_out["err"],
                                lk_out["flow"], lk_out["info"])

        def pm_track():
            ctx.track_device(pm, 0, 1, n, d_ref, d_init, d_aff, d_st, pm_out)

        steps = {"LK: pyramid of the current frame + track": (lk_pyramid, lk_track),
                 "LK: pyramid of the current frame": (lk_pyramid,),
                 "LK: track": (lk_track,),
                 "PatchMatch (type 4): pyramid of the current frame + track": (lambda: set_frame(1), pm_track),
                 "PatchMatch (type 4): track": (pm_track,)}
        # direct calls first: they size every buffer, and their result is checked before anything is timed
        set_frame(0)
        set_frame(1)
        ctx.lk_pyramid_device(lk, 0)
        for fns in steps.values():
            for fn in fns:
                fn()
        stream.synchronize()
        got = {k: v.cpu().numpy() for k, v in lk_out.items()}
        bad = lu.differing(got, want)
        if bad:
            raise SystemExit(f"the device result differs from the restatement in {bad}: no time is reported")
        pm_status = pm_out["status"].cpu().numpy()
        kept3 = capi.post_filter(wl.half_patch, pm_status, pm_out["pix_err"].cpu().numpy(), pm_out["dist_pred"].cpu().numpy(),
                                 pm_out["pt_dist"].cpu().numpy(), pm_out["pt_un"].cpu().numpy())[0]
        d_lk = np.hypot(*(got["pt_out"].astype(np.float64) - wl.pt_true).T)[got["status"] > 0]
        d_pm = np.hypot(*(pm_out["pt_un"].cpu().numpy().astype(np.float64) - wl.pt_true).T)[pm_status > 0]
        print(f"{wl.name}: {w} x {h}, {n} keypoints, half patch {wl.half_patch}; the Lucas-Kanade result equals the restatement", flush=True)
        print(f"LK info {got['info'][:6].tolist()}: kept {int(got['status'].sum())} of {n} ({got['status'].mean():.3f}), raw status "
              f"{int(got['status_raw'].sum())}; median distance of the kept to the true position {np.median(d_lk):.3f} px", flush=True)
        print(f"PatchMatch (type 4): status {int(pm_status.sum())} of {n} ({pm_status.mean():.3f}), after the Step-3 filter {kept3} "
              f"({kept3 / n:.3f}); median distance of status 1 to the true position {np.median(d_pm):.3f} px", flush=True)
        graphs = {}
        for name, fns in steps.items():
            ctx.graph_begin()
            try:
                for fn in fns:
                    fn()
            finally:
                graphs[name] = ctx.graph_end()
        times = {name: [] for name in steps}
        for name, gid in graphs.items():      # warm-up of every graph
            for _ in range(20):
                ctx.graph_launch(gid)
        stream.synchronize()
        for _ in range(a.repeats):            # the windows of the five steps in turn
            for name, gid in graphs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.replays):
                    ctx.graph_launch(gid)
                e1.record(stream)
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / a.replays)
        for name, t in times.items():
            print(f"{name}: {statistics.median(t):8.1f} us per replay (min {min(t):.1f}, max {max(t):.1f} over {a.repeats} windows of "
                  f"{a.replays} replays)", flush=True)
        again = {k: v.cpu().numpy() for k, v in lk_out.items()}
        if lu.differing(again, want):
            raise SystemExit("the replayed graphs left a result that differs from the restatement")
        for gid in graphs.values():
            ctx.graph_destroy(gid)
    ctx.set_stream(None)
    ctx.close()


if __name__ == "__main__":
    main()
