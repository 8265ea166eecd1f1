"""Device time of pagk_geometry_validation_device (compaction, both RANSAC fits with the default budgets, scoring,
model choice, status update) at n = 1000 and n = 20000 correspondences.  Usage: python tools/geometry_fit_time.py
Each line: mean over K back-to-back calls on one stream (HIP events), and the same K calls replayed from one graph."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, synth  # noqa: E402


def scene(n, seed=1, outliers=0.25, noise=0.4):
    """A general two-view scene (EuRoC camera, depths 2-12 m, a 0.7 m baseline) with outliers."""
    rng = np.random.default_rng(seed)
    cam = synth.EUROC
    K = np.array([[cam.fx, 0, cam.cx], [0, cam.fy, cam.cy], [0, 0, 1]])
    R, t = synth.rodrigues(np.array([0.01, -0.02, 0.03])), np.array([0.6, -0.3, 0.2])
    uv1 = np.c_[rng.uniform(20, 732, n), rng.uniform(20, 460, n)]
    X2 = R @ ((np.linalg.inv(K) @ np.c_[uv1, np.ones(n)].T) * rng.uniform(2.0, 12.0, n)) + t[:, None]
    uv2 = (K @ X2).T
    uv2 = uv2[:, :2] / uv2[:, 2:] + rng.normal(0, noise, (n, 2))
    bad = rng.random(n) < outliers
    uv2[bad] += rng.uniform(-30, 30, (int(bad.sum()), 2))
    return np.ascontiguousarray(uv1, np.float32), np.ascontiguousarray(uv2, np.float32)


def main():
    fp = capi.fit_params_default(seed=1)
    stream = torch.cuda.Stream()
    c = capi.Context(0)
    try:
        with torch.cuda.stream(stream):
            c.set_stream(stream.cuda_stream)
            for n in (1000, 20000):
                p1, p2 = scene(n)
                d1, d2 = torch.from_numpy(p1).cuda(), torch.from_numpy(p2).cuda()
                st = torch.ones(n, dtype=torch.uint8, device="cuda")
                st0 = st.clone()
                cnt, sc = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, device="cuda")
                call = lambda: c.geometry_validation_device(fp, n, d1, d2, st, 1.0, cnt, sc)  # noqa: E731
                for _ in range(10):
                    st.copy_(st0)
                    call()
                stream.synchronize()
                K = 200
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(K):
                    call()
                e1.record(stream)
                e1.synchronize()
                direct = e0.elapsed_time(e1) * 1e3 / K
                c.graph_begin()
                try:
                    for _ in range(20):
                        call()
                finally:
                    gid = c.graph_end()
                c.graph_launch(gid)
                stream.synchronize()
                e0.record(stream)
                for _ in range(K // 20):
                    c.graph_launch(gid)
                e1.record(stream)
                e1.synchronize()
                graph = e0.elapsed_time(e1) * 1e3 / K
                c.graph_destroy(gid)
                print(f"n={n}: pagk_geometry_validation_device {direct:7.1f} us/call direct, {graph:7.1f} us/call "
                      f"from a graph (iters_H {fp.iters_H}, iters_F {fp.iters_F}; cnt_inlier {int(cnt.item())})",
                      flush=True)
    finally:
        c.set_stream(None)
        c.close()


if __name__ == "__main__":
    main()
