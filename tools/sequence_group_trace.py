#!/usr/bin/env python3
"""The workload of tools/sequence_time.py --cameras K as direct steps in a process that ends normally, for a kernel trace:

    rocprofv3 --kernel-trace --stats -d out -- python tools/sequence_group_trace.py --cameras 2 --arm group

(the timed loops of sequence_time.py replay graphs and leave through os._exit, which a trace does not survive).  --arm group
steps a sequence group of K cameras, --arm singles K sequences one after another; 96 steps of the rig after the start.
--lk and --lk-gyro make the rig a Lucas-Kanade one (pagk_sequence_group_create_lk); --tree DIR imports the package and the test
helpers from another built checkout (--arm singles --cameras 1 on the parent commit's tree: the single-camera path, kernel by
kernel)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in sys.argv[1:-1]:   # (before the package is imported)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, N, NF = 752, 480, 1000, 9
CAP, RATIO = 1024, 0.8


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, default=2)
    ap.add_argument("--arm", choices=("group", "singles"), default="group")
    ap.add_argument("--steps", type=int, default=96)
    ap.add_argument("--lk", action="store_true", help="Lucas-Kanade (tracker type 0)")
    ap.add_argument("--lk-gyro", action="store_true", help="Lucas-Kanade started from the gyro prediction")
    ap.add_argument("--tree", default=None, help="a built checkout to import the package and the test helpers from")
    a = ap.parse_args()
    import handover_ref_util as hu
    from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, runtime, synth
    K = a.cameras
    cam, imgs, Rs, KRKs, rot9, rng = hu.rotating_sequence(synth, NF, W, H, 0x5EED0B20, (0.004, -0.005, 0.006))
    u = rng.uniform(2 * 4 * N)
    cand = np.stack([8 + u[0::2] * (W - 16), 8 + u[1::2] * (H - 16)], axis=1).astype(np.float32)
    lists = [[np.roll(cand, 97 * k + 13 * j, axis=0) for k in range(NF)] for j in range(K)]
    p = capi.make_params(half_patch=10, iterations=30, pyramids=3, has_gyro=True, camera=cam)
    tracker = capi.SEQ_LK if a.lk or a.lk_gyro else capi.SEQ_PATCHMATCH
    sp = capi.sequence_params_default(track=p, lk=capi.lk_params_default(), fit=capi.fit_params_default(seed=0x5EED0F17),
                                      tracker=tracker, lk_initial_flow=1 if a.lk_gyro else 0, width=W, height=H, cap=CAP, target_n=N, new_point_threshold=N * RATIO, detector=0, cand_cap=len(cand),
                                      validate=1, sigma=1.0)
    if a.arm == "group":
        g = runtime.DeviceSequenceGroup(sp, K)
        g.start([imgs[0]] * K, [lists[j][0] for j in range(K)])
        for i in range(a.steps):
            k = 1 + i % (NF - 1)
            g.step([imgs[k]] * K, [rot9[k - 1]] * K, [lists[j][k] for j in range(K)], mode="direct")
        print("live features of camera 0:", int(g.read(0)["state"][0]))
        g.close()
    else:
        seqs = [runtime.DeviceSequence(sp) for _ in range(K)]
        for j, sq in enumerate(seqs):
            sq.start(imgs[0], lists[j][0])
        for i in range(a.steps):
            k = 1 + i % (NF - 1)
            for j, sq in enumerate(seqs):
                sq.step(imgs[k], rot9[k - 1], lists[j][k], mode="direct")
        print("live features of camera 0:", int(seqs[0].read()["state"][0]))
        for sq in seqs:
            sq.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
