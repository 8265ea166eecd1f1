"""The hint of csrc/pagk_prio.h measured the honest way: the resident tracker steps through the sequence of tools/hint_pairs.py (the same
keypoints, another camera motion and gyro error per pair), so the hints a launch reads always come from a DIFFERENT pair -- what a tracker
gets -- as far as this sequence goes: the REFERENCE frame and the keypoints never change (only the current frame, the prediction, the
affine and the incoming status do), so the reference patches that make a feature slow are the same in every pair, while a real tracker's
reference frame is new every frame.  An upper bound on what footage would give.  Two trackers, one created with PAGK_PRIO_HINT=0 and one with the default (or PAGK_HINT_T), take turns on every pair; the tracking
launch is timed by the library's own events (pagk_last_kernel_ms).  For comparison the same pairs with the pair's own counts as the hint
(the benchmark's situation: a replayed pair).  Usage: python tools/hint_sequence.py [n] [rounds] [config] [arm]
arm = order: the same measurement of the dispatch order of csrc/pagk_order.h -- both trackers keep the default hint threshold, "off" is
created with PAGK_DISPATCH_ORDER=0 -- so that its two figures (the previous pair's counts, the pair's own) stand beside the hint's.
Another config than 1 has no sequence (tools/hint_pairs.py varies configs[1]'s motion): its one pair is replayed, both figures are the
exact-hint case."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
import hint_pairs
from pixel_aware_gyro_aided_klt_feature_tracker_amd import capi, runtime, synth

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
cfg = int(sys.argv[3]) if len(sys.argv) > 3 else 1
pairs = [hint_pairs.workload(synth, 1, n, j) for j in range(len(hint_pairs.PAIRS))] if cfg == 1 else [synth.config(cfg, n=n)]
w0 = pairs[0]
p = capi.make_params(half_patch=w0.half_patch, iterations=w0.iterations, pyramids=w0.pyramids, has_gyro=w0.has_gyro, camera=w0.camera)


arm = sys.argv[4] if len(sys.argv) > 4 else "hint"
assert arm in ("hint", "order"), arm


def make(threshold, name="PAGK_PRIO_HINT"):
    old = os.environ.get(name)
    if threshold is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = str(threshold)
    rt = runtime.ResidentTracker(p, device=0)
    if old is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = old
    rt.load_pair(w0.img_ref, w0.img_cur)
    rt.set_features(w0.pt_ref, w0.pt_init, w0.affine, w0.status_in)
    return rt


def show(w, rt):
    """Pair w into the tracker's buffers: a new current frame and a new prediction for the SAME features at the same indices (no
    set_features: that would install new features and clear the hints)."""
    with torch.cuda.stream(rt.main):
        rt.img_cur.copy_(torch.from_numpy(np.ascontiguousarray(w.img_cur)).to(rt.dev))
        rt.d_pt_init.copy_(torch.from_numpy(w.pt_init).to(rt.dev))
        rt.d_affine.copy_(torch.from_numpy(w.affine).to(rt.dev))
        rt.d_status.copy_(torch.from_numpy(w.status_in).to(rt.dev))


def launch(rt):
    with torch.cuda.stream(rt.main):
        rt.rebuild_current_pyramid(1)
        rt.track_shard(1)
        return rt.ctx.last_kernel_ms()[0] * 1e3


if arm == "order":
    on, off = make(None, "PAGK_DISPATCH_ORDER"), make(0, "PAGK_DISPATCH_ORDER")
    print(f"configs[{cfg}] scene, {n} features, {len(pairs)} pairs, {rounds} rounds; dispatch order: on = {on.ctx.dispatch_order_enabled()}, "
          f"off = {off.ctx.dispatch_order_enabled()}; hint threshold of both = {on.ctx.prio_hint_threshold()}")
else:
    on, off = make(os.environ.get("PAGK_HINT_T")), make(0)
    print(f"configs[{cfg}] scene, {n} features, {len(pairs)} pairs, {rounds} rounds; thresholds: on = {on.ctx.prio_hint_threshold()}, off = {off.ctx.prio_hint_threshold()}")
seq = {"on": [], "off": []}
exact = {"on": [], "off": []}
for r in range(rounds + 1):          # (round 0 warms up)
    for j, w in enumerate(pairs):
        for name, rt in (("on", on), ("off", off)) if (r + j) % 2 == 0 else (("off", off), ("on", on)):
            show(w, rt)
            t_seq = launch(rt)       # hints: the previous pair's counts (pair 0: the last pair's of the round before)
            t_own = launch(rt)       # hints: this pair's own counts, as in a replayed pair
            if r > 0:
                seq[name].append((j, t_seq))
                exact[name].append((j, t_own))
on.synchronize(), off.synchronize()
its = on.out["iters"][:n].cpu().numpy()
print(f"last pair: mean {its.mean():.2f} / max {its.max()} iterations; hints left = iters: {np.array_equal(on.ctx.prio_hint_get(n), its)}")


def per_round(v):
    a = np.array([t for _, t in v]).reshape(rounds, len(pairs))
    return a.mean(1)


for what, d in ((f"{arm} from the previous pair's counts (a tracker)", seq), (f"{arm} from the pair's own counts (a replayed pair)", exact)):
    a_on, a_off = per_round(d["on"]), per_round(d["off"])
    print(f"{what}: tracking launch, mean over the pairs, per round (us)")
    print("   on : " + "  ".join(f"{x:.2f}" for x in a_on) + f"   median {np.median(a_on):.2f}")
    print("   off: " + "  ".join(f"{x:.2f}" for x in a_off) + f"   median {np.median(a_off):.2f}   spread (max - min) {a_off.max() - a_off.min():.2f}")
    print(f"   gain {np.median(a_off) - np.median(a_on):.2f} us = {100 * (1 - np.median(a_on) / np.median(a_off)):.1f} %; every on-round faster than every off-round: {a_on.max() < a_off.min()}")
    diff = a_off - a_on   # the two trackers take turns inside a round: the round's drift is common to both
    q1, q3 = np.percentile(diff, [25, 75])
    print(f"   paired per round, off - on: median {np.median(diff):+.2f} us, quartiles {q1:+.2f} .. {q3:+.2f}, rounds with on faster: {(diff > 0).sum()} of {rounds}")
    pj_on = np.array([t for _, t in d["on"]]).reshape(rounds, len(pairs)).mean(0)
    pj_off = np.array([t for _, t in d["off"]]).reshape(rounds, len(pairs)).mean(0)
    print("   per pair, off - on: " + "  ".join(f"{b - a:+.2f}" for a, b in zip(pj_on, pj_off)))
on.close(), off.close()
