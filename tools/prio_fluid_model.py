"""A fluid model of one CU under the 4-wave kernels' issue-priority rule (csrc/pagk_prio.h), driven by the per-level iteration counts of a
workload (tools/iter_trace.py -> tools/data/*.npy).  A workgroup alone runs one iteration per LONE cycles and uses LONE_SHARE of the CU's VALU
while it does; workgroups share the VALU by strict priority, equals equally; a level set-up costs SETUP lone-equivalent cycles.  Workgroup i
starts on CU i mod 256 (4 slots per CU), a finished one is replaced by the next index.  The model knows nothing of memory, barriers or
the pipeline inside an iteration: it under-states the crowded launch by ~9 us, and it RANKS thresholds as the hardware does
(profiles/r04_ab8_priority_by_remaining_work.log): K = 4 < 3 ~ 5 < 6 at 1000 features.   python tools/prio_fluid_model.py
The HINT (pagk_prio.h): simulate(..., hint=h, T=t) starts workgroup i at priority 3 from its first iteration when h[i] > t; the cumulative
rule goes on applying to everyone.  `python tools/prio_fluid_model.py hint` prints the makespan over T with the workload's OWN counts as the
hint (a replayed frame pair: the benchmark) and with the PREVIOUS pair's counts over the sequence of tools/hint_pairs.py (a tracker), the
workgroups per CU that start boosted, and how much of each pair's slowest 2 % the previous pair's hint flags."""
import os, sys
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
LONE, SHARE, SETUP, GHZ = 6100.0, 2650.0, 1300.0, 2.4   # measured: lone iteration, crowded iteration / 4, level set-up (cycles)
U = SHARE / LONE

def simulate(it, policy, slots=4, ncu=256, dt=100.0, hint=None, T=0):
    n, L = it.shape
    nxt, live = 0, 0
    cus = [[] for _ in range(ncu)]
    def new(i): return dict(i=i, lv=L - 1, done=0.0, iters=0, cur=0, its=it[i], setup=SETUP, boost=bool(hint is not None and T > 0 and hint[i] > T))
    for _ in range(slots):
        for c in range(ncu):
            if nxt < n:
                cus[c].append(new(nxt)); nxt += 1; live += 1
    t, end = 0.0, 0.0
    while live:
        for alive in cus:
            if not alive:
                continue
            pr = [policy(s, L) for s in alive]
            cap, rate = 1.0, [0.0] * len(alive)
            for p in sorted(set(pr), reverse=True):
                idx = [k for k in range(len(alive)) if pr[k] == p]
                want = U * len(idx)
                give = U if want <= cap else cap / len(idx)
                for k in idx:
                    rate[k] = give
                cap = max(0.0, cap - want)
            fin = []
            for k, s in enumerate(alive):
                prog = rate[k] / U * dt
                if s["setup"] > 0:
                    s["setup"] -= prog
                    continue
                s["done"] += prog / LONE
                while s["done"] >= 1.0:
                    s["done"] -= 1.0; s["iters"] += 1; s["cur"] += 1
                    if s["cur"] >= s["its"][s["lv"]]:
                        s["cur"] = 0
                        if s["lv"] == 0:
                            fin.append(s); break
                        s["lv"] -= 1; s["setup"] = SETUP
            for s in fin:
                alive.remove(s); live -= 1; end = t + dt
                if nxt < n:
                    alive.append(new(nxt)); nxt += 1; live += 1
        t += dt
    return end / (GHZ * 1e3)

def by_phase_only(s, L): return 0
def behind(K): return lambda s, L: 3 if s["boost"] or s["iters"] + 1 > K * (L - s["lv"]) else 0

def boosted_per_cu(hint, T, slots=4, ncu=256):
    """Workgroups of the first round (workgroup i on CU i mod ncu, `slots` per CU) that start boosted: (mean per CU, CUs with more than one)."""
    first = np.asarray(hint[:slots * ncu]) > T if T > 0 else np.zeros(min(len(hint), slots * ncu), bool)
    per = np.bincount(np.arange(first.size) % ncu, weights=first, minlength=ncu)
    return float(per.mean()), int((per > 1).sum())

def flagged_share(hint, nxt, T, share=0.02):
    """The share of the next pair's slowest `share` of the features that hint > T flags."""
    k = max(1, int(round(share * len(nxt))))
    top = np.argsort(-np.asarray(nxt), kind="stable")[:k]
    return float((np.asarray(hint)[top] > T).mean())

def hint_tables(out=sys.stdout, K=4, Ts=(10, 12, 14, 15, 16, 17, 18, 19, 20, 22, 24)):
    seq = [np.loadtxt(os.path.join(HERE, "data", f"iters_seq_cfg1_1000_p{j}.txt"), dtype=int, ndmin=2) for j in range(7)]
    tot = [s.sum(1) for s in seq]
    pairs = list(range(1, 7))   # pair j tracked with pair j - 1's totals as the hint
    base = {j: simulate(seq[j], behind(K)) for j in range(7)}
    print(f"configs[1], 1000 features, K = {K}.  Makespan (us) of the fluid model; 'off' is the K rule alone.", file=out)
    print(f"(a) the hint is the pair's OWN counts (a replayed pair: the benchmark), pair 0 = tools/data/iters_cfg1_1000.npy: off {base[0]:.1f}", file=out)
    print("      T   makespan   gain   boosted/CU   CUs with > 1", file=out)
    exact = {}
    for T in Ts:
        exact[T] = simulate(seq[0], behind(K), hint=tot[0], T=T)
        m, c = boosted_per_cu(tot[0], T)
        print(f"    {T:3d}   {exact[T]:8.1f}  {base[0] - exact[T]:5.1f}   {m:10.3f}   {c:12d}", file=out)
    print(f"(b) the hint is the PREVIOUS pair's counts (tools/hint_pairs.py, pairs 1..6): off, mean of the six pairs {np.mean([base[j] for j in pairs]):.1f}", file=out)
    print("      T   mean makespan   mean gain   exact-hint gain on the same pairs   recovered   boosted/CU   top 2 % flagged", file=out)
    rows = {}
    for T in Ts:
        got = [simulate(seq[j], behind(K), hint=tot[j - 1], T=T) for j in pairs]
        own = [simulate(seq[j], behind(K), hint=tot[j], T=T) for j in pairs]
        g = np.mean([base[j] - x for j, x in zip(pairs, got)])
        ge = np.mean([base[j] - x for j, x in zip(pairs, own)])
        m = np.mean([boosted_per_cu(tot[j - 1], T)[0] for j in pairs])
        f = np.mean([flagged_share(tot[j - 1], tot[j], T) for j in pairs])
        rows[T] = (float(np.mean(got)), float(g), float(ge), m, f)
        print(f"    {T:3d}   {np.mean(got):13.1f}   {g:9.1f}   {ge:33.1f}   {g / ge if ge > 0 else float('nan'):9.2f}   {m:10.3f}   {f:15.2f}", file=out)
    best = min(Ts, key=lambda T: (round(rows[T][0], 1), T))   # (ties: the smallest T flags the most stragglers)
    best_exact = max(exact, key=lambda T: base[0] - exact[T])
    print(f"chosen T = {best} (the least mean makespan of (b)): sequence hints recover {rows[best][1]:.1f} us, exact hints at their best T = {best_exact} "
          f"recover {base[0] - exact[best_exact]:.1f} us on pair 0 and {max(r[2] for r in rows.values()):.1f} us on pairs 1..6", file=out)
    return best, rows, exact, base
def by_level(s, L): return s["lv"]

def dispatch_order(hint, key_max=127):
    """csrc/pagk_order.h: the features by clamped hint, descending, ties in index order (workgroup b runs feature order[b])."""
    return np.argsort(-np.clip(np.asarray(hint, np.int64), 0, key_max), kind="stable")

def simulate_ordered(it, hint, order, K=4, T=14, **kw):
    """simulate() with workgroup b running feature order[b]: the features and their hints are permuted, the placement rule is untouched."""
    return simulate(it[order], behind(K), hint=np.asarray(hint)[order], T=T, **kw)

def order_tables(out=sys.stdout, K=4):
    """`python tools/prio_fluid_model.py order`: the makespan with the workgroups in index order (today) and in hint-descending order,
    beside the slowest feature's own time -- the replayed pair (own counts), the sequence of tools/hint_pairs.py (the previous pair's
    counts), other orders on pair 0, and the launches of several rounds."""
    seq = [np.loadtxt(os.path.join(HERE, "data", f"iters_seq_cfg1_1000_p{j}.txt"), dtype=int, ndmin=2) for j in range(7)]
    tot = [s.sum(1) for s in seq]
    alone = lambda it: ((it.sum(1).max() * LONE + it.shape[1] * SETUP) / (GHZ * 1e3))   # noqa: E731
    ident = np.arange(1000)
    print(f"K = {K}, T = 14 per three levels, four slots per CU unless stated.  Makespan (us) of the fluid model.", file=out)
    print("workload, hint                                   identity   hint-descending   slowest feature alone", file=out)
    def row(name, it, hint, T=14, **kw):
        a = simulate_ordered(it, hint, np.arange(len(hint)), K, T, **kw)
        b = simulate_ordered(it, hint, dispatch_order(hint), K, T, **kw)
        print(f"{name:48s} {a:8.2f}   {b:15.2f}   {alone(it):21.2f}", file=out)
        return a, b
    rows = {0: row("configs[1] pair 0, own counts (a replayed pair)", seq[0], tot[0])}
    for j in range(1, 7):
        rows[j] = row(f"pair {j}, previous pair's counts", seq[j], tot[j - 1])
    d = [rows[j][1] - rows[j][0] for j in range(1, 7)]
    print(f"   pairs 1..6, ordered - identity: mean {np.mean(d):+.2f} us, worst {max(d):+.2f}, best {min(d):+.2f}", file=out)
    rng = np.random.default_rng(0)
    print("other orders on pair 0 (own counts):", file=out)
    for name, order in (("random permutation", rng.permutation(1000)), ("ascending", dispatch_order(tot[0])[::-1].copy()),
                        ("snake over the layers", _snake(tot[0]))):
        print(f"   {name:24s} {simulate_ordered(seq[0], tot[0], order, K):8.2f}", file=out)
    print(f"   {'snake, pair 3 with pair 2 counts':24s} {simulate_ordered(seq[3], tot[2], _snake(tot[2]), K):8.2f}", file=out)
    print("launches of several rounds (own counts):", file=out)
    for name, T, slots in (("iters_cfg2_2000.npy", 19, 4), ("iters_cfg1_2000.txt", 14, 4), ("iters_cfg1_1100.txt", 14, 5)):
        path = os.path.join(HERE, "data", name)
        it = (np.load(path) if name.endswith(".npy") else np.loadtxt(path, dtype=int, ndmin=2)).astype(int)
        row(f"{name[:-4]}, T = {T}, {slots} slots per CU", it, it.sum(1), T=T, slots=slots)
    return rows

def _snake(hint):
    """hint-descending with every other layer of 256 reversed: the longest features get the shortest CU-mates"""
    o = dispatch_order(hint).copy()
    for layer in range(1, (len(o) + 255) // 256, 2):
        o[layer * 256:(layer + 1) * 256] = o[layer * 256:(layer + 1) * 256][::-1].copy()
    return o

if __name__ == "__main__" and sys.argv[1:] == ["hint"]:
    hint_tables()
elif __name__ == "__main__" and sys.argv[1:] == ["order"]:
    order_tables()
elif __name__ == "__main__":
    for name in ("iters_cfg1_1000.npy", "iters_cfg2_2000.npy"):
        it = np.load(os.path.join(HERE, "data", name)).astype(int)
        tot = it.sum(1)
        print(f"{name}: mean {tot.mean():.2f} / max {tot.max()} iterations; the slowest feature alone: {(tot.max() * LONE + it.shape[1] * SETUP) / (GHZ * 1e3):.1f} us")
        print(f"   by phase only: {simulate(it, by_phase_only):6.1f} us")
        for K in (3, 4, 5, 6):
            print(f"   behind, K = {K}: {simulate(it, behind(K)):6.1f} us")
        print(f"   by level     : {simulate(it, by_level):6.1f} us")
