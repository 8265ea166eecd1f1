// pagk_order.h -- which feature each workgroup of a 4-wave launch runs: longest first by last launch's counts.
// Host only: plain C++17, no HIP (the kernel that builds the array is order_block in pagk_kernels.h; tests/test_dispatch_order_cpu.py
// compiles this header by itself).  DESIGN.md section 4.4 has the why and the figures.
//
// The hardware places workgroup b of a launch on CU b mod (number of CUs) while every workgroup is resident, and hands the rest out in
// index order as slots free up.  order[b] = the feature with the b-th largest hint (pagk_prio.h: the iterations the slot ran in the
// previous launch) therefore puts the longest features on different CUs, gives each of them the next layers down as CU-mates, and is
// longest-processing-time-first list scheduling for a launch of several rounds.  The order decides WHEN a feature runs and beside whom,
// never what it computes: every other index of the kernels (inputs, outputs, hints) stays the feature's.
//
// The rule: a stable counting sort of the keys, descending, ties in index order; key = the hint clamped to [0, kOrderKeyMax]
// (pagk_prio_hint_set accepts any int32).  A zeroed hint array gives the identity.
#pragma once

#include <cstdint>

namespace pagk {

constexpr int kOrderKeyMax = 127;    // 30 iterations on each of four levels is 120: every count of the BASELINE shapes is its own class
constexpr int kOrderClasses = kOrderKeyMax + 1;
constexpr int kOrderMaxN = 8192;     // the builder's LDS copy of the keys: one byte per feature (the 4-wave kernels serve up to ~6000)

constexpr int order_key(int32_t hint) { return hint < 0 ? 0 : (hint > kOrderKeyMax ? kOrderKeyMax : (int)hint); }

// The contract of the device build (and of pagk_dispatch_order_get), restated on the host.
inline void order_reference(int n, const int32_t *hints, int32_t *order)
{
    int start[kOrderClasses + 1] = {};
    for (int i = 0; i < n; i++) start[kOrderKeyMax - order_key(hints[i]) + 1]++;   // class 0 = the largest key
    for (int c = 0; c < kOrderClasses; c++) start[c + 1] += start[c];
    for (int i = 0; i < n; i++) order[start[kOrderKeyMax - order_key(hints[i])]++] = i;
}

// LDS of the workgroup that builds the order of n features: 4 x kOrderClasses counters, then a class number per feature.
constexpr unsigned order_lds_bytes(int n) { return n > 0 ? 4u * kOrderClasses * 4u + (((unsigned)n + 255u) & ~255u) : 0u; }

// Is a launch of n features one the order applies to?  More than a workgroup per CU (below that nobody shares a CU), and what the
// builder's LDS holds.
constexpr bool order_serves(long long n, int cus) { return n > cus && n <= kOrderMaxN; }

// What the host knows about the order array, and the conservative rule by which a launch may use it.  A stream is an opaque handle.
// A launch gets the array only when ALL of this holds, otherwise null (the kernel then runs the identity):
//   - a build for exactly this n was enqueued on this stream since the last hinted launch or hint write (the array then is a
//     permutation of [0, n) made from the counts this launch's features ran last);
//   - nothing cleared or rewrote the hints since (new features in the slots: their old counts forecast nothing);
//   - nobody rewrites the array while a launch may read it.  The array is BOUND to one stream, `home`: the stream on which its last
//     build, its last reader or the last replay of a graph that holds either was enqueued for execution.  It stays bound until the host
//     has waited for that stream; meanwhile no other stream builds or reads, so stream order separates every writer from every reader.
//     The pyramid blocks of a reader's own launch never build.  A replay binds the array to the stream it is launched on, and one that
//     finds it bound elsewhere must wait for the device first (replay() says so): its nodes cannot be taken back;
//   - no live graph froze the array for another n (a replayed node would index n features with a permutation of another length).
// What is recorded into a graph has not run: it binds nothing and leaves no build behind (capture_ended()).  A capture that is not
// the context's own (`capture` 2: nobody tells us when its graph is replayed or dies) neither builds nor reads.
struct OrderState {
    bool on = true;              // PAGK_DISPATCH_ORDER=0: identity everywhere, nothing is built
    int want_n = 0;              // n of the last hinted 4-wave launch: what the next pyramid launch builds for (0: nothing)
    int built_n = 0;             // a build for this n is enqueued and still current (0: none)
    const void *built_on = nullptr;   // ... on this stream
    const void *home = nullptr;  // the stream the array is bound to (null: none yet, or the host has waited for it)
    int frozen_n = 0;            // a live graph of the context holds a launch that reads, or a build that writes, the array for this n (0: none)
    bool in_capture = false;     // the open capture has recorded such a node

    // a pyramid launch on `stream` is about to be enqueued: the n its order workgroup builds for, or 0 for none
    // (`capture`: 0 the launch executes, 1 it is recorded into a graph of the context, 2 into any other graph)
    int build_n(const void *stream, int cus, long long hint_slots, long long order_slots, int capture) const
    {
        if (!on || capture == 2 || !order_serves(want_n, cus) || hint_slots < want_n || order_slots < want_n) return 0;
        if (home && home != stream) return 0;                // bound to another stream: a build or a reader may still be running there
        if (frozen_n && frozen_n != want_n) return 0;        // a live graph reads it as a permutation of another length
        return want_n;
    }
    void built(int n, const void *stream, int capture)
    {
        built_n = n;
        built_on = stream;
        touch(n, stream, capture);
    }
    // a hinted 4-wave launch of n features on `stream` is about to be enqueued: may it read the array?
    bool usable(int n, const void *stream, int cus, int capture) const
    {
        return on && capture != 2 && order_serves(n, cus) && built_n == n && built_on == stream && (!home || home == stream) &&
               (!frozen_n || frozen_n == n);
    }
    // ... and it was enqueued (`used`: with the array): it rewrites the hints, so the build is history
    void launched(int n, const void *stream, bool used, int capture)
    {
        want_n = n;
        built_n = 0;
        if (used) touch(n, stream, capture);
    }
    // the context's capture is over: did it record a build or a reader (then its graph's replays go through replay())?  A build that
    // was only recorded has not run, so no launch behind the capture may count on it.
    bool capture_ended()
    {
        const bool carried = in_capture;
        in_capture = false;
        built_n = 0;
        return carried;
    }
    // a graph that holds a build or a reader is about to be replayed on `stream`: true when the caller must wait for the device first
    bool replay(const void *stream)
    {
        const bool elsewhere = home && home != stream;
        home = stream;
        built_n = 0;
        return elsewhere;
    }
    // the hints were zeroed (new features in the slots; the host-buffer calls): equal counts sort to the identity, nothing to build
    void hints_cleared() { built_n = want_n = 0; }
    // the caller installed n hints of its own (pagk_prio_hint_set): the next pyramid launch sorts them
    void hints_set(int n) { built_n = 0, want_n = n; }
    void array_replaced() { built_n = 0; }                   // the buffer grew: nothing built is left
    void stream_idle(const void *stream) { if (home == stream) home = nullptr; }   // the host waited for `stream`
    void graphs_gone() { frozen_n = 0; }                     // the context's last graph was destroyed

private:
    void touch(int n, const void *stream, int capture)
    {
        if (capture) frozen_n = n, in_capture = true;
        else home = stream;
    }
};

}  // namespace pagk
