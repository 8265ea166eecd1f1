// pagk_layout.h -- how the host side carves one device block into parts.  Host only: plain C++17, no HIP.
#pragma once

#include <cstddef>
#include <cstdint>

namespace pagk {

constexpr size_t kPartAlign = 256;   // every part of a block starts on such a boundary

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Offsets of up to N parts laid one behind the other, and the bytes they take together.
template <int N>
struct Layout {
    size_t off[N] = {};
    size_t total = 0;
    Layout() = default;
    Layout(const size_t *sizes, int count) { carve(sizes, count); }
    explicit Layout(const size_t (&sizes)[N]) { carve(sizes, N); }
    template <class T>
    T *at(void *base, int k) const { return reinterpret_cast<T *>(static_cast<uint8_t *>(base) + off[k]); }

private:
    void carve(const size_t *sizes, int count)
    {
        for (int k = 0; k < count; k++) {
            off[k] = total;
            total = align_up(total + sizes[k], kPartAlign);
        }
    }
};

// The workspace of a one-level-per-wave launch (k_track_quad<.., LEVELS>) of n features in nq quads:
//   ticket counters | ready lists | hand-over count | hand-over list | float state[4] and SuspState per feature
// Everything up to the hand-over list must be zero before the launch and is cleared with one memset; the two state
// arrays follow each other unpadded.
constexpr size_t kLvCounterBytes = 32768;   // 8 ticket sequences of 4096 B
constexpr size_t kSuspCountBytes = 256;     // the hand-over count, alone in its part
constexpr size_t kLvStateBytes = 16;        // float state[4] of a feature
constexpr size_t kSuspStateBytes = 32;      // sizeof(SuspState), pagk_device.h

struct LevelsLayout {
    size_t ready, susp_count, susp_list, state, susp_state, total;
};

inline LevelsLayout levels_layout(size_t n, size_t nq, int pyramids)
{
    // a ready list per level below the top: 8 sequences x ceil(nq / 8) words
    const size_t sizes[5] = {kLvCounterBytes, (size_t)(pyramids - 1) * 8 * ((nq + 7) / 8) * 4, kSuspCountBytes, n * 4,
                             n * (kLvStateBytes + kSuspStateBytes)};
    const Layout<5> l(sizes);
    return {l.off[1], l.off[2], l.off[3], l.off[4], l.off[4] + n * kLvStateBytes, l.off[4] + sizes[4]};
}

}  // namespace pagk
