// pagk_select.h -- which tracking variant a launch runs, and the template arguments a half patch stands for.
// Host only: plain C++17, no HIP.  DESIGN.md section 4.3 has the rule as a table; tests/test_select_cpu.py holds it
// against the chain of booleans it replaced.
#pragma once

namespace pagk {

// What the tracking kernels' template arguments are for a half patch h (1..15): P = (2h + 1)^2 pixels per patch.
struct PatchShape {
    int P;         // pixels
    int nr, tail;  // 4-wave workgroup: rounds of 256 pixels, P mod 32 (an odd square: 1, 9, 17 or 25)
    int nch;       // chunks of 64 pixels (one wave per feature, four features per wave)
    int mfma_nr;   // 2-wave workgroup: rounds of 128 pixels
};

constexpr PatchShape patch_shape(int h)
{
    const int P = (2 * h + 1) * (2 * h + 1);
    return {P, (P + 255) / 256, P % 32, (P + 63) / 64, (P + 127) / 128};
}

// The patch sizes every variant is instantiated for; the others run the 4-wave kernel (or the thread kernel).
constexpr bool common_patch(int h) { return h == 5 || h == 7 || h == 10; }

struct SelectIn {
    int kernel;          // pagk_set_kernel: 0 = by launch size, 1..7 = that variant where it can run
    int half;
    bool calc_ncc;
    int pyramids, iterations;
    long long n;         // features of the launch
    int concurrency;     // pagk_set_concurrency: the automatic thresholds are applied to n * concurrency
    bool lv_error;       // the level workspace's error word exists
    bool levels_shared;  // PAGK_LEVELS_SHARED: variant 7 also for contexts that share the device
    int mfma_min, wave_min, quad_min, levels_min;
    bool all_variants;   // the build carries variants 2 and 6
};

// The variant (0..7, pagk_last_variant) of a launch.  A forced variant that cannot run these parameters falls to the
// next one that can: 7 -> 5 -> 3 -> 0, 6 -> 5.
inline int select_variant(const SelectIn &s)
{
    if (s.kernel == 1) return 1;                  // one thread per feature: any patch size
    if (!common_patch(s.half)) return 0;
    const long long n_sel = s.n * s.concurrency;
    const bool automatic = s.kernel == 0;
    const bool quad_like = s.kernel == 5 || s.kernel == 6 || s.kernel == 7;
    if (!s.calc_ncc) {                            // four features per wave: no NCC epilogue
        // one level per wave needs more than one level to differ from the quad kernel
        if (s.pyramids >= 2 && s.lv_error &&
            (s.kernel == 7 || (automatic && (s.concurrency == 1 || s.levels_shared) && n_sel >= s.levels_min)))
            return 7;
        if (s.all_variants && s.kernel == 6 && s.iterations >= 1) return 6;
        if (quad_like || (automatic && n_sel >= s.quad_min)) return 5;
    }
    if (s.kernel == 3 || quad_like || (automatic && n_sel >= s.wave_min)) return 3;
    if (s.kernel == 4) return 4;                  // relaxed-order experiment: never chosen automatically
    if (s.all_variants && (s.kernel == 2 || (automatic && n_sel >= s.mfma_min))) return 2;
    return 0;
}

// pagk_track_device_batch: one launch for all streams (total_q quads, total_n features), or each stream on its own?
inline bool select_batched(SelectIn s, long long total_n, int total_q)
{
    s.n = total_n;
    s.concurrency = 1;
    return total_q > 0 && select_variant(s) == 7;
}

// The 4-wave kernel at h = 10 with lean parameters: its build for five workgroups per CU, from block5_min features on
// and -- `window` -- for launches that five workgroups per CU hold in one round but four do not.
constexpr bool select_block5(long long n, int block5_min, bool window, int cus)
{
    return n >= block5_min || (window && n > 4ll * cus && n <= 5ll * cus);
}

}  // namespace pagk
