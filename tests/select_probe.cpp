// Probe of csrc/pagk_select.h for tests/test_select_cpu.py: the selection rule over arrays of inputs, as plain C calls.
#include <cstdint>

#include "pagk_select.h"

// rows of 14 int64: kernel, half, calc_ncc, pyramids, iterations, n, concurrency, lv_error, levels_shared,
//                   mfma_min, wave_min, quad_min, levels_min, all_variants
static pagk::SelectIn select_in(const int64_t *r)
{
    return {(int)r[0], (int)r[1], r[2] != 0, (int)r[3], (int)r[4], (long long)r[5], (int)r[6], r[7] != 0, r[8] != 0,
            (int)r[9], (int)r[10], (int)r[11], (int)r[12], r[13] != 0};
}

extern "C" void select_probe(const int64_t *rows, int64_t count, int32_t *variant)
{
    for (int64_t k = 0; k < count; k++) variant[k] = pagk::select_variant(select_in(rows + 14 * k));
}

// ... with two more columns: total_n, total_q of a batch (the row's own n and concurrency are then the lead context's)
extern "C" void batched_probe(const int64_t *rows, int64_t count, int32_t *batched)
{
    for (int64_t k = 0; k < count; k++) {
        const int64_t *r = rows + 16 * k;
        batched[k] = pagk::select_batched(select_in(r), (long long)r[14], (int)r[15]);
    }
}

extern "C" int32_t block5_probe(int64_t n, int32_t block5_min, int32_t window, int32_t cus)
{
    return pagk::select_block5((long long)n, block5_min, window != 0, cus);
}

extern "C" void shape_probe(int32_t h, int32_t *out5)
{
    const pagk::PatchShape s = pagk::patch_shape(h);
    const int32_t v[5] = {s.P, s.nr, s.tail, s.nch, s.mfma_nr};
    for (int k = 0; k < 5; k++) out5[k] = v[k];
}

extern "C" int32_t common_probe(int32_t h) { return pagk::common_patch(h); }
