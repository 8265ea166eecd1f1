// Probe of csrc/pagk_layout.h for tests/test_layout_cpu.py: the carver and the level workspace, as plain C calls.
#include "pagk_layout.h"

extern "C" uint64_t layout_probe(const uint64_t *sizes, int32_t count, uint64_t *off)
{
    size_t s[16] = {};
    for (int k = 0; k < count; k++) s[k] = (size_t)sizes[k];
    const pagk::Layout<16> lay(s, count);
    for (int k = 0; k < count; k++) off[k] = lay.off[k];
    return lay.total;
}

extern "C" void levels_probe(uint64_t n, uint64_t nq, int32_t pyramids, uint64_t *out6)
{
    const pagk::LevelsLayout l = pagk::levels_layout(n, nq, pyramids);
    const uint64_t v[6] = {l.ready, l.susp_count, l.susp_list, l.state, l.susp_state, l.total};
    for (int k = 0; k < 6; k++) out6[k] = v[k];
}
