// pagk_prio_env.h -- PAGK_PRIO_HINT as text (host only, no HIP: tests/test_prio_hint_cpu.py compiles it by itself).
//
// The hint's threshold (pagk_prio.h).  The default is what tools/prio_fluid_model.py chose on a sequence whose hints come from
// the previous pair.  The text is a whole non-negative number, 0 = off; signs, blanks, a trailing word or
// an overflow leave the fallback in place -- a mistyped knob must not silently switch the rule off.
#pragma once

namespace pagk {

constexpr int kPrioHintDefault = 14;

inline int prio_hint_parse(const char *text, int fallback)
{
    if (!text || !*text) return fallback;
    long v = 0;
    for (const char *c = text; *c; c++) {
        if (*c < '0' || *c > '9') return fallback;
        v = v * 10 + (*c - '0');
        if (v > 1000000) return fallback;
    }
    return (int)v;
}

}  // namespace pagk
