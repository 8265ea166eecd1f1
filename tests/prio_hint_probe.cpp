// Host-side probe of csrc/pagk_prio_env.h for tests/test_prio_hint_cpu.py: the header compiled by itself, as the library includes it.
#include "pagk_prio_env.h"

extern "C" int prio_hint_parse_probe(const char *text, int fallback) { return pagk::prio_hint_parse(text, fallback); }
extern "C" int prio_hint_default_probe() { return pagk::kPrioHintDefault; }
