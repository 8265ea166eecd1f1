// Host-side probe of csrc/pagk_order.h for tests/test_dispatch_order_cpu.py: the header compiled by itself, as the library includes it.
#include "pagk_order.h"

extern "C" int order_key_probe(int hint) { return pagk::order_key(hint); }
extern "C" int order_key_max_probe() { return pagk::kOrderKeyMax; }
extern "C" int order_max_n_probe() { return pagk::kOrderMaxN; }
extern "C" int order_serves_probe(long long n, int cus) { return pagk::order_serves(n, cus); }
extern "C" void order_reference_probe(int n, const int *hints, int *order) { pagk::order_reference(n, hints, order); }

// The validity rule as a script: one state, driven by (op, n, stream, arg) records; every record's answer goes to out[].
//   0 build_n(stream; cus = 256, both arrays hold `arg` slots; the launch executes), and -- when it answers n > 0 -- built(n, stream, 0)
//   1 the same, recorded into a graph of the context (capture = 1)      2 ... into somebody else's graph (capture = 2)
//   3 usable(n, stream, capture = arg) -> answer, then launched(n, stream, answer, capture = arg)
//   4 hints_cleared      5 hints_set(n)      6 stream_idle(stream)      7 graphs_gone      8 usable(n, stream, 0) only
//   9 switch: on = arg   10 capture_ended -> did the capture record a build or a reader
//   11 replay(stream) of a graph that did -> must the caller wait for the device first      12 array_replaced
extern "C" void order_state_probe(int records, const int *script, int *out)
{
    pagk::OrderState st;
    static const int streams[4] = {0, 1, 2, 3};
    for (int k = 0; k < records; k++) {
        const int op = script[4 * k], n = script[4 * k + 1], arg = script[4 * k + 3];
        const void *stream = &streams[script[4 * k + 2] & 3];
        int ans = 0;
        switch (op) {
            case 0: case 1: case 2:
                ans = st.build_n(stream, 256, arg, arg, op);
                if (ans > 0) st.built(ans, stream, op);
                break;
            case 3:
                ans = st.usable(n, stream, 256, arg);
                st.launched(n, stream, ans != 0, arg);
                break;
            case 4: st.hints_cleared(); break;
            case 5: st.hints_set(n); break;
            case 6: st.stream_idle(stream); break;
            case 7: st.graphs_gone(); break;
            case 8: ans = st.usable(n, stream, 256, 0); break;
            case 9: st.on = arg != 0; break;
            case 10: ans = st.capture_ended(); break;
            case 11: ans = st.replay(stream); break;
            case 12: st.array_replaced(); break;
        }
        out[k] = ans;
    }
}
