/* results_ref.c -- the track-id rule of include/pagk.h ("The result ring of a sequence") restated sequentially in plain C: one
 * pass over the rows of the new key set in row order.  The library's own definition; the reference hands over
 * mvPtIndexInLastFrame only (src/frame.cpp:135,192).  tests/results_model.py is the same rule in numpy (a cumulative sum
 * instead of a running counter); the two must agree byte for byte. */
#include <stdint.h>

/* One frame.  index_in_last, id, age: cap rows; id_last, age_last: the previous frame's cap rows (not read at a start, where
 * no row has a predecessor).  *next_id is advanced by the frame's new rows; their number is returned. */
int32_t results_ref_frame(int32_t cap, int32_t n_live, const int32_t *index_in_last, const int64_t *id_last,
                          const int32_t *age_last, int64_t *next_id, int64_t *id, int32_t *age)
{
    int32_t n_new = 0;
    if (n_live < 0) n_live = 0;
    if (n_live > cap) n_live = cap;
    for (int32_t j = 0; j < cap; j++) {
        if (j >= n_live) {
            id[j] = -1;
            age[j] = 0;
        } else if (index_in_last[j] >= 0) {
            id[j] = id_last[index_in_last[j]];
            age[j] = age_last[index_in_last[j]] + 1;
        } else {
            id[j] = *next_id + n_new;
            age[j] = 0;
            n_new++;
        }
    }
    *next_id += n_new;
    return n_new;
}

/* A whole run: nf frames of cap rows each (index_in_last and the outputs frame after frame), n_live per frame; next_id and
 * n_new per frame out.  A start: next_id = 0. */
void results_ref_run(int32_t nf, int32_t cap, const int32_t *n_live, const int32_t *index_in_last, int64_t *id, int32_t *age,
                     int32_t *n_new, int64_t *next_id)
{
    int64_t next = 0;
    for (int32_t f = 0; f < nf; f++) {
        const int64_t o = (int64_t)f * cap, l = f ? o - cap : 0;
        n_new[f] = results_ref_frame(cap, n_live[f], index_in_last + o, id + l, age + l, &next, id + o, age + o);
        next_id[f] = next;
    }
}
