/* associate_ref.c -- the definition of include/pagk.h ("Track-to-detection association") restated sequentially in plain C, the
 * way the reference writes it: MatchFeatures with its std::set and erase loop (reference src/gyro_aided_tracker.cpp:949-1008),
 * the flow error of SearchByGyroPredict (:928-933), and Steps 1 to 4 of SearchByOpencvKLT (:1044-1130) with radiusMatch as a
 * sorted neighbour list, the std::set of found keypoints and the iterator loop of the disparity filter.  No dependencies.
 * Build: gcc -std=c99 -O2 -ffp-contract=off -shared -fPIC associate_ref.c -lm */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define ASSOC_INFO_WORDS 8
#define ASSOC_STATS_WORDS 8

/* std::set<int>: a sorted array */
typedef struct {
    int *v;
    size_t n, room;
} IntSet;

static int set_find(const IntSet *s, int key)
{
    size_t lo = 0, hi = s->n;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (s->v[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo < s->n && s->v[lo] == key;
}

static int set_insert(IntSet *s, int key)
{
    size_t pos = 0;
    if (set_find(s, key)) return 0;
    if (s->n == s->room) {
        const size_t room = s->room ? 2 * s->room : 16;
        int *v = (int *)realloc(s->v, room * sizeof(int));
        if (!v) return -1;
        s->v = v, s->room = room;
    }
    while (pos < s->n && s->v[pos] < key) pos++;
    memmove(s->v + pos + 1, s->v + pos, (s->n - pos) * sizeof(int));
    s->v[pos] = key, s->n++;
    return 0;
}

typedef struct {
    int queryIdx, trainIdx;
    float distance, ncc;
} sMatch;

/* MatchFeatures (:949-1008) and the flow error (:928-933).  Returns vMatches.size(), or -1 without memory. */
int assoc_ref_match(int32_t n, int32_t m, int32_t cap, const int32_t *count, const int32_t *nbr_idx, const float *nbr_dist,
                    const float *nbr_ncc, int32_t use_ncc, float th_high, float th_low, float th_ratio,
                    const float *keys_cur_un, const float *pt_predict_un, int32_t *match_query, int32_t *match_train,
                    float *match_dist, float *match_ncc, float *flows_err, int32_t *info)
{
    IntSet found = {0, 0, 0}, banned = {0, 0, 0};
    sMatch *vMatches = (sMatch *)malloc(sizeof(sMatch) * (size_t)(n > 0 ? n : 1));
    size_t size = 0;
    int rc = 0;
    if (!vMatches) return -1;
    memset(info, 0, sizeof(int32_t) * ASSOC_INFO_WORDS);
    for (int i = 0; i < n && !rc; i++) {
        const int c = count[i];
        const float *ncc = nbr_ncc + (size_t)i * cap, *dist = nbr_dist + (size_t)i * cap;
        sMatch _m;
        if (c <= 0) continue;              /* :955 */
        if (c > cap) {                     /* the library's rule: an over-long list takes part in nothing */
            info[1]++;
            continue;
        }
        if (use_ncc) {                     /* :959-975 */
            if (ncc[0] > th_high) {
            } else if (c > 1) {
                if (ncc[0] < th_low) continue;
                if (ncc[1] < ncc[0] * th_ratio) {
                } else
                    continue;
            } else
                continue;
        } else {                           /* :977-989 */
            if (c == 1) {
            } else if (dist[0] < dist[1] * th_ratio) {
            } else
                continue;
        }
        _m.queryIdx = i, _m.trainIdx = nbr_idx[(size_t)i * cap], _m.distance = dist[0], _m.ncc = ncc[0];
        if (_m.trainIdx < 0 || _m.trainIdx >= m) {   /* the library's rule: the reference has no such index */
            info[2]++;
            continue;
        }
        info[0]++;
        if (!set_find(&found, _m.trainIdx)) {        /* :993-996 */
            vMatches[size++] = _m;
            rc = set_insert(&found, _m.trainIdx);
        } else {                                     /* :997-1007 */
            size_t it = 0;
            while (it != size) {
                if (vMatches[it].trainIdx == _m.trainIdx) {
                    memmove(vMatches + it, vMatches + it + 1, (size - it - 1) * sizeof(sMatch));   /* it = erase(it) */
                    size--;
                } else
                    it++;
            }
            rc = set_insert(&banned, _m.trainIdx);
        }
    }
    if (!rc) {
        for (int k = 0; k < n; k++) {
            const int on = (size_t)k < size;
            match_query[k] = on ? vMatches[k].queryIdx : -1;
            match_train[k] = on ? vMatches[k].trainIdx : -1;
            if (match_dist) match_dist[k] = on ? vMatches[k].distance : 0.0f;
            if (match_ncc) match_ncc[k] = on ? vMatches[k].ncc : 0.0f;
        }
        if (flows_err) {                             /* :928-933 */
            for (int i = 0; i < n; i++) flows_err[2 * i] = flows_err[2 * i + 1] = 0.0f;
            for (size_t k = 0; k < size; k++) {
                const int q = vMatches[k].queryIdx, t = vMatches[k].trainIdx;
                flows_err[2 * q] = keys_cur_un[2 * t] - pt_predict_un[2 * q];
                flows_err[2 * q + 1] = keys_cur_un[2 * t + 1] - pt_predict_un[2 * q + 1];
            }
        }
        info[3] = (int32_t)banned.n, info[4] = (int32_t)size;
    }
    free(found.v), free(banned.v), free(vMatches);
    return rc ? -1 : (int)size;
}

typedef struct {
    int queryIdx, trainIdx;
    float distance;
} DMatch;

/* Steps 1 to 4 of SearchByOpencvKLT (:1044-1130) on Lucas-Kanade's outputs: status (after the err filter) and pt_lk, cap rows
 * of which the first n are live candidates.  Returns mvMatches.size(), or -1 without memory. */
int assoc_ref_klt(int32_t cap, int32_t n, int32_t m, const uint8_t *status, const float *pt_lk, const float *pt_ref,
                  const float *keys_cur, float max_distance, double ratio, double factor, int32_t *match_query,
                  int32_t *match_train, float *match_dist, double *disparity, double *stats, int32_t *info)
{
    const size_t rows = (size_t)(cap > 0 ? cap : 1), mm = (size_t)(m > 0 ? m : 1);
    int *find_index = (int *)malloc(sizeof(int) * rows);          /* pt_cur_klt_find_index */
    float *find = (float *)malloc(sizeof(float) * 2 * rows);      /* pt_cur_klt_find */
    DMatch *nn = (DMatch *)malloc(sizeof(DMatch) * mm);           /* nearest_neighbors[i] */
    DMatch *mvMatches = (DMatch *)malloc(sizeof(DMatch) * rows);
    double *mvDisparities = (double *)malloc(sizeof(double) * rows);
    IntSet found = {0, 0, 0};
    size_t nfind = 0, size = 0, before;
    double maxDisparity_1 = 0, sumDisparity_1 = 0, maxDisparity_2 = 0, sumDisparity_2 = 0, avgDisparity_1, avgDisparity_2, th;
    int rc = 0;
    if (!find_index || !find || !nn || !mvMatches || !mvDisparities) {
        free(find_index), free(find), free(nn), free(mvMatches), free(mvDisparities);
        return -1;
    }
    memset(info, 0, sizeof(int32_t) * ASSOC_INFO_WORDS);
    n = n < 0 ? 0 : (n > cap ? cap : n);
    m = m < 0 ? 0 : m;
    for (int i = 0; i < n; i++)                                    /* Step 1, :1047-1057 */
        if (status[i]) {
            find_index[nfind] = i;
            find[2 * nfind] = pt_lk[2 * i], find[2 * nfind + 1] = pt_lk[2 * i + 1];
            nfind++;
        }
    info[0] = (int32_t)nfind;
    for (size_t i = 0; i < nfind && !rc; i++) {
        size_t cnt = 0;
        DMatch _m;
        for (int j = 0; j < m; j++) {                              /* radiusMatch, :1067: within the radius, nearest first */
            const float dx = find[2 * i] - keys_cur[2 * j], dy = find[2 * i + 1] - keys_cur[2 * j + 1];
            const float d = sqrtf(dx * dx + dy * dy);
            if (d <= max_distance) {
                size_t p = cnt;
                while (p > 0 && d < nn[p - 1].distance) {          /* a stable insertion: equal distances keep their index order */
                    nn[p] = nn[p - 1];
                    p--;
                }
                nn[p].queryIdx = (int)i, nn[p].trainIdx = j, nn[p].distance = d;
                cnt++;
            }
        }
        info[cnt == 0 ? 1 : (cnt == 1 ? 2 : 3)]++;
        if (cnt == 1) {                                            /* :1076 */
            _m = nn[0];
        } else if (cnt > 1) {                                      /* :1079-1085 */
            const double r = nn[0].distance / nn[1].distance;
            if (r < ratio)
                _m = nn[0];
            else {
                info[4]++;
                continue;
            }
        } else
            continue;
        if (!set_find(&found, _m.trainIdx)) {                      /* :1089-1105 */
            const float *pr, *pc;
            double disp;
            _m.queryIdx = find_index[_m.queryIdx];
            mvMatches[size] = _m;
            pr = pt_ref + 2 * (size_t)_m.queryIdx, pc = keys_cur + 2 * (size_t)_m.trainIdx;
            disp = sqrtf((pr[0] - pc[0]) * (pr[0] - pc[0]) + (pr[1] - pc[1]) * (pr[1] - pc[1]));
            mvDisparities[size++] = disp;
            sumDisparity_1 += disp;
            maxDisparity_1 = disp > maxDisparity_1 ? disp : maxDisparity_1;
            rc = set_insert(&found, _m.trainIdx);
        } else
            info[5]++;
    }
    avgDisparity_1 = sumDisparity_1 / (double)size;                /* :1109 */
    th = avgDisparity_1 * factor;                                  /* :1116 */
    before = size;
    {
        size_t it = 0;                                             /* itDisp and itMatch move together, :1117-1129 */
        while (it != size) {
            if (mvDisparities[it] > th) {
                memmove(mvDisparities + it, mvDisparities + it + 1, (size - it - 1) * sizeof(double));
                memmove(mvMatches + it, mvMatches + it + 1, (size - it - 1) * sizeof(DMatch));
                size--;
            } else {
                sumDisparity_2 += mvDisparities[it];
                maxDisparity_2 = mvDisparities[it] > maxDisparity_2 ? mvDisparities[it] : maxDisparity_2;
                it++;
            }
        }
    }
    avgDisparity_2 = sumDisparity_2 / (double)size;                /* :1130 */
    for (int k = 0; k < cap; k++) {
        const int on = (size_t)k < size;
        match_query[k] = on ? mvMatches[k].queryIdx : -1;
        match_train[k] = on ? mvMatches[k].trainIdx : -1;
        if (match_dist) match_dist[k] = on ? mvMatches[k].distance : 0.0f;
        disparity[k] = on ? mvDisparities[k] : 0.0;
    }
    info[6] = (int32_t)(before - size), info[7] = (int32_t)size;
    if (stats) {
        stats[0] = avgDisparity_1, stats[1] = avgDisparity_2, stats[2] = maxDisparity_1, stats[3] = maxDisparity_2;
        stats[4] = th, stats[5] = sumDisparity_1, stats[6] = sumDisparity_2, stats[7] = 0.0;
    }
    free(find_index), free(find), free(nn), free(mvMatches), free(mvDisparities), free(found.v);
    return rc ? -1 : (int)size;
}
