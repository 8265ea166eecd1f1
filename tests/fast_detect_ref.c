/* fast_detect_ref.c -- plain-C restatement of the FAST-cells-and-quadtree detector defined in include/pagk.h
 * (pagk_detect_fast_device): sequential and literal.  One loop over the cells, each a sub-image with its own score map;
 * the list of nodes is a doubly linked list of heap nodes with explicit creation numbers; the inner loop sorts
 * (size, creation number) pairs and walks them from the back.  Written from the definition, for the tests only. */
#include <assert.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define MIN_BORDER 16
#define CELL 30

typedef struct {
    int n_cols, n_rows, w_cell, h_cell, max_bx, max_by, n_ini;
    float hx;
} grid_t;

static int grid_of(int w, int h, grid_t *g)
{
    if (w < 62 || h < 62 || w > 32767 || h > 32767) return -1;
    g->max_bx = w - MIN_BORDER, g->max_by = h - MIN_BORDER;
    const float width = (float)(g->max_bx - MIN_BORDER), height = (float)(g->max_by - MIN_BORDER);
    g->n_cols = (int)(width / CELL), g->n_rows = (int)(height / CELL);
    if (g->n_cols < 1 || g->n_rows < 1) return -1;
    g->w_cell = (int)ceilf(width / g->n_cols), g->h_cell = (int)ceilf(height / g->n_rows);
    g->n_ini = (int)roundf(width / height);
    if (g->n_ini < 1) return -1;
    g->hx = width / g->n_ini;
    return 0;
}

int fdr_bounds(int w, int h, int n_features, int *raw_bound, int *out_bound)
{
    grid_t g;
    if (n_features < 1 || grid_of(w, h, &g)) return -1;
    *raw_bound = g.n_rows * g.n_cols * ((g.w_cell + 1) / 2) * ((g.h_cell + 1) / 2);
    *out_bound = n_features + 2 > 4 * g.n_ini ? n_features + 2 : 4 * g.n_ini;
    return 0;
}

/* the ring in OpenCV's order from (0, 3) */
static const int RX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
static const int RY[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};

static int m_of(const uint8_t *sub, int pitch, int x, int y)
{
    const int c = sub[y * pitch + x];
    int best = -1000;
    for (int start = 0; start < 16; start++)
        for (int pol = 0; pol < 2; pol++) {
            int lo = 1000;
            for (int k = 0; k < 9; k++) {
                const int r = (start + k) % 16;
                const int v = sub[(y + RY[r]) * pitch + x + RX[r]];
                const int d = pol ? c - v : v - c;
                if (d < lo) lo = d;
            }
            if (lo > best) best = lo;
        }
    return best;
}

/* FAST with non-maximum suppression on a w x h sub-image at threshold t -> keypoints in raster order; returns their number */
static int fast_sub(const uint8_t *sub, int pitch, int w, int h, int t, int *S, int *kx, int *ky, int *ks)
{
    memset(S, 0, sizeof(int) * (size_t)w * h);
    for (int y = 3; y < h - 3; y++)
        for (int x = 3; x < w - 3; x++) {
            const int m = m_of(sub, pitch, x, y);
            S[y * w + x] = m > t ? m - 1 : 0;
        }
    int n = 0;
    for (int y = 3; y < h - 3; y++)
        for (int x = 3; x < w - 3; x++) {
            const int s = S[y * w + x];
            int keep = 1;
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++)
                    if ((dx || dy) && !(s > S[(y + dy) * w + x + dx])) keep = 0;   /* (the ring of 3 around the region is 0) */
            if (keep) kx[n] = x, ky[n] = y, ks[n] = s, n++;
        }
    return n;
}

/* the raw list.  counts: [0] keys, [1] cells whose first pass was empty, [2] cells empty after both, [3] cells */
int fdr_cells(const uint8_t *img, int w, int h, int64_t step, int t_ini, int t_min, float *raw_xy, int *raw_score, int *counts)
{
    grid_t g;
    if (grid_of(w, h, &g)) return -1;
    int raw_bound, ob;
    fdr_bounds(w, h, 1, &raw_bound, &ob);
    const int seg = ((g.w_cell + 1) / 2) * ((g.h_cell + 1) / 2);
    int *S = malloc(sizeof(int) * 70 * 70), *kx = malloc(sizeof(int) * 70 * 70), *ky = malloc(sizeof(int) * 70 * 70),
        *ks = malloc(sizeof(int) * 70 * 70);
    int n = 0, first_empty = 0, empty = 0, cells = 0;
    for (int i = 0; i < g.n_rows; i++) {
        const int ini_y = MIN_BORDER + i * g.h_cell;
        int max_y = ini_y + g.h_cell + 6;
        if (ini_y >= g.max_by - 3) continue;
        if (max_y > g.max_by) max_y = g.max_by;
        for (int j = 0; j < g.n_cols; j++) {
            const int ini_x = MIN_BORDER + j * g.w_cell;
            int max_x = ini_x + g.w_cell + 6;
            if (ini_x >= g.max_bx - 6) continue;
            if (max_x > g.max_bx) max_x = g.max_bx;
            cells++;
            const uint8_t *sub = img + (int64_t)ini_y * step + ini_x;
            const int cw = max_x - ini_x, ch = max_y - ini_y;
            assert(cw <= 65 && ch <= 65);
            int k = fast_sub(sub, (int)step, cw, ch, t_ini, S, kx, ky, ks);
            if (k == 0) {
                first_empty++;
                k = fast_sub(sub, (int)step, cw, ch, t_min, S, kx, ky, ks);
                if (k == 0) empty++;
            }
            assert(k <= seg);   /* at most one pixel of any 2 x 2 block */
            for (int q = 0; q < k; q++) {
                assert(n < raw_bound);
                raw_xy[2 * n] = (float)(kx[q] + j * g.w_cell);
                raw_xy[2 * n + 1] = (float)(ky[q] + i * g.h_cell);
                raw_score[n] = ks[q];
                n++;
            }
        }
    }
    free(S), free(kx), free(ky), free(ks);
    counts[0] = n, counts[1] = first_empty, counts[2] = empty, counts[3] = cells;
    return 0;
}

/* ---- the list of nodes ---------------------------------------------------------------------------------------------- */
typedef struct node {
    int ulx, uly, urx, ury, blx, bly, brx, bry;
    int *keys, n_keys;
    int no_more, seq;
    struct node *prev, *next;
} node_t;

typedef struct {
    node_t *head, *tail;
    int size, next_seq;
} list_t;

static void push_front(list_t *L, node_t *n)
{
    n->seq = L->next_seq++;
    n->prev = NULL, n->next = L->head;
    if (L->head) L->head->prev = n;
    else L->tail = n;
    L->head = n;
    L->size++;
}
static void push_back(list_t *L, node_t *n)
{
    n->seq = L->next_seq++;
    n->next = NULL, n->prev = L->tail;
    if (L->tail) L->tail->next = n;
    else L->head = n;
    L->tail = n;
    L->size++;
}
static node_t *erase(list_t *L, node_t *n)   /* returns the node behind it */
{
    node_t *nx = n->next;
    if (n->prev) n->prev->next = n->next;
    else L->head = n->next;
    if (n->next) n->next->prev = n->prev;
    else L->tail = n->prev;
    L->size--;
    free(n->keys);
    free(n);
    return nx;
}

static node_t *new_node(int cap)
{
    node_t *n = calloc(1, sizeof *n);
    n->keys = malloc(sizeof(int) * (size_t)(cap > 0 ? cap : 1));
    return n;
}

/* ExtractorNode::DivideNode */
static void divide(const node_t *p, const float *xy, node_t *c[4])
{
    const int half_x = (int)ceilf((float)(p->urx - p->ulx) / 2), half_y = (int)ceilf((float)(p->bry - p->uly) / 2);
    for (int q = 0; q < 4; q++) c[q] = new_node(p->n_keys);
    node_t *n1 = c[0], *n2 = c[1], *n3 = c[2], *n4 = c[3];
    n1->ulx = p->ulx, n1->uly = p->uly, n1->urx = p->ulx + half_x, n1->ury = p->uly;
    n1->blx = p->ulx, n1->bly = p->uly + half_y, n1->brx = p->ulx + half_x, n1->bry = p->uly + half_y;
    n2->ulx = n1->urx, n2->uly = n1->ury, n2->urx = p->urx, n2->ury = p->ury;
    n2->blx = n1->brx, n2->bly = n1->bry, n2->brx = p->urx, n2->bry = p->uly + half_y;
    n3->ulx = n1->blx, n3->uly = n1->bly, n3->urx = n1->brx, n3->ury = n1->bry;
    n3->blx = p->blx, n3->bly = p->bly, n3->brx = n1->brx, n3->bry = p->bly;
    n4->ulx = n3->urx, n4->uly = n3->ury, n4->urx = n2->brx, n4->ury = n2->bry;
    n4->blx = n3->brx, n4->bly = n3->bry, n4->brx = p->brx, n4->bry = p->bry;
    for (int k = 0; k < p->n_keys; k++) {
        const int id = p->keys[k];
        const float x = xy[2 * id], y = xy[2 * id + 1];
        node_t *t;
        if (x < (float)n1->urx) t = y < (float)n1->bry ? n1 : n3;
        else t = y < (float)n1->bry ? n2 : n4;
        t->keys[t->n_keys++] = id;
    }
    for (int q = 0; q < 4; q++)
        if (c[q]->n_keys == 1) c[q]->no_more = 1;
}

typedef struct {
    int size, seq;
    node_t *node;
} cand_t;

static int g_reverse_tie;
static int cand_cmp(const void *a, const void *b)
{
    const cand_t *x = a, *y = b;
    if (x->size != y->size) return x->size < y->size ? -1 : 1;
    if (x->seq == y->seq) return 0;
    return ((x->seq < y->seq) != (g_reverse_tie != 0)) ? -1 : 1;
}

/* push the non-empty children to the front (n1 .. n4), note the ones with more than one key; returns how many those are */
static int push_children(list_t *L, node_t *c[4], cand_t *cand, int *n_cand)
{
    int more = 0;
    for (int q = 0; q < 4; q++) {
        if (c[q]->n_keys > 0) {
            push_front(L, c[q]);
            if (c[q]->n_keys > 1) {
                more++;
                cand[*n_cand].size = c[q]->n_keys, cand[*n_cand].seq = c[q]->seq, cand[*n_cand].node = c[q];
                (*n_cand)++;
            }
        } else {
            free(c[q]->keys);
            free(c[q]);
        }
    }
    return more;
}

/* The detector.  stats (or NULL): [0] pairs of equal size met by the inner loop's sorts, [1] inner passes, [2] nIni,
 * [3] the longest list seen.  reverse_tie != 0 turns the creation-number rule round (tests: is the rule exercised?). */
int fdr_detect(const uint8_t *img, int w, int h, int64_t step, const uint8_t *mask, int t_ini, int t_min, int n_features, int cap,
               float *kp, float *resp, int *info, int *stats, int reverse_tie)
{
    grid_t g;
    int raw_bound, out_bound;
    if (t_ini < 0 || t_ini > 255 || t_min < 0 || t_min > 255) return -1;
    if (fdr_bounds(w, h, n_features, &raw_bound, &out_bound) || cap < out_bound) return -1;
    grid_of(w, h, &g);
    float *xy = malloc(sizeof(float) * 2 * (size_t)raw_bound);
    int *score = malloc(sizeof(int) * (size_t)raw_bound);
    int counts[4];
    fdr_cells(img, w, h, step, t_ini, t_min, xy, score, counts);
    const int n = counts[0], N = n_features;
    g_reverse_tie = reverse_tie;

    list_t L = {NULL, NULL, 0, 0};
    const int min_x = MIN_BORDER, max_x = g.max_bx, min_y = MIN_BORDER, max_y = g.max_by;
    const int n_ini = (int)roundf((float)(max_x - min_x) / (max_y - min_y));
    const float hx = (float)(max_x - min_x) / n_ini;
    node_t **ini = malloc(sizeof(node_t *) * (size_t)n_ini);
    for (int i = 0; i < n_ini; i++) {
        node_t *ni = new_node(n);
        ni->ulx = (int)(hx * (float)i), ni->uly = 0;
        ni->urx = (int)(hx * (float)(i + 1)), ni->ury = 0;
        ni->blx = ni->ulx, ni->bly = max_y - min_y;
        ni->brx = ni->urx, ni->bry = max_y - min_y;
        push_back(&L, ni);
        ini[i] = ni;
    }
    for (int k = 0; k < n; k++) {
        node_t *t = ini[(int)(xy[2 * k] / hx)];
        t->keys[t->n_keys++] = k;
    }
    free(ini);
    for (node_t *it = L.head; it;) {
        if (it->n_keys == 1) it->no_more = 1, it = it->next;
        else if (it->n_keys == 0) it = erase(&L, it);
        else it = it->next;
    }
    cand_t *cand = malloc(sizeof(cand_t) * (size_t)(4 * out_bound + 4)), *prev_cand = malloc(sizeof(cand_t) * (size_t)(4 * out_bound + 4));
    int n_cand = 0, passes = 0, inner = 0, ties = 0, longest = L.size, finish = 0, first_round = 1;
    while (!finish) {
        passes++;
        const int prev_size = L.size;
        int to_expand = 0;
        n_cand = 0;
        node_t *it = L.head;
        /* (nodes pushed to the front during the walk lie in front of `it`: the walk does not meet them) */
        while (it) {
            if (it->no_more) {
                it = it->next;
                continue;
            }
            node_t *c[4];
            divide(it, xy, c);
            to_expand += push_children(&L, c, cand, &n_cand);
            it = erase(&L, it);
        }
        if (L.size > longest) longest = L.size;
        /* the bound of include/pagk.h: a full round ends at most at N, except the first, which ends at most at 4 * nIni */
        assert(L.size <= (first_round ? 4 * n_ini : (N > 4 * n_ini ? N : 4 * n_ini)));
        first_round = 0;
        if (L.size >= N || L.size == prev_size) {
            finish = 1;
        } else if (L.size + to_expand * 3 > N) {
            while (!finish) {
                passes++, inner++;
                const int prev2 = L.size;
                const int n_prev = n_cand;
                memcpy(prev_cand, cand, sizeof(cand_t) * (size_t)n_prev);
                n_cand = 0;
                qsort(prev_cand, (size_t)n_prev, sizeof(cand_t), cand_cmp);
                for (int j = 1; j < n_prev; j++) ties += prev_cand[j].size == prev_cand[j - 1].size;
                for (int j = n_prev - 1; j >= 0; j--) {
                    node_t *c[4];
                    divide(prev_cand[j].node, xy, c);
                    push_children(&L, c, cand, &n_cand);
                    erase(&L, prev_cand[j].node);
                    if (L.size > longest) longest = L.size;
                    assert(L.size <= N + 2);
                    if (L.size >= N) break;
                }
                if (L.size >= N || L.size == prev2) finish = 1;
            }
        }
    }
    assert(L.size <= out_bound);
    /* the best key of every node, list order; minBorder; the mask */
    int n_out = 0;
    for (node_t *it = L.head; it; it = it->next) {
        int b = it->keys[0];
        for (int k = 1; k < it->n_keys; k++)
            if (score[it->keys[k]] > score[b]) b = it->keys[k];
        const float x = xy[2 * b] + (float)min_x, y = xy[2 * b + 1] + (float)min_y;
        if (mask && mask[(int64_t)(int)y * w + (int)x] == 0) continue;
        kp[2 * n_out] = x, kp[2 * n_out + 1] = y;
        if (resp) resp[n_out] = (float)score[b];
        n_out++;
    }
    for (int i = n_out; i < cap; i++) {
        kp[2 * i] = kp[2 * i + 1] = 0.0f;
        if (resp) resp[i] = 0.0f;
    }
    memset(info, 0, sizeof(int) * 8);
    info[0] = n_out, info[1] = n, info[2] = counts[1], info[3] = counts[2], info[4] = L.size, info[5] = passes;
    if (stats) stats[0] = ties, stats[1] = inner, stats[2] = n_ini, stats[3] = longest;
    while (L.head) erase(&L, L.head);
    free(cand), free(prev_cand), free(xy), free(score);
    return 0;
}
