/*
 * inverse_sanitize.c -- the restatement of the template-Jacobian mode (tests/inverse_ref.c) under AddressSanitizer and UBSan.
 *
 * A stand-alone program: compiled together with tests/inverse_ref.c and oracle/pagk_oracle.c with
 * -fsanitize=address,undefined and run as an executable (tests/test_inverse_cpu.py).  Every image, and every pyramid level
 * the restatement builds, sits in a heap block of exactly its size, so that a read outside it is an error.  Features sit on
 * and beyond every border, NaN, infinite and huge coordinates included, with and without the warp, the penalty and NCC.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../oracle/pagk_oracle.h"

int inverse_ref_track(const pagk_params *p, const pagk_image *ref, const pagk_image *cur, int32_t n, const float *pt_ref,
                      const float *pt_init, const float *affine, const uint8_t *status_in, const pagk_outputs *out);

static uint32_t rng_state = 0x5EED5A0Cu;
static uint32_t rng(void)
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

static uint8_t *texture(int w, int h, int shift)
{
    uint8_t *img = (uint8_t *)malloc((size_t)w * (size_t)h); /* exactly its size */
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            double v = 128 + 60 * sin(0.37 * (x + shift) + 0.11 * y) + 50 * cos(0.23 * y - 0.05 * (x + shift));
            img[(size_t)y * w + x] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
        }
    return img;
}

#define N 40

static int run(int w, int h, int levels, int half)
{
    uint8_t *a = texture(w, h, 0), *b = texture(w, h, 1);
    const pagk_image ia = {a, w, h, w}, ib = {b, w, h, w};
    float pt_ref[2 * N], pt_init[2 * N], affine[4 * N];
    uint8_t status_in[N];
    const float fw = (float)w, fh = (float)h;
    /* on and beyond every border, the corners, and coordinates no image holds */
    const float special[][2] = {{0, 0},          {fw - 1, 0},     {0, fh - 1},      {fw - 1, fh - 1}, {fw, fh},
                                {-1, -1},        {fw + 3, -2},    {-2.5f, fh + 7},  {fw * 0.5f, -40}, {fw * 0.5f, fh + 40},
                                {-1e30f, 1e30f}, {NAN, 3},        {4, NAN},         {INFINITY, 2},    {2, -INFINITY},
                                {0.5f, 0.5f},    {fw - 0.5f, fh - 0.5f}};
    const int ns = (int)(sizeof special / sizeof special[0]);
    for (int i = 0; i < N; i++) {
        if (i < ns) {
            pt_ref[2 * i] = special[i][0];
            pt_ref[2 * i + 1] = special[i][1];
        } else {
            pt_ref[2 * i] = (float)(rng() % (uint32_t)(w * 16)) / 16.0f;
            pt_ref[2 * i + 1] = (float)(rng() % (uint32_t)(h * 16)) / 16.0f;
        }
        pt_init[2 * i] = pt_ref[2 * i] + 1.25f;
        pt_init[2 * i + 1] = pt_ref[2 * i + 1] - 0.75f;
        affine[4 * i] = 1.02f, affine[4 * i + 1] = -0.03f, affine[4 * i + 2] = 0.04f, affine[4 * i + 3] = 0.97f;
        status_in[i] = (uint8_t)(i % 7 != 6);
    }
    float pt_un[2 * N], pt_dist[2 * N], ncc[N];
    uint8_t status[N];
    double pix_err[N], dist_pred[N];
    int32_t iters[N];
    const pagk_outputs out = {pt_un, pt_dist, status, pix_err, dist_pred, ncc, iters};
    int tracked = 0;
    for (int mode = 0; mode < 4; mode++) {
        pagk_params p;
        memset(&p, 0, sizeof p);
        p.half_patch = half, p.iterations = 8, p.pyramids = levels;
        p.inverse = PAGK_INVERSE_TEMPLATE;
        p.has_gyro_predict_initial = (uint8_t)(mode != 1);
        p.consider_illumination = (uint8_t)(mode != 2);
        p.consider_affine = (uint8_t)(mode & 1);
        p.regularization_penalty = (uint8_t)(mode >= 2);
        p.calculate_ncc = (uint8_t)(mode != 0);
        p.lambda = 1.0f, p.alpha = 0.5f, p.max_distance = 25;
        p.fx = p.fy = 200.0f, p.cx = fw * 0.5f, p.cy = fh * 0.5f;
        p.dist_coef[0] = mode == 3 ? -0.28f : 0.0f, p.dist_coef[1] = 0.07f, p.dist_coef[4] = 0.01f;
        p.n_dist_coef = mode == 3 ? 5 : 4;
        const int rc = inverse_ref_track(&p, &ia, &ib, N, pt_ref, pt_init, affine, status_in, &out);
        if (rc != PAGK_OK) {
            printf("%dx%d L%d h%d mode %d: rc %d\n", w, h, levels, half, mode, rc);
            return -1;
        }
        for (int i = 0; i < N; i++) tracked += status[i];
    }
    free(a);
    free(b);
    return tracked;
}

int main(void)
{
    const int cases[][4] = {{96, 64, 2, 5}, {40, 24, 4, 10}, {33, 31, 5, 1}, {64, 64, 7, 15}};
    int images = 0, tracked = 0;
    for (size_t k = 0; k < sizeof cases / sizeof cases[0]; k++) {
        const int t = run(cases[k][0], cases[k][1], cases[k][2], cases[k][3]);
        if (t < 0) return 1;
        tracked += t;
        images++;
    }
    printf("%d images, %d results with status 1\n", images, tracked);
    return 0;
}
