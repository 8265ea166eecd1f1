/* A stand-alone program for AddressSanitizer and UBSan: the restatement of "ORB over a scale pyramid"
 * (tests/orb_levels_ref.c, with tests/fast_detect_ref.c and tests/orb_ref.c) runs an extract and a masked detect at
 * 97 x 80 with 2 levels (the smallest legal two-level image) and at 160 x 120 with 4.  Every buffer is a heap block of
 * exactly its size, so that an access outside it is an error. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int olr_levels(int n_features, float scale_factor, int n_levels, int W, int H, int *lw, int *lh, float *sc, int *quota,
               int *size, int *out_bound);
int olr_extract(const uint8_t *img, int W, int H, int64_t step, int n_features, float scale_factor, int n_levels, int t_ini,
                int t_min, const int32_t *wt, const int32_t *pattern, const uint8_t *mask, int cap, float *kp, int32_t *octave,
                float *resp, float *angle, uint8_t *desc, int32_t *info, uint8_t *levels);

static uint32_t g_state = 12345u;
static uint32_t next_u32(void)
{
    g_state = g_state * 1664525u + 1013904223u;
    return g_state >> 8;
}

static int run(int W, int H, int n_levels, int n_features)
{
    int lw[8], lh[8], quota[8], size[8], cap;
    float sc[8];
    if (olr_levels(n_features, 1.2f, n_levels, W, H, lw, lh, sc, quota, size, &cap)) return 1;
    uint8_t *img = malloc((size_t)W * H), *mask = malloc((size_t)W * H);
    /* blocks of 8 x 8 pixels with random values: plenty of corners on every level */
    uint8_t block[64][64];
    for (int y = 0; y < 64; y++)
        for (int x = 0; x < 64; x++) block[y][x] = (uint8_t)(next_u32() & 255u);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            img[(size_t)y * W + x] = block[(y / 8) & 63][(x / 8) & 63];
            mask[(size_t)y * W + x] = (uint8_t)((x / 16 + y / 16) & 1);
        }
    int32_t pattern[1024];
    for (int k = 0; k < 1024; k++) pattern[k] = (int32_t)(next_u32() % 27u) - 13;
    const int32_t wt[4] = {54, 49, 34, 18};
    float *kp = malloc(sizeof(float) * 2 * (size_t)cap), *resp = malloc(sizeof(float) * (size_t)cap);
    float *angle = malloc(sizeof(float) * (size_t)cap);
    int32_t *octave = malloc(sizeof(int32_t) * (size_t)cap), info[32];
    uint8_t *desc = malloc((size_t)cap * 32);
    size_t px = 0;
    for (int l = 0; l < n_levels; l++) px += (size_t)lw[l] * lh[l];
    uint8_t *levels = malloc(px);
    int bad = 0;
    if (olr_extract(img, W, H, W, n_features, 1.2f, n_levels, 20, 7, wt, pattern, NULL, cap, kp, octave, resp, angle, desc, info,
                    levels))
        bad = 1;
    const int n_all = info[0];
    int sum = 0;
    for (int l = 0; l < n_levels; l++) sum += info[8 + l];
    if (sum != n_all || n_all < 1 || info[2] != n_levels) bad = 1;
    if (olr_extract(img, W, H, W, n_features, 1.2f, n_levels, 20, 7, wt, NULL, mask, cap, kp, octave, resp, NULL, NULL, info, NULL))
        bad = 1;
    if (info[0] >= n_all || info[0] < 1) bad = 1; /* the checkerboard mask drops some and keeps some */
    for (int k = 0; k < info[0]; k++)
        if (mask[(size_t)(int)kp[2 * k + 1] * W + (int)kp[2 * k]] == 0) bad = 1;
    printf("%d x %d, %d levels: %d keypoints, %d behind the mask\n", W, H, n_levels, n_all, info[0]);
    free(img), free(mask), free(kp), free(resp), free(angle), free(octave), free(desc), free(levels);
    return bad;
}

int main(void)
{
    int bad = run(97, 80, 2, 300);
    bad |= run(160, 120, 4, 400);
    bad |= run(160, 120, 4, 3); /* quotas 1 1 1 0 */
    if (!bad) printf("3 runs clean\n");
    return bad;
}
