#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include "pagk.h"
#include "pagk_oracle.h"
/* Sanitizer driver of the oracle's sampler (built with -fsanitize=address,undefined by tests/test_sampler_cpu.py):
 * pagk_oracle_sample over the coordinate set of tests/sampler_cases.py -- every multiple of 0.25 in [-2, size + 2], the
 * float neighbours of 0, size - 1, size and of every integer position, -0.0, NaN, +-inf, +-1e30 -- on a 1 x 1 and a 2 x 1
 * image and on a 13 x 7 view of rows 16 bytes apart.  Every image is a heap block of exactly rows * step bytes, so a tap
 * outside the buffer is a report; every sample must be finite and within 0..255. */
static int axis(int size, float *v)
{
    int n = 0;
    for (int k = -8; k <= 4 * (size + 2); k++) v[n++] = (float)k * 0.25f;
    for (int p = 0; p <= size; p++) {
        v[n++] = nextafterf((float)p, -INFINITY);
        v[n++] = (float)p;
        v[n++] = nextafterf((float)p, INFINITY);
    }
    const float special[] = {-0.0f, NAN, INFINITY, -INFINITY, 1e30f, -1e30f};
    for (size_t k = 0; k < sizeof special / sizeof special[0]; k++) v[n++] = special[k];
    return n;
}

int main(void)
{
    const int shapes[3][3] = {{1, 1, 1}, {2, 1, 2}, {13, 7, 16}}; /* cols, rows, step */
    for (int s = 0; s < 3; s++) {
        const int cols = shapes[s][0], rows = shapes[s][1], step = shapes[s][2];
        unsigned char *data = malloc((size_t)rows * step);
        for (int i = 0; i < rows * step; i++) data[i] = (unsigned char)(1 + (i * 37 + s) % 255);
        float xs[256], ys[256];
        const int nx = axis(cols, xs), ny = axis(rows, ys), n = nx * ny;
        float *xy = malloc(sizeof(float) * 2 * (size_t)n), *out = malloc(sizeof(float) * (size_t)n);
        for (int i = 0; i < nx; i++)
            for (int j = 0; j < ny; j++) xy[2 * (i * ny + j)] = xs[i], xy[2 * (i * ny + j) + 1] = ys[j];
        pagk_image im = {data, cols, rows, step};
        int rc = pagk_oracle_sample(&im, n, xy, out);
        if (rc != PAGK_OK) { printf("image %d: rc %d\n", s, rc); return 1; }
        for (int i = 0; i < n; i++)
            if (!(out[i] >= 0.0f && out[i] <= 255.0f)) { printf("image %d: sample %d = %g\n", s, i, out[i]); return 1; }
        free(data); free(xy); free(out);
    }
    printf("sampler sanitize ok: 3 images\n");
    return 0;
}
