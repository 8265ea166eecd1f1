/* gyro_integrate_sanitize.c -- a stand-alone program around tests/gyro_integrate_ref.c, built with
 * -fsanitize=address,undefined by tests/test_gyro_integrate_cpu.py: it reads the edge table the test wrote (exact-length
 * heap arrays, so a read beyond a window is seen), runs the restatement on every case and prints the result bytes.
 * File: int32 cases; per case Rbc[9] f32, fx fy cx cy f32, t_ref t_cur f64, int32 n, int32 imu_cap, t[n] f64, w[3 n] f32,
 * bias[3] f32.  Output per case: the window check's code, the integration's code and 18 floats as hex words. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int gyro_ref_window_check(double t_ref, double t_cur, int32_t n, const double *t, const float *w, const float bias[3],
                          int32_t imu_cap);
int gyro_ref_integrate(const float Rbc[9], float fx, float fy, float cx, float cy, double t_ref, double t_cur, int32_t n_samples,
                       const double *t, const float *w, const float bias[3], float Rcl[9], float rot9[9]);
void gyro_ref_flow_velocity(int32_t cap, int32_t live, const float *normal_cur, const float *normal_last,
                            const int32_t *index_in_last, double t_cur, double t_last, float *v);

static int get(FILE *f, void *p, size_t bytes) { return bytes == 0 || fread(p, bytes, 1, f) == 1; }

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t cases = 0;
    if (!get(f, &cases, 4)) return 2;
    for (int32_t k = 0; k < cases; k++) {
        float Rbc[9], cam[4], bias[3];
        double tt[2];
        int32_t n = 0, cap = 0;
        if (!get(f, Rbc, sizeof Rbc) || !get(f, cam, sizeof cam) || !get(f, tt, sizeof tt) || !get(f, &n, 4) || !get(f, &cap, 4) ||
            n < 0 || n > 4096)
            return 2;
        double *t = malloc(n ? (size_t)n * 8 : 1);
        float *w = malloc(n ? (size_t)n * 12 : 1);
        if (!t || !w || !get(f, t, (size_t)n * 8) || !get(f, w, (size_t)n * 12) || !get(f, bias, sizeof bias)) return 2;
        float out[18];
        memset(out, 0, sizeof out);
        const int chk = gyro_ref_window_check(tt[0], tt[1], n, t, w, bias, cap);
        const int rc = chk ? chk : gyro_ref_integrate(Rbc, cam[0], cam[1], cam[2], cam[3], tt[0], tt[1], n, t, w, bias, out, out + 9);
        printf("%d %d", chk, rc);
        for (int j = 0; j < 18; j++) {
            uint32_t u;
            memcpy(&u, out + j, 4);
            printf(" %08x", u);
        }
        printf("\n");
        free(t);
        free(w);
    }
    fclose(f);
    /* the flow velocity on exact-length arrays: a survivor, a top-up row, a row beyond the live count */
    {
        const int32_t cap = 5, live = 4;
        float *cur = malloc(cap * 8), *last = malloc(cap * 8), *v = malloc(cap * 8);
        int32_t *idx = malloc(cap * 4);
        if (!cur || !last || !v || !idx) return 2;
        for (int j = 0; j < cap; j++) {
            cur[2 * j] = 0.01f * (float)j, cur[2 * j + 1] = -0.02f * (float)j;
            last[2 * j] = 0.015f * (float)j, last[2 * j + 1] = 0.005f;
            idx[j] = j == 1 ? -1 : cap - 1 - j;
        }
        gyro_ref_flow_velocity(cap, live, cur, last, idx, 2.5, 2.25, v);
        printf("velocity");
        for (int j = 0; j < 2 * cap; j++) {
            uint32_t u;
            memcpy(&u, v + j, 4);
            printf(" %08x", u);
        }
        printf("\n");
        free(cur), free(last), free(v), free(idx);
    }
    return 0;
}
