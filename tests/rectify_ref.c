/* rectify_ref.c -- sequential plain-C restatement of the rectification defined in include/pagk.h ("rectification: a raw
 * camera frame into a frame slot"): cv::remap(INTER_LINEAR, BORDER_CONSTANT 0, planar CV_32FC1 maps) of an 8-bit image
 * with 1, 3 or 4 channels (reference Examples/Demo/RealSenseD435i.cpp:202, Examples/ROS/.../feature_tracker.cpp:137), and
 * the 8-bit RGB-to-gray step of Frame::Frame behind it (reference src/frame.cpp:81-87).  One pixel at a time, one step of
 * the header's text per statement; the tests compare the library with this byte for byte.
 * Build: gcc -O2 -ffp-contract=off (tests/rectify_ref_util.py). */
#include <math.h>
#include <stdint.h>

/* header "fixed point" + "no pixel": sx = rne(m * 32); 0 = no pixel */
static int fixed_point(float m, int32_t *s)
{
    float p = m * 32.0f;                     /* exact: a power of two (or +-inf on overflow) */
    if (!(fabsf(p) < 2147483648.0f)) return 0; /* NaN, +-inf, |m * 32| >= 2^31 */
    *s = (int32_t)nearbyintf(p);             /* round to nearest, ties to even (default rounding mode) */
    return 1;
}

/* header "split": sat_i16 */
static int32_t sat_i16(int32_t v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

/* header "taps": a tap outside [0, Ws) x [0, Hs) is 0 */
static int32_t tap(const uint8_t *src, int32_t Ws, int32_t Hs, int64_t step, int32_t cn, int32_t x, int32_t y, int32_t c)
{
    if (x < 0 || x >= Ws || y < 0 || y >= Hs) return 0;
    return src[(int64_t)y * step + (int64_t)x * cn + c];
}

/* The whole definition.  map_x / map_y: H rows of W floats, map_step bytes apart; src: Hs rows of src_step bytes, Ws
 * pixels of cn bytes; dst: H rows of W bytes, dst_step apart.  Returns 0, or -1 for arguments the header refuses. */
int32_t rcr_rectify(const float *map_x, const float *map_y, int32_t W, int32_t H, int64_t map_step, const uint8_t *src,
                    int32_t Ws, int32_t Hs, int64_t src_step, int32_t cn, const int32_t *gray_weight, int32_t gray_shift,
                    uint8_t *dst, int64_t dst_step)
{
    if (!map_x || !map_y || !src || !dst || W < 1 || H < 1) return -1;
    if (Ws < 1 || Hs < 1 || Ws > 32767 || Hs > 32767) return -1;            /* header "limits" */
    if (cn != 1 && cn != 3 && cn != 4) return -1;
    if (src_step < (int64_t)Ws * cn) return -1;
    if (cn != 1) {                                                          /* header: the rule for the weights */
        if (!gray_weight || gray_shift < 1 || gray_shift > 15) return -1;
        if (gray_weight[0] < 0 || gray_weight[1] < 0 || gray_weight[2] < 0) return -1;
        if ((int64_t)gray_weight[0] + gray_weight[1] + gray_weight[2] != ((int64_t)1 << gray_shift)) return -1;
    }
    for (int32_t r = 0; r < H; r++) {
        const float *mx = (const float *)((const char *)map_x + (int64_t)r * map_step);
        const float *my = (const float *)((const char *)map_y + (int64_t)r * map_step);
        for (int32_t c = 0; c < W; c++) {
            uint8_t *out = dst + (int64_t)r * dst_step + c;
            int32_t sx, sy;
            if (!fixed_point(mx[c], &sx) || !fixed_point(my[c], &sy)) {     /* header "no pixel" */
                *out = 0;
                continue;
            }
            /* header "split": arithmetic shift, mask on the two's-complement value */
            int32_t ix = sat_i16(sx >> 5), fx = sx & 31;
            int32_t iy = sat_i16(sy >> 5), fy = sy & 31;
            int32_t v[3] = {0, 0, 0};
            int32_t nv = cn == 1 ? 1 : 3;                                   /* header "gray": channel 3 is ignored */
            for (int32_t k = 0; k < nv; k++) {
                int32_t p00 = tap(src, Ws, Hs, src_step, cn, ix, iy, k);
                int32_t p01 = tap(src, Ws, Hs, src_step, cn, ix + 1, iy, k);
                int32_t p10 = tap(src, Ws, Hs, src_step, cn, ix, iy + 1, k);
                int32_t p11 = tap(src, Ws, Hs, src_step, cn, ix + 1, iy + 1, k);
                /* header "interpolate" */
                v[k] = (p00 * (32 - fx) * (32 - fy) + p01 * fx * (32 - fy) + p10 * (32 - fx) * fy + p11 * fx * fy + 512) >> 10;
            }
            if (cn == 1)
                *out = (uint8_t)v[0];
            else                                                            /* header "gray" */
                *out = (uint8_t)((v[0] * gray_weight[0] + v[1] * gray_weight[1] + v[2] * gray_weight[2] +
                                  (1 << (gray_shift - 1))) >> gray_shift);
        }
    }
    return 0;
}
