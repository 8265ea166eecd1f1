/* pagk_oracle_cv.h -- part of the CPU oracle (TEST INFRASTRUCTURE, see pagk_oracle.h): OpenCV's arithmetic under the
 * reference's src/ORBextractor.cc.  A header of its own, so that the programs that include pagk_oracle.h alone
 * (oracle/_ref/ref_patchmatch, ref_tracker) do not change with it. */
#ifndef PAGK_ORACLE_CV_H
#define PAGK_ORACLE_CV_H

#include "pagk_oracle.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- OpenCV's arithmetic under the reference's src/ORBextractor.cc (third-party arithmetic: this project's definition as
 * include/pagk.h states it, oracle/README.md).  The stand-in OpenCV of oracle/ref_shim/orb calls these; the restatements
 * tests/fast_detect_ref.c, tests/orb_ref.c and tests/orb_levels_ref.c keep copies of their own (they build stand-alone), and
 * tests/test_reference_orb_cpu.py holds every copy byte-equal to these ------------------------------------------------------ */
/* cv::FAST(sub, keys, threshold, true) on a w x h sub-image with a row step: m(p) over the 9-arcs of the 16-ring, score
 * m - 1 where m > threshold, strict 3 x 3 non-maximum suppression inside the sub-image (what lies outside counts as 0),
 * raster order.  xys: cap x 3 (x, y, score).  Returns the count, or PAGK_E_ARG where cap is too small. */
int pagk_oracle_fast9(const uint8_t *sub, int64_t step, int32_t w, int32_t h, int32_t threshold, int32_t cap, int32_t *xys);
/* cv::resize(src, dst, Size(dw, dh), 0, 0, INTER_LINEAR) on 8UC1 */
int pagk_oracle_resize_linear(const uint8_t *src, int32_t sw, int32_t sh, int64_t sstep, uint8_t *dst, int32_t dw, int32_t dh,
                              int64_t dstep);
/* copyMakeBorder(..., border on every side, BORDER_REFLECT_101): buf holds (w + 2 border) x (h + 2 border) bytes whose
 * interior (the w x h image at (border, border)) is set; the border is filled from the interior alone (BORDER_ISOLATED or not:
 * the same).  fill >= 0: the border is that byte instead (tests: does anything read it?). */
int pagk_oracle_border_reflect101(uint8_t *buf, int64_t step, int32_t w, int32_t h, int32_t border, int32_t fill);
/* GaussianBlur(Size(7, 7), 2, 2, BORDER_REFLECT_101) on 8UC1 in Q8 taps wt[|k|] (54, 49, 34, 18): rows, then columns, one
 * rounding (+ 32768) >> 16.  out may not alias img. */
int pagk_oracle_blur7(const uint8_t *img, int32_t w, int32_t h, int64_t step, const int32_t *wt, uint8_t *out, int64_t ostep);
/* cv::fastAtan2: the f32 polynomial, degrees in [0, 360) */
float pagk_oracle_fast_atan2(float y, float x);
/* pow(base, n) for an integer n in [0, 64]: the repeated product from 1.0, n factors.  *ok = 0 (and 0.0) for any other n. */
double pagk_oracle_pow_int(double base, double n, int32_t *ok);

#ifdef __cplusplus
}
#endif
#endif
