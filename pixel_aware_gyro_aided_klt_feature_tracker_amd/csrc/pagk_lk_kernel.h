// pagk_lk_kernel.h -- pyramidal Lucas-Kanade, the image-only baseline of the reference's comparison (tracker type 0,
// reference src/gyro_aided_tracker.cpp:353-380).  The definition is in include/pagk.h ("Pyramidal Lucas-Kanade");
// tests/lk_ref.c restates it in plain C.
//
// Shapes:
//   k_lk_pyrdown  one thread per pixel of level l + 1: the 25 taps of level l through the reflected index, exact integers.
//   k_lk_track    one wavefront per feature, four features per workgroup, the levels of a feature in a loop (they depend on
//                 each other).  A lane owns NPIX = ceil(win^2 / 64) window pixels (rounded up to a power of two: one
//                 instantiation each) and keeps their Ival and the packed (ix, iy) pair in registers for the level.  The
//                 wave stages a (win + 3)^2 tile of I in its own part of the LDS, the border reflected while loading, and
//                 forms the Scharr derivatives from it (zero at positions outside the level): no derivative plane exists.
//                 Every iteration stages the (win + 1)^2 tile of J the same way.  The per-lane partial sums are int32 (at
//                 most 16 terms of at most 3.4e7), the sums over the wave are int64 butterflies: exact, so every lane holds
//                 the same integers and runs the same f32 tail, one rounding per operation -- every branch of the level
//                 loop is uniform over the wave.  The tile is private to the wave, whose LDS accesses complete in program
//                 order: the kernel has no workgroup barrier at all.  The counters are integer atomics.
//   k_lk_flow     the same wavefront per feature started from an initial point (OpenCV 3.4's OPTFLOW_USE_INITIAL_FLOW
//                 branch, the reference's open experiment at :364-365), live rows only (status_in), the distorted point
//                 (:379, DistortVecPoints) written by lane 0 in the epilogue.  Both kernels are the text of pagk_lk_body.h:
//                 one body, so the two cannot drift; with pt_init bit-equal to pt_ref and every status_in set the outputs
//                 are those of k_lk_track byte for byte.
// No launch is sized by a count: the grid comes from the capacity, the count is read on the device.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pagk {

constexpr int kLkInfoWords = 8;    // PAGK_LK_INFO_WORDS
constexpr int kLkMaxLevels = 8;    // PAGK_MAX_PYRAMIDS: levels 0 .. 7
constexpr int kLkMaxWin = 31;      // 2 * PAGK_MAX_HALF_PATCH + 1
constexpr int kLkMaxRows = 1 << 24;

// BORDER_REFLECT_101 for i in [-n + 1, 2 n - 2]; any other i is clamped into the level (such a pixel only feeds a
// derivative at a position outside the level, which is zero by the definition)
__device__ __forceinline__ int lk_reflect(int i, int n)
{
    i = i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i);
    return min(max(i, 0), n - 1);
}

// ---- the pyramid ----------------------------------------------------------------------------------------------------
struct LkPyrArgs {
    const uint8_t *src;   // sh rows of spitch bytes
    long long spitch;
    uint8_t *dst;         // dh rows of dw bytes
    int sw, sh, dw, dh;
};

// the body of k_lk_pyrdown and of k_group_lk_pyrdown (pagk_group_lk_kernel.h): blockIdx.x and blockIdx.y tile the level.
// (The arguments one by one, as the other *_body functions take theirs: behind a struct the compiler schedules the kernel differently.)
__device__ __forceinline__ void lk_pyrdown_body(const uint8_t *src, long long spitch, uint8_t *dst, int sw, int sh, int dw, int dh)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= dw || y >= dh) return;
    int cx[5];
#pragma unroll
    for (int i = 0; i < 5; i++) cx[i] = lk_reflect(2 * x + i - 2, sw);
    int s = 128;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const uint8_t *row = src + (long long)lk_reflect(2 * y + j - 2, sh) * spitch;
        const int r = row[cx[0]] + row[cx[4]] + 4 * (row[cx[1]] + row[cx[3]]) + 6 * row[cx[2]];
        s += (j == 0 || j == 4 ? 1 : (j == 2 ? 6 : 4)) * r;
    }
    dst[(size_t)y * dw + x] = (uint8_t)(s >> 8);
}

__global__ __launch_bounds__(256) void k_lk_pyrdown(LkPyrArgs a) { lk_pyrdown_body(a.src, a.spitch, a.dst, a.sw, a.sh, a.dw, a.dh); }

// ---- the tracker ----------------------------------------------------------------------------------------------------
struct LkLevel {
    const uint8_t *I, *J;   // the level of the reference and of the current frame
    long long pitch_i, pitch_j;
    int w, h;
};

struct LkTrackArgs {
    LkLevel lv[kLkMaxLevels];
    const float *pt_ref;    // cap x 2
    const int32_t *n;       // device count, or nullptr: cap
    float *pt_out;          // cap x 2
    uint8_t *status;        // cap
    uint8_t *status_raw;    // cap, or nullptr
    float *err;             // cap
    float *flow;            // cap x 2, or nullptr
    int32_t *info;          // kLkInfoWords, zeroed before the launch
    double eps2;            // epsilon * epsilon
    double min_eig;
    float err_threshold;
    int cap, win, top, max_count;
};

// what k_lk_flow takes on top of LkTrackArgs
struct LkFlowArgs {
    LkTrackArgs t;
    const float *pt_init;      // cap x 2, or nullptr: pt_ref
    const uint8_t *status_in;  // cap, or nullptr: every row below the count is live
    float *pt_out_dist;        // cap x 2, or nullptr
    // the camera of DistortVecPoints (src/utils.cpp:49-76), as fill_param_args takes it from pagk_params
    float fx, fy, cx, cy, fx_inv, fy_inv, k1, k2, p1, p2, k3;
    int distort_on;            // dist_coef[0] != 0
};

// the largest window an instantiation serves, and the bytes of its tile
__host__ __device__ constexpr int lk_max_win(int npix) { return npix == 1 ? 7 : npix == 2 ? 11 : npix == 4 ? 15 : npix == 8 ? 21 : 31; }
__host__ __device__ constexpr int lk_tile_bytes(int npix) { return ((lk_max_win(npix) + 3) * (lk_max_win(npix) + 3) + 15) & ~15; }
// the instantiation of a window: the smallest power of two with 64 NPIX >= win^2
constexpr int lk_npix(int win) { return win <= 7 ? 1 : win <= 11 ? 2 : win <= 15 ? 4 : win <= 21 ? 8 : 16; }

// i / d for 0 <= i < d^2 and 2 <= d <= 34 as (i * lk_magic(d)) >> 16
__host__ __device__ constexpr unsigned lk_magic(int d) { return 65536u / (unsigned)d + 1u; }
constexpr bool lk_magic_ok()
{
    for (int d = 2; d <= kLkMaxWin + 3; d++)
        for (int i = 0; i < d * d; i++)
            if ((int)(((unsigned)i * lk_magic(d)) >> 16) != i / d) return false;
    return true;
}
static_assert(lk_magic_ok(), "the reciprocal multiply must divide every tile and window index exactly");

// step 2 of the definition: the range test on the floored coordinates in f32 (a NaN fails the finiteness test)
__device__ __forceinline__ bool lk_out_of_range(float fx, float fy, int win, int w, int h)
{
    if (!(fabsf(fx) < __builtin_inff()) || !(fabsf(fy) < __builtin_inff())) return true;
    return fx < (float)-win || fx >= (float)w || fy < (float)-win || fy >= (float)h;
}

// step 3
__device__ __forceinline__ void lk_weights(float a, float b, int &w00, int &w01, int &w10, int &w11)
{
    w00 = (int)rintf((1.f - a) * (1.f - b) * 16384.f);
    w01 = (int)rintf(a * (1.f - b) * 16384.f);
    w10 = (int)rintf((1.f - a) * b * 16384.f);
    w11 = 16384 - w00 - w01 - w10;
}

// side x side pixels of a level from (x0, y0) into the wave's tile (rows of `side` bytes), the border reflected
__device__ __forceinline__ void lk_stage(uint8_t *tile, const uint8_t *img, long long pitch, int w, int h, int x0, int y0,
                                         int side, int lane)
{
    const unsigned magic = lk_magic(side);
    for (int i = lane; i < side * side; i += 64) {
        const int ty = (int)(((unsigned)i * magic) >> 16), tx = i - ty * side;
        tile[i] = img[(long long)lk_reflect(y0 + ty, h) * pitch + lk_reflect(x0 + tx, w)];
    }
}

// The wave's LDS accesses complete in program order; this keeps the compiler from moving them across the hand-over
// between the lanes that wrote a tile and the lanes that read it.  It stands on both sides of every lk_stage: in front of
// it (the lanes that still read the tile before) and behind it (the lanes that read this one).
__device__ __forceinline__ void lk_tile_handover()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ long long lk_wave_sum(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ((sum J iw + 256) >> 9) at window pixel `off` of a (win + 1)-wide tile
__device__ __forceinline__ int lk_sample(const uint8_t *tile, int off, int side, int w00, int w01, int w10, int w11)
{
    return (tile[off] * w00 + tile[off + 1] * w01 + tile[off + side] * w10 + tile[off + side + 1] * w11 + 256) >> 9;
}

// DistortVecPoints, src/utils.cpp:49-76, one point: the arithmetic of distort_point (pagk_device.h), f32, uncontracted
__device__ __forceinline__ void lk_distort_point(const LkFlowArgs &a, float ux, float uy, float &ox, float &oy)
{
    if (!a.distort_on) {
        ox = ux;
        oy = uy;
        return;
    }
    float x = (ux - a.cx) * a.fx_inv;
    float y = (uy - a.cy) * a.fy_inv;
    float r2 = x * x + y * y;
    float r4 = r2 * r2;
    float r6 = r4 * r2;
    float xd = x * (1 + a.k1 * r2 + a.k2 * r4 + a.k3 * r6) + 2 * a.p1 * x * y + a.p2 * (r2 + 2 * x * x);
    float yd = y * (1 + a.k1 * r2 + a.k2 * r4 + a.k3 * r6) + a.p1 * (r2 + 2 * y * y) + 2 * a.p2 * x * y;
    ox = a.fx * xd + a.cx;
    oy = a.fy * yd + a.cy;
}

template <int NPIX>
__global__ __launch_bounds__(256) void k_lk_track(LkTrackArgs a)
{
#define PAGK_LK_FLOW 0
#include "pagk_lk_body.h"
#undef PAGK_LK_FLOW
}

template <int NPIX>
__global__ __launch_bounds__(256) void k_lk_flow(LkFlowArgs f)
{
    const LkTrackArgs &a = f.t;
#define PAGK_LK_FLOW 1
#include "pagk_lk_body.h"
#undef PAGK_LK_FLOW
}

}  // namespace pagk
