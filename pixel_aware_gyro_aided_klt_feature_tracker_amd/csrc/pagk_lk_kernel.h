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

__global__ __launch_bounds__(256) void k_lk_pyrdown(LkPyrArgs a)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.dw || y >= a.dh) return;
    int cx[5];
#pragma unroll
    for (int i = 0; i < 5; i++) cx[i] = lk_reflect(2 * x + i - 2, a.sw);
    int s = 128;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const uint8_t *row = a.src + (long long)lk_reflect(2 * y + j - 2, a.sh) * a.spitch;
        const int r = row[cx[0]] + row[cx[4]] + 4 * (row[cx[1]] + row[cx[3]]) + 6 * row[cx[2]];
        s += (j == 0 || j == 4 ? 1 : (j == 2 ? 6 : 4)) * r;
    }
    a.dst[(size_t)y * a.dw + x] = (uint8_t)(s >> 8);
}

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

template <int NPIX>
__global__ __launch_bounds__(256) void k_lk_track(LkTrackArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t tiles[4 * lk_tile_bytes(NPIX)];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = blockIdx.x * 4 + wave;   // the wave's feature
    if (k >= a.cap) return;
    const int n = a.n ? min(max(*a.n, 0), a.cap) : a.cap;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.info[0] = n, a.info[3] = a.top;
    if (k >= n) {   // rows at or beyond the count are zeroed
        if (lane == 0) {
            a.pt_out[2 * k] = 0.f, a.pt_out[2 * k + 1] = 0.f, a.status[k] = 0, a.err[k] = 0.f;
            if (a.status_raw) a.status_raw[k] = 0;
            if (a.flow) a.flow[2 * k] = 0.f, a.flow[2 * k + 1] = 0.f;
        }
        return;
    }
    uint8_t *tile = tiles + wave * lk_tile_bytes(NPIX);
    const int win = a.win, npx = win * win, side_i = win + 3, side_j = win + 1;
    const unsigned magic_win = lk_magic(win);
    const float half = (float)(win - 1) * 0.5f;
    const float rx = a.pt_ref[2 * k], ry = a.pt_ref[2 * k + 1];
    int st = 1, lost_eig = 0, lost_range = 0;
    float e = 0.f, nx = 0.f, ny = 0.f;
    int tI[NPIX], tG[NPIX];   // Ival; ix in the low, iy in the high half

    for (int l = a.top; l >= 0; l--) {
        const LkLevel &L = a.lv[l];
        const float sc = __int_as_float((127 - l) << 23);   // 2^-l
        const float px = rx * sc - half, py = ry * sc - half;
        if (l == a.top)
            nx = rx * sc, ny = ry * sc;
        else
            nx = 2.f * nx, ny = 2.f * ny;
        const float fx = floorf(px), fy = floorf(py);
        if (lk_out_of_range(fx, fy, win, L.w, L.h)) {
            if (l == 0) st = 0, e = 0.f, lost_range = 1;
            continue;
        }
        const int ipx = (int)fx, ipy = (int)fy;
        int w00, w01, w10, w11;
        lk_weights(px - fx, py - fy, w00, w01, w10, w11);
        // the template: gray tile from (ipx - 1, ipy - 1), derivatives formed from it
        lk_tile_handover();   // (the reads of the level above are done)
        lk_stage(tile, L.I, L.pitch_i, L.w, L.h, ipx - 1, ipy - 1, side_i, lane);
        lk_tile_handover();
        int s11 = 0, s12 = 0, s22 = 0;
#pragma unroll
        for (int c = 0; c < NPIX; c++) {
            const int p = lane + 64 * c;
            tI[c] = 0, tG[c] = 0;
            if (p < npx) {
                const int y = (int)(((unsigned)p * magic_win) >> 16), x = p - y * win;
                int g[4][4];
#pragma unroll
                for (int r = 0; r < 4; r++)
#pragma unroll
                    for (int q = 0; q < 4; q++) g[r][q] = tile[(y + r) * side_i + x + q];
                int dxs = 8192, dys = 8192;
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const int r = 1 + (t >> 1), q = 1 + (t & 1);   // the tap's centre in g
                    const int gx = ipx + x + (t & 1), gy = ipy + y + (t >> 1);
                    const int wt = t == 0 ? w00 : (t == 1 ? w01 : (t == 2 ? w10 : w11));
                    int dx = 3 * (g[r - 1][q + 1] + g[r + 1][q + 1]) + 10 * g[r][q + 1] -
                             (3 * (g[r - 1][q - 1] + g[r + 1][q - 1]) + 10 * g[r][q - 1]);
                    int dy = 3 * ((g[r + 1][q - 1] - g[r - 1][q - 1]) + (g[r + 1][q + 1] - g[r - 1][q + 1])) +
                             10 * (g[r + 1][q] - g[r - 1][q]);
                    if (gx < 0 || gx >= L.w || gy < 0 || gy >= L.h) dx = 0, dy = 0;   // the constant border of the derivatives
                    dxs += dx * wt, dys += dy * wt;
                }
                const int ix = dxs >> 14, iy = dys >> 14;
                tI[c] = (g[1][1] * w00 + g[1][2] * w01 + g[2][1] * w10 + g[2][2] * w11 + 256) >> 9;
                tG[c] = (int)((unsigned)(ix & 0xffff) | ((unsigned)iy << 16));
                s11 += ix * ix, s12 += ix * iy, s22 += iy * iy;
            }
        }
        const long long S11 = lk_wave_sum(s11), S12 = lk_wave_sum(s12), S22 = lk_wave_sum(s22);
        const float A11 = (float)S11 * 0x1p-20f, A12 = (float)S12 * 0x1p-20f, A22 = (float)S22 * 0x1p-20f;
        float D = A11 * A22 - A12 * A12;
        const float min_eig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (float)(2 * win * win);
        if ((double)min_eig < a.min_eig || D < 0x1p-23f) {   // FLT_EPSILON
            if (l == 0) st = 0, lost_eig = 1;
            continue;
        }
        D = 1.f / D;
        float qx = nx - half, qy = ny - half, pdx = 0.f, pdy = 0.f;
        for (int j = 0; j < a.max_count; j++) {
            const float gx = floorf(qx), gy = floorf(qy);
            if (lk_out_of_range(gx, gy, win, L.w, L.h)) {
                if (l == 0) st = 0, lost_range = 1;
                break;
            }
            lk_weights(qx - gx, qy - gy, w00, w01, w10, w11);
            lk_tile_handover();   // (the reads of the tile before this one are done)
            lk_stage(tile, L.J, L.pitch_j, L.w, L.h, (int)gx, (int)gy, side_j, lane);
            lk_tile_handover();
            int b1 = 0, b2 = 0;
#pragma unroll
            for (int c = 0; c < NPIX; c++) {
                const int p = lane + 64 * c;
                if (p < npx) {
                    const int y = (int)(((unsigned)p * magic_win) >> 16), x = p - y * win;
                    const int diff = lk_sample(tile, y * side_j + x, side_j, w00, w01, w10, w11) - tI[c];
                    b1 += diff * (int)(short)(tG[c] & 0xffff), b2 += diff * (tG[c] >> 16);
                }
            }
            const long long B1 = lk_wave_sum(b1), B2 = lk_wave_sum(b2);
            const float fb1 = (float)B1 * 0x1p-20f, fb2 = (float)B2 * 0x1p-20f;
            const float ddx = (A12 * fb2 - A22 * fb1) * D, ddy = (A12 * fb1 - A11 * fb2) * D;
            qx += ddx, qy += ddy;
            nx = qx + half, ny = qy + half;
            if ((double)ddx * (double)ddx + (double)ddy * (double)ddy <= a.eps2) break;
            if (j > 0 && (double)fabsf(ddx + pdx) < 0.01 && (double)fabsf(ddy + pdy) < 0.01) {
                nx -= ddx * 0.5f, ny -= ddy * 0.5f;
                break;
            }
            pdx = ddx, pdy = ddy;
        }
        if (l == 0 && st) {   // step 7
            const float ex = nx - half, ey = ny - half, gx = floorf(ex), gy = floorf(ey);
            if (lk_out_of_range(gx, gy, win, L.w, L.h)) {
                st = 0, lost_range = 1;
            } else {
                lk_weights(ex - gx, ey - gy, w00, w01, w10, w11);
                lk_tile_handover();
                lk_stage(tile, L.J, L.pitch_j, L.w, L.h, (int)gx, (int)gy, side_j, lane);
                lk_tile_handover();
                int es = 0;
#pragma unroll
                for (int c = 0; c < NPIX; c++) {
                    const int p = lane + 64 * c;
                    if (p < npx) {
                        const int y = (int)(((unsigned)p * magic_win) >> 16), x = p - y * win;
                        es += abs(lk_sample(tile, y * side_j + x, side_j, w00, w01, w10, w11) - tI[c]);
                    }
                }
                const long long E = lk_wave_sum(es);
                e = (float)E / (float)(32 * win * win);
            }
        }
    }
    if (lane == 0) {
        const int kept = st && !(e >= a.err_threshold);
        a.pt_out[2 * k] = nx, a.pt_out[2 * k + 1] = ny;
        a.err[k] = e;
        a.status[k] = (uint8_t)kept;
        if (a.status_raw) a.status_raw[k] = (uint8_t)st;
        if (a.flow) a.flow[2 * k] = nx - rx, a.flow[2 * k + 1] = ny - ry;
        if (st) atomicAdd(a.info + 1, 1);
        if (kept) atomicAdd(a.info + 2, 1);
        if (lost_eig) atomicAdd(a.info + 4, 1);
        if (lost_range) atomicAdd(a.info + 5, 1);
    }
}

}  // namespace pagk
