// pagk_detect_kernel.h -- the reference's corner detector on the device (include/pagk.h: pagk_detect_corners_device,
// pagk_frame_handover_detect_device).  Frame::DetectKeyPoints (reference src/frame.cpp:156-218) ends in
//     cv::goodFeaturesToTrack(mGray, corners_un, n_new, 0.005, 20, mMask, 3, true, 0.04)           (:181-184)
// which is a Harris response on a 3 x 3 block, a threshold against the strongest unmasked response, a 3 x 3 non-maximum
// test, strongest first, a greedy minimum distance.  The definition the kernels implement is the one written down in
// include/pagk.h and restated in plain C in tests/corner_detect_ref.c; no parity with OpenCV's own arithmetic is claimed.
//   k_handover_plan      (fused call only) survivors, the top-up rule and n_new, so that the detector knows its limit
//   k_detect_response    Sobel, block sums, response R (f32) and Rmax over the unmasked pixels, one pass from LDS tiles
//   k_detect_nms         threshold, mask, the tie rule; raw candidates appended as 64-bit keys, one atomic per wave
//   k_detect_sort_local  bitonic sort, descending: the stages that stay inside a block of 16384 keys, in LDS
//   k_detect_sort_step   ... one compare-exchange step across blocks, in global memory
//   k_detect_walk        the greedy minimum distance over the sorted keys, one wave, accepted corners in a grid of cells
// Every count stays on the device: launches are sized by W, H, raw_cap and cap, and a kernel whose share of the padding
// holds nothing returns at once.  Plain HIP C++, vector stores and C++ atomics only.  No kernel waits for another wave.
// Barriers sit in loops bounded by kernel arguments or by values every lane of the workgroup reads from one address.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pagk {

constexpr int kDetectInfoWords = 8;      // PAGK_DETECT_INFO_WORDS
constexpr int kDetTileW = 64;            // k_detect_response: pixels of a tile (256 threads, four rows each)
constexpr int kDetTileH = 16;
constexpr int kDetSortBlock = 16384;     // keys a workgroup sorts in LDS (128 KiB of the CU's 160, dynamic: the host sets the attribute)
constexpr int kDetGridLds = 12288;       // cells of the distance grid that fit the walk's LDS (48 KiB)

// control words in the context's workspace: [0] bits of Rmax (0: none, or Rmax <= 0), [1] raw candidates found,
// [2] (fused call) the detector's limit = n_new or 0, [3] (fused call) 1 = the top-up does not run: every kernel returns
enum { kDetCtlRmax = 0, kDetCtlCount = 1, kDetCtlLimit = 2, kDetCtlSkip = 3 };

// index -1 is 1, index n is n - 2 (no repeated edge); one reflection serves -2 .. n + 1 for n >= 4
__device__ __forceinline__ int det_reflect(int i, int n)
{
    i = i < 0 ? -i : i;
    return i >= n ? 2 * n - 2 - i : i;
}

// The hand-over's decision in front of the detector: num_predicted, the top-up rule (src/frame.cpp:164-169), n_new (:168).
// (the body is a function of its own so that pagk_group_sensor_kernel.h can run it for one of several cameras per launch)
__device__ __forceinline__ void handover_plan_body(int32_t cap, int32_t target_n, double new_point_threshold,
                                                   const uint8_t *status, const int32_t *state, int32_t *ctl)
{
    __shared__ int32_t s_cnt[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t cnt = 0;
    for (int i = tid; i < cap; i += 1024) cnt += status[i] != 0 ? 1 : 0;
    for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_down(cnt, off, 64);
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    if (tid == 0) {
        int32_t m = 0;
        for (int w = 0; w < 16; w++) m += s_cnt[w];
        const int32_t n_new = target_n - m;
        const bool topup = ((double)m < new_point_threshold || !state[1]) && n_new > 0;
        ctl[kDetCtlLimit] = topup ? n_new : 0;
        ctl[kDetCtlSkip] = topup ? 0 : 1;
    }
}

__global__ void __launch_bounds__(1024) k_handover_plan(int32_t cap, int32_t target_n, double new_point_threshold,
                                                        const uint8_t *status, const int32_t *state, int32_t *ctl)
{
    handover_plan_body(cap, target_n, new_point_threshold, status, state, ctl);
}

// One tile of 64 x 16 pixels per workgroup.  The u8 tile is staged with a halo of 2, the reflection taken there; the
// gradients are computed once per position of tile + 1.  A position outside the image takes the gradient OF ITS REFLECTED
// PIXEL (the product maps are what is reflected: a Sobel over the reflected image would flip the sign of dx * dy there).
// A thread owns four vertically adjacent pixels of one column: six row sums of three products each, shared by its pixels.
__global__ void __launch_bounds__(256) k_detect_response(const uint8_t *__restrict__ img, int64_t pitch, int32_t W, int32_t H,
                                                         const uint8_t *__restrict__ mask, double harris_k,
                                                         float *__restrict__ R, int32_t *ctl, const int32_t *skip)
{
    __shared__ uint8_t s_img[kDetTileH + 4][kDetTileW + 4];
    __shared__ int16_t s_dx[kDetTileH + 2][kDetTileW + 2], s_dy[kDetTileH + 2][kDetTileW + 2];
    __shared__ uint32_t s_max[4];
    if (skip && *skip) return;   // (one address: the whole workgroup takes the same way)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * kDetTileW, y0 = blockIdx.y * kDetTileH;
    for (int t = tid; t < (kDetTileH + 4) * (kDetTileW + 4); t += 256) {
        const int ly = t / (kDetTileW + 4), lx = t - ly * (kDetTileW + 4);
        // (positions beyond W + 1 / H + 1 belong to no pixel of the image: clamped so that the reflection stays inside)
        const int gx = x0 - 2 + lx < W + 1 ? x0 - 2 + lx : W + 1, gy = y0 - 2 + ly < H + 1 ? y0 - 2 + ly : H + 1;
        s_img[ly][lx] = img[(int64_t)det_reflect(gy, H) * pitch + det_reflect(gx, W)];
    }
    __syncthreads();
    for (int t = tid; t < (kDetTileH + 2) * (kDetTileW + 2); t += 256) {
        const int ly = t / (kDetTileW + 2), lx = t - ly * (kDetTileW + 2);
        const int gx = x0 - 1 + lx < W ? x0 - 1 + lx : W, gy = y0 - 1 + ly < H ? y0 - 1 + ly : H;
        const int cx = det_reflect(gx, W) - (x0 - 2), cy = det_reflect(gy, H) - (y0 - 2);   // 1 .. tile + 2, in s_img
        const int p00 = s_img[cy - 1][cx - 1], p01 = s_img[cy - 1][cx], p02 = s_img[cy - 1][cx + 1];
        const int p10 = s_img[cy][cx - 1], p12 = s_img[cy][cx + 1];
        const int p20 = s_img[cy + 1][cx - 1], p21 = s_img[cy + 1][cx], p22 = s_img[cy + 1][cx + 1];
        s_dx[ly][lx] = (int16_t)((p02 + 2 * p12 + p22) - (p00 + 2 * p10 + p20));
        s_dy[ly][lx] = (int16_t)((p20 + 2 * p21 + p22) - (p00 + 2 * p01 + p02));
    }
    __syncthreads();
    const int tx = tid & 63, r0 = (tid >> 6) * 4;
    int32_t hxx[6], hxy[6], hyy[6];
#pragma unroll
    for (int r = 0; r < 6; r++) {
        int32_t sxx = 0, sxy = 0, syy = 0;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int32_t gx = s_dx[r0 + r][tx + c], gy = s_dy[r0 + r][tx + c];
            sxx += gx * gx, sxy += gx * gy, syy += gy * gy;
        }
        hxx[r] = sxx, hxy[r] = sxy, hyy[r] = syy;
    }
    uint32_t best = 0;   // bits of the largest positive unmasked response of this thread
    const int x = x0 + tx;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int y = y0 + r0 + j;
        if (x < W && y < H) {
            const double a = (double)(hxx[j] + hxx[j + 1] + hxx[j + 2]);
            const double b = (double)(hxy[j] + hxy[j + 1] + hxy[j + 2]);
            const double c = (double)(hyy[j] + hyy[j + 1] + hyy[j + 2]);
            // a * c, b * b, their difference and (a + c)^2 are exact (integers below 2^53): two roundings, never an FMA
            const double det = __dsub_rn(__dmul_rn(a, c), __dmul_rn(b, b));
            const double tr = a + c;
            const float r = (float)__dsub_rn(det, __dmul_rn(harris_k, __dmul_rn(tr, tr)));
            const int64_t p = (int64_t)y * W + x;
            R[p] = r;
            if (r > 0.0f && (!mask || mask[p] != 0)) {
                const uint32_t bits = __float_as_uint(r);   // (positive floats order like their bits)
                best = bits > best ? bits : best;
            }
        }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)best, off, 64);
        best = o > best ? o : best;
    }
    if (lane == 0) s_max[wave] = best;
    __syncthreads();
    if (tid == 0) {
        uint32_t m = s_max[0];
        for (int w = 1; w < 4; w++) m = s_max[w] > m ? s_max[w] : m;
        if (m) atomicMax(reinterpret_cast<uint32_t *>(ctl) + kDetCtlRmax, m);
    }
}

// One thread per pixel (64 x 4 per workgroup).  A pixel reads its neighbours only once it has passed the threshold and
// the mask.  Candidates of a wave are appended with one atomic; all are counted, the ones beyond raw_cap are not stored.
__global__ void __launch_bounds__(256) k_detect_nms(const float *__restrict__ R, int32_t W, int32_t H,
                                                    const uint8_t *__restrict__ mask, double quality_level, int32_t *ctl,
                                                    uint64_t *__restrict__ keys, int32_t raw_cap, const int32_t *skip)
{
    if (skip && *skip) return;
    const uint32_t rmax_bits = (uint32_t)ctl[kDetCtlRmax];
    if (rmax_bits == 0) return;   // no unmasked pixel, or Rmax <= 0: no corners
    const double thr = quality_level * (double)__uint_as_float(rmax_bits);
    const int lane = threadIdx.x & 63;
    const int x = blockIdx.x * 64 + lane, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    bool cand = false;
    uint64_t key = 0;
    if (x >= 1 && x <= W - 2 && y >= 1 && y <= H - 2) {
        const int64_t p = (int64_t)y * W + x;
        const float r = R[p];
        if ((double)r > thr && (!mask || mask[p] != 0)) {
            const float *u = R + p - W, *d = R + p + W;
            // >= the four neighbours in front in raster order, > the four behind: of an exact tie the later pixel stays
            cand = r >= u[-1] && r >= u[0] && r >= u[1] && r >= R[p - 1] && r > R[p + 1] && r > d[-1] && r > d[0] && r > d[1];
            key = ((uint64_t)__float_as_uint(r) << 32) | (uint64_t)(uint32_t)p;
        }
    }
    const unsigned long long bal = __ballot(cand);
    if (bal == 0) return;   // (wave-uniform)
    int32_t base = 0;
    if (lane == 0) base = atomicAdd(&ctl[kDetCtlCount], (int32_t)__popcll(bal));
    base = __shfl(base, 0, 64);
    const int32_t pos = base + (int32_t)__popcll(bal & ((1ull << lane) - 1ull));
    if (cand && pos < raw_cap) keys[pos] = key;
}

// keys to sort: none when more candidates were found than fit (the call then returns no corners)
__device__ __forceinline__ uint32_t det_sort_count(const int32_t *ctl, int32_t raw_cap)
{
    const int32_t c = ctl[kDetCtlCount];
    return c > raw_cap || c < 0 ? 0u : (uint32_t)c;
}
// the power of two the bitonic network runs on: at least one block
__device__ __forceinline__ uint32_t det_sort_extent(uint32_t n)
{
    uint32_t e = kDetSortBlock;
    while (e < n) e <<= 1;
    return e;
}
// compare-exchange (i, i | j) of merge size k, descending overall
__device__ __forceinline__ bool det_sort_swap(uint64_t a, uint64_t b, uint32_t gi, uint32_t k)
{
    return (gi & k) == 0 ? a < b : a > b;
}

// merge == 0: sorts every block of 16384 keys (entries behind the count enter as 0, the smallest key: R > 0 in every real
// one).  merge > 16384: the steps j = 8192 .. 1 of that merge.  Blocks behind the extent, and merges beyond it, return.
__global__ void __launch_bounds__(1024) k_detect_sort_local(uint64_t *keys, const int32_t *ctl, int32_t raw_cap,
                                                            uint32_t merge, const int32_t *skip)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char det_sort_lds[];
    uint64_t *s = reinterpret_cast<uint64_t *>(det_sort_lds);
    if (skip && *skip) return;
    const uint32_t n = det_sort_count(ctl, raw_cap);
    if (n == 0) return;
    const uint32_t extent = det_sort_extent(n), base = blockIdx.x * kDetSortBlock;
    if (base >= extent || merge > extent) return;
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < kDetSortBlock; i += 1024) s[i] = (merge == 0 && base + i >= n) ? 0ull : keys[base + i];
    __syncthreads();
    for (uint32_t k = merge ? merge : 2; k <= (merge ? merge : (uint32_t)kDetSortBlock); k <<= 1) {
        for (uint32_t j = (merge ? kDetSortBlock : k) >> 1; j > 0; j >>= 1) {
            for (uint32_t t = tid; t < kDetSortBlock / 2; t += 1024) {
                const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const uint64_t a = s[i], b = s[l];
                if (det_sort_swap(a, b, base + i, k)) s[i] = b, s[l] = a;
            }
            __syncthreads();
        }
        if (merge) break;
    }
    for (uint32_t i = tid; i < kDetSortBlock; i += 1024) keys[base + i] = s[i];
}

// one step (k, j) with j >= 16384: a thread per pair
__global__ void __launch_bounds__(256) k_detect_sort_step(uint64_t *keys, const int32_t *ctl, int32_t raw_cap, uint32_t k,
                                                          uint32_t j, const int32_t *skip)
{
    if (skip && *skip) return;
    const uint32_t n = det_sort_count(ctl, raw_cap);
    if (n == 0) return;
    const uint32_t extent = det_sort_extent(n);
    if (k > extent) return;
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
    if (l >= extent) return;
    const uint64_t a = keys[i], b = keys[l];
    if (det_sort_swap(a, b, i, k)) keys[i] = b, keys[l] = a;
}

struct DetectWalkArgs {
    const uint64_t *keys;
    const int32_t *ctl;
    const int32_t *max_corners;   // device word, or NULL: cap
    const int32_t *skip;          // device word, or NULL
    int32_t raw_cap, cap, width, height;
    double min_distance;
    int32_t cell, grid_w, grid_h, reach;   // the grid: cells of `cell` pixels, at most one corner each; cells to look around
    int32_t *grid;                // in global memory when it does not fit the LDS, else NULL
    float *corners;
    int32_t *info;
};

// is an accepted corner closer than min_distance to (x, y)?  A cell holds pixel index + 1, or 0.
__device__ __forceinline__ bool det_near(const volatile int32_t *grid, const DetectWalkArgs &a, int x, int y, double d2)
{
    const int cx = x / a.cell, cy = y / a.cell;
    const int gx0 = cx - a.reach > 0 ? cx - a.reach : 0, gx1 = cx + a.reach < a.grid_w - 1 ? cx + a.reach : a.grid_w - 1;
    const int gy0 = cy - a.reach > 0 ? cy - a.reach : 0, gy1 = cy + a.reach < a.grid_h - 1 ? cy + a.reach : a.grid_h - 1;
    for (int gy = gy0; gy <= gy1; gy++)
        for (int gx = gx0; gx <= gx1; gx++) {
            const int32_t v = grid[gy * a.grid_w + gx];
            if (v) {
                const int py = (v - 1) / a.width, px = (v - 1) - py * a.width;
                const int64_t ddx = x - px, ddy = y - py;
                if ((double)(ddx * ddx + ddy * ddy) < d2) return true;
            }
        }
    return false;
}

// One workgroup: all threads clear the grid and, at the end, the tail of the output; wave 0 walks.  It takes 64
// candidates in order, every lane tests its own against the grid, then the batch is resolved in order: the lowest lane
// still standing is accepted (nothing accepted earlier is near it) and knocks out the later lanes within the distance.
// That is the sequential walk.  The cell size is at most min_distance / sqrt(2), so two pixels of one cell are always
// too close and a cell never holds two corners.
__global__ void __launch_bounds__(1024) k_detect_walk(DetectWalkArgs a)
{
    __shared__ int32_t s_grid[kDetGridLds];
    __shared__ int32_t s_acc, s_visited;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool skip = a.skip && *a.skip;
    const int32_t count = skip ? 0 : a.ctl[kDetCtlCount];
    const bool overflow = count > a.raw_cap;
    const int32_t n = overflow ? 0 : count;
    int32_t limit = a.max_corners ? *a.max_corners : a.cap;
    limit = limit < 0 ? 0 : (limit > a.cap ? a.cap : limit);
    if (skip) limit = 0;
    const bool dist_on = a.min_distance >= 1.0;
    volatile int32_t *grid = a.grid ? a.grid : s_grid;
    if (dist_on && n > 0 && limit > 0)
        for (int i = tid; i < a.grid_w * a.grid_h; i += 1024) grid[i] = 0;
    if (tid == 0) s_acc = 0, s_visited = 0;
    __syncthreads();
    if (wave == 0) {
        const double d2 = a.min_distance * a.min_distance;
        int32_t acc = 0, visited = 0;
        for (int32_t base = 0; base < n && acc < limit; base += 64) {   // (n, acc, limit: the same in every lane)
            const int32_t i = base + lane;
            bool alive = i < n;
            int x = 0, y = 0;
            int32_t idx = 0;
            if (alive) {
                idx = (int32_t)(uint32_t)a.keys[i];
                y = idx / a.width, x = idx - y * a.width;
                if (dist_on) alive = !det_near(grid, a, x, y, d2);
            }
            int last = -1;   // the lane at which the limit was reached
            unsigned long long m = __ballot(alive);
            while (m) {
                const int L = __ffsll((long long)m) - 1;
                const int lx = __shfl(x, L, 64), ly = __shfl(y, L, 64);
                if (lane == L) {
                    a.corners[2 * acc] = (float)x, a.corners[2 * acc + 1] = (float)y;
                    if (dist_on) grid[(y / a.cell) * a.grid_w + x / a.cell] = idx + 1;
                    alive = false;
                }
                acc++;
                if (acc >= limit) {
                    last = L;
                    break;
                }
                if (dist_on && alive) {
                    const int64_t ddx = x - lx, ddy = y - ly;
                    if ((double)(ddx * ddx + ddy * ddy) < d2) alive = false;
                }
                m = __ballot(alive);
            }
            __threadfence_block();   // the grid entries of this batch, in front of the next batch's look-ups
            visited = last >= 0 ? base + last + 1 : (n - base < 64 ? n : base + 64);
        }
        if (lane == 0) s_acc = acc, s_visited = visited;
    }
    __syncthreads();
    const int32_t acc = s_acc;
    for (int i = tid; i < a.cap; i += 1024)
        if (i >= acc) a.corners[2 * i] = a.corners[2 * i + 1] = 0.0f;
    if (tid == 0) {
        a.info[0] = acc;
        a.info[1] = count;
        a.info[2] = overflow ? 1 : 0;
        a.info[3] = skip ? 0 : a.ctl[kDetCtlRmax];
        a.info[4] = s_visited;
        a.info[5] = a.info[6] = a.info[7] = 0;
    }
}

}  // namespace pagk
