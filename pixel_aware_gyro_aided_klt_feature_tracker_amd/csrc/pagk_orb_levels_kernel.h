// pagk_orb_levels_kernel.h -- ORB over a scale pyramid (include/pagk.h "ORB over a scale pyramid"): ORBextractor with
// nlevels up to 8 (reference src/ORBextractor.cc:434-470 the level table, :1207-1230 the pyramid, :789-875 the per-level
// detection, :1066-1146 operator(), :1148-1205 DetectFeatures).  tests/orb_levels_ref.c restates the definition in plain C.
//
// Shapes:
//   k_orb_resize          OpenCV 3.4's 8-bit INTER_LINEAR for an arbitrary ratio, as include/pagk.h writes it out: one lane
//                         produces four adjacent destination pixels and stores one dword (a level's pitch is a multiple of
//                         four; the bytes between the width and the pitch are written as 0).  Coordinates and Q11
//                         coefficients are computed in the kernel from the f64 scales.  No LDS; memory bound.
//   k_*_levels            the stages of the one-level detector and describer (pagk_fast_kernel.h, pagk_orb_kernel.h), their
//                         bodies unchanged, with the level as a grid dimension: a block's level index selects one of up to
//                         eight argument sets passed by value, and a block beyond that level's own grid leaves at once (the
//                         whole workgroup: no barrier is skipped by a part of one).  Eight single-workgroup trees then run
//                         side by side instead of one after the other.
//   k_orb_pack            one workgroup: levels in ascending order, the tree's list order kept inside a level, the mask test
//                         of DetectFeatures at the scaled coordinates (a compaction: an ordered scan), coordinates scaled,
//                         octave written, descriptors copied as 16-byte rows, the tail zeroed, the info words written.
// No launch is sized by a count: the grids come from the level table, the counts are read on the device.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pagk_fast_kernel.h"
#include "pagk_orb_kernel.h"

namespace pagk {

constexpr int kOrbMaxLevels = 8;          // PAGK_ORB_MAX_LEVELS
constexpr int kOrbLevelsInfoWords = 32;   // PAGK_ORB_LEVELS_INFO_WORDS

// ---- the resize -----------------------------------------------------------------------------------------------------
struct OrbResizeArgs {
    const uint8_t *src;   // sh rows of spitch bytes
    long long spitch;
    uint8_t *dst;         // dh rows of dpitch bytes, dpitch a multiple of 4 and >= dw
    int sw, sh, dw, dh, dpitch;
    double scale_x, scale_y;   // 1 / ((double)dw / sw), 1 / ((double)dh / sh)
};

__global__ __launch_bounds__(256) void k_orb_resize(OrbResizeArgs a)
{
    const int xg = blockIdx.x * 64 + (threadIdx.x & 63), dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (4 * xg >= a.dpitch || dy >= a.dh) return;
    float fy = (float)(((double)dy + 0.5) * a.scale_y - 0.5);
    const int sy = (int)floorf(fy);
    fy -= (float)sy;
    const int b0 = (int)rintf((1.0f - fy) * 2048.0f), b1 = (int)rintf(fy * 2048.0f);
    const int y0 = min(max(sy, 0), a.sh - 1), y1 = min(max(sy + 1, 0), a.sh - 1);   // both rows clipped into the image
    const uint8_t *r0 = a.src + (long long)y0 * a.spitch, *r1 = a.src + (long long)y1 * a.spitch;
    uint32_t word = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int dx = 4 * xg + k;
        if (dx >= a.dw) break;   // (padding bytes stay 0)
        float fx = (float)(((double)dx + 0.5) * a.scale_x - 0.5);
        int sx = (int)floorf(fx);
        fx -= (float)sx;
        bool single = false;
        if (sx < 0) fx = 0.0f, sx = 0;
        if (sx + 1 >= a.sw) {
            single = true;
            if (sx >= a.sw - 1) fx = 0.0f, sx = a.sw - 1;
        }
        const int a0 = (int)rintf((1.0f - fx) * 2048.0f), a1 = (int)rintf(fx * 2048.0f);
        int S0, S1;
        if (single) {
            S0 = r0[sx] * 2048, S1 = r1[sx] * 2048;
        } else {
            S0 = r0[sx] * a0 + r0[sx + 1] * a1, S1 = r1[sx] * a0 + r1[sx + 1] * a1;
        }
        const int v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
        word |= ((uint32_t)v & 255u) << (8 * k);
    }
    *reinterpret_cast<uint32_t *>(a.dst + (size_t)dy * a.dpitch + 4 * xg) = word;
}

// ---- the one-level stages with the level as a grid dimension ---------------------------------------------------------
struct FastCellLevels {
    FastCellArgs a[kOrbMaxLevels];
    int32_t n_cells[kOrbMaxLevels];
};
__global__ void __launch_bounds__(256) k_fast_cells_levels(FastCellLevels s)
{
    const int l = blockIdx.y;
    if ((int)blockIdx.x >= s.n_cells[l]) return;
    fast_cells_body(s.a[l]);
}

struct FastListArgs {   // what k_fast_offsets and k_fast_gather take as single arguments
    int32_t n_cells, seg;
    const int32_t *cell_cnt;
    int32_t *cell_off, *ctl;
    const uint32_t *seg_xy;
    const int32_t *seg_score;
    uint32_t *kxy;
    int32_t *kscore;
};
struct FastListLevels {
    FastListArgs a[kOrbMaxLevels];
};
__global__ void __launch_bounds__(1024) k_fast_offsets_levels(FastListLevels s)
{
    const FastListArgs &a = s.a[blockIdx.x];
    fast_offsets_body(a.n_cells, a.cell_cnt, a.cell_off, a.ctl, nullptr);
}
__global__ void __launch_bounds__(256) k_fast_gather_levels(FastListLevels s)
{
    const FastListArgs &a = s.a[blockIdx.y];
    if ((int)blockIdx.x >= a.n_cells) return;
    fast_gather_body(a.seg, a.cell_cnt, a.cell_off, a.seg_xy, a.seg_score, a.kxy, a.kscore, nullptr);
}

struct FastTreeLevels {
    FastTreeArgs a[kOrbMaxLevels];
};
__global__ void __launch_bounds__(1024) k_fast_tree_levels(FastTreeLevels s) { fast_tree_body(s.a[blockIdx.x]); }

struct OrbBlurLevels {
    OrbBlurArgs a[kOrbMaxLevels];
    int32_t nbx[kOrbMaxLevels], nby[kOrbMaxLevels];
};
__global__ __launch_bounds__(256) void k_orb_blur_levels(OrbBlurLevels s)
{
    const int l = blockIdx.z;
    if ((int)blockIdx.x >= s.nbx[l] || (int)blockIdx.y >= s.nby[l]) return;
    orb_blur_body(s.a[l], blockIdx.x, blockIdx.y);
}

struct OrbDescLevels {
    OrbDescArgs a[kOrbMaxLevels];
    int32_t n_blocks[kOrbMaxLevels];
};
__global__ __launch_bounds__(256) void k_orb_describe_levels(OrbDescLevels s)
{
    const int l = blockIdx.y;
    if ((int)blockIdx.x >= s.n_blocks[l]) return;
    orb_describe_body(s.a[l], blockIdx.x);
}

// ---- packing --------------------------------------------------------------------------------------------------------
struct OrbPackLevel {
    const float *kp;          // seg_cap x 2: the tree's output of the level, level coordinates
    const float *resp;        // seg_cap
    const float *angle;       // seg_cap, or nullptr (DetectFeatures)
    const uint8_t *desc;      // seg_cap x 32, 16-byte aligned, or nullptr
    const int32_t *fast_info; // kDetectInfoWords of the level: [0] keypoints, [1] raw keypoints
    const int32_t *orb_info;  // kOrbInfoWords of the level ([1] outside the border), or nullptr
    int32_t seg_cap, quota;
    float scale;              // sc[l]
};
struct OrbPackArgs {
    OrbPackLevel lv[kOrbMaxLevels];
    int32_t n_levels, cap, W, H;
    const uint8_t *mask;      // W x H of the ORIGINAL image, or nullptr
    float *kp;                // cap x 2
    int32_t *octave;          // cap
    float *resp, *angle;      // cap each
    uint8_t *desc;            // cap x 32, 16-byte aligned
    int32_t *info;            // kOrbLevelsInfoWords
};

__global__ void __launch_bounds__(1024) k_orb_pack(OrbPackArgs a)
{
    __shared__ int32_t s_wtot[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t base = 0, outside = 0;
    int32_t my_cnt = 0, my_raw = 0, my_quota = 0;   // lane l < 8 keeps the words of level l
    for (int l = 0; l < a.n_levels; l++) {
        const OrbPackLevel &v = a.lv[l];
        const int32_t n = min(max(v.fast_info[0], 0), v.seg_cap);   // (one address: the same in every lane)
        const int32_t first = base;
        for (int c0 = 0; c0 < n; c0 += 1024) {
            const int i = c0 + tid;
            bool ok = i < n;
            float x = 0.0f, y = 0.0f;
            if (ok) {
                x = v.kp[2 * i], y = v.kp[2 * i + 1];
                if (l != 0) x = x * v.scale, y = y * v.scale;   // :1132-1139
                if (a.mask) {   // :1199-1203; a scaled coordinate lies inside the image (include/pagk.h): the test only guards the read
                    const int ix = (int)x, iy = (int)y;
                    ok = ix >= 0 && ix < a.W && iy >= 0 && iy < a.H && a.mask[(int64_t)iy * a.W + ix] != 0;
                }
            }
            int32_t tot;
            const int32_t o = base + fast_scan1024(ok ? 1 : 0, s_wtot, lane, wave, tot);
            if (ok && o < a.cap) {
                a.kp[2 * o] = x, a.kp[2 * o + 1] = y;
                a.octave[o] = l;
                a.resp[o] = v.resp[i];
                if (a.angle) a.angle[o] = v.angle ? v.angle[i] : 0.0f;
                if (a.desc) {
                    uint4 *d = reinterpret_cast<uint4 *>(a.desc) + 2 * (size_t)o;
                    if (v.desc) {
                        const uint4 *s = reinterpret_cast<const uint4 *>(v.desc) + 2 * (size_t)i;
                        d[0] = s[0], d[1] = s[1];
                    } else {
                        d[0] = d[1] = make_uint4(0u, 0u, 0u, 0u);
                    }
                }
            }
            base += tot;
        }
        if (v.orb_info) outside += v.orb_info[1];
        if (tid == l) my_cnt = base - first, my_raw = v.fast_info[1], my_quota = v.quota;
    }
    const int32_t nout = min(base, a.cap);
    for (int i = nout + tid; i < a.cap; i += 1024) {
        a.kp[2 * i] = a.kp[2 * i + 1] = 0.0f;
        a.octave[i] = 0;
        a.resp[i] = 0.0f;
        if (a.angle) a.angle[i] = 0.0f;
        if (a.desc) {
            uint4 *d = reinterpret_cast<uint4 *>(a.desc) + 2 * (size_t)i;
            d[0] = d[1] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
    if (tid < kOrbLevelsInfoWords) {
        int32_t w = 0;
        if (tid == 0) w = nout;
        if (tid == 1) w = outside;
        if (tid == 2) w = a.n_levels;
        a.info[tid] = w;
    }
    __syncthreads();
    if (tid < a.n_levels) a.info[8 + tid] = my_cnt, a.info[16 + tid] = my_raw, a.info[24 + tid] = my_quota;
}

}  // namespace pagk
