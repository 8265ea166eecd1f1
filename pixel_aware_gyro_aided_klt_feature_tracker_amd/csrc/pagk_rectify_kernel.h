// pagk_rectify_kernel.h -- cv::remap(INTER_LINEAR, BORDER_CONSTANT 0) of a raw camera frame through a fixed map pair, and
// the 8-bit RGB-to-gray step of Frame::Frame behind it, as ONE pass (reference Examples/Demo/RealSenseD435i.cpp:202,
// src/frame.cpp:81-87).  The definition is in include/pagk.h ("rectification"); tests/rectify_ref.c restates it.
//
// The maps never change between two pagk_rectify_set_maps calls, so the float step of the definition (rne(map * 32), the
// split into integer tap and 5-bit fraction, the saturation, the "no pixel" rule) is done once on the host: the kernel
// reads one packed 8-byte RectEntry per destination pixel and is integer arithmetic from there.
//
// Shape: memory bound.  A thread produces four consecutive destination pixels of one row: its four entries are two
// 16-byte loads (the entry rows are padded to a multiple of four entries, so they are always aligned and never guarded),
// the taps are gathered two at a time (the horizontal neighbours of a source row are one 2- to 8-byte load; a lens map is
// close to the identity: neighbouring lanes read neighbouring source bytes, the lines stay in L1 / L2), the four results
// leave as one dword when the destination width is a multiple of four and as guarded bytes otherwise.  Out-of-source taps are handled without a branch: the address is clamped into the source and
// the tap's weight is zeroed, so no lane ever forms an address outside the source image.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pagk {

// lo = (ix & 0xffff) | (iy << 16)   (int16 each)      hi = fx | (fy << 8)   (0 .. 31 each)
// "no pixel" (non-finite map value, |map * 32| >= 2^31) and the padding of a row: ix = iy = -32768, fx = fy = 0 -- every
// tap of such an entry lies left of / above the source, so the pixel is 0 by the border rule itself.
struct RectEntry {
    uint32_t lo, hi;
};
static_assert(sizeof(RectEntry) == 8, "one 8-byte entry per destination pixel");
constexpr uint32_t kRectNoPixelLo = 0x80008000u;

struct RectArgs {
    const RectEntry *entries;   // H rows of wp entries, wp = W rounded up to a multiple of 4
    const uint8_t *src;         // Hs rows of src_step bytes, Ws pixels of CN interleaved bytes
    uint8_t *dst;               // H rows of W bytes
    long long src_step;
    int W, H, wp, Ws, Hs;
    int gw0, gw1, gw2, gshift;  // CN = 3 / 4: gray = (v0 gw0 + v1 gw1 + v2 gw2 + (1 << (gshift - 1))) >> gshift
};

// The two horizontally adjacent taps of one source row, CN channels each, as ONE or TWO wide loads instead of 2 * NV byte
// loads: p points at pixel xb of the row, xb + 1 is inside the row too.  Global loads need no alignment on gfx950.
template <int CN, int NV>
__device__ __forceinline__ void rect_load_pair(const uint8_t *p, int (&lo)[NV], int (&hi)[NV])
{
    if constexpr (CN == 1) {
        uint16_t t;
        __builtin_memcpy(&t, p, 2);
        lo[0] = t & 255, hi[0] = t >> 8;
    } else if constexpr (CN == 3) {
        uint32_t t;
        uint16_t u;
        __builtin_memcpy(&t, p, 4);
        __builtin_memcpy(&u, p + 4, 2);
        lo[0] = t & 255, lo[1] = (t >> 8) & 255, lo[2] = (t >> 16) & 255;
        hi[0] = t >> 24, hi[1] = u & 255, hi[2] = u >> 8;
    } else {
        uint32_t t[2];
        __builtin_memcpy(t, p, 8);
        lo[0] = t[0] & 255, lo[1] = (t[0] >> 8) & 255, lo[2] = (t[0] >> 16) & 255;
        hi[0] = t[1] & 255, hi[1] = (t[1] >> 8) & 255, hi[2] = (t[1] >> 16) & 255;
    }
}

// One destination pixel: the four taps of its entry, CN channels together, then the gray step.
// PAIR (sources at least two pixels wide): the taps (ix, y) and (ix + 1, y) are neighbours in memory, so each row is read
// as one pair starting at xb = clamp(ix, 0, Ws - 2); a tap clamped onto the other pixel of the pair (or a tap outside the
// source, whose weight is 0) selects that pixel's bytes.
template <int CN, bool PAIR>
__device__ __forceinline__ uint32_t rectify_pixel(const RectArgs &a, uint32_t lo, uint32_t hi)
{
    const int ix = (int)(short)(lo & 0xffffu), iy = (int)(short)(lo >> 16);
    const int fx = (int)(hi & 31u), fy = (int)((hi >> 8) & 31u);
    // a tap outside [0, Ws) x [0, Hs) is 0: weight 0 on a clamped (always valid) address
    const int in_x0 = (unsigned)ix < (unsigned)a.Ws, in_x1 = (unsigned)(ix + 1) < (unsigned)a.Ws;
    const int in_y0 = (unsigned)iy < (unsigned)a.Hs, in_y1 = (unsigned)(iy + 1) < (unsigned)a.Hs;
    const int x0 = min(max(ix, 0), a.Ws - 1), x1 = min(max(ix + 1, 0), a.Ws - 1);
    const int y0 = min(max(iy, 0), a.Hs - 1), y1 = min(max(iy + 1, 0), a.Hs - 1);
    const int w00 = (32 - fx) * (32 - fy) * (in_x0 & in_y0), w01 = fx * (32 - fy) * (in_x1 & in_y0);
    const int w10 = (32 - fx) * fy * (in_x0 & in_y1), w11 = fx * fy * (in_x1 & in_y1);
    const uint8_t *r0 = a.src + (long long)y0 * a.src_step, *r1 = a.src + (long long)y1 * a.src_step;
    constexpr int NV = CN == 1 ? 1 : 3;   // (channel 3 of a 4-channel frame is never read)
    int v[NV];
    if constexpr (PAIR) {
        const int xb = min(x0, a.Ws - 2);          // x0, x1 are both xb or xb + 1
        const bool s0 = x0 != xb, s1 = x1 != xb;
        int t0[NV], t1[NV], b0[NV], b1[NV];
        rect_load_pair<CN, NV>(r0 + xb * CN, t0, t1);
        rect_load_pair<CN, NV>(r1 + xb * CN, b0, b1);
#pragma unroll
        for (int c = 0; c < NV; c++)
            v[c] = ((s0 ? t1[c] : t0[c]) * w00 + (s1 ? t1[c] : t0[c]) * w01 + (s0 ? b1[c] : b0[c]) * w10 +
                    (s1 ? b1[c] : b0[c]) * w11 + 512) >> 10;
    } else {
        const uint8_t *p00 = r0 + x0 * CN, *p01 = r0 + x1 * CN, *p10 = r1 + x0 * CN, *p11 = r1 + x1 * CN;
#pragma unroll
        for (int c = 0; c < NV; c++)
            v[c] = ((int)p00[c] * w00 + (int)p01[c] * w01 + (int)p10[c] * w10 + (int)p11[c] * w11 + 512) >> 10;
    }
    if constexpr (CN == 1)
        return (uint32_t)v[0];
    else
        return (uint32_t)((v[0] * a.gw0 + v[1] * a.gw1 + v[2] * a.gw2 + (1 << (a.gshift - 1))) >> a.gshift);
}

// (the body is a function of its own so that pagk_group_sensor_kernel.h can run it for one of several cameras per launch)
template <int CN, bool PAIR>
__device__ __forceinline__ void rectify_body(const RectArgs &a)
{
    const int quads = a.wp >> 2;                                    // threads per destination row
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)quads * a.H) return;
    const int r = (int)(t / quads), q = (int)(t - (long long)r * quads);
    const uint4 *e = reinterpret_cast<const uint4 *>(a.entries + (size_t)r * a.wp + 4 * q);   // 32-byte aligned
    const uint4 e01 = e[0], e23 = e[1];
    const uint32_t g0 = rectify_pixel<CN, PAIR>(a, e01.x, e01.y), g1 = rectify_pixel<CN, PAIR>(a, e01.z, e01.w);
    const uint32_t g2 = rectify_pixel<CN, PAIR>(a, e23.x, e23.y), g3 = rectify_pixel<CN, PAIR>(a, e23.z, e23.w);
    uint8_t *d = a.dst + (size_t)r * a.W + 4 * q;
    if (!(a.W & 3)) {   // every row starts on a dword and has no tail
        *reinterpret_cast<uint32_t *>(d) = g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
        return;
    }
    const int left = a.W - 4 * q;   // >= 1
    d[0] = (uint8_t)g0;
    if (left > 1) d[1] = (uint8_t)g1;
    if (left > 2) d[2] = (uint8_t)g2;
    if (left > 3) d[3] = (uint8_t)g3;
}

template <int CN, bool PAIR>
__global__ __launch_bounds__(256) void k_rectify(RectArgs a)
{
    rectify_body<CN, PAIR>(a);
}

}  // namespace pagk
