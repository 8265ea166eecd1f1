// pagk_orb_kernel.h -- the describe and match halves of the reference's ORB baseline for one level: the 7 x 7 blur,
// IC_Angle, the steered rBRIEF descriptor (reference src/ORBextractor.cc:101-171, 1057-1064, 1113-1130) and the
// brute-force Hamming matcher with its distance filter (src/ORBDetectAndDespMatcher.cpp:55-91).  The definition is in
// include/pagk.h ("ORB descriptors and matching"); tests/orb_ref.c restates it in plain C.
//
// Shapes:
//   k_orb_blur      a workgroup produces a 64 x 16 tile: the 70 x 22 source bytes go into the LDS once (one global read per
//                   pixel, the border reflected while loading), the horizontal pass leaves exact integers in the LDS, the
//                   vertical pass reads them as 16-byte rows and a thread stores its four pixels as one dword (the blurred
//                   image has a pitch that is a multiple of four).  Workgroup (0, 0) also zeroes the info words, so the
//                   describe kernel behind it can count with atomics and no extra node is needed.
//   k_orb_describe  one wavefront per keypoint.  The 31 x 31 square around the centre is walked 64 pixels at a time, the
//                   pixels outside the disc masked; the two int32 moments are reduced over the wave (integers: the order
//                   does not matter).  Every lane then computes the same angle and steering pair, compares its own four
//                   tap pairs (its 16 pattern integers are four 16-byte loads), four ballots collect the 256 bits and two
//                   lanes store the 32 bytes as two 16-byte rows.
//   k_orb_match     a wave holds 64 query rows in registers (eight dwords per lane) and walks chunks of 128 train rows
//                   staged in the LDS (every lane reads the same row: a broadcast).  The best (distance << 20 | index) of a
//                   chunk goes into the query's key with an integer atomicMin: order-free, so the train set is split over
//                   workgroups.  k_orb_match_finish, one workgroup, takes the minimum over all queries, applies the filter
//                   and writes the outputs.
// No launch is sized by a count: the grids come from the capacities, the counts are read on the device.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pagk {

constexpr int kOrbEdge = 19;          // EDGE_THRESHOLD
constexpr int kOrbHalfPatch = 15;     // HALF_PATCH_SIZE
constexpr int kOrbInfoWords = 8;      // PAGK_ORB_INFO_WORDS
constexpr int kOrbPatternInts = 1024; // 512 points, x then y
constexpr int kOrbMaxRows = 1 << 20;  // cap, cap_q, cap_t: an index fits the low 20 bits of a match key
constexpr int kOrbBlurTx = 64, kOrbBlurTy = 16;
constexpr int kOrbMatchChunk = 128;   // train rows staged per step
constexpr int kOrbMatchMaxChunkGroups = 512;

// umax[v] of ORBextractor's constructor (:478-493) for HALF_PATCH_SIZE 15: 749 pixels in the disc
static __device__ const int8_t kOrbUmax[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};

// ---- the arithmetic of the definition -------------------------------------------------------------------------------
// cv::fastAtan2's scalar form in f32, one rounding per operation (degrees)
__device__ __forceinline__ float orb_fast_atan2(float y, float x)
{
    constexpr float p1 = 0x1.ca44dep+5f, p3 = -0x1.2aaddcp+4f, p5 = 0x1.1d3f7ep+3f, p7 = -0x1.4515b2p+1f, eps = 0x1p-52f;
    const float ax = fabsf(x), ay = fabsf(y);
    float a;
    if (ax >= ay) {
        const float c = ay / (ax + eps), c2 = c * c;
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    } else {
        const float c = ax / (ay + eps), c2 = c * c;
        a = 90.0f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    }
    if (x < 0.0f) a = 180.0f - a;
    if (y < 0.0f) a = 360.0f - a;
    return a;
}

// a = (float)cos(r), b = (float)sin(r) for r >= 0 by the algorithm stated in include/pagk.h: f64 + - * only
__device__ __forceinline__ void orb_cos_sin(float r, float *a, float *b)
{
    constexpr double two_over_pi = 0x1.45f306dc9c883p-1, pio2_hi = 0x1.921fb544p+0, pio2_lo = 0x1.0b4611a626331p-34;
    constexpr double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                     S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    constexpr double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                     C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double x = (double)r;
    const int k = (int)(x * two_over_pi + 0.5);
    const double kd = (double)k;
    const double t = (x - kd * pio2_hi) - kd * pio2_lo;
    const double z = t * t;
    const double s = t + t * (z * (S1 + z * (S2 + z * (S3 + z * (S4 + z * (S5 + z * S6))))));
    const double c = 1.0 - z * (0.5 - z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6))))));
    const int q = k & 3;
    const double co = q == 0 ? c : (q == 1 ? -s : (q == 2 ? -c : s));
    const double si = q == 0 ? s : (q == 1 ? c : (q == 2 ? -s : -c));
    *a = (float)co, *b = (float)si;
}

// BORDER_REFLECT_101 for i in [-3, n + 2], n >= 4; any other i is clamped into the image (such a pixel only feeds
// outputs that are never stored)
__device__ __forceinline__ int orb_reflect(int i, int n)
{
    i = i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i);
    return min(max(i, 0), n - 1);
}

// ---- the blur -------------------------------------------------------------------------------------------------------
struct OrbBlurArgs {
    const uint8_t *img;   // H rows of pitch bytes
    long long pitch;
    uint8_t *blur;        // H rows of wp bytes, wp = W rounded up to a multiple of 4
    int32_t *info;        // kOrbInfoWords, zeroed here
    int W, H, wp;
    int w0, w1, w2, w3;   // Q8 taps for offsets 0, +-1, +-2, +-3
};

// (the bodies of the blur and the describe kernel are functions of their own so that pagk_orb_levels_kernel.h can run them on
// one of several levels per launch; bx, by / block: the workgroup's place in the level's own grid)
__device__ __forceinline__ void orb_blur_body(const OrbBlurArgs &a, int bx, int by)
{
    constexpr int SW = kOrbBlurTx + 6, SH = kOrbBlurTy + 6, SP = 72;
    __shared__ uint8_t src[SH * SP];
    __shared__ __attribute__((aligned(16))) uint32_t hor[SH * kOrbBlurTx];
    const int tid = threadIdx.x, x0 = bx * kOrbBlurTx, y0 = by * kOrbBlurTy;
    if (bx == 0 && by == 0 && tid < kOrbInfoWords) a.info[tid] = 0;
    for (int i = tid; i < SW * SH; i += 256) {
        const int ry = i / SW, rx = i - ry * SW;
        const int gy = orb_reflect(y0 + ry - 3, a.H), gx = orb_reflect(x0 + rx - 3, a.W);
        src[ry * SP + rx] = a.img[(long long)gy * a.pitch + gx];
    }
    __syncthreads();
    for (int i = tid; i < SH * kOrbBlurTx; i += 256) {
        const int r = i >> 6, c = i & 63;
        const uint8_t *p = src + r * SP + c;   // p[3] is the centre
        hor[i] = (uint32_t)(a.w0 * p[3] + a.w1 * (p[2] + p[4]) + a.w2 * (p[1] + p[5]) + a.w3 * (p[0] + p[6]));
    }
    __syncthreads();
    const int xg = tid & 15, row = tid >> 4;
    const int gx = x0 + 4 * xg, gy = y0 + row;
    if (gx >= a.wp || gy >= a.H) return;
    const uint4 *h = reinterpret_cast<const uint4 *>(hor) + row * (kOrbBlurTx / 4) + xg;   // h[k * 16]: row + k
    const int wk[7] = {a.w3, a.w2, a.w1, a.w0, a.w1, a.w2, a.w3};
    uint32_t s0 = 32768u, s1 = 32768u, s2 = 32768u, s3 = 32768u;
#pragma unroll
    for (int k = 0; k < 7; k++) {
        const uint4 v = h[k * (kOrbBlurTx / 4)];
        s0 += (uint32_t)wk[k] * v.x, s1 += (uint32_t)wk[k] * v.y, s2 += (uint32_t)wk[k] * v.z, s3 += (uint32_t)wk[k] * v.w;
    }
    *reinterpret_cast<uint32_t *>(a.blur + (size_t)gy * a.wp + gx) =
        (s0 >> 16) | ((s1 >> 16) << 8) | ((s2 >> 16) << 16) | ((s3 >> 16) << 24);
}

__global__ __launch_bounds__(256) void k_orb_blur(OrbBlurArgs a) { orb_blur_body(a, blockIdx.x, blockIdx.y); }

// ---- orientation and descriptor -------------------------------------------------------------------------------------
struct OrbDescArgs {
    const uint8_t *img;       // the unblurred image (orientation)
    long long pitch;
    const uint8_t *blur;      // the blurred image (descriptor), pitch wp
    const int32_t *pattern;   // kOrbPatternInts, every value in [-13, 13]
    const float *keypoints;   // cap x 2
    const int32_t *n;         // device count
    float *angle;             // cap, or nullptr
    uint8_t *desc;            // cap x 32, 16-byte aligned
    int32_t *info;
    int W, H, wp, cap;
};

__device__ __forceinline__ void orb_describe_body(const OrbDescArgs &a, int block)
{
    const int lane = threadIdx.x & 63;
    const int k = block * 4 + (threadIdx.x >> 6);   // the wave's keypoint
    if (k >= a.cap) return;
    const int n = min(max(*a.n, 0), a.cap);
    uint4 *out = reinterpret_cast<uint4 *>(a.desc + (size_t)k * 32);
    // cvRound, then the border test on the float (a NaN or a huge coordinate fails it before any conversion)
    float fx = 0.0f, fy = 0.0f;
    bool inside = false;
    if (k < n) {
        fx = rintf(a.keypoints[2 * k]), fy = rintf(a.keypoints[2 * k + 1]);
        inside = fx >= (float)kOrbEdge && fx < (float)(a.W - kOrbEdge) && fy >= (float)kOrbEdge && fy < (float)(a.H - kOrbEdge);
    }
    if (!inside) {   // wave-uniform: past the count (angle 0), or outside the border (angle -1, counted)
        if (lane < 2) out[lane] = make_uint4(0u, 0u, 0u, 0u);
        if (lane == 0) {
            if (a.angle) a.angle[k] = k < n ? -1.0f : 0.0f;
            if (k < n) atomicAdd(a.info + 1, 1);
        }
        return;
    }
    const int cx = (int)fx, cy = (int)fy;
    // IC_Angle: the 31 x 31 square, 64 pixels per step, masked to the disc
    int m10 = 0, m01 = 0;
    const uint8_t *c0 = a.img + (long long)cy * a.pitch + cx;
    for (int p = lane; p < 31 * 31; p += 64) {
        const int v = p / 31 - kOrbHalfPatch, u = p - (v + kOrbHalfPatch) * 31 - kOrbHalfPatch;
        if (abs(u) <= kOrbUmax[abs(v)]) {
            const int val = c0[(long long)v * a.pitch + u];
            m10 += u * val, m01 += v * val;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m10 += __shfl_xor(m10, o, 64), m01 += __shfl_xor(m01, o, 64);
    const float ang = orb_fast_atan2((float)m01, (float)m10);
    constexpr float factor_pi = 0x1.1df46ap-6f;   // (float)(CV_PI / 180.f)
    float ca, sb;
    orb_cos_sin(ang * factor_pi, &ca, &sb);
    // the lane's four comparisons: pairs 4 * lane .. 4 * lane + 3, sixteen pattern integers
    const int4 *pat = reinterpret_cast<const int4 *>(a.pattern) + 4 * lane;
    const uint8_t *b0 = a.blur + (size_t)cy * a.wp + cx;
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int4 q = pat[j];   // x0 y0 x1 y1
        const float x0 = (float)q.x, y0 = (float)q.y, x1 = (float)q.z, y1 = (float)q.w;
        int r0 = (int)rintf(x0 * sb + y0 * ca), c0x = (int)rintf(x0 * ca - y0 * sb);
        int r1 = (int)rintf(x1 * sb + y1 * ca), c1x = (int)rintf(x1 * ca - y1 * sb);
        // |tap| <= 18 by the pattern's range (include/pagk.h); the clamp never acts, it only keeps every address inside
        // the image whatever the pattern buffer holds
        r0 = min(max(r0, -18), 18), c0x = min(max(c0x, -18), 18), r1 = min(max(r1, -18), 18), c1x = min(max(c1x, -18), 18);
        const int t0 = b0[r0 * a.wp + c0x], t1 = b0[r1 * a.wp + c1x];
        bits |= (uint32_t)(t0 < t1) << j;
    }
    // descriptor bit 4 * l + j = bit l of ballot j; lanes 0 and 1 assemble sixteen bytes each
    const unsigned long long bal0 = __ballot(bits & 1u), bal1 = __ballot(bits & 2u), bal2 = __ballot(bits & 4u),
                             bal3 = __ballot(bits & 8u);
    if (lane < 2) {
        uint32_t w[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int first = 32 * lane + 8 * i;   // the eight lanes whose nibbles make this dword
            const uint32_t n0 = (uint32_t)(bal0 >> first) & 255u, n1 = (uint32_t)(bal1 >> first) & 255u,
                           n2 = (uint32_t)(bal2 >> first) & 255u, n3 = (uint32_t)(bal3 >> first) & 255u;
            uint32_t word = 0;
#pragma unroll
            for (int l = 0; l < 8; l++)
                word |= (((n0 >> l) & 1u) | (((n1 >> l) & 1u) << 1) | (((n2 >> l) & 1u) << 2) | (((n3 >> l) & 1u) << 3)) << (4 * l);
            w[i] = word;
        }
        out[lane] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    if (lane == 0) {
        if (a.angle) a.angle[k] = ang;
        atomicAdd(a.info, 1);
    }
}

__global__ __launch_bounds__(256) void k_orb_describe(OrbDescArgs a) { orb_describe_body(a, blockIdx.x); }

// ---- matching -------------------------------------------------------------------------------------------------------
struct OrbMatchArgs {
    const uint8_t *desc_q, *desc_t;   // cap_q x 32, cap_t x 32, 16-byte aligned
    const int32_t *nq, *nt;           // device counts
    uint32_t *keys;                   // cap_q, 0xffffffff before k_orb_match
    int32_t *train_idx, *distance;    // cap_q each
    uint8_t *keep;                    // cap_q
    int32_t *info;
    int cap_q, cap_t, match_floor;
};

__global__ __launch_bounds__(64) void k_orb_match(OrbMatchArgs a)
{
    __shared__ uint4 rows[kOrbMatchChunk * 2];
    const int lane = threadIdx.x;
    const int nq = min(max(*a.nq, 0), a.cap_q), nt = min(max(*a.nt, 0), a.cap_t);
    const int q = blockIdx.x * 64 + lane;
    if ((int)blockIdx.x * 64 >= nq) return;   // (the whole wave)
    uint4 qa = make_uint4(0u, 0u, 0u, 0u), qb = qa;
    if (q < nq) {
        const uint4 *p = reinterpret_cast<const uint4 *>(a.desc_q) + 2 * (size_t)q;
        qa = p[0], qb = p[1];
    }
    uint32_t best = 0xffffffffu;
    for (int t0 = blockIdx.y * kOrbMatchChunk; t0 < nt; t0 += gridDim.y * kOrbMatchChunk) {
        const int cnt = min(kOrbMatchChunk, nt - t0);
        __syncthreads();
        const uint4 *g = reinterpret_cast<const uint4 *>(a.desc_t) + 2 * (size_t)t0;
        for (int i = lane; i < 2 * cnt; i += 64) rows[i] = g[i];
        __syncthreads();
        for (int r = 0; r < cnt; r++) {
            const uint4 ta = rows[2 * r], tb = rows[2 * r + 1];
            const uint32_t d = __popc(qa.x ^ ta.x) + __popc(qa.y ^ ta.y) + __popc(qa.z ^ ta.z) + __popc(qa.w ^ ta.w) +
                               __popc(qb.x ^ tb.x) + __popc(qb.y ^ tb.y) + __popc(qb.z ^ tb.z) + __popc(qb.w ^ tb.w);
            best = min(best, (d << 20) | (uint32_t)(t0 + r));
        }
    }
    if (q < nq && best != 0xffffffffu) atomicMin(a.keys + q, best);
}

// minimum / maximum / sum over a workgroup of 1024 (every thread calls; scratch: 3 x 16 words)
__device__ __forceinline__ void orb_block_reduce(int &mn, int &mx, int &sum, int *scratch)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = min(mn, __shfl_xor(mn, o, 64)), mx = max(mx, __shfl_xor(mx, o, 64)), sum += __shfl_xor(sum, o, 64);
    }
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[wave] = mn, scratch[16 + wave] = mx, scratch[32 + wave] = sum;
    __syncthreads();
    mn = scratch[0], mx = scratch[16], sum = scratch[32];
    for (int w = 1; w < 16; w++) mn = min(mn, scratch[w]), mx = max(mx, scratch[16 + w]), sum += scratch[32 + w];
}

__global__ __launch_bounds__(1024) void k_orb_match_finish(OrbMatchArgs a)
{
    __shared__ int scratch[48];
    const int tid = threadIdx.x;
    const int nq = min(max(*a.nq, 0), a.cap_q), nt = min(max(*a.nt, 0), a.cap_t);
    const int matches = nt > 0 ? nq : 0;
    int mn = 257, mx = 0, kept = 0;
    for (int q = tid; q < matches; q += 1024) {
        const int d = (int)(a.keys[q] >> 20);
        mn = min(mn, d), mx = max(mx, d);
    }
    orb_block_reduce(mn, mx, kept, scratch);
    if (!matches) mn = 0;
    const int thr = max(2 * mn, a.match_floor);
    kept = 0;
    for (int q = tid; q < a.cap_q; q += 1024) {
        int idx = -1, d = 257, kp = 0;
        if (q < matches) {
            const uint32_t key = a.keys[q];
            idx = (int)(key & 0xfffffu), d = (int)(key >> 20), kp = d <= thr;
        }
        a.train_idx[q] = idx, a.distance[q] = d, a.keep[q] = (uint8_t)kp;
        kept += kp;
    }
    int m2 = 0, x2 = 0;
    orb_block_reduce(m2, x2, kept, scratch);
    if (tid < kOrbInfoWords) {
        const int words[kOrbInfoWords] = {nq, matches, kept, mn, mx, thr, 0, 0};
        a.info[tid] = words[tid];
    }
}

}  // namespace pagk
