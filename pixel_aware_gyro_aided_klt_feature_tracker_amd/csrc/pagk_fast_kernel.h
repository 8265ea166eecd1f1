// pagk_fast_kernel.h -- the detector the reference's front-ends run, on the device (include/pagk.h: pagk_detect_fast_device,
// pagk_frame_handover_fast_device).  ORBextractor::DetectFeatures (reference src/ORBextractor.cc:1148-1205) with one level:
// FAST-9/16 with non-maximum suppression in cells of about 30 pixels and a per-cell fall-back threshold
// (ComputeKeyPointsOctTree, :789-871), DistributeOctTree (:563-787), the mask test (:1199-1203).  The definition the
// kernels implement is the one written down in include/pagk.h and restated in plain C in tests/fast_detect_ref.c; it is
// integer arithmetic throughout.  No parity with cv::FAST is claimed.
//   k_fast_cells    one workgroup per cell: the window in LDS, m(p) once per pixel, suppression at the first threshold and,
//                   if that leaves nothing, at the second; survivors into the cell's fixed segment in raster order
//   k_fast_offsets  where every cell's keys start in the raw list; the counts of the info words
//   k_fast_gather   the segments into the raw list (cells in loop order, raster order inside a cell)
//   k_fast_tree     one workgroup: the quadtree pass by pass, the best key of every node, the mask, the ordered output
// How the tree is held.  The reference's std::list is an array of nodes in list order, rebuilt by every pass (two buffers
// in turn); a key knows the list position of its node.  A pass counts the keys of every node it may split per quadrant
// (integer atomics: the sums do not depend on their order), decides which nodes are split, and computes the new list from
// the push-front rule: the c-th child created in the pass (parents in walk order, n1 .. n4) lands at position C - 1 - c of
// C children, the nodes that were not split follow in their old order.  The keys of a node are never moved: "the first key
// with the largest response" of a node is the one with the smallest raw index, because every split keeps the order of the
// raw list inside a child.
// The phase-2 walk sorts by (size, creation number) and goes from the back.  Its candidates are exactly the children of
// the pass before, which stand at the front of the list in reverse creation order: the larger creation number is the
// smaller list position.  So the walk order is: size descending, then list position ascending, and no creation number is
// stored.  The walk's break is a prefix sum over that order.
// Every count stays on the device: launches are sized by W, H and the bounds.  Plain HIP C++, vector stores and C++
// atomics only.  No kernel waits for another workgroup.  Barriers sit in loops bounded by kernel arguments or by values
// every lane of the workgroup reads from one address.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pagk {

constexpr int kFastBorder = 16;      // minBorder = EDGE_THRESHOLD - 3 (:797)
constexpr int kFastCell = 30;        // W of ComputeKeyPointsOctTree (:793)
constexpr int kFastWin = 65;         // the largest cell window: wCell <= 59, plus 6
constexpr int kFastWinPitch = 68;

// control words in the workspace: [0] raw keys, [1] cells whose first pass was empty, [2] (fused call) unused: the plan's
// n_new, [3] (fused call) 1 = the top-up does not run (the indices k_handover_plan writes), [4] cells empty after both
enum { kFastCtlCount = 0, kFastCtlFirstEmpty = 1, kFastCtlSkip = 3, kFastCtlEmpty = 4 };
constexpr int32_t kFastCellFirstEmpty = 1 << 30, kFastCellEmpty = 1 << 29, kFastCellCountMask = (1 << 24) - 1;

// The cell grid of :805-830 and the initial nodes of :565-590, computed once on the host.
struct FastGrid {
    int32_t W, H, n_cols, n_rows, w_cell, h_cell, max_bx, max_by;
    int32_t seg;     // keys a cell can yield: ceil(w_cell / 2) * ceil(h_cell / 2)
    int32_t n_ini;   // initial nodes
    float hx;        // their width
};

struct FastCellArgs {
    const uint8_t *img;
    int64_t pitch;
    FastGrid g;
    int32_t t_ini, t_min;
    uint32_t *seg_xy;     // x | y << 16, relative to minBorder
    int32_t *seg_score;
    int32_t *cell_cnt;
    const int32_t *skip;
};

// exclusive rank of this lane's `take` among the workgroup's 256 in thread order, and the workgroup's total
__device__ __forceinline__ int32_t fast_scan256(bool take, int32_t *wtot, int lane, int wave, int32_t &tot)
{
    const unsigned long long bal = __ballot(take);
    if (lane == 0) wtot[wave] = __popcll(bal);
    __syncthreads();
    int32_t off = 0;
    tot = 0;
    for (int w = 0; w < 4; w++) {
        off += w < wave ? wtot[w] : 0;
        tot += wtot[w];
    }
    __syncthreads();
    return off + __popcll(bal & ((1ull << lane) - 1ull));
}

// m(p): the largest, over the 16 arcs of 9 consecutive ring pixels and both polarities, of the smallest difference on the arc
__device__ __forceinline__ int fast_m(const uint8_t (*s)[kFastWinPitch], int y, int x)
{
    // the Bresenham circle of radius 3 in OpenCV's order, from (0, 3)
    constexpr int rx[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
    constexpr int ry[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};
    const int c = s[y][x];
    int d[16], lo2[16], hi2[16], lo4[16], hi4[16], lo8[16], hi8[16];
#pragma unroll
    for (int k = 0; k < 16; k++) d[k] = (int)s[y + ry[k]][x + rx[k]] - c;
#pragma unroll
    for (int k = 0; k < 16; k++) lo2[k] = min(d[k], d[(k + 1) & 15]), hi2[k] = max(d[k], d[(k + 1) & 15]);
#pragma unroll
    for (int k = 0; k < 16; k++) lo4[k] = min(lo2[k], lo2[(k + 2) & 15]), hi4[k] = max(hi2[k], hi2[(k + 2) & 15]);
#pragma unroll
    for (int k = 0; k < 16; k++) lo8[k] = min(lo4[k], lo4[(k + 4) & 15]), hi8[k] = max(hi4[k], hi4[(k + 4) & 15]);
    int m = -255;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const int lo9 = min(lo8[k], d[(k + 8) & 15]), hi9 = max(hi8[k], d[(k + 8) & 15]);
        m = max(m, max(lo9, -hi9));   // ring brighter by at least lo9 on the arc; darker by at least -hi9
    }
    return m;
}

// S_t: the score of a corner at threshold t, 0 for everything else
__device__ __forceinline__ int fast_score(int m, int t) { return m > t ? m - 1 : 0; }

// (the body is a function of its own so that pagk_orb_levels_kernel.h can run it on one of several levels per launch)
__device__ __forceinline__ void fast_cells_body(const FastCellArgs &a)
{
    __shared__ uint8_t s_img[kFastWin][kFastWinPitch];
    __shared__ uint8_t s_m[kFastWin][kFastWinPitch];   // max(m, 0); 0 outside the cell's detection region
    __shared__ int32_t s_wtot[4];
    if (a.skip && *a.skip) return;   // (one address: the whole workgroup takes the same way)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const FastGrid &g = a.g;
    const int cell = blockIdx.x, ci = cell / g.n_cols, cj = cell - ci * g.n_cols;
    const int ini_y = kFastBorder + ci * g.h_cell, ini_x = kFastBorder + cj * g.w_cell;
    if (ini_y >= g.max_by - 3 || ini_x >= g.max_bx - 6) {   // :818, :827: no such cell
        if (tid == 0) a.cell_cnt[cell] = 0;
        return;
    }
    const int max_y = min(ini_y + g.h_cell + 6, g.max_by), max_x = min(ini_x + g.w_cell + 6, g.max_bx);
    const int w = max_x - ini_x, h = max_y - ini_y;   // at most 65 each
    for (int t = tid; t < w * h; t += 256) {
        const int ly = t / w, lx = t - ly * w;
        s_img[ly][lx] = a.img[(int64_t)(ini_y + ly) * a.pitch + ini_x + lx];
        s_m[ly][lx] = 0;
    }
    __syncthreads();
    const int rw = w - 6, rh = h - 6;
    const int npx = rw > 0 && rh > 0 ? rw * rh : 0;
    for (int t = tid; t < npx; t += 256) {
        const int y = t / rw + 3, x = t - (t / rw) * rw + 3;
        const int m = fast_m(s_img, y, x);
        s_m[y][x] = (uint8_t)(m > 0 ? m : 0);
    }
    __syncthreads();
    const size_t seg0 = (size_t)cell * g.seg;
    int32_t total = 0;
    int pass = 0;
    for (; pass < 2; pass++) {   // :833-840: the second threshold only where the first found nothing
        const int thr = pass ? a.t_min : a.t_ini;
        for (int c0 = 0; c0 < npx; c0 += 256) {   // raster order, 256 pixels at a time
            const int t = c0 + tid;
            bool keep = false;
            int x = 0, y = 0, sc = 0;
            if (t < npx) {
                y = t / rw + 3, x = t - (t / rw) * rw + 3;
                sc = fast_score(s_m[y][x], thr);
                if (sc > 0) {
                    keep = true;
#pragma unroll
                    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                        for (int dx = -1; dx <= 1; dx++)
                            if (dx | dy) keep = keep && sc > fast_score(s_m[y + dy][x + dx], thr);
                }
            }
            int32_t tot;
            const int32_t o = total + fast_scan256(keep, s_wtot, lane, wave, tot);
            if (keep && o < g.seg) {
                a.seg_xy[seg0 + o] = (uint32_t)(x + cj * g.w_cell) | ((uint32_t)(y + ci * g.h_cell) << 16);   // :846-847
                a.seg_score[seg0 + o] = sc;
            }
            total += tot;
        }
        if (total > 0) break;   // (the same value in every lane)
    }
    if (tid == 0)
        a.cell_cnt[cell] = (total < g.seg ? total : g.seg) | (pass >= 1 ? kFastCellFirstEmpty : 0) | (pass >= 2 ? kFastCellEmpty : 0);
}

__global__ void __launch_bounds__(256) k_fast_cells(FastCellArgs a) { fast_cells_body(a); }

// exclusive prefix of v over the workgroup's 1024 in thread order, and the workgroup's total
__device__ __forceinline__ int32_t fast_scan1024(int32_t v, int32_t *wtot, int lane, int wave, int32_t &tot)
{
    int32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int32_t o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    int32_t off = 0;
    tot = 0;
    for (int w = 0; w < 16; w++) {
        off += w < wave ? wtot[w] : 0;
        tot += wtot[w];
    }
    __syncthreads();
    return off + inc - v;
}

// One workgroup: cell_off[c] = the keys of the cells in front of c; the control words.
__device__ __forceinline__ void fast_offsets_body(int32_t n_cells, const int32_t *cell_cnt, int32_t *cell_off, int32_t *ctl,
                                                  const int32_t *skip)
{
    __shared__ int32_t s_wtot[16];
    if (skip && *skip) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t base = 0, first = 0, empty = 0;
    for (int c0 = 0; c0 < n_cells; c0 += 1024) {
        const int c = c0 + tid;
        const int32_t v = c < n_cells ? cell_cnt[c] : 0;
        int32_t tot, t2;
        const int32_t o = base + fast_scan1024(v & kFastCellCountMask, s_wtot, lane, wave, tot);
        if (c < n_cells) cell_off[c] = o;
        base += tot;
        (void)fast_scan1024(((v & kFastCellFirstEmpty) ? 1 : 0) | ((v & kFastCellEmpty) ? 1 << 16 : 0), s_wtot, lane, wave, t2);
        first += t2 & 0xffff, empty += t2 >> 16;   // (at most 1024 per round: the two halves do not meet)
    }
    if (tid == 0) ctl[kFastCtlCount] = base, ctl[kFastCtlFirstEmpty] = first, ctl[kFastCtlEmpty] = empty;
}

__global__ void __launch_bounds__(1024) k_fast_offsets(int32_t n_cells, const int32_t *cell_cnt, int32_t *cell_off, int32_t *ctl,
                                                       const int32_t *skip)
{
    fast_offsets_body(n_cells, cell_cnt, cell_off, ctl, skip);
}

// one workgroup per cell: its segment to its place in the raw list
__device__ __forceinline__ void fast_gather_body(int32_t seg, const int32_t *cell_cnt, const int32_t *cell_off,
                                                 const uint32_t *seg_xy, const int32_t *seg_score, uint32_t *kxy,
                                                 int32_t *kscore, const int32_t *skip)
{
    if (skip && *skip) return;
    const int cell = blockIdx.x;
    const int32_t cnt = cell_cnt[cell] & kFastCellCountMask, off = cell_off[cell];
    const size_t seg0 = (size_t)cell * seg;
    for (int r = threadIdx.x; r < cnt && r < seg; r += 256) kxy[off + r] = seg_xy[seg0 + r], kscore[off + r] = seg_score[seg0 + r];
}

__global__ void __launch_bounds__(256) k_fast_gather(int32_t seg, const int32_t *cell_cnt, const int32_t *cell_off,
                                                     const uint32_t *seg_xy, const int32_t *seg_score, uint32_t *kxy,
                                                     int32_t *kscore, const int32_t *skip)
{
    fast_gather_body(seg, cell_cnt, cell_off, seg_xy, seg_score, kxy, kscore, skip);
}

struct FastTreeArgs {
    FastGrid g;
    int32_t n_features, cap, out_bound, raw_bound;
    uint32_t sort_slots;      // a power of two >= out_bound
    const int32_t *ctl;
    const uint32_t *kxy;
    const int32_t *kscore;
    int32_t *knode;           // raw_bound: the list position of the key's node
    int4 *box[2];             // out_bound each: x0, y0, x1, y1 = UL.x, UL.y, BR.x, BR.y
    int32_t *ncnt[2];         // keys of the node
    int32_t *ncand[2];        // 1 = created by the pass before with more than one key (vSizeAndPointerToNode)
    int32_t *cnt4;            // 4 * out_bound: keys per quadrant
    int32_t *cbase;           // out_bound: a split node's first creation index; another node's new position
    int32_t *split;           // out_bound
    unsigned long long *sortk;   // sort_slots
    unsigned long long *best;    // out_bound
    const uint8_t *mask;      // W * H, or NULL
    float *out_xy, *out_resp;
    int32_t *info;
    const int32_t *skip;
};

// the quadrant of ExtractorNode::DivideNode (:505-561): 0 = n1 (upper left), 1 = n2, 2 = n3, 3 = n4
__device__ __forceinline__ int fast_quadrant(const int4 b, uint32_t xy)
{
    const int x = (int)(xy & 0xffffu), y = (int)(xy >> 16);
    const int mx = b.x + ((b.z - b.x + 1) >> 1), my = b.y + ((b.w - b.y + 1) >> 1);   // ceil(extent / 2)
    return (x < mx ? 0 : 1) + (y < my ? 0 : 2);
}
__device__ __forceinline__ int4 fast_child_box(const int4 b, int q)
{
    const int mx = b.x + ((b.z - b.x + 1) >> 1), my = b.y + ((b.w - b.y + 1) >> 1);
    return make_int4(q & 1 ? mx : b.x, q & 2 ? my : b.y, q & 1 ? b.z : mx, q & 2 ? b.w : my);
}

__device__ __forceinline__ void fast_tree_body(const FastTreeArgs &a)
{
    __shared__ int32_t s_wtot[16];
    __shared__ int32_t s_nexp;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool skip = a.skip && *a.skip;
    const int32_t N = a.n_features;
    int32_t n = skip ? 0 : a.ctl[kFastCtlCount];
    n = n < 0 ? 0 : (n > a.raw_bound ? a.raw_bound : n);
    int32_t T = 0, passes = 0;
    int cur = 0;
    bool bad = false;
    if (!skip) {
        // the initial nodes (:565-612): key to node int(x / hX); the empty ones are erased
        const int32_t n_ini = a.g.n_ini;
        for (int i = tid; i < n_ini; i += 1024) a.cnt4[i] = 0;
        __syncthreads();
        for (int k = tid; k < n; k += 1024) {
            int ni = (int)((float)(a.kxy[k] & 0xffffu) / a.g.hx);
            ni = ni < n_ini ? ni : n_ini - 1;
            a.knode[k] = ni;
            atomicAdd(&a.cnt4[ni], 1);
        }
        __syncthreads();
        for (int c0 = 0; c0 < n_ini; c0 += 1024) {
            const int i = c0 + tid;
            const int32_t cnt = i < n_ini ? a.cnt4[i] : 0;
            int32_t tot;
            const int32_t o = T + fast_scan1024(cnt > 0 ? 1 : 0, s_wtot, lane, wave, tot);
            if (i < n_ini) a.cbase[i] = o;
            if (cnt > 0) {
                a.box[0][o] = make_int4((int)(a.g.hx * (float)i), 0, (int)(a.g.hx * (float)(i + 1)), a.g.max_by - kFastBorder);
                a.ncnt[0][o] = cnt;
                a.ncand[0][o] = cnt > 1 ? 1 : 0;
            }
            T += tot;
        }
        __syncthreads();
        for (int k = tid; k < n; k += 1024) a.knode[k] = a.cbase[a.knode[k]];
        __syncthreads();

        bool fin = false, phase2 = false;
        while (!fin) {   // (fin, phase2, T: the same in every lane)
            passes++;
            const int32_t prev = T;
            const int4 *box = a.box[cur];
            const int32_t *ncand = a.ncand[cur];
            for (int i = tid; i < 4 * T; i += 1024) a.cnt4[i] = 0;
            for (int i = tid; i < T; i += 1024) a.split[i] = 0;
            if (tid == 0) s_nexp = 0;
            __syncthreads();
            for (int k = tid; k < n; k += 1024) {
                const int32_t p = a.knode[k];
                if (ncand[p]) atomicAdd(&a.cnt4[4 * p + fast_quadrant(box[p], a.kxy[k])], 1);
            }
            __syncthreads();
            int32_t C = 0, nsplit = 0;
            if (!phase2) {
                // an outer round (:618-691): every node that is not final is split, front to back
                for (int c0 = 0; c0 < T; c0 += 1024) {
                    const int p = c0 + tid;
                    int32_t nch = 0;
                    const bool sp = p < T && ncand[p] != 0;
                    if (sp)
                        for (int q = 0; q < 4; q++) nch += a.cnt4[4 * p + q] > 0 ? 1 : 0;
                    int32_t tot, tot2;
                    const int32_t o = C + fast_scan1024(nch, s_wtot, lane, wave, tot);
                    (void)fast_scan1024(sp ? 1 : 0, s_wtot, lane, wave, tot2);
                    if (sp) a.cbase[p] = o, a.split[p] = 1;
                    C += tot, nsplit += tot2;
                }
            } else {
                // an inner pass (:700-761): the candidates by size, the largest first, equal sizes by list position; one
                // is split while the list is still shorter than N
                const uint32_t M = a.sort_slots;
                for (uint32_t i = tid; i < M; i += 1024)
                    a.sortk[i] = (i < (uint32_t)T && ncand[i]) ? ((unsigned long long)(uint32_t)a.ncnt[cur][i] << 32) | (0xffffffffu - i) : 0ull;
                __syncthreads();
                for (uint32_t k = 2; k <= M; k <<= 1)
                    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                        for (uint32_t t = tid; t < M / 2; t += 1024) {
                            const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                            const unsigned long long x = a.sortk[i], y = a.sortk[l];
                            if ((i & k) == 0 ? x < y : x > y) a.sortk[i] = y, a.sortk[l] = x;   // descending overall
                        }
                        __syncthreads();
                    }
                int32_t pre = 0;   // children of the candidates in front of the running group, split or not
                for (int c0 = 0; c0 < T; c0 += 1024) {   // (the candidates are the first entries; the rest are 0)
                    const int w = c0 + tid;
                    const unsigned long long key = w < T ? a.sortk[w] : 0ull;
                    const int32_t p = (int32_t)(0xffffffffu - (uint32_t)key);
                    int32_t nch = 0;
                    if (key)
                        for (int q = 0; q < 4; q++) nch += a.cnt4[4 * p + q] > 0 ? 1 : 0;
                    int32_t tot;
                    const int32_t ex = pre + fast_scan1024(nch, s_wtot, lane, wave, tot);
                    // the list's length in front of this split: T + children so far - parents so far.  It never
                    // shrinks along the walk (a candidate has at least one child): the splits are a prefix of it
                    const bool sp = key != 0 && T + ex - w < N;
                    if (sp) a.cbase[p] = ex, a.split[p] = 1;
                    int32_t tc, ts;
                    (void)fast_scan1024(sp ? nch : 0, s_wtot, lane, wave, tc);
                    (void)fast_scan1024(sp ? 1 : 0, s_wtot, lane, wave, ts);
                    pre += tot, C += tc, nsplit += ts;
                }
            }
            __syncthreads();
            const int32_t Tn = C + (T - nsplit);
            // never, by the bound in include/pagk.h and by the depth of the tree (a node of more than one key is wider
            // than a pixel: at most 16 halvings of 32767): nothing is written past a buffer, nothing runs without end
            if (Tn > a.out_bound || passes > 64) {
                bad = true;
                break;
            }
            // the new list: children to the front in reverse creation order, the others behind in their order
            int4 *nbox = a.box[cur ^ 1];
            int32_t *nncnt = a.ncnt[cur ^ 1], *nncand = a.ncand[cur ^ 1];
            int32_t rem = 0;
            for (int c0 = 0; c0 < T; c0 += 1024) {
                const int p = c0 + tid;
                const bool in = p < T, sp = in && a.split[p] != 0;
                int32_t tot;
                const int32_t r = rem + fast_scan1024(in && !sp ? 1 : 0, s_wtot, lane, wave, tot);
                if (sp) {
                    int32_t c = a.cbase[p];
                    for (int q = 0; q < 4; q++) {
                        const int32_t cnt = a.cnt4[4 * p + q];
                        if (cnt > 0) {
                            const int32_t np = C - 1 - c;
                            nbox[np] = fast_child_box(box[p], q);
                            nncnt[np] = cnt;
                            nncand[np] = cnt > 1 ? 1 : 0;
                            if (cnt > 1) atomicAdd(&s_nexp, 1);
                            c++;
                        }
                    }
                } else if (in) {
                    const int32_t np = C + r;
                    nbox[np] = box[p];
                    nncnt[np] = a.ncnt[cur][p];
                    nncand[np] = 0;
                    a.cbase[p] = np;
                }
                rem += tot;
            }
            __syncthreads();
            for (int k = tid; k < n; k += 1024) {
                const int32_t p = a.knode[k];
                int32_t np = a.cbase[p];
                if (a.split[p]) {
                    const int q = fast_quadrant(box[p], a.kxy[k]);
                    for (int qq = 0; qq < q; qq++) np += a.cnt4[4 * p + qq] > 0 ? 1 : 0;
                    np = C - 1 - np;
                }
                a.knode[k] = np;
            }
            __syncthreads();
            const int32_t n_expand = s_nexp;
            __syncthreads();
            T = Tn;
            cur ^= 1;
            if (T >= N || T == prev) fin = true;                  // :693, :758
            else if (!phase2 && T + 3 * n_expand > N) phase2 = true;   // :697
        }
    }
    // the best key of every node (:768-784): the largest response, the first of the raw list on a tie
    if (bad) T = 0;
    for (int i = tid; i < T; i += 1024) a.best[i] = 0ull;
    __syncthreads();
    if (!bad)
        for (int k = tid; k < n; k += 1024)
            atomicMax(&a.best[a.knode[k]], ((unsigned long long)(uint32_t)a.kscore[k] << 32) | (0xffffffffu - (uint32_t)k));
    __syncthreads();
    // minBorder added (:866-867), the mask test (:1199-1203), list order kept
    int32_t nout = 0;
    for (int c0 = 0; c0 < T; c0 += 1024) {
        const int p = c0 + tid;
        bool ok = false;
        int x = 0, y = 0, sc = 0;
        if (p < T) {
            const unsigned long long key = a.best[p];
            const uint32_t k = 0xffffffffu - (uint32_t)key, xy = a.kxy[k];
            x = (int)(xy & 0xffffu) + kFastBorder, y = (int)(xy >> 16) + kFastBorder, sc = (int)(key >> 32);
            ok = !a.mask || a.mask[(int64_t)y * a.g.W + x] != 0;
        }
        int32_t tot;
        const int32_t o = nout + fast_scan1024(ok ? 1 : 0, s_wtot, lane, wave, tot);
        if (ok && o < a.cap) {
            a.out_xy[2 * o] = (float)x, a.out_xy[2 * o + 1] = (float)y;
            if (a.out_resp) a.out_resp[o] = (float)sc;
        }
        nout += tot;
    }
    nout = nout < a.cap ? nout : a.cap;
    for (int i = tid; i < a.cap; i += 1024)
        if (i >= nout) {
            a.out_xy[2 * i] = a.out_xy[2 * i + 1] = 0.0f;
            if (a.out_resp) a.out_resp[i] = 0.0f;
        }
    if (tid == 0) {
        a.info[0] = nout;
        a.info[1] = n;
        a.info[2] = skip ? 0 : a.ctl[kFastCtlFirstEmpty];
        a.info[3] = skip ? 0 : a.ctl[kFastCtlEmpty];
        a.info[4] = T;
        a.info[5] = passes;
        a.info[6] = 0;
        a.info[7] = bad ? -1 : 0;
    }
}

__global__ void __launch_bounds__(1024) k_fast_tree(FastTreeArgs a) { fast_tree_body(a); }

}  // namespace pagk
