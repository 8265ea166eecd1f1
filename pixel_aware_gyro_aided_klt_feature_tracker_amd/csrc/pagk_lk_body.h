// pagk_lk_body.h -- the one body of k_lk_track<NPIX> and k_lk_flow<NPIX> (pagk_lk_kernel.h): the statements of a kernel,
// included once in each of them, so that the two cannot drift.  No include guard.  The including kernel provides NPIX, `a`
// (its LkTrackArgs) and PAGK_LK_FLOW: 0 for k_lk_track; 1 for k_lk_flow, which also provides `f`, its LkFlowArgs (the initial
// point, the live mask, the distorted output).
// Why text and not a __device__ function: with the body behind a function boundary (forced inline, the arguments by
// reference or by value, with or without the early exits) the compiler builds k_lk_track with more branches and reloads
// kernel arguments inside the level loop: 310.3 us against 303.8 us for 1000 features at 752 x 480, h = 10 on MI355X.
// Included in the kernel itself, k_lk_track compiles to the instructions it had before k_lk_flow existed.
    __shared__ __attribute__((aligned(16))) uint8_t tiles[4 * lk_tile_bytes(NPIX)];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = blockIdx.x * 4 + wave;   // the wave's feature
    if (k >= a.cap) return;
    const int n = a.n ? min(max(*a.n, 0), a.cap) : a.cap;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.info[0] = n, a.info[3] = a.top;
#if PAGK_LK_FLOW
    const bool skipped = k < n && f.status_in && f.status_in[k] == 0;   // switched off by status_in (uniform over the wave)
    if (k >= n || skipped) {   // rows at or beyond the count, and rows that are not live, are zeroed
#else
    if (k >= n) {   // rows at or beyond the count are zeroed
#endif
        if (lane == 0) {
            a.pt_out[2 * k] = 0.f, a.pt_out[2 * k + 1] = 0.f, a.status[k] = 0, a.err[k] = 0.f;
            if (a.status_raw) a.status_raw[k] = 0;
            if (a.flow) a.flow[2 * k] = 0.f, a.flow[2 * k + 1] = 0.f;
#if PAGK_LK_FLOW
            if (f.pt_out_dist) f.pt_out_dist[2 * k] = 0.f, f.pt_out_dist[2 * k + 1] = 0.f;
            if (skipped) atomicAdd(a.info + 6, 1);
#endif
        }
        return;
    }
    uint8_t *tile = tiles + wave * lk_tile_bytes(NPIX);
    const int win = a.win, npx = win * win, side_i = win + 3, side_j = win + 1;
    const unsigned magic_win = lk_magic(win);
    const float half = (float)(win - 1) * 0.5f;
    const float rx = a.pt_ref[2 * k], ry = a.pt_ref[2 * k + 1];
#if PAGK_LK_FLOW
    float sx = rx, sy = ry;   // where the search starts at the top level
    if (f.pt_init) sx = f.pt_init[2 * k], sy = f.pt_init[2 * k + 1];
#else
    const float sx = rx, sy = ry;
#endif
    int st = 1, lost_eig = 0, lost_range = 0;
    float e = 0.f, nx = 0.f, ny = 0.f;
    int tI[NPIX], tG[NPIX];   // Ival; ix in the low, iy in the high half

    for (int l = a.top; l >= 0; l--) {
        const LkLevel &L = a.lv[l];
        const float sc = __int_as_float((127 - l) << 23);   // 2^-l
        const float px = rx * sc - half, py = ry * sc - half;
        if (l == a.top)
            nx = sx * sc, ny = sy * sc;
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
#if PAGK_LK_FLOW
        if (f.pt_out_dist) {   // :379 distorts every tracked row, whatever its status
            float ox, oy;
            lk_distort_point(f, nx, ny, ox, oy);
            f.pt_out_dist[2 * k] = ox, f.pt_out_dist[2 * k + 1] = oy;
        }
#endif
        if (st) atomicAdd(a.info + 1, 1);
        if (kept) atomicAdd(a.info + 2, 1);
        if (lost_eig) atomicAdd(a.info + 4, 1);
        if (lost_range) atomicAdd(a.info + 5, 1);
    }
