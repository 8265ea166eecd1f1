// pagk_results_kernel.h -- the output half of the sequence (include/pagk.h: "The result ring of a sequence").  The last launch
// of a frame packs everything pagk_sequence_read, pagk_sequence_read_pair and pagk_sequence_read_velocity deliver, and a
// persistent track id and age per row, into ONE record in device memory; behind the step one asynchronous copy puts that
// record into a pinned host block.  The reference hands over mvPtIndexInLastFrame only (src/frame.cpp:135,192): the chain of
// ids is a function of index_in_last and the live count, which the device holds, so the device carries it.
//
// The record: 15 parts, each on a multiple of 256 bytes (results_layout below is the one definition, host and device):
//   header | state | info | keys | keys_un | keys_normal | index_in_last | live | track_id | age | velocity |
//   status | pt_predict | pt_predict_un | err
//
// A workgroup of 1024 owns a chunk of 1024 rows (one round of the ballot scan of pagk_handover_kernel.h) and a grid-stride share
// of the copies.  No workgroup waits for another: each counts the new rows in front of its chunk itself (ballots over the
// index array, a few KB), the ids and next_id are read from the OTHER parity's arrays, and the last workgroup -- whose prefix
// plus own total is the frame's n_new -- writes the header and this parity's next_id.  There is no early exit at all.
// The frame number and the time stamp come from the fixed input block (spare bytes of the n_cand part, written by the host
// with the frame): kernel arguments are frozen in a replayed graph.
// Plain HIP C++, vector stores only; no scratch; LDS: the scan's 16 words.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pagk_group_kernel.h"

namespace pagk {

constexpr int kResultsParts = 15;
enum ResultsPart {
    RES_HEADER, RES_STATE, RES_INFO, RES_KEYS, RES_KEYS_UN, RES_KEYS_NORMAL, RES_INDEX, RES_LIVE, RES_TRACK_ID, RES_AGE,
    RES_VELOCITY, RES_STATUS, RES_PT_PREDICT, RES_PT_PREDICT_UN, RES_ERR
};
constexpr int kResultsFrameOff = 8, kResultsTimeOff = 16;   // in the n_cand part of the input block: int32 frame, f64 t

// bytes per row of each part (0: a fixed part of 256 bytes)
__host__ __device__ inline int64_t results_row_bytes(int part)
{
    switch (part) {
        case RES_HEADER: case RES_STATE: case RES_INFO: return 0;
        case RES_LIVE: case RES_STATUS: return 1;
        case RES_INDEX: case RES_AGE: case RES_ERR: return 4;
        default: return 8;
    }
}

// off[part], off[kResultsParts] = the record's size
__host__ __device__ inline void results_layout(int64_t cap, int64_t *off)
{
    int64_t total = 0;
    for (int k = 0; k < kResultsParts; k++) {
        off[k] = total;
        const int64_t row = results_row_bytes(k);
        total += row ? (cap * row + 255) / 256 * 256 : 256;
    }
    off[kResultsParts] = total;
}

struct ResultsHeader {   // the first 32 bytes of the header part
    int32_t frame, cap, n_live, n_new;
    int64_t next_id;
    double t;
};

struct ResultsArgs {
    const uint8_t *words;        // the n_cand part of the input block
    const int32_t *state, *info;
    const float *keys, *keys_un, *keys_normal;
    const int32_t *index_in_last;
    const uint8_t *live;
    const float *velocity;       // NULL: zeros (a plain sequence, or flow_velocity = 0)
    const uint8_t *status;
    const float *pt_predict, *pt_predict_un, *err;
    const int64_t *id_last;      // the other parity's
    const int32_t *age_last;
    const int64_t *next_last;
    int64_t *id_cur, *next_cur;
    int32_t *age_cur;
    uint8_t *rec;
    int32_t cap, sensor;
};

// `bytes` from src (NULL: zeros) to dst, both on 16-byte boundaries: 16-byte units, then the tail by bytes
__device__ __forceinline__ void results_copy(uint8_t *dst, const void *src, int64_t bytes, int64_t gtid, int64_t gsize)
{
    const int64_t units = bytes >> 4;
    const uint4 *s = static_cast<const uint4 *>(src);
    uint4 *d = reinterpret_cast<uint4 *>(dst);
    for (int64_t u = gtid; u < units; u += gsize) d[u] = s ? s[u] : make_uint4(0u, 0u, 0u, 0u);
    const int64_t done = units << 4;
    if (gtid < bytes - done) dst[done + gtid] = s ? static_cast<const uint8_t *>(src)[done + gtid] : (uint8_t)0;
}

__device__ __forceinline__ void results_pack_body(const ResultsArgs &a)
{
    __shared__ int32_t wtot[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t cap = a.cap;
    const int64_t gtid = (int64_t)blockIdx.x * 1024 + tid, gsize = (int64_t)gridDim.x * 1024;
    int64_t off[kResultsParts + 1];
    results_layout(cap, off);
    const int32_t n_state = a.state[0];
    const int64_t n_live = n_state < 0 ? 0 : (n_state > cap ? cap : n_state);
    // the new rows in front of this chunk, in row order
    const int64_t c0 = (int64_t)blockIdx.x * 1024;
    int32_t mine = 0;   // (the same in every lane of a wave)
    for (int64_t b = 0; b < c0; b += 1024) {
        const int64_t j = b + tid;
        mine += __popcll(__ballot(j < n_live && a.index_in_last[j] < 0));
    }
    const int64_t i = c0 + tid;
    const int32_t idx = i < cap ? a.index_in_last[i] : 0;
    const bool fresh = i < n_live && idx < 0;
    const unsigned long long bal = __ballot(fresh);
    if (lane == 0) wtot[wave] = mine;
    // (what the scan does not need: the copies, in front of its barriers)
    results_copy(a.rec + off[RES_STATE], a.state, 32, gtid, gsize);
    results_copy(a.rec + off[RES_INFO], a.info, 32, gtid, gsize);
    results_copy(a.rec + off[RES_KEYS], a.keys, cap * 8, gtid, gsize);
    results_copy(a.rec + off[RES_KEYS_UN], a.keys_un, cap * 8, gtid, gsize);
    results_copy(a.rec + off[RES_KEYS_NORMAL], a.keys_normal, cap * 8, gtid, gsize);
    results_copy(a.rec + off[RES_INDEX], a.index_in_last, cap * 4, gtid, gsize);
    results_copy(a.rec + off[RES_LIVE], a.live, cap, gtid, gsize);
    results_copy(a.rec + off[RES_VELOCITY], a.velocity, cap * 8, gtid, gsize);
    results_copy(a.rec + off[RES_STATUS], a.status, cap, gtid, gsize);
    results_copy(a.rec + off[RES_PT_PREDICT], a.pt_predict, cap * 8, gtid, gsize);
    results_copy(a.rec + off[RES_PT_PREDICT_UN], a.pt_predict_un, cap * 8, gtid, gsize);
    results_copy(a.rec + off[RES_ERR], a.err, cap * 4, gtid, gsize);
    __syncthreads();
    int32_t front = 0;   // every wave saw 64 of every 1024 rows in front of the chunk
    for (int w = 0; w < 16; w++) front += wtot[w];
    __syncthreads();
    if (lane == 0) wtot[wave] = __popcll(bal);
    __syncthreads();
    int32_t before = front, total = front;   // new rows in front of this wave's rows; up to the end of this chunk
    for (int w = 0; w < 16; w++) {
        before += w < wave ? wtot[w] : 0;
        total += wtot[w];
    }
    const int64_t next = a.next_last[0];
    if (i < cap) {
        int64_t id = -1;
        int32_t age = 0;
        if (i < n_live) {
            if (idx >= 0) {
                const int64_t from = idx < cap ? idx : cap - 1;
                id = a.id_last[from], age = a.age_last[from] + 1;
            } else {
                id = next + before + __popcll(bal & ((1ull << lane) - 1ull));
            }
        }
        a.id_cur[i] = id, a.age_cur[i] = age;
        reinterpret_cast<int64_t *>(a.rec + off[RES_TRACK_ID])[i] = id;
        reinterpret_cast<int32_t *>(a.rec + off[RES_AGE])[i] = age;
    }
    if (blockIdx.x == gridDim.x - 1 && tid == 0) {
        ResultsHeader h;
        h.frame = *reinterpret_cast<const int32_t *>(a.words + kResultsFrameOff);
        h.cap = a.cap, h.n_live = n_state, h.n_new = total;
        h.next_id = next + total;
        h.t = a.sensor ? *reinterpret_cast<const double *>(a.words + kResultsTimeOff) : 0.0;
        *reinterpret_cast<ResultsHeader *>(a.rec + off[RES_HEADER]) = h;
        a.next_cur[0] = h.next_id;
    }
}

__global__ void __launch_bounds__(1024) k_results_pack(ResultsArgs a) { results_pack_body(a); }

// k cameras at once (the sequence group): the camera is blockIdx.y, its record comes from a third table the lead owns
__global__ void __launch_bounds__(1024) k_group_results_pack(const ResultsArgs *__restrict__ table)
{
    ResultsArgs a = group_global(table)[blockIdx.y];
#define PAGK_RESULTS_GLOBAL(x) a.x = group_global(a.x)
    PAGK_RESULTS_GLOBAL(words), PAGK_RESULTS_GLOBAL(state), PAGK_RESULTS_GLOBAL(info), PAGK_RESULTS_GLOBAL(keys);
    PAGK_RESULTS_GLOBAL(keys_un), PAGK_RESULTS_GLOBAL(keys_normal), PAGK_RESULTS_GLOBAL(index_in_last), PAGK_RESULTS_GLOBAL(live);
    PAGK_RESULTS_GLOBAL(velocity), PAGK_RESULTS_GLOBAL(status), PAGK_RESULTS_GLOBAL(pt_predict), PAGK_RESULTS_GLOBAL(pt_predict_un);
    PAGK_RESULTS_GLOBAL(err), PAGK_RESULTS_GLOBAL(id_last), PAGK_RESULTS_GLOBAL(age_last), PAGK_RESULTS_GLOBAL(next_last);
    PAGK_RESULTS_GLOBAL(id_cur), PAGK_RESULTS_GLOBAL(next_cur), PAGK_RESULTS_GLOBAL(age_cur), PAGK_RESULTS_GLOBAL(rec);
#undef PAGK_RESULTS_GLOBAL
    results_pack_body(a);
}

}  // namespace pagk
