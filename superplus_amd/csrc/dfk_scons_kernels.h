// superplus_amd/csrc/dfk_scons_kernels.h -- Stackster's stack consensus (dfk_scons.h) on the device (gfx950, wave64): Consensus1 with
// qualities of a stack (a workgroup a TILE of 256 columns, a lane a column), the MIN_FLAT pass (a lane a column of the range), the
// conflicting columns per offset (a workgroup a pair, a lane an offset index).  No MFMA: byte loads, dependent double adds, integer
// counts.  The decode and the lowering of a batch's reads are dfk_cons_kernels.h's k_cn_decode and dfk_walks_kernels.h's k_wk_lower.
//
// The cell, the sums, top_two, the rounding, the cap, the recount, the flat test and the conflict test are the header's own functions,
// which the CPU test runs too.  A column's four sums and four counts live in one lane from the first live row to the last: nothing is
// reduced across rows, nothing is contracted (adds only, and the build has no fast-math flag).
//
// No atomic takes part.  A live row that had a defined cell in some column gets the flag 1 (every writer writes 1, from LDS first,
// then one store a row and tile); the counts of a tile or a block are a tree over the lanes (integers) written at their own place.
// Every index stays inside its table: a column below the stack's cols, a row inside [live_first[s], live_first[s + 1]), a cell inside
// its read (cell_index), an offset index below n1 + n2 <= 800.
#pragma once
#include "dfk_walks_kernels.h"
#include "dfk_scons.h"

namespace dfk {

// the stacks [b0, b0 + n) of a range in one batch; stack s of the range is side s & 1 of its pair
struct ScBatch {
    uint64_t b0, n;
    const int32_t* M;                  // [range stacks]
    const uint64_t* out_first;         // [range stacks + 1] where a stack's columns start in con / conq
    const uint64_t* live_first;        // [range stacks + 1] into the range's live rows
    const int32_t* l_start; const uint32_t* l_len;                            // the range's live rows: start, len | rc << 31
    const uint32_t* l_slot;            // [the batch's live rows] the read's slot in the batch; live row l of the range is l - live0 here
    uint64_t live0;
    const uint64_t* b_at; const uint64_t* q_at;                               // [slots + 1] where a slot's bases and qualities start
    const uint8_t* bases; const uint8_t* quals;                               // quals: decoded and lowered
};
constexpr uint32_t SC_COUNTS = 3;      // per tile: defined cells added, columns capped at 100, columns the recount zeroed

__global__ void __launch_bounds__(256)
k_sc_consensus(ScBatch B, uint8_t* __restrict__ con, uint8_t* __restrict__ conq, uint32_t* __restrict__ defined /* [the range's live rows] 1: had a defined cell */,
               unsigned long long* __restrict__ counts /* [n * TILES * SC_COUNTS] */)
{
    __shared__ int32_t h_start[dfk_scons::GROUP];
    __shared__ uint32_t h_len[dfk_scons::GROUP];
    __shared__ uint64_t h_b[dfk_scons::GROUP], h_q[dfk_scons::GROUP];
    __shared__ uint32_t h_def[dfk_scons::GROUP];
    __shared__ unsigned long long red[SC_COUNTS][dfk_scons::GROUP];
    const uint32_t t = threadIdx.x;
    for (uint64_t item = blockIdx.x; item < B.n * dfk_scons::TILES; item += gridDim.x) {
        const uint64_t s = B.b0 + item / dfk_scons::TILES, tile = item % dfk_scons::TILES;
        const long long M = B.M[s], w0 = dfk_scons::window_start(M), cols = M - w0;
        if ((long long)(tile * dfk_scons::GROUP) >= cols) {                  // (the whole workgroup: no column of the stack lies here)
            if (t < SC_COUNTS) counts[item * SC_COUNTS + t] = 0;
            continue;
        }
        const long long c = (long long)(tile * dfk_scons::GROUP + t);
        const bool has = c < cols, rev = (s & 1) != 0;
        const long long sc = dfk_scons::stack_column(w0, cols, rev, has ? c : 0);
        double sum[4] = {0., 0., 0., 0.};
        uint32_t bad[4] = {0, 0, 0, 0};
        unsigned long long my_cells = 0;
        const uint64_t l0 = B.live_first[s], l1 = B.live_first[s + 1];
        for (uint64_t c0 = l0; c0 < l1; c0 += dfk_scons::GROUP) {
            const uint32_t n = (uint32_t)(l1 - c0 < dfk_scons::GROUP ? l1 - c0 : dfk_scons::GROUP);
            __syncthreads();                                                 // the chunk before is done with
            if (t < n) {
                const uint32_t slot = B.l_slot[c0 + t - B.live0];
                h_start[t] = B.l_start[c0 + t]; h_len[t] = B.l_len[c0 + t]; h_b[t] = B.b_at[slot]; h_q[t] = B.q_at[slot]; h_def[t] = 0;
            }
            __syncthreads();
            if (has)
                for (uint32_t r = 0; r < n; ++r)                             // the rows in order: the header is the same for every lane
                    if (dfk_scons::add_row(sum, bad, h_start[r], h_len[r] & 0x7FFFFFFFu, (h_len[r] >> 31) != 0, rev, sc, B.bases + h_b[r], B.quals + h_q[r])) { h_def[r] = 1; ++my_cells; }   // (every writer writes 1)
            __syncthreads();
            if (t < n && h_def[t]) defined[c0 + t] = 1;
        }
        dfk_scons::Conq k{0, false, false};
        if (has) {
            const dfk_scons::TopTwo tt = dfk_scons::top_two(sum);
            k = dfk_scons::conq_of(tt, bad);
            con[B.out_first[s] + (uint64_t)c] = (uint8_t)tt.id0; conq[B.out_first[s] + (uint64_t)c] = k.conq;
        }
        // the tile's counts: a tree over the lanes (integers)
        __syncthreads();
        red[0][t] = my_cells; red[1][t] = k.capped ? 1u : 0u; red[2][t] = k.recount ? 1u : 0u;
        __syncthreads();
        for (uint32_t d = dfk_scons::GROUP / 2; d >= 1; d >>= 1) {
            if (t < d) { red[0][t] += red[0][t + d]; red[1][t] += red[1][t + d]; red[2][t] += red[2][t + d]; }
            __syncthreads();
        }
        if (t < SC_COUNTS) counts[item * SC_COUNTS + t] = red[t][0];
        __syncthreads();                                                     // (the next item writes red and the staging arrays)
    }
}

// ---- the flat pass: column g of the range's n_cols columns; in place -- a lane reads con alone and writes its own conq
__global__ void __launch_bounds__(256)
k_sc_flat(const uint8_t* __restrict__ con, const uint64_t* __restrict__ out_first, uint64_t n_stacks, uint64_t n_cols, uint8_t* __restrict__ conq, unsigned long long* __restrict__ flat /* [gridDim.x] */)
{
    __shared__ unsigned long long red[256];
    const uint32_t t = threadIdx.x;
    unsigned long long mine = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * 256 + t; g < n_cols; g += (uint64_t)gridDim.x * 256) {
        const uint64_t s = dfk_cons::owner_of(out_first, n_stacks, g), o = out_first[s];       // (empty stacks before: owner_of takes the last that starts at or before g)
        if (dfk_scons::flat_at(con + o, (long long)(out_first[s + 1] - o), (long long)(g - o))) { conq[g] = 0; ++mine; }
    }
    red[t] = mine;
    __syncthreads();
    for (uint32_t d = 128; d >= 1; d >>= 1) { if (t < d) red[t] += red[t + d]; __syncthreads(); }
    if (t == 0) flat[blockIdx.x] = red[0];
}

// ---- the conflicts: pair p of the range's n_pairs; its two stacks' con and conq in LDS; offset index k = offset + n2 a lane
__global__ void __launch_bounds__(256)
k_sc_conflicts(const uint8_t* __restrict__ con, const uint8_t* __restrict__ conq, const uint64_t* __restrict__ out_first, const uint64_t* __restrict__ cnt_first /* [n_pairs + 1] */, uint64_t n_pairs,
               uint16_t* __restrict__ counts)
{
    __shared__ uint8_t s_con[2][dfk_scons::MAX_WIDTH], s_q[2][dfk_scons::MAX_WIDTH];
    const uint32_t t = threadIdx.x;
    for (uint64_t p = blockIdx.x; p < n_pairs; p += gridDim.x) {
        const uint64_t k0 = cnt_first[p], nk = cnt_first[p + 1] - k0;
        if (!nk) continue;                                                   // (the whole workgroup: the pair does not yield)
        const uint64_t o1 = out_first[2 * p], o2 = out_first[2 * p + 1];
        const long long n1 = (long long)(o2 - o1), n2 = (long long)(out_first[2 * p + 2] - o2);
        if (n1 > dfk_scons::MAX_WIDTH || n2 > dfk_scons::MAX_WIDTH || (long long)nk != n1 + n2) continue;      // (the host refuses such tables before the launch)
        __syncthreads();                                                     // the pair before is done with
        for (uint32_t i = t; i < (uint32_t)n1; i += 256) { s_con[0][i] = con[o1 + i]; s_q[0][i] = conq[o1 + i]; }
        for (uint32_t i = t; i < (uint32_t)n2; i += 256) { s_con[1][i] = con[o2 + i]; s_q[1][i] = conq[o2 + i]; }
        __syncthreads();
        for (uint64_t k = t; k < nk; k += 256)
            counts[k0 + k] = (uint16_t)dfk_scons::conflicts_at(s_con[0], s_q[0], n1, s_con[1], s_q[1], n2, (long long)k - n2);
    }
}

} // namespace dfk
