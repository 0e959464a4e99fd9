// superplus_amd/csrc/dfk_closures_kernels.h -- CloseGap2's closures (dfk_closures.h) on the device (gfx950, wave64): the consensus of
// the two stacks of a pair merged at an offset.  A workgroup takes a TILE of 256 merged columns of a closure, a lane a column; the
// live rows of stack 0, then those of stack 1, are walked once in order with their headers staged through LDS 256 at a time, and a
// lane whose column the row covers loads the 2-bit base and the quality byte and adds one double.  No MFMA: byte loads and dependent
// double adds.  The dimensions, the live rows and the decode are dfk_cons_kernels.h's own kernels, launched by dfk_cons.inc's shared
// steps.
//
// The merged width, the two column maps, the cell, the sums and the (sum, id) maximum are the headers' own functions, which the CPU
// test runs too.  A column's four sums live in one lane from the first row of stack 0 to the last of stack 1: nothing is reduced
// across rows or stacks, nothing is contracted (adds only, and the build has no fast-math flag).
//
// No atomic takes part.  A live row that had a defined cell in some column gets the flag 1 (every writer writes 1, from LDS first,
// then one store a row and tile); the counts of a tile are a tree over the lanes (integers) written at the tile's own place.
#pragma once
#include "dfk_cons_kernels.h"
#include "dfk_closures.h"

namespace dfk {

// the closures [0, n) of a batch; stacks are numbered within the range: pair p of the range has stacks 2 p and 2 p + 1
struct CsBatch {
    uint64_t n;
    const uint32_t* cl_pair;           // [n] the closure's pair, relative to the range
    const int32_t* cl_off;             // [n]
    const uint64_t* out_first;         // [n + 1] where a closure's columns start in `out`
    uint64_t q0;                       // the range's first stack among the closable pairs' stacks
    const long long* M; const int32_t* side_ne; const uint8_t* side_rev;      // M per stack of the range; ne and reversed per stack
    const uint64_t* live_first;        // [range stacks + 1] into the range's live rows
    const int32_t* l_pos; const uint32_t* l_len;                              // the range's live rows
    const uint32_t* l_slot;            // [the batch's live rows] the read's slot in the batch; live row l of the range is l - live0 here
    uint64_t live0;
    const uint64_t* b_at; const uint64_t* q_at;                               // [slots + 1] where a slot's bases and qualities start
    const uint8_t* bases; const uint8_t* quals;
};

__global__ void __launch_bounds__(256)
k_cs_closures(CsBatch B, uint8_t* __restrict__ out, uint32_t* __restrict__ defined /* [the range's live rows] 1: had a defined cell */,
              unsigned long long* __restrict__ cells /* [n * TILES] defined cells added */, uint32_t* __restrict__ empty /* [n * TILES] columns nothing was added to */)
{
    __shared__ int32_t h_pos[dfk_closures::GROUP];
    __shared__ uint32_t h_len[dfk_closures::GROUP];
    __shared__ uint64_t h_b[dfk_closures::GROUP], h_q[dfk_closures::GROUP];
    __shared__ uint32_t h_def[dfk_closures::GROUP];
    __shared__ unsigned long long red[dfk_closures::GROUP];
    const uint32_t t = threadIdx.x;
    for (uint64_t item = blockIdx.x; item < B.n * dfk_closures::TILES; item += gridDim.x) {
        const uint64_t k = item / dfk_closures::TILES, tile = item % dfk_closures::TILES;
        const uint64_t s0 = 2 * (uint64_t)B.cl_pair[k];
        const long long off = B.cl_off[k];
        const long long M0 = B.M[s0], M1 = B.M[s0 + 1], w00 = dfk_cons::window_start(M0), w01 = dfk_cons::window_start(M1);
        const long long cols0 = M0 - w00, cols1 = M1 - w01, C = dfk_closures::merged_cols(cols0, cols1, off);
        if ((long long)(tile * dfk_closures::GROUP) >= C) {                  // (the whole workgroup: no column of the closure lies here)
            if (t == 0) { cells[item] = 0; empty[item] = 0; }
            continue;
        }
        const long long c = (long long)(tile * dfk_closures::GROUP + t);
        const bool has = c < C;
        double sum[4] = {0., 0., 0., 0.};
        unsigned long long my_cells = 0;
        for (int side = 0; side < 2; ++side) {                               // stack 0's rows, then stack 1's: one run of sums
            const uint64_t s = s0 + side;
            const long long w0 = side ? w01 : w00, cols = side ? cols1 : cols0;
            const int32_t ne = B.side_ne[B.q0 + s];
            const bool rev = B.side_rev[B.q0 + s] != 0;
            const long long x = has ? dfk_closures::column_of_side(side, cols, off, c) : -1;
            const bool covers = x >= 0;
            const long long sc = dfk_cons::stack_column(w0, cols, rev, covers ? x : 0);
            const uint64_t l0 = B.live_first[s], l1 = B.live_first[s + 1];
            for (uint64_t c0 = l0; c0 < l1; c0 += dfk_closures::GROUP) {
                const uint32_t n = (uint32_t)(l1 - c0 < dfk_closures::GROUP ? l1 - c0 : dfk_closures::GROUP);
                __syncthreads();                                             // the chunk before is done with
                if (t < n) {
                    const uint32_t slot = B.l_slot[c0 + t - B.live0];
                    h_pos[t] = B.l_pos[c0 + t]; h_len[t] = B.l_len[c0 + t]; h_b[t] = B.b_at[slot]; h_q[t] = B.q_at[slot]; h_def[t] = 0;
                }
                __syncthreads();
                if (covers)
                    for (uint32_t r = 0; r < n; ++r) {                       // the rows in order: the header is the same for every lane
                        const uint32_t len = h_len[r] & 0x7FFFFFFFu;
                        if (dfk_cons::add_row(sum, (h_len[r] >> 31) != 0, h_pos[r], len, ne, rev, sc, B.bases + h_b[r], B.quals + h_q[r])) { h_def[r] = 1; ++my_cells; }   // (every writer writes 1)
                    }
                __syncthreads();
                if (t < n && h_def[t]) defined[c0 + t] = 1;
            }
        }
        if (has) out[B.out_first[k] + (uint64_t)c] = (uint8_t)dfk_closures::last_max(sum);
        // the tile's two counts: a tree over the lanes (integers)
        __syncthreads();
        red[t] = my_cells; h_def[t] = has && my_cells == 0 ? 1u : 0u;
        __syncthreads();
        for (uint32_t d = dfk_closures::GROUP / 2; d >= 1; d >>= 1) { if (t < d) { red[t] += red[t + d]; h_def[t] += h_def[t + d]; } __syncthreads(); }
        if (t == 0) { cells[item] = red[0]; empty[item] = h_def[0]; }
        __syncthreads();                                                     // (the next item's staging writes h_def)
    }
}

} // namespace dfk
