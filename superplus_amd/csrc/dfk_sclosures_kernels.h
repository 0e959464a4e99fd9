// superplus_amd/csrc/dfk_sclosures_kernels.h -- Stackster's closures (dfk_sclosures.h) on the device (gfx950, wave64): the consensus of
// the two stacks of a pair trimmed to the edges and merged at a kept offset.  A workgroup takes a TILE of 256 merged columns of a
// closure, a lane a column; the live rows of stack 0, then those of stack 1, are walked once in order with their headers staged through
// LDS 256 at a time, and a lane whose column the row covers loads the 2-bit base and the lowered quality byte and adds one double.  No
// MFMA: byte loads and dependent double adds.  The decode and the lowering of a batch's reads are dfk_cons_kernels.h's k_cn_decode and
// dfk_walks_kernels.h's k_wk_lower.
//
// New over k_cs_closures: a row spans about 100 of up to 792 merged columns, so most ( row, tile ) visits add nothing.  While a chunk is
// staged each staging lane tests its row's span against the stack columns the tile shows (tile_span, row_meets) and leaves the answer in
// LDS; the row loop reads it through readfirstlane, so a row that misses the tile costs the whole workgroup one LDS read and a scalar
// branch.  A side the tile shows nothing of is passed over without staging.  Skipping changes no sum: such a row has no cell there.
//
// The merged width, the two column maps, the tile's span, the cell, the sums and the ( sum, id ) maximum are the headers' own functions,
// which the CPU test runs too.  A column's four sums live in one lane from the first row of stack 0 to the last of stack 1: nothing is
// reduced across rows or stacks, nothing is contracted (adds only, and the build has no fast-math flag).
//
// No atomic takes part.  A ( closure, live row ) that had a defined cell in some merged column gets the flag 1 (every writer writes 1,
// from LDS first, then one store a row and tile); k_scl_rows counts the flags per closure and side with a tree over the lanes.  Every
// index stays inside its table: a merged column below C = offset + n2, a row inside [live_first[s], live_first[s + 1]), its flag inside
// [flag_first[k], flag_first[k + 1]), a cell inside its read (cell_index).
#pragma once
#include "dfk_scons_kernels.h"
#include "dfk_sclosures.h"

namespace dfk {

// the closures [0, n) of a batch; stacks are numbered within the range: closable pair p of the range has stacks 2 p and 2 p + 1
struct SclBatch {
    uint64_t n;
    const uint32_t* cl_pair;           // [n] the closure's pair, relative to the range
    const int32_t* cl_off;             // [n]
    const uint64_t* out_first;         // [n + 1] where a closure's columns start in `out`
    const uint64_t* flag_first;        // [n + 1] where a closure's flags start: one a live row of its pair, stack 0's first
    const int32_t* M;                  // [range stacks]
    const uint64_t* live_first;        // [range stacks + 1] into the range's live rows
    const int32_t* l_start; const uint32_t* l_len;                            // the range's live rows: start, len | rc << 31
    const uint32_t* l_slot;            // [the batch's live rows] the read's slot in the batch; live row l of the range is l - live0 here
    uint64_t live0;
    const uint64_t* b_at; const uint64_t* q_at;                               // [slots + 1] where a slot's bases and qualities start
    const uint8_t* bases; const uint8_t* quals;                               // quals: decoded and lowered
};
constexpr uint32_t SCL_COUNTS = 4;     // per tile: defined cells added, columns nothing was added to, ( row, tile ) visits, visits skipped

__global__ void __launch_bounds__(256)
k_scl_closures(SclBatch B, uint8_t* __restrict__ out, uint32_t* __restrict__ flags /* 1: the closure's live row had a defined cell */, unsigned long long* __restrict__ counts /* [n * TILES * SCL_COUNTS] */)
{
    __shared__ int32_t h_start[dfk_sclosures::GROUP];
    __shared__ uint32_t h_len[dfk_sclosures::GROUP];
    __shared__ uint64_t h_b[dfk_sclosures::GROUP], h_q[dfk_sclosures::GROUP];
    __shared__ uint32_t h_meet[dfk_sclosures::GROUP], h_def[dfk_sclosures::GROUP];
    __shared__ unsigned long long red[dfk_sclosures::GROUP];
    const uint32_t t = threadIdx.x;
    for (uint64_t item = blockIdx.x; item < B.n * dfk_sclosures::TILES; item += gridDim.x) {
        const uint64_t k = item / dfk_sclosures::TILES, tile = item % dfk_sclosures::TILES;
        const uint64_t s0 = 2 * (uint64_t)B.cl_pair[k];
        const long long off = B.cl_off[k];
        const long long M0 = B.M[s0], M1 = B.M[s0 + 1], w00 = dfk_scons::window_start(M0), w01 = dfk_scons::window_start(M1);
        const long long n1 = M0 - w00, n2 = M1 - w01, C = dfk_sclosures::merged_cols(n2, off);
        const long long c0 = (long long)(tile * dfk_sclosures::GROUP);
        if (c0 >= C) {                                                       // (the whole workgroup: no column of the closure lies here)
            if (t < SCL_COUNTS) counts[item * SCL_COUNTS + t] = 0;
            continue;
        }
        const long long c1 = C < c0 + (long long)dfk_sclosures::GROUP ? C : c0 + (long long)dfk_sclosures::GROUP, c = c0 + t;
        const bool has = c < c1;
        const uint64_t f0 = B.flag_first[k], lbase = B.live_first[s0];
        double sum[4] = {0., 0., 0., 0.};
        unsigned long long my_cells = 0, visits = 0, skipped = 0;            // (visits, skipped: the same in every lane)
        for (int side = 0; side < 2; ++side) {                               // stack 0's rows, then stack 1's: one run of sums
            const uint64_t s = s0 + side;
            const long long w0 = side ? w01 : w00, cols = side ? n2 : n1;
            const bool rev = side == 1;
            const uint64_t l0 = B.live_first[s], l1 = B.live_first[s + 1];
            int64_t lo = 0, hi = 0;
            visits += l1 - l0;
            if (!dfk_sclosures::tile_span(side, n1, n2, off, w0, rev, c0, c1, &lo, &hi)) { skipped += l1 - l0; continue; }      // (the whole workgroup: the tile shows nothing of this stack)
            const long long x = has ? dfk_sclosures::column_of_side(side, n1, n2, off, c) : -1;
            const bool covers = x >= 0;
            const long long sc = dfk_scons::stack_column(w0, cols, rev, covers ? x : 0);
            for (uint64_t g0 = l0; g0 < l1; g0 += dfk_sclosures::GROUP) {
                const uint32_t n = (uint32_t)(l1 - g0 < dfk_sclosures::GROUP ? l1 - g0 : dfk_sclosures::GROUP);
                __syncthreads();                                             // the chunk before is done with
                if (t < n) {
                    const uint32_t slot = B.l_slot[g0 + t - B.live0];
                    const int32_t start = B.l_start[g0 + t]; const uint32_t len = B.l_len[g0 + t];
                    h_start[t] = start; h_len[t] = len; h_b[t] = B.b_at[slot]; h_q[t] = B.q_at[slot]; h_def[t] = 0;
                    h_meet[t] = dfk_sclosures::row_meets(start, len & 0x7FFFFFFFu, lo, hi) ? 1u : 0u;
                }
                __syncthreads();
                for (uint32_t r = 0; r < n; ++r) {                           // the rows in order: the header is the same for every lane
                    if (!__builtin_amdgcn_readfirstlane(h_meet[r])) { ++skipped; continue; }      // the row's span misses the tile: it adds nothing
                    if (covers && dfk_sclosures::add_row(sum, h_start[r], h_len[r] & 0x7FFFFFFFu, (h_len[r] >> 31) != 0, rev, sc, B.bases + h_b[r], B.quals + h_q[r])) { h_def[r] = 1; ++my_cells; }   // (every writer writes 1)
                }
                __syncthreads();
                if (t < n && h_def[t]) flags[f0 + (g0 + t - lbase)] = 1;
            }
        }
        if (has) out[B.out_first[k] + (uint64_t)c] = (uint8_t)dfk_closures::last_max(sum);
        // the tile's counts: a tree over the lanes (integers)
        __syncthreads();
        red[t] = my_cells; h_def[t] = has && my_cells == 0 ? 1u : 0u;
        __syncthreads();
        for (uint32_t d = dfk_sclosures::GROUP / 2; d >= 1; d >>= 1) { if (t < d) { red[t] += red[t + d]; h_def[t] += h_def[t + d]; } __syncthreads(); }
        if (t == 0) { counts[item * SCL_COUNTS] = red[0]; counts[item * SCL_COUNTS + 1] = h_def[0]; counts[item * SCL_COUNTS + 2] = visits; counts[item * SCL_COUNTS + 3] = skipped; }
        __syncthreads();                                                     // (the next item's staging writes h_def)
    }
}

// ---- the rows: the flags of closure k counted per side: rows[2 k], rows[2 k + 1]; a workgroup a closure, integers, order-free
__global__ void __launch_bounds__(256)
k_scl_rows(uint64_t n, const uint32_t* __restrict__ cl_pair, const uint64_t* __restrict__ flag_first, const uint64_t* __restrict__ live_first, const uint32_t* __restrict__ flags, uint32_t* __restrict__ rows /* [2 n] */)
{
    __shared__ uint32_t red[2][256];
    const uint32_t t = threadIdx.x;
    for (uint64_t k = blockIdx.x; k < n; k += gridDim.x) {
        const uint64_t s0 = 2 * (uint64_t)cl_pair[k], l0 = live_first[s0], lm = live_first[s0 + 1], l1 = live_first[s0 + 2], f0 = flag_first[k];
        uint32_t a = 0, b = 0;
        for (uint64_t l = l0 + t; l < l1; l += 256) { const uint32_t f = flags[f0 + (l - l0)] != 0 ? 1u : 0u; if (l < lm) a += f; else b += f; }
        __syncthreads();                                                     // the closure before is done with
        red[0][t] = a; red[1][t] = b;
        __syncthreads();
        for (uint32_t d = 128; d >= 1; d >>= 1) { if (t < d) { red[0][t] += red[0][t + d]; red[1][t] += red[1][t + d]; } __syncthreads(); }
        if (t < 2) rows[2 * k + t] = red[t][0];
    }
}

} // namespace dfk
