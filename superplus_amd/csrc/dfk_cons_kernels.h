// superplus_amd/csrc/dfk_cons_kernels.h -- CloseGap2's stack consensus (dfk_cons.h) on the device (gfx950, wave64): the dimensions of
// a range of stacks (a wave a stack, a maximum over its rows), the live rows (flag, scan, emit), the decode of a batch's reads (a
// thread a read, the pather's PQVec decoder), the consensus (a workgroup a stack, a lane a column, the live rows walked once in
// order with their headers staged through LDS).  No MFMA: byte loads and dependent double adds.
//
// The cell, the window, the sums and the first maximum are the header's own functions, which the CPU test runs too.  The sums are
// IEEE doubles added in row order by one lane per column: nothing is reduced across rows, nothing is contracted (adds only, and
// the build has no fast-math flag).  A base is loaded as the byte that holds it and a quality as its byte: a read may start at any
// byte and the last of a buffer ends with the allocation.
//
// Nothing that reaches a file depends on the order in which atomics arrive: every place comes from an exclusive scan; the one
// atomic counts the streams that did not decode (an integer, and any value but 0 refuses the call).
#pragma once
#include "dfk_paths_kernels.h"    // decode_quals
#include "dfk_cons.h"

namespace dfk {

// the stacks [q0, q0 + n_stacks): stack s has the rows locs[loc_first[k] ..) of its rank k, then parts[part_first[q ^ 1] ..)
struct CnStacks {
    const uint32_t* side_rank;        // [all stacks]
    const int32_t* side_ne;           // [all stacks] hb.Bases(e)
    const uint64_t* row_first;        // [n_stacks + 1], of this range
    const uint64_t* loc_first; const uint64_t* locs; const uint64_t* part_first; const uint64_t* parts;
    const uint32_t* read_len;
    uint64_t q0, n_stacks, n_items;
};
struct CnRow { uint32_t id, len; int32_t pos; bool fw; };
__device__ __forceinline__ CnRow cn_row(const CnStacks& S, uint64_t s, uint64_t r)
{
    const uint64_t q = S.q0 + s, k = S.side_rank[q], nl = S.loc_first[k + 1] - S.loc_first[k];
    const uint64_t* recs = r < nl ? S.locs : S.parts;
    const uint64_t at = r < nl ? S.loc_first[k] + r : S.part_first[q ^ 1] + (r - nl);
    const uint32_t id = (uint32_t)dfk_cons::rec_id(recs, at);
    return CnRow{id, S.read_len[id], dfk_cons::rec_pos(recs, at), dfk_cons::rec_fw(recs, at)};
}

// ---- dimensions: a wave a stack; M the maximum of row_end over its rows, from 0
__global__ void __launch_bounds__(256)
k_cn_dims(CnStacks S, long long* __restrict__ M /* [n_stacks] */)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t s = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); s < S.n_stacks; s += (uint64_t)gridDim.x * 4) {
        const uint64_t n = S.row_first[s + 1] - S.row_first[s];
        const int32_t ne = S.side_ne[S.q0 + s];
        long long m = 0;
        for (uint64_t r = lane; r < n; r += 64) {
            const CnRow w = cn_row(S, s, r);
            const long long e = dfk_cons::row_end(w.fw, w.pos, w.len, ne);
            m = e > m ? e : m;
        }
        for (int d = 32; d >= 1; d >>= 1) { const long long o = __shfl_xor(m, d, 64); m = o > m ? o : m; }
        if (lane == 0) M[s] = m;
    }
}

// ---- live rows: an item is a row of a stack of the range
__device__ __forceinline__ bool cn_item(const CnStacks& S, const long long* M, uint64_t i, CnRow* w)
{
    const uint64_t s = dfk_cons::owner_of(S.row_first, S.n_stacks, i);
    *w = cn_row(S, s, i - S.row_first[s]);
    return dfk_cons::row_live(w->fw, w->pos, w->len, S.side_ne[S.q0 + s], dfk_cons::window_start(M[s]));
}
__global__ void __launch_bounds__(256)
k_cn_flag(CnStacks S, const long long* __restrict__ M, uint64_t* __restrict__ flags /* [n_items + 1], 0 behind the last */)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i <= S.n_items; i += (uint64_t)gridDim.x * 256) {
        CnRow w;
        flags[i] = i < S.n_items && cn_item(S, M, i, &w) ? 1u : 0u;
    }
}
__global__ void __launch_bounds__(256)
k_cn_emit(CnStacks S, const long long* __restrict__ M, const uint64_t* __restrict__ flags, const uint64_t* __restrict__ place /* exclusive scan of flags */,
          uint32_t* __restrict__ l_id, int32_t* __restrict__ l_pos, uint32_t* __restrict__ l_len /* | fw << 31 */)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < S.n_items; i += (uint64_t)gridDim.x * 256) {
        if (!flags[i]) continue;
        CnRow w;
        (void)cn_item(S, M, i, &w);
        l_id[place[i]] = w.id; l_pos[place[i]] = w.pos; l_len[place[i]] = w.len | (w.fw ? 0x80000000u : 0u);
    }
}
// where every stack's live rows start: the scanned places at the stacks' first rows
__global__ void __launch_bounds__(256)
k_cn_live_first(const uint64_t* __restrict__ row_first, const uint64_t* __restrict__ place, uint64_t n_stacks, uint64_t* __restrict__ live_first /* [n_stacks + 1] */)
{
    for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s <= n_stacks; s += (uint64_t)gridDim.x * 256) live_first[s] = place[row_first[s]];
}

// ---- the decode: a thread a read of the batch
__global__ void __launch_bounds__(256)
k_cn_decode(const uint8_t* __restrict__ pq, const uint64_t* __restrict__ pq_at /* [n + 1] */, const uint64_t* __restrict__ q_at /* [n + 1] */, uint64_t n, uint8_t* __restrict__ quals,
            unsigned long long* __restrict__ bad)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
        if (!decode_quals(pq, pq_at[i], pq_at[i + 1], quals + q_at[i], (uint32_t)(q_at[i + 1] - q_at[i]))) atomicAdd(bad, 1ull);
}

// ---- the consensus: a workgroup a stack of the batch [b0, b0 + n) of the range
struct CnBatch {
    uint64_t b0, n;                    // the batch's stacks, relative to the range
    uint64_t q0;                       // the range's first stack
    const long long* M; const int32_t* side_ne; const uint8_t* side_rev;      // M per stack of the range; ne and reversed per stack
    const uint64_t* live_first;        // [range stacks + 1] into the range's live rows
    const int32_t* l_pos; const uint32_t* l_len;                              // the range's live rows
    const uint32_t* l_slot;            // [the batch's live rows] the read's slot in the batch; live row l of the range is l - live0 here
    uint64_t live0;
    const uint64_t* b_at; const uint64_t* q_at;                               // [slots + 1] where a slot's bases and qualities start
    const uint8_t* bases; const uint8_t* quals;
    const uint64_t* out_first;         // [range stacks + 1] where a stack's columns start in `out`, relative to the batch's first
};
__global__ void __launch_bounds__(256)
k_cn_consensus(CnBatch B, uint8_t* __restrict__ out, uint32_t* __restrict__ kept /* [n] live rows with a defined cell */, unsigned long long* __restrict__ cells /* [n] defined cells added */)
{
    __shared__ int32_t h_pos[dfk_cons::GROUP];
    __shared__ uint32_t h_len[dfk_cons::GROUP];
    __shared__ uint64_t h_b[dfk_cons::GROUP], h_q[dfk_cons::GROUP];
    __shared__ uint32_t h_def[dfk_cons::GROUP];
    __shared__ unsigned long long red[dfk_cons::GROUP];
    const uint32_t t = threadIdx.x;
    for (uint64_t i = blockIdx.x; i < B.n; i += gridDim.x) {
        const uint64_t s = B.b0 + i;
        const long long M = B.M[s], w0 = dfk_cons::window_start(M), cols = M - w0;
        const int32_t ne = B.side_ne[B.q0 + s];
        const bool rev = B.side_rev[B.q0 + s] != 0;
        const uint64_t l0 = B.live_first[s], l1 = B.live_first[s + 1];
        const bool has0 = (long long)t < cols, has1 = (long long)t + dfk_cons::GROUP < cols;
        const long long sc0 = dfk_cons::stack_column(w0, cols, rev, t), sc1 = dfk_cons::stack_column(w0, cols, rev, (long long)t + dfk_cons::GROUP);
        double sum0[4] = {0., 0., 0., 0.}, sum1[4] = {0., 0., 0., 0.};
        uint32_t my_kept = 0;
        unsigned long long my_cells = 0;
        for (uint64_t c0 = l0; c0 < l1; c0 += dfk_cons::GROUP) {
            const uint32_t n = (uint32_t)(l1 - c0 < dfk_cons::GROUP ? l1 - c0 : dfk_cons::GROUP);
            __syncthreads();                                                 // the chunk before is done with
            if (t < n) {
                const uint32_t slot = B.l_slot[c0 + t - B.live0];
                h_pos[t] = B.l_pos[c0 + t]; h_len[t] = B.l_len[c0 + t]; h_b[t] = B.b_at[slot]; h_q[t] = B.q_at[slot]; h_def[t] = 0;
            }
            __syncthreads();
            for (uint32_t r = 0; r < n; ++r) {                               // the rows in order: the header is the same for every lane
                const int32_t pos = h_pos[r];
                const uint32_t len = h_len[r] & 0x7FFFFFFFu;
                const bool fw = (h_len[r] >> 31) != 0;
                const uint8_t* rb = B.bases + h_b[r];
                const uint8_t* rq = B.quals + h_q[r];
                uint32_t d = 0;
                if (has0 && dfk_cons::add_row(sum0, fw, pos, len, ne, rev, sc0, rb, rq)) ++d;
                if (has1 && dfk_cons::add_row(sum1, fw, pos, len, ne, rev, sc1, rb, rq)) ++d;
                if (d) { h_def[r] = 1; my_cells += d; }                      // (every writer writes 1)
            }
            __syncthreads();
            if (t < n && h_def[t]) ++my_kept;
        }
        const uint64_t o = B.out_first[s] - B.out_first[B.b0];
        if (has0) out[o + t] = (uint8_t)dfk_cons::first_max(sum0);
        if (has1) out[o + t + dfk_cons::GROUP] = (uint8_t)dfk_cons::first_max(sum1);
        // the stack's two counts: a tree over the lanes (integers)
        __syncthreads();
        red[t] = my_cells; h_def[t] = my_kept;
        __syncthreads();
        for (uint32_t d = dfk_cons::GROUP / 2; d >= 1; d >>= 1) { if (t < d) { red[t] += red[t + d]; h_def[t] += h_def[t + d]; } __syncthreads(); }
        if (t == 0) { kept[i] = h_def[0]; cells[i] = red[0]; }
    }
}

} // namespace dfk
