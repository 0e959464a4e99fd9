// superplus_amd/csrc/dfk_translate_kernels.h -- the read paths moved onto the patched graph (gfx950, wave64).  The rule, the bound and
// the plan: dfk_translate.h.  Three kernels a batch of paths, each a 256-lane workgroup over units of 256 reads (dfk_translate::UNIT):
//   k_tp_decide    a lane a read: its record {new offset, new edge or -1}, the unit's word count, the flagged reads' numbers
//   k_tp_override  the records of the reads the host settled, and what their units' word counts gain
//   k_tp_emit      behind the scan over the units' word counts: the new var image and elem_off, the digest, Validate's count
// No global atomic but the wave-aggregated append of flagged reads; the counters go through ballots to lane-uniform registers, one LDS
// word a wave and one slot row a workgroup (TP_SLOTS words, added to by that workgroup alone: the launches follow each other on one
// stream), which the host adds up.
#pragma once
#include "dfk_check_kernels.h"
#include "dfk_translate.h"

namespace dfk {

enum { TP_PLACED_BEFORE = 0, TP_STEP2 = 1, TP_WALK = 2, TP_CLEARED_EMPTY = 3, TP_FLAGGED = 4, TP_EDGE_CHANGED = 5, TP_OFFSET_CHANGED = 6, TP_BAD = 7,
       TP_N_DECIDE = 8, TP_INVALID = 8, TP_SUM = 9, TP_XOR = 10, TP_SLOTS = 16 };

struct TpTables {
    const uint64_t* to3_first; const int32_t* to3; const int32_t* left3; const int32_t* kmers3;
    uint32_t n_edges, n_edges3; int32_t K;
};

__global__ void __launch_bounds__(256)
k_tp_decide(const uint32_t* __restrict__ var, const uint32_t* __restrict__ elem_off, uint64_t nb, uint64_t var_bytes, TpTables T,
            int2* __restrict__ records /* [nb] */, uint64_t* __restrict__ words /* [n_units + 1] */, uint32_t* __restrict__ flagged /* [nb] */,
            unsigned int* __restrict__ n_flagged, unsigned long long* __restrict__ slots /* [gridDim.x][TP_SLOTS] */)
{
    __shared__ uint32_t wave_words[4];
    __shared__ uint64_t part[TP_N_DECIDE][4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t below = (1ull << lane) - 1;
    uint64_t acc[TP_N_DECIDE];                                         // the same in every lane of a wave
#pragma unroll
    for (int k = 0; k < TP_N_DECIDE; ++k) acc[k] = 0;
    const uint64_t n_units = (nb + dfk_translate::UNIT - 1) / dfk_translate::UNIT;
    for (uint64_t u = blockIdx.x; u < n_units; u += gridDim.x) {
        const uint64_t i = u * dfk_translate::UNIT + threadIdx.x;
        const bool live = i < nb;
        int32_t off = 0, edge = -1;
        bool before = false, step2 = false, walked = false, no_to3 = false, flag = false, bad = false, edge_ch = false, off_ch = false;
        if (live) {
            const uint64_t w0 = elem_off[i] >> 2, w1 = (i + 1 < nb ? (uint64_t)elem_off[i + 1] : var_bytes) >> 2;
            off = (int32_t)var[w0];
            if (w1 - w0 > 2) {
                before = true;
                const uint32_t e0 = var[w0 + 2];
                if (e0 >= T.n_edges) bad = true;                       // (the host has checked every id: counted, never followed)
                else {
                    const uint64_t t0 = T.to3_first[e0], t1 = T.to3_first[e0 + 1];
                    if (t1 == t0) no_to3 = true;
                    else {
                        const int32_t start = dfk_translate::start_of(off, T.left3[e0]);
                        const int32_t id0 = T.to3[t0];
                        if (dfk_translate::first_edge_takes(start, T.kmers3[id0], T.K)) { step2 = true; edge = id0; off_ch = start != off; off = start; }
                        else {
                            const dfk_translate::Walk w = dfk_translate::walk_first(T.to3 + t0, t1 - t0, T.kmers3, T.K, start);
                            if (w.edge < 0) flag = true;
                            else { walked = true; edge = w.edge; off_ch = w.offset != off; off = w.offset; }
                        }
                    }
                    edge_ch = !flag && (uint32_t)edge != e0;           // (a cleared read's edge has changed: it has none)
                }
            }
            records[i] = make_int2(off, edge);
        }
        const uint64_t m_live = __ballot(live), m_placed = __ballot(live && edge >= 0), m_flag = __ballot(flag);
        acc[TP_PLACED_BEFORE] += __popcll(__ballot(before)); acc[TP_STEP2] += __popcll(__ballot(step2)); acc[TP_WALK] += __popcll(__ballot(walked));
        acc[TP_CLEARED_EMPTY] += __popcll(__ballot(no_to3)); acc[TP_FLAGGED] += __popcll(m_flag); acc[TP_EDGE_CHANGED] += __popcll(__ballot(edge_ch));
        acc[TP_OFFSET_CHANGED] += __popcll(__ballot(off_ch)); acc[TP_BAD] += __popcll(__ballot(bad));
        if (m_flag) {                                                  // wave-uniform: one add a wave, the lanes' places by their rank in the mask
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(n_flagged, (unsigned int)__popcll(m_flag));
            base = (uint32_t)__shfl((int)base, 0, 64);
            if (flag) flagged[base + __popcll(m_flag & below)] = (uint32_t)i;
        }
        if (lane == 0) wave_words[wave] = 2u * (uint32_t)__popcll(m_live) + (uint32_t)__popcll(m_placed);
        __syncthreads();
        if (threadIdx.x == 0) words[u] = (uint64_t)wave_words[0] + wave_words[1] + wave_words[2] + wave_words[3];
        __syncthreads();
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) words[n_units] = 0;       // the scan's last word: its output there is the batch's total
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < TP_N_DECIDE; ++k) part[k][wave] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < TP_N_DECIDE) slots[(uint64_t)blockIdx.x * TP_SLOTS + threadIdx.x] += part[threadIdx.x][0] + part[threadIdx.x][1] + part[threadIdx.x][2] + part[threadIdx.x][3];
}

// fixes: {read in the batch, offset, edge or -1, 0}, a read once; gains: {unit, words to add}, a unit once
__global__ void __launch_bounds__(256)
k_tp_override(const int4* __restrict__ fixes, uint32_t n_fixes, const uint2* __restrict__ gains, uint32_t n_gains, int2* __restrict__ records, uint64_t* __restrict__ words)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t < n_fixes) { const int4 f = fixes[t]; records[f.x] = make_int2(f.y, f.z); }
    if (t < n_gains) { const uint2 g = gains[t]; words[g.x] += g.y; }
}

__global__ void __launch_bounds__(256)
k_tp_emit(const int2* __restrict__ records, uint64_t nb, uint64_t r0, const uint64_t* __restrict__ unit_at /* [n_units + 1]: words before a unit */, int64_t n_edges3,
          uint32_t* __restrict__ var, uint32_t* __restrict__ elem_off, unsigned long long* __restrict__ slots)
{
    __shared__ uint32_t stage[3 * dfk_translate::UNIT];
    __shared__ uint32_t wave_words[4];
    __shared__ uint64_t part[3][4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t below = (1ull << lane) - 1;
    uint64_t sum = 0, xr = 0, invalid = 0;
    const uint64_t n_units = (nb + dfk_translate::UNIT - 1) / dfk_translate::UNIT;
    for (uint64_t u = blockIdx.x; u < n_units; u += gridDim.x) {
        const uint64_t i = u * dfk_translate::UNIT + threadIdx.x;
        const bool live = i < nb;
        const int2 rec = live ? records[i] : make_int2(0, -1);
        const bool placed = live && rec.y >= 0;
        const uint64_t m_live = __ballot(live), m_placed = __ballot(placed);
        if (lane == 0) wave_words[wave] = 2u * (uint32_t)__popcll(m_live) + (uint32_t)__popcll(m_placed);
        __syncthreads();
        uint32_t at = 2u * (uint32_t)__popcll(m_live & below) + (uint32_t)__popcll(m_placed & below), total = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4; ++w) { if (w < wave) at += wave_words[w]; total += wave_words[w]; }
        const uint64_t base = unit_at[u];
        if (live) {
            elem_off[i] = (uint32_t)((base + at) * 4);
            stage[at] = (uint32_t)rec.x; stage[at + 1] = 0u;
            if (placed) stage[at + 2] = (uint32_t)rec.y;
            const uint64_t h = dfk_translate::read_digest(r0 + i, rec.x, rec.y);
            sum += h; xr ^= dfk_translate::mix64(h + dfk_translate::DIGEST_XOR);
            invalid += placed && !dfk_translate::valid_id(rec.y, n_edges3);
        }
        __syncthreads();
        // the unit's words go out from LDS: single words up to the first 16-byte boundary of the image, 16 bytes a lane, single words behind
        const uint32_t head = min(total, (uint32_t)((4 - (base & 3)) & 3)), n16 = (total - head) >> 2, tail_at = head + 4 * n16;
        if (threadIdx.x < head) var[base + threadIdx.x] = stage[threadIdx.x];
        if (threadIdx.x < n16) {
            const uint32_t s = head + 4 * threadIdx.x;
            *reinterpret_cast<uint4*>(var + base + s) = make_uint4(stage[s], stage[s + 1], stage[s + 2], stage[s + 3]);
        }
        if (threadIdx.x < total - tail_at) var[base + tail_at + threadIdx.x] = stage[tail_at + threadIdx.x];
        __syncthreads();
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { sum += __shfl_down(sum, d, 64); xr ^= __shfl_down(xr, d, 64); invalid += __shfl_down(invalid, d, 64); }
    if (lane == 0) { part[0][wave] = invalid; part[1][wave] = sum; part[2][wave] = xr; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long* s = slots + (uint64_t)blockIdx.x * TP_SLOTS;
        s[TP_INVALID] += part[0][0] + part[0][1] + part[0][2] + part[0][3];
        s[TP_SUM] += part[1][0] + part[1][1] + part[1][2] + part[1][3];
        s[TP_XOR] ^= part[2][0] ^ part[2][1] ^ part[2][2] ^ part[2][3];
    }
}

} // namespace dfk
