// superplus_amd/csrc/dfk_soffsets_kernels.h -- Stackster's stack offsets (dfk_soffsets.h) on the device (gfx950, wave64): the search (a
// workgroup a pair, a wave a live row of either stack: the row's 8-mers against the other side's acceptable consensus 8-mers, the bits
// of every ( row, offset ) seen, the pair's table of greatest bits and results per offset, its records compacted ascending) and the
// emit (the records at their scanned places).  No MFMA: byte and bit work, dependent gathers from the table of log binomial sums.  The
// decode and the lowering of a batch's reads are dfk_cons_kernels.h's k_cn_decode and dfk_walks_kernels.h's k_wk_lower.
//
// acceptable, the row 8-mer with its all-defined test, offset_of, overlap_of, the mismatch bit, the cell, minp over a start's windows,
// bits_of, passes and kept are the header's own functions, which the CPU test runs too.
//
// The only atomics are LDS ones and order-free: a bit-or into the wave's bitmap of offsets seen, a u64 max and a u32 add into the pair's
// table.  Nothing in HBM is written by more than one lane.  Every index stays inside its table: a column below the stack's cols <= 400
// (the host refuses wider ones before the launch, the kernel skips them), an offset index below n1 + n2 <= 800, an overlap position
// below the overlap, T's row n <= overlap <= 400 and cell k <= n, a record inside the pair's slot of n1 + n2 records.
#pragma once
#include "dfk_scons_kernels.h"
#include "dfk_soffsets.h"

namespace dfk {

// the pairs [p0, p0 + n) of a range in one batch
struct SoBatch {
    uint64_t p0, n;
    const int32_t* M;                  // [range stacks]
    const uint64_t* col_first;         // [range stacks + 1] where a stack's columns start in con
    const uint8_t* con;                // the range's consensus bases
    const uint64_t* cnt_first;         // [range pairs + 1] where a pair's conflict counts start; its slot of records lies there too
    const uint16_t* counts;
    const uint64_t* live_first;        // [range stacks + 1] into the range's live rows
    const int32_t* l_start; const uint32_t* l_len;                            // the range's live rows: start, len | rc << 31
    const uint32_t* l_slot;            // [the batch's live rows] the read's slot in the batch; live row l of the range is l - live0 here
    uint64_t live0;
    const uint64_t* b_at; const uint64_t* q_at;                               // [slots + 1]
    const uint8_t* bases; const uint8_t* quals;                               // quals: decoded and lowered
    const double* T;                   // [T_DIM][T_DIM]
};

__device__ __forceinline__ unsigned long long so_wave_sum(unsigned long long v) { for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64); return v; }

__global__ void __launch_bounds__(256)
k_so_search(SoBatch B, dfk_soffsets::Rec* __restrict__ slots /* at cnt_first[p] - cnt_first[p0] */, uint64_t* __restrict__ n_recs /* [n + 1], 0 behind the last */,
            dfk_soffsets::PairWords* __restrict__ words /* [n] */, unsigned long long* __restrict__ counts /* [n * N_COUNTS] */)
{
    using namespace dfk_soffsets;
    __shared__ uint8_t s_con[2][MAX_WIDTH + MM];
    __shared__ uint16_t s_km[2][MAX_WIDTH];
    __shared__ uint32_t s_allowed[BITMAP_WORDS];
    __shared__ unsigned long long s_max[N_IDX];
    __shared__ uint32_t s_cnt[N_IDX];
    __shared__ uint8_t w_cell[WAVES][MAX_WIDTH + MM];
    __shared__ unsigned long long w_def[WAVES][MASK_WORDS], w_odef[WAVES][MASK_WORDS], w_mis[WAVES][MASK_WORDS];
    __shared__ uint32_t w_bitmap[WAVES][BITMAP_WORDS];
    __shared__ uint16_t w_S[WAVES][MAX_WIDTH + 2];
    __shared__ unsigned long long red[N_COUNTS][WAVES];
    __shared__ uint32_t s_scan[GROUP];
    __shared__ unsigned long long s_best[GROUP];
    const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63u;
    for (uint64_t p = blockIdx.x; p <= B.n; p += gridDim.x) {
        if (p == B.n) { if (t == 0) n_recs[p] = 0; continue; }
        const uint64_t P = B.p0 + p, k0 = B.cnt_first[P], nk = B.cnt_first[P + 1] - k0;
        const uint64_t o1 = B.col_first[2 * P], o2 = B.col_first[2 * P + 1];
        const int n1 = (int)(o2 - o1), n2 = (int)(B.col_first[2 * P + 2] - o2);
        if (!nk || n1 > MAX_WIDTH || n2 > MAX_WIDTH || (long long)nk != (long long)n1 + n2) {     // (the whole workgroup) the pair does not yield; the host refuses the rest before the launch
            if (t == 0) { n_recs[p] = 0; words[p] = PairWords{0, 0, 0, 0}; }
            if (t < N_COUNTS) counts[p * N_COUNTS + t] = 0;
            continue;
        }
        __syncthreads();                                                     // the pair before is done with
        for (uint32_t i = t; i < (uint32_t)MAX_WIDTH + MM; i += GROUP) { s_con[0][i] = i < (uint32_t)n1 ? B.con[o1 + i] : 0; s_con[1][i] = i < (uint32_t)n2 ? B.con[o2 + i] : 0; }
        for (uint32_t i = t; i < N_IDX; i += GROUP) { s_max[i] = 0; s_cnt[i] = 0; }
        if (t < BITMAP_WORDS) {
            uint32_t w = 0;
            for (uint32_t b = 0; b < 32; ++b) { const uint32_t idx = 32 * t + b; if (idx < (uint32_t)nk && B.counts[k0 + idx] < dfk_scons::CONFLICTS) w |= 1u << b; }
            s_allowed[t] = w;
        }
        __syncthreads();
        unsigned long long my[N_COUNTS] = {};
        for (uint32_t i = t; i < 2 * (uint32_t)MAX_WIDTH; i += GROUP) {
            const uint32_t s = i >= (uint32_t)MAX_WIDTH, j = i - s * (uint32_t)MAX_WIDTH;
            const uint16_t km = con_kmer(s_con[s], s ? n2 : n1, (int)j);
            s_km[s][j] = km;
            my[C_ACCEPTABLE] += km != NO_KMER;
        }
        __syncthreads();
        // ---- a wave a live row: the rows of stack t2 are searched with s = 1 - t2
        const uint64_t la = B.live_first[2 * P], lb = B.live_first[2 * P + 1], lc = B.live_first[2 * P + 2];
        for (uint64_t l = la + wave; l < lc; l += WAVES) {
            const int t2 = l >= lb, s = 1 - t2, cols2 = t2 ? n2 : n1, cols1 = s ? n2 : n1;
            const long long M = B.M[2 * P + t2], w0 = dfk_scons::window_start(M);
            const int32_t start = B.l_start[l];
            const uint32_t len = B.l_len[l] & 0x7FFFFFFFu, slot = B.l_slot[l - B.live0];
            const bool rc = (B.l_len[l] >> 31) != 0;
            const uint8_t* pk = B.bases + B.b_at[slot];
            const uint8_t* qq = B.quals + B.q_at[slot];
            wave_sync();                                                     // the row before is done with
            _Pragma("unroll 1")
            for (uint32_t k = 0; k < MASK_WORDS; ++k) {
                const int c = (int)(64 * k + lane);
                uint8_t v = BLANK;
                if (c < cols2) v = cell_of(start, len, rc, t2 == 1, dfk_scons::stack_column(w0, cols2, t2 == 1, c), pk, qq);
                if (c < (int)MAX_WIDTH + MM) w_cell[wave][c] = v & 7u;
                const unsigned long long b = __ballot((v & DEF_BIT) != 0);
                if (lane == 0) w_def[wave][k] = b;
            }
            if (lane < BITMAP_WORDS) w_bitmap[wave][lane] = 0;
            wave_sync();
            for (int l8 = (int)lane; l8 + MM <= cols2; l8 += 64) {
                uint16_t km;
                if (!row_kmer(w_cell[wave], w_def[wave], l8, &km)) continue;
                ++my[C_KMERS];
                if (!acceptable(km)) continue;
                for (int j = 0; j + MM <= cols1; ++j) {
                    if (s_km[s][j] != km) continue;
                    ++my[C_HITS];
                    const uint32_t idx = (uint32_t)(offset_of(s, j, l8) + n2);                  // in [0, n1 + n2): j - l or l - j with both below their cols
                    if (s_allowed[idx >> 5] >> (idx & 31u) & 1u) atomicOr(&w_bitmap[wave][idx >> 5], 1u << (idx & 31u)); else ++my[C_DISALLOWED];
                }
            }
            wave_sync();
            // ---- the offsets this row saw, one after the other
            for (uint32_t bw = 0; bw < BITMAP_WORDS; ++bw) {
                uint32_t word = uniform32(w_bitmap[wave][bw]);               // (the same in every lane)
                while (word) {
                    const uint32_t idx = 32 * bw + (uint32_t)__ffs((int)word) - 1;
                    word &= word - 1;
                    const int offx = offx_of(s, (int)idx - n2), pos1 = pos1_of(offx), pos2 = pos2_of(offx), overlap = overlap_of(offx, cols1, cols2);
                    wave_sync();                                             // the offset before is done with
                    _Pragma("unroll 1")
                    for (uint32_t k = 0; k < MASK_WORDS; ++k) {
                        const int v = (int)(64 * k + lane);
                        const bool in = v < overlap;
                        const unsigned long long bm = __ballot(in && mismatch(s_con[s][pos1 + (in ? v : 0)], w_cell[wave][pos2 + (in ? v : 0)]));
                        const unsigned long long bd = __ballot(in && bit_at(w_def[wave], pos2 + (in ? v : 0)));
                        if (lane == 0) { w_mis[wave][k] = bm; w_odef[wave][k] = bd; }
                    }
                    wave_sync();
                    {
                        uint32_t before = 0;                                 // the mismatches in front of word k, then in front of position v
                        for (uint32_t k = 0; k < MASK_WORDS - 1; ++k) {
                            const int v = (int)(64 * k + lane);
                            const unsigned long long m = w_mis[wave][k];
                            if (v <= overlap) w_S[wave][v] = (uint16_t)(before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)));
                            before += (uint32_t)__popcll(m);
                        }
                    }
                    wave_sync();
                    double minp = 0.;
                    uint32_t looked = 0;
                    for (int st = (int)lane; st < overlap; st += 64) minp = minp_of_start(w_S[wave], w_odef[wave], overlap, st, B.T, minp, &looked);
                    for (int d = 32; d >= 1; d >>= 1) minp = dfk_offsets::min_of(minp, __shfl_xor(minp, d, 64));
                    my[C_LOOKUPS] += looked;
                    const double bits = bits_of(minp);
                    if (lane == 0) {
                        ++my[C_SEEN];
                        if (passes(bits)) {
                            ++my[C_RESULTS];
                            atomicMax(&s_max[idx], (unsigned long long)__double_as_longlong(bits));       // bits >= 20: ordered like its pattern
                            atomicAdd(&s_cnt[idx], 1u);
                        }
                    }
                }
            }
        }
        // ---- the pair's counts: over the lanes by shuffles, over the waves through LDS
        for (uint32_t k = 0; k < N_COUNTS; ++k) { const unsigned long long v = so_wave_sum(my[k]); if (lane == 0) red[k][wave] = v; }
        __syncthreads();                                                     // every row is done: the table stands
        // ---- the records: best by a tree, the table compacted ascending (a thread four offset indices in a row)
        unsigned long long mine_best = 0;
        uint32_t mine = 0;
        for (uint32_t i = 4 * t; i < 4 * t + 4 && i < N_IDX; ++i) if (s_cnt[i]) { ++mine; mine_best = s_max[i] > mine_best ? s_max[i] : mine_best; }
        s_scan[t] = mine; s_best[t] = mine_best;
        __syncthreads();
        for (uint32_t d = 1; d < GROUP; d <<= 1) {                           // inclusive scan of the counts, the maximum beside it
            const uint32_t add = t >= d ? s_scan[t - d] : 0;
            const unsigned long long other = t >= d ? s_best[t - d] : 0;
            __syncthreads();
            s_scan[t] += add; s_best[t] = other > s_best[t] ? other : s_best[t];
            __syncthreads();
        }
        const double best = __longlong_as_double((long long)s_best[GROUP - 1]);
        uint32_t at = s_scan[t] - mine, n_kept = 0;
        Rec* out = slots + (k0 - B.cnt_first[B.p0]);
        for (uint32_t i = 4 * t; i < 4 * t + 4 && i < N_IDX; ++i) {
            if (!s_cnt[i]) continue;
            const double score = __longlong_as_double((long long)s_max[i]);
            const bool k = kept(best, score);
            out[at++] = Rec{(int32_t)i - n2, s_cnt[i], score, k ? KEPT : DROPPED, 0u};           // at < n1 + n2: a record an index with a result
            n_kept += k;
        }
        const uint32_t total = s_scan[GROUP - 1];
        __syncthreads();
        s_scan[t] = n_kept;
        __syncthreads();
        for (uint32_t d = GROUP / 2; d >= 1; d >>= 1) { if (t < d) s_scan[t] += s_scan[t + d]; __syncthreads(); }
        if (t == 0) {
            const uint32_t kk = s_scan[0];
            n_recs[p] = total;
            words[p] = PairWords{(uint32_t)(red[C_SEEN][0] + red[C_SEEN][1] + red[C_SEEN][2] + red[C_SEEN][3]), (uint32_t)(red[C_RESULTS][0] + red[C_RESULTS][1] + red[C_RESULTS][2] + red[C_RESULTS][3]), kk,
                                 closable(kk) ? 1u : 0u};
        }
        if (t < N_COUNTS) counts[p * N_COUNTS + t] = red[t][0] + red[t][1] + red[t][2] + red[t][3];
    }
}

// ---- the records of the batch's pairs at their scanned places: a thread a record of the slots
__global__ void __launch_bounds__(256)
k_so_emit(SoBatch B, const dfk_soffsets::Rec* __restrict__ slots, const uint64_t* __restrict__ n_recs, const uint64_t* __restrict__ place /* [n + 1] */, dfk_soffsets::Rec* __restrict__ recs)
{
    const uint64_t k00 = B.cnt_first[B.p0], n_slots = B.cnt_first[B.p0 + B.n] - k00;
    for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g < n_slots; g += (uint64_t)gridDim.x * 256) {
        const uint64_t p = dfk_cons::owner_of(B.cnt_first + B.p0, B.n, k00 + g), i = k00 + g - B.cnt_first[B.p0 + p];     // (pairs without entries before: owner_of takes the last that starts at or before)
        if (i < n_recs[p]) recs[place[p] + i] = slots[g];
    }
}

} // namespace dfk
