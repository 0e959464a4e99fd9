// superplus_amd/csrc/dfk_offsets_kernels.h -- GetOffsets1 (dfk_offsets.h) on the device (gfx950, wave64): the candidate offsets of a
// batch of pairs (a workgroup a pair, the 8-mers of both sequences in LDS, a bitmap of offsets), their emission at scanned places, the
// bits test (a workgroup a candidate: mismatch ballots, prefix sums from popcounts into LDS, bad windows, a lane a start and its mirror
// gathering the table), the compaction of those that pass.  No MFMA: LDS words, popcounts and dependent gathers of doubles from a
// 1.29-MB table that stays in L2.
//
// The 8-mer packing, the bitmap place of an offset, the mismatch bit, bad_window from prefix sums, a start's last n, Min and the bits
// are the header's own functions, which the CPU test runs too.  The table is built on the host; no logarithm is taken here.  The
// minimum is Min( a, b ) = b < a ? b : a over values none of which is a NaN: the same in any order.  bits is one negation, one
// multiplication and one division of IEEE doubles (nothing to contract; the build has no fast-math flag).
//
// The LDS bit-or that sets an offset's bit is the only atomic, and order-free.  Every place comes from an exclusive scan.
#pragma once
#include "dfk_offsets.h"

namespace dfk {

// the batch's sequences: element q = 2 * pair + side at bases[first[q] - first[0] ..)
struct OfBatch {
    const uint64_t* first;            // [2 * n + 1], absolute; the batch's bases start at first[0]
    const uint8_t* bases;
    uint64_t n;                       // pairs
};
struct OfCand { int32_t offset, overlap, mismatch; uint32_t lookups; double bits; };      // 24 bytes

// ---- candidates: a workgroup a pair
__global__ void __launch_bounds__(256)
k_of_candidates(OfBatch B, uint32_t* __restrict__ bitmaps /* [n][BITMAP_WORDS] */, uint64_t* __restrict__ counts /* [n + 1], 0 behind the last */)
{
    using namespace dfk_offsets;
    __shared__ uint16_t km1[MAX_N], km2[MAX_N];
    __shared__ uint32_t bm[BITMAP_WORDS];
    const uint32_t t = threadIdx.x;
    for (uint64_t p = blockIdx.x; p <= B.n; p += gridDim.x) {
        if (p == B.n) { if (t == 0) counts[p] = 0; continue; }
        const uint8_t* con1 = B.bases + (B.first[2 * p] - B.first[0]);
        const uint8_t* con2 = B.bases + (B.first[2 * p + 1] - B.first[0]);
        const int n1 = (int)(B.first[2 * p + 1] - B.first[2 * p]), n2 = (int)(B.first[2 * p + 2] - B.first[2 * p + 1]);
        const int m1 = n1 - MIN_STRETCH + 1, m2 = n2 - MIN_STRETCH + 1;                  // 8-mers of each; <= MAX_N - 7
        __syncthreads();                                                                 // the pair before is done with
        if (t < BITMAP_WORDS) bm[t] = 0;
        for (int j = (int)t; j < m1; j += 256) km1[j] = pack8(con1 + j);
        for (int j = (int)t; j < m2; j += 256) km2[j] = pack8(con2 + j);
        __syncthreads();
        for (int j1 = (int)t; j1 < m1; j1 += 256) {
            const uint16_t x = km1[j1];
            for (int j2 = 0; j2 < m2; ++j2)
                if (km2[j2] == x) { const uint32_t bit = cand_bit(j1, j2, n2); atomicOr(&bm[bit >> 5], 1u << (bit & 31u)); }     // bit <= n1 + n2 - 9 < 800
        }
        __syncthreads();
        if (t < BITMAP_WORDS) bitmaps[p * BITMAP_WORDS + t] = bm[t];
        if (t == 0) {
            uint32_t c = 0;
            for (uint32_t w = 0; w < BITMAP_WORDS; ++w) c += (uint32_t)__popc(bm[w]);
            counts[p] = c;
        }
    }
}

// ---- the candidates at their places, ascending: a thread a pair
__global__ void __launch_bounds__(256)
k_of_emit(OfBatch B, const uint32_t* __restrict__ bitmaps, const uint64_t* __restrict__ place /* exclusive scan of counts */, uint32_t* __restrict__ c_pair, int32_t* __restrict__ c_off)
{
    using namespace dfk_offsets;
    for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < B.n; p += (uint64_t)gridDim.x * 256) {
        const int n2 = (int)(B.first[2 * p + 2] - B.first[2 * p + 1]);
        uint64_t at = place[p];
        for (uint32_t w = 0; w < BITMAP_WORDS; ++w) {
            uint32_t x = bitmaps[p * BITMAP_WORDS + w];
            while (x) {
                const uint32_t b = (uint32_t)__ffs((int)x) - 1u;
                x &= x - 1u;
                c_pair[at] = (uint32_t)p; c_off[at] = cand_offset(32 * w + b, n2); ++at;
            }
        }
    }
}

// prefix sums read off ballots: the set bits in front of position i
struct OfSums {
    const uint64_t* mask; const uint16_t* before;                                        // [8] ballots; [8] set bits in front of each word
    __device__ __forceinline__ int operator[](int i) const { return (int)before[i >> 6] + __popcll(mask[i >> 6] & ((1ull << (i & 63)) - 1ull)); }
};
// the first set bit at or behind position i among `words` ballots, or -1
__device__ __forceinline__ int of_next_set(const uint64_t* mask, int i, int words)
{
    int w = i >> 6;
    uint64_t x = mask[w] & ~((1ull << (i & 63)) - 1ull);
    while (!x) { if (++w >= words) return -1; x = mask[w]; }
    return 64 * w + (int)__ffsll((long long)x) - 1;
}

// ---- the bits test: a workgroup a candidate
__global__ void __launch_bounds__(256)
k_of_bits(OfBatch B, const uint32_t* __restrict__ c_pair, const int32_t* __restrict__ c_off, uint64_t n_cand, const double* __restrict__ T /* [T_DIM][T_DIM] */,
          OfCand* __restrict__ out, uint64_t* __restrict__ flags /* [n_cand + 1], 0 behind the last */)
{
    using namespace dfk_offsets;
    constexpr int WORDS = 8;                                                             // 512 positions in two rounds of 256 lanes
    __shared__ uint64_t mm[WORDS], bw[WORDS];
    __shared__ uint16_t mm_before[WORDS], S[2 * GROUP];                                  // S[i]: the mismatches in front of overlap position i
    __shared__ double red_min[4];
    __shared__ uint32_t red_n[4];
    const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63u;
    for (uint64_t ci = blockIdx.x; ci <= n_cand; ci += gridDim.x) {
        if (ci == n_cand) { if (t == 0) flags[ci] = 0; continue; }
        const uint64_t p = c_pair[ci];
        const uint8_t* con1 = B.bases + (B.first[2 * p] - B.first[0]);
        const uint8_t* con2 = B.bases + (B.first[2 * p + 1] - B.first[0]);
        const int n1 = (int)(B.first[2 * p + 1] - B.first[2 * p]), n2 = (int)(B.first[2 * p + 2] - B.first[2 * p + 1]);
        const int o = c_off[ci], pos1 = pos1_of(o), pos2 = pos2_of(o), overlap = overlap_of(o, n1, n2);     // 8 <= overlap <= MAX_N
        __syncthreads();                                                                 // the candidate before is done with
        // the mismatch bits of the overlap as ballots
        for (int r = 0; r < 2; ++r) {
            const int i = (int)t + 256 * r;
            const uint64_t b = __ballot(i < overlap && mismatch_at(con1, con2, pos1, pos2, i));
            if (lane == 0) mm[wave + 4 * r] = b;
        }
        __syncthreads();
        if (t == 0) { uint32_t s = 0; for (int w = 0; w < WORDS; ++w) { mm_before[w] = (uint16_t)s; s += (uint32_t)__popcll(mm[w]); } }
        __syncthreads();
        {
            const OfSums from_ballots{mm, mm_before};
            for (int i = (int)t; i <= overlap; i += 256) S[i] = (uint16_t)from_ballots[i];
        }
        __syncthreads();
        // bad_window: index bad_index(m) for every bad m <= overlap - 40; the indices 0 and m - 40 (m > 40) are distinct, and index 0
        // collects m = 0..40
        for (int r = 0; r < 2; ++r) {
            const int i = (int)t + 256 * r;                                              // the index; m = i + 40 for i > 0
            bool bad = false;
            if (i == 0) { for (int m = 0; m <= WX && m <= overlap - WX; ++m) bad = bad || window_is_bad(S, m); }
            else if (i + WX <= overlap - WX) bad = window_is_bad(S, i + WX);
            const uint64_t b = __ballot(bad);
            if (lane == 0) bw[wave + 4 * r] = b;
        }
        __syncthreads();
        // a lane a start, and the start mirrored from 511
        double minp = 0.;
        uint32_t looked = 0;
        for (int r = 0; r < 2; ++r) {
            const int start = r ? 2 * (int)GROUP - 1 - (int)t : (int)t;
            if (start >= overlap) continue;
            const int last = last_n(start, overlap, of_next_set(bw, start, WORDS)), s0 = (int)S[start];
            for (int n = W; n <= last; ++n) minp = min_of(minp, T[n * T_DIM + ((int)S[start + n] - s0)]);
            if (last >= W) looked += (uint32_t)(last - W + 1);
        }
        for (int d = 32; d >= 1; d >>= 1) { minp = min_of(minp, __shfl_xor(minp, d, 64)); looked += __shfl_xor(looked, d, 64); }
        if (lane == 0) { red_min[wave] = minp; red_n[wave] = looked; }
        __syncthreads();
        if (t == 0) {
            const double m = min_of(min_of(red_min[0], red_min[1]), min_of(red_min[2], red_min[3]));
            const double bits = bits_of(m);
            out[ci] = OfCand{o, overlap, (int32_t)S[overlap], red_n[0] + red_n[1] + red_n[2] + red_n[3], bits};
            flags[ci] = bits >= MIN_BITS ? 1u : 0u;
        }
    }
}

// ---- those that passed at their places, the order kept
__global__ void __launch_bounds__(256)
k_of_compact(OfBatch B, const OfCand* __restrict__ cand, const uint32_t* __restrict__ c_pair, const uint64_t* __restrict__ flags, const uint64_t* __restrict__ place, uint64_t n_cand,
             dfk_offsets::Rec* __restrict__ recs, uint32_t* __restrict__ rec_pair)
{
    for (uint64_t ci = (uint64_t)blockIdx.x * 256 + threadIdx.x; ci < n_cand; ci += (uint64_t)gridDim.x * 256) {
        if (!flags[ci]) continue;
        const OfCand c = cand[ci];
        const uint64_t p = c_pair[ci];
        const int n2 = (int)(B.first[2 * p + 2] - B.first[2 * p + 1]);
        recs[place[ci]] = dfk_offsets::Rec{c.offset, c.overlap, c.offset + n2, c.mismatch, c.bits, 0u, 0u};
        rec_pair[place[ci]] = (uint32_t)p;
    }
}

} // namespace dfk
