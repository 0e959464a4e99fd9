// superplus_amd/csrc/dfk_subset_kernels.h -- the subset of interest (dfk_subset.h) on the device (gfx950, wave64): memory-bound
// sweeps and compactions over the pather's batches.  No LDS tables, no MFMA.
//
// A batch is addressed as k_pidx_count addresses it: read i's element is the words [elem_off[i] / 4, elem_off[i + 1] / 4) of
// `var` (var_bytes / 4 for the last), two header words {offset, lastSkip} and then the path's edges.  The kernels keep the
// path kernels' shape, a thread per read: an element is 8 bytes and 4 per edge (13 bytes a read on average), so the 64 reads of
// a wave lie in about a kilobyte of consecutive addresses and every cache line fetched is used whole; lanes over words would
// buy coalescing the loads have already and cost a search for the word's read.
//
// Nothing that reaches a file depends on the order in which atomics arrive: the marks are ORed bits (every writer stores the
// same value), the counters are integer sums, and every place in an output comes from an exclusive scan.
#pragma once
#include "dfk_check_kernels.h"
#include "dfk_subset.h"

namespace dfk {

// ---- marks: pairs -> in_pairs (RunStages.cc:213-219)
__global__ void __launch_bounds__(256)
k_sub_mark(const int32_t* __restrict__ pairs, uint64_t n_words /* 2 per pair */, const int32_t* __restrict__ inv, uint32_t* __restrict__ marks)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_words; i += (uint64_t)gridDim.x * 256) {
        const uint32_t e = (uint32_t)pairs[i], o = (uint32_t)inv[e];
        atomicOr(&marks[e / dfk_subset::MARK_WORD_BITS], 1u << (e % dfk_subset::MARK_WORD_BITS));
        atomicOr(&marks[o / dfk_subset::MARK_WORD_BITS], 1u << (o % dfk_subset::MARK_WORD_BITS));
    }
}
// the scan's input: 1 per marked edge, and 0 behind the last
__global__ void __launch_bounds__(256)
k_sub_flags(const uint32_t* __restrict__ marks, uint64_t n_edges, uint64_t* __restrict__ flags /* [n_edges + 1] */)
{
    for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e <= n_edges; e += (uint64_t)gridDim.x * 256)
        flags[e] = e < n_edges && dfk_subset::marked(marks, (uint32_t)e) ? 1u : 0u;
}
// eoi = the compaction (:222-226); rank_of as 32-bit words for the sort's keys
__global__ void __launch_bounds__(256)
k_sub_eoi(const uint32_t* __restrict__ marks, const uint64_t* __restrict__ rank /* exclusive scan of flags */, uint64_t n_edges,
          uint64_t* __restrict__ eoi, uint32_t* __restrict__ rank_of)
{
    for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < n_edges; e += (uint64_t)gridDim.x * 256) {
        rank_of[e] = (uint32_t)rank[e];
        if (dfk_subset::marked(marks, (uint32_t)e)) eoi[rank[e]] = e;
    }
}

// ---- the hit sweep (:228-240): hit[r] = any marked edge on read r's path, by the whole set's read number
__global__ void __launch_bounds__(256)
k_sub_hit(const uint32_t* __restrict__ var, const uint32_t* __restrict__ elem_off, uint64_t nb, uint64_t r0, uint64_t var_bytes,
          const uint32_t* __restrict__ marks, uint8_t* __restrict__ hit)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nb; i += (uint64_t)gridDim.x * 256) {
        const uint64_t w0 = elem_off[i] >> 2, w1 = (i + 1 < nb ? (uint64_t)elem_off[i + 1] : var_bytes) >> 2;
        bool h = false;
        for (uint64_t w = w0 + 2; w < w1; ++w) h |= dfk_subset::marked(marks, var[w]);
        hit[r0 + i] = h ? 1 : 0;
    }
}
// the fold per pair, after every batch (mates can sit in different batches): a bit per pair, a wave's ballot a word; how many
// are taken, and how many through one read only
__global__ void __launch_bounds__(256)
k_sub_fold(const uint8_t* __restrict__ hit, uint64_t n_pairs, unsigned long long* __restrict__ bits /* [pair_words(n_pairs)] */,
           unsigned long long* __restrict__ ctr /* [0] pairs taken, [1] through one read only */)
{
    const int lane = threadIdx.x & 63;
    uint64_t taken = 0, one = 0;
    // (base is the same for the 64 lanes of a wave and a multiple of 64: the ballot below is one word of the bit set)
    for (uint64_t base = (uint64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); base < n_pairs; base += (uint64_t)gridDim.x * 256) {
        const uint64_t p = base + lane;
        bool a = false, b = false;
        if (p < n_pairs) { a = hit[2 * p] != 0; b = hit[2 * p + 1] != 0; }
        const bool t = dfk_subset::pair_taken(a, b);
        const unsigned long long word = __ballot(t);
        if (lane == 0) bits[base / dfk_subset::PAIR_WORD_BITS] = word;
        taken += t; one += a != b;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { taken += __shfl_down(taken, d, 64); one += __shfl_down(one, d, 64); }
    if (lane == 0 && (taken | one)) { atomicAdd(&ctr[0], taken); atomicAdd(&ctr[1], one); }
}

// ---- ids and paths gather of one batch: the words of the scan (dfk_subset::gather_word), then every taken element to its place
__global__ void __launch_bounds__(256)
k_sub_sizes(const uint32_t* __restrict__ elem_off, uint64_t nb, uint64_t r0, uint64_t var_bytes, const unsigned long long* __restrict__ bits,
            uint64_t* __restrict__ words /* [nb + 1] */)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i <= nb; i += (uint64_t)gridDim.x * 256) {
        uint64_t s = 0;
        if (i < nb && dfk_subset::pair_bit(bits, (r0 + i) >> 1)) {
            const uint64_t b0 = elem_off[i], b1 = i + 1 < nb ? (uint64_t)elem_off[i + 1] : var_bytes;
            s = dfk_subset::gather_word(b1 - b0);
        }
        words[i] = s;
    }
}
// ids_out: the batch's taken read ids; off_out (or null): their elements' absolute offsets in a.sub.paths, the batch's data
// starting at file_off0; var_out (or null): the elements themselves.  The relative order is kept by construction.
__global__ void __launch_bounds__(256)
k_sub_gather(const uint32_t* __restrict__ var, const uint32_t* __restrict__ elem_off, uint64_t nb, uint64_t r0, uint64_t var_bytes,
             const unsigned long long* __restrict__ bits, const uint64_t* __restrict__ place /* exclusive scan of words */, uint64_t file_off0,
             uint64_t* __restrict__ ids_out, uint64_t* __restrict__ off_out, uint32_t* __restrict__ var_out)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nb; i += (uint64_t)gridDim.x * 256) {
        if (!dfk_subset::pair_bit(bits, (r0 + i) >> 1)) continue;
        const uint64_t k = dfk_subset::gather_rank(place[i]), b = dfk_subset::gather_byte(place[i]);
        ids_out[k] = r0 + i;
        if (off_out) off_out[k] = file_off0 + b;
        if (var_out) {
            const uint64_t w0 = elem_off[i] >> 2, w1 = (i + 1 < nb ? (uint64_t)elem_off[i + 1] : var_bytes) >> 2;
            uint32_t* out = var_out + (b >> 2);
            for (uint64_t w = w0; w < w1; ++w) out[w - w0] = var[w];
        }
    }
}

// ---- the index subset: entries per rank (integer sums), then -- a range of ranks [k0, k1) at a time -- k_pidx_range_count /
// k_pidx_range_pairs with "edge in [e0, e1)" replaced by "marked and rank in [k0, k1)"
__global__ void __launch_bounds__(256)
k_sub_rank_count(const uint32_t* __restrict__ var, const uint32_t* __restrict__ elem_off, uint64_t nb, uint64_t var_bytes,
                 const uint32_t* __restrict__ marks, const uint32_t* __restrict__ rank_of, unsigned long long* __restrict__ counts /* [n_eoi] */)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nb; i += (uint64_t)gridDim.x * 256) {
        const uint64_t w0 = elem_off[i] >> 2, w1 = (i + 1 < nb ? (uint64_t)elem_off[i + 1] : var_bytes) >> 2;
        for (uint64_t w = w0 + 2; w < w1; ++w) { const uint32_t e = var[w]; if (dfk_subset::marked(marks, e)) atomicAdd(&counts[rank_of[e]], 1ull); }
    }
}
__global__ void __launch_bounds__(256)
k_sub_range_count(const uint32_t* __restrict__ var, const uint32_t* __restrict__ elem_off, uint64_t nb, uint64_t var_bytes,
                  const uint32_t* __restrict__ marks, const uint32_t* __restrict__ rank_of, uint32_t k0, uint32_t k1, uint64_t* __restrict__ n_in /* [nb + 1] */)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i <= nb; i += (uint64_t)gridDim.x * 256) {
        uint64_t n = 0;
        if (i < nb) {
            const uint64_t w0 = elem_off[i] >> 2, w1 = (i + 1 < nb ? (uint64_t)elem_off[i + 1] : var_bytes) >> 2;
            for (uint64_t w = w0 + 2; w < w1; ++w) {
                const uint32_t e = var[w];
                if (dfk_subset::marked(marks, e)) { const uint32_t k = rank_of[e]; n += k >= k0 && k < k1; }
            }
        }
        n_in[i] = n;
    }
}
__global__ void __launch_bounds__(256)
k_sub_range_pairs(const uint32_t* __restrict__ var, const uint32_t* __restrict__ elem_off, uint64_t nb, uint64_t r0, uint64_t var_bytes,
                  const uint32_t* __restrict__ marks, const uint32_t* __restrict__ rank_of, uint32_t k0, uint32_t k1,
                  const uint64_t* __restrict__ at_of /* exclusive scan of n_in */, uint64_t pair_base, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nb; i += (uint64_t)gridDim.x * 256) {
        const uint64_t w0 = elem_off[i] >> 2, w1 = (i + 1 < nb ? (uint64_t)elem_off[i + 1] : var_bytes) >> 2;
        uint64_t at = pair_base + at_of[i];
        for (uint64_t w = w0 + 2; w < w1; ++w) {
            const uint32_t e = var[w];
            if (!dfk_subset::marked(marks, e)) continue;
            const uint32_t k = rank_of[e];
            if (k >= k0 && k < k1) { keys[at] = k - k0; vals[at] = (uint32_t)(r0 + i); ++at; }
        }
    }
}

} // namespace dfk
