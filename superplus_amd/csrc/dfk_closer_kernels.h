// superplus_amd/csrc/dfk_closer_kernels.h -- the closers' read sets per edge (dfk_closer.h) on the device (gfx950, wave64):
// memory-bound sweeps over the pather's batches, then sorts and compactions of what they emit.  No LDS tables, no MFMA.
//
// A batch is addressed as k_pidx_count addresses it (see dfk_subset_kernels.h), a thread per read.  Every sweep runs
// dfk_closer::walk_read -- the one statement of what a read contributes, which the CPU test runs too -- with a sink of its own:
// per-rank weights (k_cl_weigh), per-read counts for the scans (k_cl_count), the records at their scanned places (k_cl_emit).
// A read that meets no closer edge costs its path's words and a bit test per edge.
//
// Nothing that reaches a file depends on the order in which atomics arrive: the marks are ORed bits, the weights and the
// per-rank counts are integer sums, and every place in an output comes from an exclusive scan or a stable sort.
#pragma once
#include "dfk_subset_kernels.h"
#include "dfk_closer.h"

namespace dfk {

// ---- marks: pairs -> closer edges {first, inv[second]} (Closomatic.cc:503-504); ranks and ce by k_sub_flags / k_sub_eoi
__global__ void __launch_bounds__(256)
k_cl_mark(const int32_t* __restrict__ pairs, uint64_t n_pairs, const int32_t* __restrict__ inv, uint32_t* __restrict__ marks)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_pairs; i += (uint64_t)gridDim.x * 256) {
        const uint32_t e = (uint32_t)pairs[2 * i], o = (uint32_t)inv[pairs[2 * i + 1]];
        atomicOr(&marks[e / dfk_closer::MARK_WORD_BITS], 1u << (e % dfk_closer::MARK_WORD_BITS));
        atomicOr(&marks[o / dfk_closer::MARK_WORD_BITS], 1u << (o % dfk_closer::MARK_WORD_BITS));
    }
}

struct ClBatch { const uint32_t* var; const uint32_t* elem_off; uint64_t nb, r0, var_bytes; const uint8_t* dup; };

// ---- the weights: per rank what the sweep will emit (locs, prec tuples, set entries), and the counters of the whole
struct ClWeighSink {
    unsigned long long* w;                        // [3 * n_ce]
    uint64_t mates_in = 0, mates_out = 0, dup_skipped = 0;
    __device__ void entry(uint32_t k, uint32_t, bool dup) { if (dup) ++dup_skipped; else atomicAdd(&w[3 * (uint64_t)k + 2], 1ull); }
    __device__ void loc(uint32_t k, uint32_t, int32_t) { atomicAdd(&w[3 * (uint64_t)k], 1ull); }
    __device__ void prec(uint32_t k, int32_t, int32_t) { atomicAdd(&w[3 * (uint64_t)k + 1], 1ull); }
    __device__ void mate(uint32_t k, bool taken) { if (taken) { ++mates_in; atomicAdd(&w[3 * (uint64_t)k + 2], 1ull); } else ++mates_out; }
};
__global__ void __launch_bounds__(256)
k_cl_weigh(ClBatch B, dfk_closer::Tables T, uint32_t n_ce, int32_t K, unsigned long long* __restrict__ w, unsigned long long* __restrict__ ctr /* mates in, out, dup skipped */)
{
    ClWeighSink s; s.w = w;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < B.nb; i += (uint64_t)gridDim.x * 256) {
        const uint64_t w0 = B.elem_off[i] >> 2, w1 = (i + 1 < B.nb ? (uint64_t)B.elem_off[i + 1] : B.var_bytes) >> 2;
        if (w1 > w0 + 2) dfk_closer::walk_read(B.var + w0 + 2, (uint32_t)(w1 - w0 - 2), (int32_t)B.var[w0], B.dup[(B.r0 + i) >> 1] != 0, T, 0u, n_ce, K, s);
    }
    if (s.mates_in) atomicAdd(&ctr[0], (unsigned long long)s.mates_in);
    if (s.mates_out) atomicAdd(&ctr[1], (unsigned long long)s.mates_out);
    if (s.dup_skipped) atomicAdd(&ctr[2], (unsigned long long)s.dup_skipped);
}

// ---- a range of ranks [k0, k1): per read what it emits into each of the three streams (the scans' inputs, 0 behind the last)
struct ClCountSink {
    uint64_t locs = 0, prec_ = 0, entries = 0;
    __device__ void entry(uint32_t, uint32_t, bool dup) { entries += !dup; }
    __device__ void loc(uint32_t, uint32_t, int32_t) { ++locs; }
    __device__ void prec(uint32_t, int32_t, int32_t) { ++prec_; }
    __device__ void mate(uint32_t, bool taken) { entries += taken; }
};
__global__ void __launch_bounds__(256)
k_cl_count(ClBatch B, dfk_closer::Tables T, uint32_t k0, uint32_t k1, int32_t K, uint64_t* __restrict__ n_loc, uint64_t* __restrict__ n_prec, uint64_t* __restrict__ n_ent /* [nb + 1] each */)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i <= B.nb; i += (uint64_t)gridDim.x * 256) {
        ClCountSink s;
        if (i < B.nb) {
            const uint64_t w0 = B.elem_off[i] >> 2, w1 = (i + 1 < B.nb ? (uint64_t)B.elem_off[i + 1] : B.var_bytes) >> 2;
            if (w1 > w0 + 2) dfk_closer::walk_read(B.var + w0 + 2, (uint32_t)(w1 - w0 - 2), (int32_t)B.var[w0], B.dup[(B.r0 + i) >> 1] != 0, T, k0, k1, K, s);
        }
        n_loc[i] = s.locs; n_prec[i] = s.prec_; n_ent[i] = s.entries;
    }
}

// ... and the streams themselves, every read's share at its scanned place, in walk_read's order
struct ClStreams {
    uint32_t* loc_key; uint32_t* loc_seq; uint32_t* loc_id; int32_t* loc_pos;   // loc_seq: the record's own place, the value the sort carries
    uint32_t* prec_k; uint32_t* prec_g; uint32_t* prec_add;
    uint32_t* ent_k; uint32_t* ent_word;
};
struct ClEmitSink {
    ClStreams S; uint32_t k0; uint64_t id, al, ap, ae;
    __device__ void entry(uint32_t k, uint32_t pass, bool dup) { if (!dup) { S.ent_k[ae] = k - k0; S.ent_word[ae] = dfk_closer::read_word(id, pass == 0); ++ae; } }
    __device__ void loc(uint32_t k, uint32_t pass, int32_t pos) { S.loc_key[al] = dfk_closer::loc_key(k - k0, pass); S.loc_seq[al] = (uint32_t)al; S.loc_id[al] = (uint32_t)id; S.loc_pos[al] = pos; ++al; }
    __device__ void prec(uint32_t k, int32_t g, int32_t add) { S.prec_k[ap] = k - k0; S.prec_g[ap] = (uint32_t)g; S.prec_add[ap] = (uint32_t)add; ++ap; }
    __device__ void mate(uint32_t k, bool taken) { if (taken) { S.ent_k[ae] = k - k0; S.ent_word[ae] = dfk_closer::read_word(id ^ 1, false); ++ae; } }
};
__global__ void __launch_bounds__(256)
k_cl_emit(ClBatch B, dfk_closer::Tables T, uint32_t k0, uint32_t k1, int32_t K, const uint64_t* __restrict__ at_loc, const uint64_t* __restrict__ at_prec, const uint64_t* __restrict__ at_ent,
          uint64_t base_loc, uint64_t base_prec, uint64_t base_ent, ClStreams S)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < B.nb; i += (uint64_t)gridDim.x * 256) {
        if (at_loc[i + 1] == at_loc[i] && at_ent[i + 1] == at_ent[i]) continue;      // (no list entry in the range: no tuple either)
        const uint64_t w0 = B.elem_off[i] >> 2, w1 = (i + 1 < B.nb ? (uint64_t)B.elem_off[i + 1] : B.var_bytes) >> 2;
        ClEmitSink s{S, k0, B.r0 + i, base_loc + at_loc[i], base_prec + at_prec[i], base_ent + at_ent[i]};
        dfk_closer::walk_read(B.var + w0 + 2, (uint32_t)(w1 - w0 - 2), (int32_t)B.var[w0], B.dup[(B.r0 + i) >> 1] != 0, T, k0, k1, K, s);
    }
}

// ---- after the sorts
// dst[i] = src[perm[i]]: the next key of a sort by several fields, least significant first, the permutation the value it carries
__global__ void __launch_bounds__(256)
k_cl_gather(const uint32_t* __restrict__ src, const uint32_t* __restrict__ perm, uint64_t n, uint32_t* __restrict__ dst)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) dst[i] = src[perm[i]];
}
__global__ void __launch_bounds__(256)
k_cl_iota(uint32_t* __restrict__ v, uint64_t n)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) v[i] = (uint32_t)i;
}
// the locs records of a range as the file holds them: two 64-bit words a record
__global__ void __launch_bounds__(256)
k_cl_loc_records(const uint32_t* __restrict__ key /* sorted */, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ id, const int32_t* __restrict__ pos, uint64_t n,
                 uint64_t* __restrict__ out /* [2 * n] */)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint32_t p = perm[i];
        out[2 * i] = id[p]; out[2 * i + 1] = dfk_closer::loc_word1(pos[p], (key[i] & 1u) == 0);
    }
}
// 1 where a sorted sequence of (a, b, c) starts a new value (c may be null), 0 behind the last
__global__ void __launch_bounds__(256)
k_cl_heads(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, const uint32_t* __restrict__ c, uint64_t n, uint64_t* __restrict__ flags /* [n + 1] */)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * 256)
        flags[i] = i < n && (i == 0 || a[i] != a[i - 1] || b[i] != b[i - 1] || (c && c[i] != c[i - 1])) ? 1u : 0u;
}
// where each run starts, and the end of the last: heads[run[i]] = i at every head, heads[n_runs] = n
__global__ void __launch_bounds__(256)
k_cl_run_starts(const uint64_t* __restrict__ flags, const uint64_t* __restrict__ run /* exclusive scan of flags */, uint64_t n, uint64_t* __restrict__ heads /* [n_runs + 1] */)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * 256)
        if (i == n || flags[i]) heads[run[i]] = i;
}
// the runs of prec that are anchors (:542), 0 behind the last
__global__ void __launch_bounds__(256)
k_cl_keep(const uint64_t* __restrict__ heads, uint64_t n_runs, uint64_t* __restrict__ keep /* [n_runs + 1] */)
{
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r <= n_runs; r += (uint64_t)gridDim.x * 256)
        keep[r] = r < n_runs && heads[r + 1] - heads[r] >= (uint64_t)dfk_closer::MIN_EDGE_COUNT ? 1u : 0u;
}
__global__ void __launch_bounds__(256)
k_cl_anchors(const uint64_t* __restrict__ heads, const uint64_t* __restrict__ keep, const uint64_t* __restrict__ place /* exclusive scan of keep */, uint64_t n_runs,
             const uint32_t* __restrict__ k, const uint32_t* __restrict__ g, const uint32_t* __restrict__ add, uint32_t* __restrict__ out /* [3 * kept] */,
             unsigned long long* __restrict__ per_rank)
{
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n_runs; r += (uint64_t)gridDim.x * 256) {
        if (!keep[r]) continue;
        const uint64_t h = heads[r], at = place[r];
        out[3 * at] = g[h]; out[3 * at + 1] = add[h]; out[3 * at + 2] = (uint32_t)(heads[r + 1] - h);
        atomicAdd(&per_rank[k[h]], 1ull);
    }
}
// the distinct set entries of a range, widened to the file's records
__global__ void __launch_bounds__(256)
k_cl_reads_out(const uint64_t* __restrict__ flags, const uint64_t* __restrict__ place, const uint32_t* __restrict__ k, const uint32_t* __restrict__ word, uint64_t n,
               uint64_t* __restrict__ out, unsigned long long* __restrict__ per_rank)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        if (!flags[i]) continue;
        out[place[i]] = word[i];
        atomicAdd(&per_rank[k[i]], 1ull);
    }
}

} // namespace dfk
