// superplus_amd/csrc/dfk_hops_kernels.h -- FindEdgePairs (10X/Closomatic.cc:17-358) on the device.  The rule is stated in
// dfk_hops.h; host side in dfk_hops.inc.
//
// THE COMBINED INDEX.  Every method works from "the reads on e"; method 3 also needs "the reads on inv[e]".  So a path
// entry g of read id is listed twice: under key g as id << 1, under key inv[g] as id << 1 | 1, and an edge's list then holds
// both kinds (a self-inverse edge holds every read both ways, as the reference's two loops over the same list do).  Lists
// are laid out by a counting sort -- per-key counts, a scan, a cursor per key -- for a RANGE of keys at a time.  The order
// inside a list is whatever the atomics gave: every consumer below is a set (membership, "two distinct ids"), so no result
// depends on it.
//
//   k_hops_count    per-key counts of the combined index
//   k_hops_flags    bit 0: the edge passes the sink test, bit 1: the source test
//   k_hops_scatter  a range's lists
//   k_hops_mates    methods 1 and 2, the gather: (e1, e2 = inv[last edge of the mate's path]) with the read's id into an
//                   open-address table keyed by (e1, e2): the first id is kept with a CAS, a bit is set when a different one
//                   arrives (the manner of a.dup's table) -- "two distinct ids" whatever the order of arrival
//   k_hops_m1       the table's supported (e1, e2) that method 1 takes; marks e1 as served
//   k_hops_m2       ... that method 2 takes for the e1 method 1 left with nothing
//   k_hops_edges    method 3: one wave per edge, X / exts / can / too_easy in LDS, dfk_hops.h's edge_pairs() run by the wave:
//                   uniform control flow, the lanes share every membership test and copy.  An edge whose sets outgrow the
//                   capacities goes on a list for the host's exact route; nothing of it is emitted.
//   k_hops_path_lens / k_hops_path_copy   that route's fetch: the paths of an edge's reads and their mates, gathered
#pragma once
#include "dfk_hops.h"

namespace dfk {

struct HopsBatch { const uint32_t* var; const uint32_t* elem_off; uint64_t r0, n, var_bytes; };

// a read's path wherever its batch is (a mate can sit in another batch): the batches are in read order
struct HopsPaths {
    const HopsBatch* b; uint32_t nb;
    __host__ __device__ int len(uint32_t id, const int32_t** p) const
    {
        uint32_t lo = 0, hi = nb - 1;
        while (lo < hi) { const uint32_t mid = (lo + hi + 1) >> 1; if (b[mid].r0 <= id) lo = mid; else hi = mid - 1; }
        const HopsBatch& B = b[lo];
        const uint64_t i = id - B.r0;
        const uint64_t w0 = B.elem_off[i] >> 2, w1 = (i + 1 < B.n ? (uint64_t)B.elem_off[i + 1] : B.var_bytes) >> 2;
        *p = (const int32_t*)B.var + w0 + 2;                            // (two words of offset and lastSkip in front of the edges)
        return (int)(w1 - w0) - 2;
    }
};

struct HopsBad {                                                          // MarkBads' verdict on a pair, from the per-read sums
    const uint16_t* sums;
    __host__ __device__ bool operator()(uint32_t pair) const { return sums[2ull * pair] > 150u || sums[2ull * pair + 1] > 150u; }
};

struct WaveExec {                                                         // a block of one wave
    static constexpr int lanes = 64;
    __host__ __device__ int lane() const
    {
#if defined(__HIP_DEVICE_COMPILE__)
        return (int)threadIdx.x;
#else
        return 0;
#endif
    }
    __host__ __device__ bool any(bool v) const
    {
#if defined(__HIP_DEVICE_COMPILE__)
        return __any(v ? 1 : 0) != 0;
#else
        return v;
#endif
    }
    __host__ __device__ void sync() const
    {
#if defined(__HIP_DEVICE_COMPILE__)
        __syncthreads();
#endif
    }
};

// counters of a range (unsigned long long each)
enum { HC_OUT = 0, HC_M1, HC_M2, HC_M3, HC_SEARCHED, HC_EXTENDED, HC_HOST, HC_ROUNDS, HC_LARGEST_X, HC_INTERNAL, HC_N };

struct HopsOut {                                                          // (e, f, method) triplets; counted past the capacity, stored below it
    int32_t* out; uint64_t cap; unsigned long long* ctr; int method;
    __host__ __device__ void operator()(int32_t e, int32_t f) const
    {
#if defined(__HIP_DEVICE_COMPILE__)
        const uint64_t at = atomicAdd(&ctr[HC_OUT], 1ull);
        atomicAdd(&ctr[HC_M1 + method - 1], 1ull);
        if (at < cap) { out[3 * at] = e; out[3 * at + 1] = f; out[3 * at + 2] = method; }
#else
        (void)e; (void)f;
#endif
    }
};

__global__ void __launch_bounds__(256)
k_hops_count(const uint32_t* __restrict__ var, const uint32_t* __restrict__ elem_off, uint64_t nb, uint64_t var_bytes, const int32_t* __restrict__ inv,
             unsigned long long* __restrict__ counts /* 64-bit: a hot edge's count cannot wrap before the host looks at it */)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nb; i += (uint64_t)gridDim.x * 256) {
        const uint64_t w0 = elem_off[i] >> 2, w1 = (i + 1 < nb ? (uint64_t)elem_off[i + 1] : var_bytes) >> 2;
        for (uint64_t w = w0 + 2; w < w1; ++w) { const uint32_t g = var[w]; atomicAdd(&counts[g], 1ull); atomicAdd(&counts[inv[g]], 1ull); }
    }
}

__global__ void __launch_bounds__(256)
k_hops_flags(dfk_hops::Graph G, uint64_t n_he, uint8_t* __restrict__ flags)
{
    for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < n_he; e += (uint64_t)gridDim.x * 256)
        flags[e] = (uint8_t)((dfk_hops::sink_ok(G, (int32_t)e) ? 1 : 0) | (dfk_hops::source_ok(G, (int32_t)e) ? 2 : 0));
}

// first: the exclusive scan of the counts over ALL keys; a range's lists start at first[e0]
__global__ void __launch_bounds__(256)
k_hops_scatter(const uint32_t* __restrict__ var, const uint32_t* __restrict__ elem_off, uint64_t nb, uint64_t r0, uint64_t var_bytes, const int32_t* __restrict__ inv,
               uint32_t e0, uint32_t e1, const uint64_t* __restrict__ first, uint32_t* __restrict__ cursor /* [e1 - e0], zeroed */, uint32_t* __restrict__ vals)
{
    const uint64_t base = first[e0];
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nb; i += (uint64_t)gridDim.x * 256) {
        const uint64_t w0 = elem_off[i] >> 2, w1 = (i + 1 < nb ? (uint64_t)elem_off[i + 1] : var_bytes) >> 2;
        const uint32_t id2 = (uint32_t)(r0 + i) << 1;
        for (uint64_t w = w0 + 2; w < w1; ++w) {
            const uint32_t g = var[w], rg = (uint32_t)inv[g];
            if (g >= e0 && g < e1) vals[first[g] - base + atomicAdd(&cursor[g - e0], 1u)] = id2;
            if (rg >= e0 && rg < e1) vals[first[rg] - base + atomicAdd(&cursor[rg - e0], 1u)] = id2 | 1u;
        }
    }
}

__device__ inline uint64_t hops_mix(uint64_t x)
{
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; return x ^ (x >> 31);
}

constexpr uint32_t HOPS_NO_ID = 0xFFFFFFFFu;

__global__ void __launch_bounds__(64)
k_hops_mates(uint32_t e0, uint32_t e1, const uint64_t* __restrict__ first, const uint32_t* __restrict__ vals, const uint8_t* __restrict__ flags,
             const int32_t* __restrict__ inv, HopsPaths paths, const int32_t* __restrict__ bc,
             unsigned long long* __restrict__ tk /* ~0 = free */, uint32_t* __restrict__ tb /* HOPS_NO_ID = none yet */, uint8_t* __restrict__ tm, uint64_t mask)
{
    const uint64_t base = first[e0];
    for (uint64_t e = (uint64_t)e0 + blockIdx.x; e < e1; e += gridDim.x) {
        if (!(flags[e] & 1)) continue;                                    // :63-74
        const uint32_t* list = vals + (first[e] - base);
        const uint64_t n = first[e + 1] - first[e];
        for (uint64_t i = threadIdx.x; i < n; i += 64) {
            const uint32_t v = list[i];
            if (v & 1u) continue;                                         // (a read on inv[e])
            const int32_t* p2; const int n2 = paths.len((v >> 1) ^ 1u, &p2);
            if (n2 <= 0) continue;
            const uint32_t e2 = (uint32_t)inv[p2[n2 - 1]];                // :89
            if (e2 == (uint32_t)e) continue;
            const unsigned long long key = ((unsigned long long)e << 32) | e2;
            const uint32_t id = (uint32_t)bc[v >> 1];
            for (uint64_t h = hops_mix(key) & mask;; h = (h + 1) & mask) {
                const unsigned long long was = atomicCAS(&tk[h], ~0ull, key);
                if (was != ~0ull && was != key) continue;
                const uint32_t had = atomicCAS(&tb[h], HOPS_NO_ID, id);
                if (had != HOPS_NO_ID && had != id) tm[h] = 1;
                break;
            }
        }
    }
}

__global__ void __launch_bounds__(256)
k_hops_m1(const unsigned long long* __restrict__ tk, const uint8_t* __restrict__ tm, uint64_t slots, const uint8_t* __restrict__ flags, int one_good,
          uint8_t* __restrict__ seen, HopsOut out)
{
    for (uint64_t h = (uint64_t)blockIdx.x * 256 + threadIdx.x; h < slots; h += (uint64_t)gridDim.x * 256) {
        if (tk[h] == ~0ull || !tm[h]) continue;
        const uint32_t e1 = (uint32_t)(tk[h] >> 32), e2 = (uint32_t)tk[h];
        if (one_good || (flags[e2] & 2)) { out((int32_t)e1, (int32_t)e2); seen[e1] = 1; }        // :115-116, :128-130
    }
}

__global__ void __launch_bounds__(256)
k_hops_m2(const unsigned long long* __restrict__ tk, const uint8_t* __restrict__ tm, uint64_t slots, const uint8_t* __restrict__ seen, dfk_hops::Graph G, HopsOut out)
{
    for (uint64_t h = (uint64_t)blockIdx.x * 256 + threadIdx.x; h < slots; h += (uint64_t)gridDim.x * 256) {
        if (tk[h] == ~0ull || !tm[h]) continue;
        const uint32_t e1 = (uint32_t)(tk[h] >> 32), e2 = (uint32_t)tk[h];
        if (seen[e1]) continue;                                           // :138
        if (G.kmers[e2] >= dfk_hops::MIN_LANDING && G.to_right[e1] != G.to_left[e2]) out((int32_t)e1, (int32_t)e2);    // :175-177
    }
}

__global__ void __launch_bounds__(64)
k_hops_edges(uint32_t e0, uint32_t e1, const uint64_t* __restrict__ first, const uint32_t* __restrict__ vals, dfk_hops::Graph G, int K, HopsPaths paths,
             const int32_t* __restrict__ bc, HopsBad bad, dfk_hops::Caps cp, HopsOut out, uint32_t* __restrict__ host_edges, unsigned long long* __restrict__ ctr)
{
    extern __shared__ int32_t hops_lds[];
    const dfk_hops::Work w(hops_lds, cp);
    const WaveExec ex;
    const uint64_t base = first[e0];
    for (uint64_t e = (uint64_t)e0 + blockIdx.x; e < e1; e += gridDim.x) {
        dfk_hops::EdgeStat st;
        const int r = dfk_hops::edge_pairs(ex, G, K, (int32_t)e, vals + (first[e] - base), first[e + 1] - first[e], paths, bc, bad, cp, w, out, &st);
        __syncthreads();                                                  // (the next edge reuses the sets)
        if (threadIdx.x != 0 || r == dfk_hops::HOPS_SKIP) continue;
        if (r == dfk_hops::HOPS_OVERFLOW) { host_edges[atomicAdd(&ctr[HC_HOST], 1ull)] = (uint32_t)e; continue; }
        if (r == dfk_hops::HOPS_INTERNAL) { atomicAdd(&ctr[HC_INTERNAL], 1ull); continue; }
        atomicAdd(&ctr[HC_SEARCHED], 1ull);
        if (r == dfk_hops::HOPS_EXTENDED) atomicAdd(&ctr[HC_EXTENDED], 1ull);
        atomicMax(&ctr[HC_ROUNDS], (unsigned long long)st.rounds);
        atomicMax(&ctr[HC_LARGEST_X], (unsigned long long)st.n_x);
    }
}

// the exact route's fetch: the lengths of the paths of reads ids[0 .. n) (each below the number of reads), then their edges at off[i]
__global__ void __launch_bounds__(256)
k_hops_path_lens(const uint32_t* __restrict__ ids, uint64_t n, HopsPaths paths, uint32_t* __restrict__ lens)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const int32_t* p; const int np = paths.len(ids[i], &p);
        lens[i] = np > 0 ? (uint32_t)np : 0u;
    }
}

__global__ void __launch_bounds__(256)
k_hops_path_copy(const uint32_t* __restrict__ ids, uint64_t n, HopsPaths paths, const uint64_t* __restrict__ off /* [n + 1]: the scan of the lengths */, int32_t* __restrict__ out)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const int32_t* p; const int np = paths.len(ids[i], &p);
        const uint64_t room = off[i + 1] - off[i];
        for (uint64_t k = 0; k < room && (int64_t)k < np; ++k) out[off[i] + k] = p[k];
    }
}

} // namespace dfk
