// superplus_amd/csrc/dfk_patch_kernels.h -- the patched graph's own kernels (gfx950, wave64); the rule and the shared pieces:
// dfk_patch.h.  The dictionary of allx is written in place from the old edges (k_patch_entries, a lane a K-mer position, streaming), checked
// (k_patch_check), the closures' K-mers are looked up in it (k_patch_closure_kmers: atomicOr where found, a wave-aggregated append where not);
// the unipath edges are dfk_graph_kernels.h's, unchanged; then the old edges' paths are read off the entries (k_patch_heads, the project's
// device_scan, k_patch_emit: no walk, no look-up, no atomic).  Integer work only.
#pragma once
#include "dfk_graph_kernels.h"
#include "dfk_patch.h"

namespace dfk {

// Sequences lie in one stream of 2-bit bases, base i at bits [2i, 2i + 2) of little-endian words (a .fastb's order), a sequence anywhere
// (not byte aligned); the stream ends with eight zero words, so the five words a K-mer may touch are there.
__device__ __forceinline__ uint32_t patch_base(const uint32_t* __restrict__ w, uint64_t pos) { return (w[pos >> 4] >> (2 * (pos & 15))) & 3u; }
// the K bases from `pos` in canonical() 's input form
__device__ __forceinline__ u128 patch_load(const uint32_t* __restrict__ w, uint64_t pos)
{
    const uint64_t i = pos >> 4;
    const uint32_t s = 2u * (uint32_t)(pos & 15);
    const uint32_t a0 = w[i], a1 = w[i + 1], a2 = w[i + 2], a3 = w[i + 3], a4 = w[i + 4];
    return u128{(uint64_t)alignbit(a1, a0, s) | ((uint64_t)alignbit(a2, a1, s) << 32), (uint64_t)alignbit(a3, a2, s) | ((uint64_t)alignbit(a4, a3, s) << 32)};
}
__device__ __forceinline__ void patch_put(uint4* e, u128 F, int bits, uint32_t ctx)
{
    const u128 kw = shl128(F, 128 - bits);                               // w0 = bases 0..31, w1 the rest, left-aligned
    e[0] = uint4{(uint32_t)kw.hi, (uint32_t)(kw.hi >> 32), (uint32_t)kw.lo, (uint32_t)(kw.lo >> 32)};
    e[1] = uint4{0xFFFFFFFFu, ctx << 24, 0xFFFFFFFFu, 0u};               // edge_id null, count 0, tempBC -1, pad 0
}

// A lane a slot = (canonical old edge, K-mer position): the dfk_entry32 of that K-mer at entries[slot], its context by
// dfk_patch::position_context(); rev_bits: bit slot = the edge reads the entry's K-mer reverse-complemented.  256 consecutive slots a
// block and pass: the entries are written in order, the edges' bases read in order.
template <int K>
__global__ void __launch_bounds__(256)
k_patch_entries(const uint32_t* __restrict__ words, const uint64_t* __restrict__ ebase, const uint64_t* __restrict__ first, const uint32_t* __restrict__ ends, uint32_t n_canon,
             uint64_t n_slots, uint4* __restrict__ entries, unsigned long long* __restrict__ rev_bits)
{
    for (uint64_t g0 = (uint64_t)blockIdx.x * 256; g0 < n_slots; g0 += (uint64_t)gridDim.x * 256) {
        const uint64_t g = g0 + threadIdx.x;
        bool rev = false;
        if (g < n_slots) {
            const uint32_t c = dfk_patch::slot_edge(first, n_canon, g);
            const uint64_t f0 = first[c], at = ebase[c];
            const uint32_t pos = (uint32_t)(g - f0), n = (uint32_t)(first[c + 1] - f0);
            const u128 F = canonical<K>(patch_load(words, at + pos), &rev);
            const uint32_t ctx = dfk_patch::position_context(ends[c], pos, n, pos ? patch_base(words, at + pos - 1) : 0u, pos + 1 < n ? patch_base(words, at + pos + K) : 0u, rev);
            patch_put(entries + 2 * g, F, KTraits<K>::BITS, ctx);
        }
        const unsigned long long mk = __ballot(rev);
        if ((threadIdx.x & 63) == 0 && g < n_slots) rev_bits[g >> 6] = mk;
    }
}

// every base entry finds itself: a K-mer with two slots finds the other one (bad |= 8)
template <int K>
__global__ void __launch_bounds__(256)
k_patch_check(PartTable pt_arg, uint64_t n, const uint32_t* __restrict__ index, uint64_t n_slots, unsigned int* __restrict__ bad)
{
    __shared__ PartLds pt;
    part_lds_init(pt_arg, pt);
    for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (uint64_t)gridDim.x * 256) {
        uint32_t ctx; bool pal;
        if (graph_lookup<K>(pt, index, n_slots, kmer_of_entry<K>(entry_ptr(pt, g)[0]), &ctx, &pal) != (uint32_t)g) atomicOr(bad, 8u);
    }
}

// A lane a closure K-mer position q in [q0, q1): found in the base dictionary -> its context OR-ed into the entry (device scope, exact
// whatever the order); not found -> (key, context) appended to `list` as a dfk_entry32 (room for q1 - q0).
// ctr: [0] appended, [1] found, [2] context bits that were not set before.
template <int K>
__global__ void __launch_bounds__(256)
k_patch_closure_kmers(PartTable pt_arg, const uint32_t* __restrict__ index, uint64_t n_slots, const uint32_t* __restrict__ words, const uint64_t* __restrict__ cbase,
                   const uint64_t* __restrict__ cfirst, uint32_t n_closures, uint64_t q0, uint64_t q1, uint4* __restrict__ list, unsigned long long* __restrict__ ctr)
{
    __shared__ PartLds pt;
    part_lds_init(pt_arg, pt);
    const int lane = threadIdx.x & 63;
    unsigned long long n_found = 0, n_bits = 0;
    for (uint64_t b = (uint64_t)blockIdx.x * 256; q0 + b < q1; b += (uint64_t)gridDim.x * 256) {
        const uint64_t q = q0 + b + threadIdx.x;
        bool fresh = false, rev = false;
        u128 F{0, 0};
        uint32_t ctx = 0;
        if (q < q1) {
            const uint32_t i = dfk_patch::slot_edge(cfirst, n_closures, q);
            const uint64_t f0 = cfirst[i], at = cbase[i];
            const uint32_t p = (uint32_t)(q - f0), n = (uint32_t)(cfirst[i + 1] - f0);
            F = canonical<K>(patch_load(words, at + p), &rev);
            ctx = dfk_patch::entry_context(p ? 1u << patch_base(words, at + p - 1) : 0u, p + 1 < n ? 1u << patch_base(words, at + p + K) : 0u, 0u, 0u, rev);
            uint32_t c2; bool pal;
            const uint32_t g = graph_lookup<K>(pt, index, n_slots, F, &c2, &pal);
            if (g == GRAPH_EMPTY) fresh = true;
            else {
                const uint32_t old = atomicOr(reinterpret_cast<unsigned int*>(entry_ptr(pt, g) + 1) + 1, ctx << 24);
                ++n_found; n_bits += __popc((ctx << 24) & ~old);
            }
        }
        const unsigned long long mk = __ballot(fresh);
        if (mk) {
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(&ctr[0], (unsigned long long)__popcll(mk));
            base = uniform64((uint64_t)base);
            if (fresh) patch_put(list + 2 * (base + __popcll(mk & ((1ull << lane) - 1ull))), F, KTraits<K>::BITS, ctx);
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { n_found += __shfl_down(n_found, d, 64); n_bits += __shfl_down(n_bits, d, 64); }
    if (lane == 0 && n_found) { atomicAdd(&ctr[1], n_found); atomicAdd(&ctr[2], n_bits); }
}

// What the walk along a canonical old edge meets at a base entry after k_graph_bases: its hb3 edge, whether the walk reads that edge
// forwards, the entry's offset in walking direction and the edge's K-mers.  Whether the edge shows the entry's canonical K-mer or its
// reverse complement is read off ONE base of the edge: the first at which the two differ (a palindrome differs nowhere: forwards).
struct PatchStep { uint32_t e3, n3, woff; bool fwd; };
template <int K>
__device__ __forceinline__ PatchStep patch_step(const PartLds& pt, uint64_t g, bool read_rev, const EdgeRec* __restrict__ recs, const uint8_t* __restrict__ store)
{
    const uint4* e = entry_ptr(pt, g);
    const uint4 b = e[1];
    const u128 F = kmer_of_entry<K>(e[0]), R = kmer_rc<K>(F);
    const uint32_t off = b.y & 0xFFFFFFu;
    const EdgeRec r = recs[b.x];
    bool stored_fwd = true;
    const u128 D{F.lo ^ R.lo, F.hi ^ R.hi};
    if (D.lo | D.hi) {
        const int msb = D.hi ? 127 - __clzll((long long)D.hi) : 63 - __clzll((long long)D.lo);
        const int i = K - 1 - (msb >> 1);
        const uint64_t q = r.byte_off * 4 + off + (uint32_t)i;
        stored_fwd = ((store[q >> 2] >> (2 * (q & 3))) & 3u) == kmer_base<K>(F, i);
    }
    PatchStep s;
    s.e3 = b.x; s.n3 = r.n;
    s.fwd = dfk_patch::walk_dir(read_rev, stored_fwd);
    s.woff = dfk_patch::walk_offset(s.fwd, off, r.n);
    return s;
}

// A block 256 consecutive slots (a wave a run of 64: the entries are read in order): head_bits: bit slot = the position starts a new id
// (dfk_patch::is_head); blk_count[block] = its heads (64 bits: device_scan's input), the waves' counts staged through LDS.
template <int K>
__global__ void __launch_bounds__(256)
k_patch_heads(PartTable pt_arg, uint64_t n_slots, const uint64_t* __restrict__ first, uint32_t n_canon, const unsigned long long* __restrict__ rev_bits,
           const EdgeRec* __restrict__ recs, const uint8_t* __restrict__ store, unsigned long long* __restrict__ head_bits, unsigned long long* __restrict__ blk_count)
{
    __shared__ PartLds pt;
    part_lds_init(pt_arg, pt);
    __shared__ uint32_t wave_heads[4];
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool head = false;
    if (g < n_slots) {
        const uint32_t c = dfk_patch::slot_edge(first, n_canon, g);
        const PatchStep s = patch_step<K>(pt, g, (rev_bits[g >> 6] >> (g & 63)) & 1ull, recs, store);
        head = dfk_patch::is_head((uint32_t)(g - first[c]), s.woff);
    }
    const unsigned long long mk = __ballot(head);
    if ((threadIdx.x & 63) == 0) { wave_heads[threadIdx.x >> 6] = (uint32_t)__popcll(mk); if (g < n_slots) head_bits[g >> 6] = mk; }
    __syncthreads();
    if (threadIdx.x == 0) blk_count[blockIdx.x] = (unsigned long long)wave_heads[0] + wave_heads[1] + wave_heads[2] + wave_heads[3];
}

// The heads write their ids where the scan has placed them (a canonical edge's ids are consecutive: its slots are); the first position
// of an edge leaves where its ids start and its left3, the last one the left3 of its inverse.
template <int K>
__global__ void __launch_bounds__(256)
k_patch_emit(PartTable pt_arg, uint64_t n_slots, const uint64_t* __restrict__ first, uint32_t n_canon, const unsigned long long* __restrict__ rev_bits,
          const EdgeRec* __restrict__ recs, const uint8_t* __restrict__ store, const unsigned long long* __restrict__ head_bits, const unsigned long long* __restrict__ blk_base,
          const int32_t* __restrict__ fwd3, const int32_t* __restrict__ rev3, int32_t* __restrict__ ids, unsigned long long* __restrict__ ids_first, int32_t* __restrict__ left,
          int32_t* __restrict__ left_inv)
{
    __shared__ PartLds pt;
    part_lds_init(pt_arg, pt);
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_slots) return;
    const uint32_t c = dfk_patch::slot_edge(first, n_canon, g);
    const uint32_t pos = (uint32_t)(g - first[c]);
    const unsigned long long word = head_bits[g >> 6];
    const bool head = (word >> (g & 63)) & 1ull, last = g + 1 == first[c + 1];
    if (!head && !last) return;
    const PatchStep s = patch_step<K>(pt, g, (rev_bits[g >> 6] >> (g & 63)) & 1ull, recs, store);
    if (head) {
        unsigned long long rank = blk_base[blockIdx.x] + __popcll(word & ((1ull << (g & 63)) - 1ull));
        for (uint64_t w = (uint64_t)blockIdx.x * 4; w < (g >> 6); ++w) rank += __popcll(head_bits[w]);
        ids[rank] = s.fwd ? fwd3[s.e3] : rev3[s.e3];
        if (pos == 0) { ids_first[c] = rank; left[c] = (int32_t)s.woff; }
    }
    if (last) left_inv[c] = dfk_patch::inv_left3(s.n3, s.woff);
}

} // namespace dfk
