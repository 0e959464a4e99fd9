// superplus_amd/csrc/dfk_subset.h -- the patching stage's subset of interest (StagePatch, 10X/runstages/RunStages.cc:208-254):
// the rule over plain arrays, the plan of the device version, the layouts of the four files a.sub.*.
//
// No HIP call and no device pointer is dereferenced here by the host, so tests/cpp/test_subset.cc compiles this header with a
// plain host compiler (and once more under -fsanitize=address,undefined) and checks it against cases recorded from
// tests/subset_oracle.py.  It is the SECOND restatement of the rule -- written from the reference's text, not from the Python.
//
// The rule (E edges, N reads, N even, the mate of id = id ^ 1):
//   in_pairs (:213-219)   in_pairs[x] = true for x in {p.first, p.second, inv[p.first], inv[p.second]} over all pairs p
//   eoi (:222-226)        the marked edges, ascending
//   hit (:228-240)        hit[r] = any(in_pairs[e] for e in path[r]).  The loop pushes id and its mate at the first marked
//                         entry of read id; on an even id it then steps over the odd one (`id++`), on an odd id -- reached only
//                         when the even one did not hit -- it pushes `id - 1`.  So pair i is taken iff hit[2i] || hit[2i+1],
//                         and a taken pair gives both ids once.
//   read_ids (:241)       the ascending list of 2i, 2i + 1 over the taken pairs
//   an unplaced read (empty path) never hits; it is in the subset when its mate does; two unplaced mates never are
//   paths subset (:253)   element k = the ReadPath of read read_ids[k] as a.paths holds it (SubsetMasterVec::build,
//                         feudal/SubsetMasterVec.h:29-38: push_back( src.at( id ) ) over the sorted ids)
//   index subset (:254)   element k = the ULongVec of edge eoi[k] as a.paths.inv holds it: ascending read ids, a read that crosses
//                         the edge twice listed twice (writePathsIndex sorts (edge, read) pairs and keeps duplicates)
//
// The files (dfk_subset_write):
//   a.sub.ids        "BINWRITE" | u64 n | n x u64   BinaryWriter::writeFile of vec<uint64_t> read_ids (:211)
//   a.sub.eoi        the same.  eoi is a vec<size_type> (:222); in RunStages.cc the unqualified size_type is the global
//                    `typedef size_t size_type` of system/Types.h:126, and SubsetMasterVec::build takes a vec<size_t>& -- 8 bytes
//   a.sub.paths      feudal ReadPathVec, the control block of a.paths {n, 1, 0, 24, 4}: data | n + 1 absolute offsets
//   a.sub.paths.inv  feudal VecULongVec, the control block of a.paths.inv {n, 1, 0, 16, 8}
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DFK_SUBSET_HD __host__ __device__ inline
#else
#define DFK_SUBSET_HD inline
#endif

namespace dfk_subset {

// ---- what the kernels share with the plan
constexpr uint32_t MARK_WORD_BITS = 32;           // in_pairs as a bit set of 32-bit words: 1e7 edges are 1.2 MB, resident in L2 under the sweep
constexpr uint32_t PAIR_WORD_BITS = 64;           // one bit per pair, a wave's ballot a word
constexpr uint64_t SALT_IDS = 0x7777ull, SALT_EOI = 0x8888ull;    // k_digest_seq's salts for read_ids and eoi

DFK_SUBSET_HD uint64_t mark_words(uint64_t n_edges) { return (n_edges + MARK_WORD_BITS - 1) / MARK_WORD_BITS; }
DFK_SUBSET_HD uint64_t pair_words(uint64_t n_pairs) { return (n_pairs + PAIR_WORD_BITS - 1) / PAIR_WORD_BITS; }
DFK_SUBSET_HD bool marked(const uint32_t* marks, uint32_t e) { return (marks[e / MARK_WORD_BITS] >> (e % MARK_WORD_BITS)) & 1u; }
DFK_SUBSET_HD bool pair_bit(const unsigned long long* bits, uint64_t pair) { return (bits[pair / PAIR_WORD_BITS] >> (pair % PAIR_WORD_BITS)) & 1ull; }

// :228-240 for one pair: its reads are in the subset iff either hits
DFK_SUBSET_HD bool pair_taken(bool hit_even, bool hit_odd) { return hit_even || hit_odd; }

// element sizes in the two feudal files: a ReadPath is {i32 offset, u32 lastSkip} and its edges; a ULongVec its ids
DFK_SUBSET_HD uint64_t path_elem_bytes(uint64_t n_path_edges) { return 8 + 4 * n_path_edges; }
DFK_SUBSET_HD uint64_t index_elem_bytes(uint64_t n_entries) { return 8 * n_entries; }

// a taken read's word of the gather's scan: its element's bytes below (a batch's data is under 2^32 bytes), one above (the
// reads taken before it); an exclusive 64-bit scan of these words gives both places at once
DFK_SUBSET_HD uint64_t gather_word(uint64_t elem_bytes) { return (1ull << 32) | elem_bytes; }
DFK_SUBSET_HD uint64_t gather_rank(uint64_t scanned) { return scanned >> 32; }
DFK_SUBSET_HD uint64_t gather_byte(uint64_t scanned) { return scanned & 0xFFFFFFFFull; }

} // namespace dfk_subset

// ---------------------------------------------------------------------------------------------------------------- host only
#include <algorithm>
#include <vector>
#include "dfk_paths_plan.h"   // FeudalHead / feudal_layout, pidx_range_cap / pidx_next_range, grid_256

namespace dfk_subset {

// :213-219.  marks: mark_words(E) words, zeroed by the caller.  -1: a pair names an edge outside [0, E) (nothing is marked then)
inline int mark_edges(const int32_t* pairs, uint64_t n_pairs, const int32_t* inv, uint64_t n_edges, uint32_t* marks)
{
    for (uint64_t i = 0; i < 2 * n_pairs; ++i) if (pairs[i] < 0 || (uint64_t)pairs[i] >= n_edges) return -1;
    auto set = [&](int32_t e) { marks[(uint32_t)e / MARK_WORD_BITS] |= 1u << ((uint32_t)e % MARK_WORD_BITS); };
    for (uint64_t i = 0; i < 2 * n_pairs; ++i) { set(pairs[i]); set(inv[pairs[i]]); }
    return 0;
}

struct HostResult {
    std::vector<uint64_t> eoi, ids;
    std::vector<uint64_t> index_first;            // [n_eoi + 1]: entries of the index subset before rank k
    uint64_t path_entries = 0, one_read_only = 0, unplaced = 0;
};

// the whole rule on the host (paths as a CSR: first[N + 1], edges), for the CPU test.  -1: an edge out of range, -2: N odd
inline int subset_host(uint64_t n_edges, const int32_t* inv, uint64_t n_reads, const uint64_t* first, const int32_t* edges,
                       const int32_t* pairs, uint64_t n_pairs, HostResult* R)
{
    if (n_reads % 2) return -2;
    std::vector<uint32_t> marks(std::max<uint64_t>(1, mark_words(n_edges)), 0u);
    if (mark_edges(pairs, n_pairs, inv, n_edges, marks.data())) return -1;
    std::vector<uint64_t> rank(n_edges + 1, 0);
    for (uint64_t e = 0; e < n_edges; ++e) {                                    // :222-226
        rank[e + 1] = rank[e];
        if (marked(marks.data(), (uint32_t)e)) { R->eoi.push_back(e); ++rank[e + 1]; }
    }
    auto hit = [&](uint64_t id) {
        for (uint64_t k = first[id]; k < first[id + 1]; ++k) if (marked(marks.data(), (uint32_t)edges[k])) return true;
        return false;
    };
    std::vector<uint64_t> counts(R->eoi.size(), 0);
    for (uint64_t p = 0; p < n_reads / 2; ++p) {                                // :228-241
        const bool a = hit(2 * p), b = hit(2 * p + 1);
        if (!pair_taken(a, b)) continue;
        R->one_read_only += a != b;
        for (uint64_t id = 2 * p; id < 2 * p + 2; ++id) {
            R->ids.push_back(id);
            R->path_entries += first[id + 1] - first[id];
            R->unplaced += first[id + 1] == first[id];
        }
    }
    for (uint64_t k = 0; k < first[n_reads]; ++k) if (marked(marks.data(), (uint32_t)edges[k])) ++counts[rank[edges[k]]];
    R->index_first = dfk::prefix_sums(counts.data(), counts.size());
    return 0;
}

// ---- the plan
// The index subset is built a range of eoi RANKS at a time, by the sizing rule of the paths index (pidx_range_cap: 24 bytes an
// entry while a range is sorted and widened; DFK_PIDX_RANGE_PAIRS forces small ranges): first[] are the n_eoi + 1 prefix sums of
// the entries per rank.  ok = false: one edge alone holds 2^32 entries or more.
inline uint64_t range_cap(uint64_t free_now, uint64_t range_pairs_switch) { return dfk::pidx_range_cap(free_now, range_pairs_switch); }
inline dfk::PidxRange next_range(const uint64_t* first, uint64_t n_eoi, uint64_t k0, uint64_t cap) { return dfk::pidx_next_range(first, n_eoi, k0, cap); }
inline uint64_t count_ranges(const uint64_t* first, uint64_t n_eoi, uint64_t cap)
{
    uint64_t n = 0;
    for (uint64_t k0 = 0; k0 < n_eoi; ++n) k0 = next_range(first, n_eoi, k0, cap).e1;
    return n;
}
inline uint32_t range_key_bits(uint64_t n_ranks) { return dfk::pidx_key_bits(n_ranks); }

// the scratch of one batch's gather: nb reads, of which `taken` with `bytes` of elements go to the files
struct GatherScratch { uint64_t words, places, ids, offsets, data; };
inline GatherScratch gather_scratch(uint64_t nb, uint64_t taken, uint64_t bytes, bool for_files)
{
    return GatherScratch{(nb + 1) * 8, (nb + 1) * 8, std::max<uint64_t>(1, taken) * 8, for_files ? std::max<uint64_t>(1, taken) * 8 : 0,
                         for_files ? std::max<uint64_t>(4, bytes) : 0};
}
// ... of one batch's share of a range of the index subset
struct RangeScratch { uint64_t counts, places; };
inline RangeScratch range_scratch(uint64_t nb) { return RangeScratch{(nb + 1) * 8, (nb + 1) * 8}; }

inline unsigned grid_reads(uint64_t n, unsigned cus) { return dfk::grid_256(n + 1, cus); }      // (n + 1: the kernels that fill a scan's input write its last word too)
inline unsigned grid_pairs(uint64_t n_pairs, unsigned cus) { return dfk::grid_256(std::max<uint64_t>(1, n_pairs), cus); }

// ---- the files' fixed parts
struct BinHead { char magic[8]; uint64_t n; };                                  // BinaryWriter::writeFile of a vec<T> (feudal/BinaryStream.h:447-462)
static_assert(sizeof(BinHead) == 16, "BINWRITE header");
inline BinHead bin_head(uint64_t n) { return BinHead{{'B', 'I', 'N', 'W', 'R', 'I', 'T', 'E'}, n}; }
inline uint64_t ids_file_size(uint64_t n) { return 16 + 8 * n; }
inline dfk::FeudalLayout paths_layout(uint64_t n_ids, uint64_t path_entries) { return dfk::feudal_layout(n_ids, 24, 4, 8 * n_ids + 4 * path_entries); }
inline dfk::FeudalLayout index_layout(uint64_t n_eoi, uint64_t index_entries) { return dfk::feudal_layout(n_eoi, 16, 8, 8 * index_entries); }

} // namespace dfk_subset
