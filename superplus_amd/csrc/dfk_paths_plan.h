// superplus_amd/csrc/dfk_paths_plan.h -- the plans of the steps after the count: every host decision between the launches of
// paths_build_typed, paths_index_write, dups_write (dfk_paths.inc) and their sharded counterparts (dfk_paths_shard.inc).
// Host-only: plain functions over read, entry and byte counts, so they run on a CPU (tests/cpp/test_paths_plan.cc).  What is
// decided here:
//   1. the grid of a 256-thread launch;
//   2. pathing: the reads a batch may hold, whether the k-mer filter is reused, built or left out, and the batches -- room, reads,
//      the halving until the real scratch fits, the scratch sizes, the retry with all slots, each batch's place in the file;
//   3. a feudal file's control block and layout, and the pieces a device range goes to a file in;
//   4. the paths index: whether the lists leave through the tail thread, the entries a range of edges may hold, the ranges,
//      the sort's key bits, whether the lists enter the file through a mapping;
//   5. the passes and the table of the duplicate marks;
//   6. a sharded run: a rank's range of edges, what it sends to every owner, its slice of the offset table.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>
#include "dfk_fallback.h"   // ceil_log2

namespace dfk {

// DFK_PATH_SLOTS, DFK_NO_FILTER, DFK_PATH_BATCH_READS: read once per pathing; DFK_PIDX_RANGE_PAIRS once per index build,
// DFK_DUP_PASSES once per marking (tests switch them between calls on one context).  path_switches (dfk_paths.inc) reads the five.
struct PathSwitches {
    uint32_t slots = 12;              // path slots a read is given before its batch is done again with one per k-mer position
    bool no_filter = false;
    uint64_t batch_reads = 0;         // tests: a pathing batch takes at most so many reads (0 = unset)
    uint64_t pidx_range_pairs = 0;    // tests: a range of the paths index holds at most so many entries (0 = unset)
    uint32_t dup_passes = 0;          // tests: at least so many passes of the duplicate table (0 = unset)
};

// ---- 1. blocks of 256 threads over n items, at most per_cu a CU.  (Where a launch has always had (n + 256) / 256 blocks --
// one more when n is a multiple of 256 -- its site passes n + 1.)
inline unsigned grid_256(uint64_t n, unsigned cus, uint32_t per_cu = 32) { return (unsigned)std::min<uint64_t>((n + 255) / 256, (uint64_t)per_cu * cus); }

// ---- 2. pathing
// The longest read bounds a batch: k_path_slots keeps two running sums in one 64-bit scan (slots low, quality bytes high),
// neither of which may pass 2^32.
inline uint64_t path_batch_bound(uint32_t max_len, uint32_t K)
{
    const uint64_t q_per_read = ((uint64_t)max_len + 3) & ~3ull, s_per_read = max_len >= K ? max_len - K + 1 : 1;
    return std::max<uint64_t>(1, std::min<uint64_t>(0xFFFFFFFFull / std::max<uint64_t>(1, q_per_read), 0xFFFFFFFFull / s_per_read) - 1);
}

// the filter in front of the index (dfk_paths_kernels.h): two bytes per k-mer.  The graph's own is taken over when it was made
// under this numbering (graph_words: its words, 0 = it has none); else one is built if the device has the room to spare.
enum class PathFilter { None, Reuse, Build };
struct PathFilterPlan { PathFilter use; uint64_t words; };
inline PathFilterPlan plan_path_filter(uint64_t n_kmers, uint64_t n_reads, uint64_t free_now, uint64_t graph_words, bool no_filter)
{
    const uint64_t words = std::max<uint64_t>(64, n_kmers / 2);
    if (graph_words == words && !no_filter) return {PathFilter::Reuse, words};
    if (!no_filter && n_kmers && free_now > words * 4 + n_reads * 18 + (4ull << 30)) return {PathFilter::Build, words};
    return {PathFilter::None, words};
}

// the scratch of a batch of nb reads holding `total` slots (k-mer positions, capped) and `qtotal` quality bytes
struct PathScratch { uint64_t parts, path, quals, o_off, o_len, o_first, sizes, size_off; };

// The batches of a pathing.  Per read of s slots a batch holds 16 s bytes of parts, 8 s + 8 of path room, its bases in decoded
// qualities, 24 of bookkeeping and 12 of results; the output (8 + 4 per path edge, + 8 of offset) stays.
// A batch's scratch comes out of what is free NOW minus what the batches still to come will leave behind (their share of the
// file: ~13 bytes of data and 4 of offset per read), so that the last batches are not squeezed into nothing; it takes what half
// of that pays for at a guess of `slots` slots a read -- checked against the real slot count, and halved until that fits.
// sw.slots slots do for nearly every read (five wrong bases make eleven parts) where one per k-mer position would be 53 to 103:
// a batch in which a read wants more says so and is done again with all of them.
//   while (b.more()) { b.begin(free); do { ...k_path_slots, scan... } while (!b.fits(total, qtotal)); ...; b.end(again, var_bytes); }
struct PathBatcher {
    uint64_t n = 0, bound = 1; PathSwitches sw;
    uint64_t r0 = 0, nb = 0, room = 0, file_base = 24;   // this attempt: reads [r0, r0 + nb), its variable data at file_base
    uint32_t cap = 0;                                   // slots a read may take in this attempt
    bool all_slots = false;                             // this batch: one slot per k-mer position

    PathBatcher(uint64_t n_reads, uint64_t batch_bound, const PathSwitches& s) : n(n_reads), bound(batch_bound), sw(s) {}
    bool more() const { return r0 < n; }
    void begin(uint64_t free_now)
    {
        cap = all_slots ? 0xFFFFFFFFu : sw.slots;
        const uint64_t to_come = (n - r0) * 18;
        room = free_now > to_come + (256ull << 20) ? free_now - to_come : free_now / 8;
        const uint64_t per_read_guess = 24ull * std::min<uint32_t>(cap, 64) + 8 + 104 + 64;
        nb = std::min<uint64_t>(n - r0, std::max<uint64_t>(1, room / 2 / per_read_guess));
        nb = std::min<uint64_t>(nb, bound);             // (k_path_slots: both offsets of a read in one word, 32 bits each)
        if (sw.batch_reads) nb = std::min<uint64_t>(nb, sw.batch_reads);
    }
    static uint64_t need(uint64_t total, uint64_t qtotal, uint64_t nb) { return 24 * total + qtotal + nb * (8 + 12 + 16) + 4096; }
    // the scan's two totals of this attempt: it is taken (a single read whatever it needs), or nb halves for the next one
    bool fits(uint64_t total, uint64_t qtotal)
    {
        if (need(total, qtotal, nb) <= room || nb == 1) return true;
        nb = std::max<uint64_t>(1, nb / 2);
        return false;
    }
    PathScratch scratch(uint64_t total, uint64_t qtotal) const
    {
        return PathScratch{std::max<uint64_t>(1, total) * 16, (2 * total + 2 * nb) * 4, qtotal + 64, nb * 4, nb * 4, nb * 4, (nb + 1) * 8, (nb + 1) * 8};
    }
    // the attempt is over: the pather asked for all slots (the same reads again), or the batch stays with var_bytes of data
    void end(bool again, uint64_t var_bytes)
    {
        all_slots = again;
        if (!again) { file_base += var_bytes; r0 += nb; }
    }
};

// ---- 3. the feudal file (feudal/FeudalControlBlock.h:159-165, FeudalFileWriter.cc:26-121): control block | variable data |
// n+1 absolute offsets | no fixed data
struct FeudalHead { uint32_t n; uint8_t flags, szFixed, szX, szA; uint64_t varTab, fixedOff; };
static_assert(sizeof(FeudalHead) == 24, "feudal control block");
struct FeudalLayout { FeudalHead head; uint64_t var_tab, file_size; };
inline FeudalLayout feudal_layout(uint64_t n, uint8_t szX, uint8_t szA, uint64_t var_bytes)
{
    const uint64_t var_tab = 24 + var_bytes, file_size = var_tab + 8 * (n + 1);
    return FeudalLayout{FeudalHead{(uint32_t)n, 1, 0, szX, szA, var_tab, file_size}, var_tab, file_size};
}

// device bytes on their way to a file (write_pieces, dfk_paths.inc): where from, how many, where to.  A piece with `widen`
// set is 32-bit values on the device that go to the file as 64-bit ones with `add` added (a feudal file's absolute element
// offsets, kept per read as 32-bit offsets inside their batch): widened on the host, in the lane.
struct FilePiece { const char* src; uint64_t bytes, file_off; bool widen = false; uint64_t add = 0; };

// `bytes` at src to file_off, in pieces of `chunk` (the transfer lanes' XFER_CHUNK)
inline void append_pieces(std::vector<FilePiece>& v, const char* src, uint64_t bytes, uint64_t file_off, uint64_t chunk)
{
    for (uint64_t o = 0; o < bytes; o += chunk) v.push_back(FilePiece{src + o, std::min<uint64_t>(chunk, bytes - o), file_off + o});
}
// ... widened: half a chunk of 32-bit values makes a chunk of the file
inline void append_wide_pieces(std::vector<FilePiece>& v, const char* src, uint64_t bytes, uint64_t file_off, uint64_t add, uint64_t chunk)
{
    for (uint64_t o = 0; o < bytes; o += chunk / 2) v.push_back(FilePiece{src + o, std::min<uint64_t>(chunk / 2, bytes - o), file_off + 2 * o, true, add});
}

// ---- 4. the paths index
// the lists of a.paths.inv may leave the device in a thread of their own (IndexTail): one range, a quarter of the room at most
inline bool pidx_tail_applies(bool have_dir, uint64_t n_pairs, uint64_t free_now)
{
    return have_dir && n_pairs && n_pairs < (1ull << 31) && 8 * n_pairs <= free_now / 4;
}
// entries a range of edges may hold: 24 bytes per entry while a range is sorted and widened
inline uint64_t pidx_range_cap(uint64_t free_now, uint64_t range_pairs_switch)
{
    return range_pairs_switch ? range_pairs_switch : std::min<uint64_t>((1ull << 31) - 1, std::max<uint64_t>(1ull << 20, free_now / 2 / 24));
}
// the range of edges from e0 on: as many as keep it at `cap` entries, one at least; first[] are the n_he + 1 prefix sums of
// the edges' entries.  ok = false: the range (a single edge) holds 2^32 entries or more, and its sort keeps 32-bit positions.
struct PidxRange { uint64_t e0, e1, n; bool ok; };
inline PidxRange pidx_next_range(const uint64_t* first, uint64_t n_he, uint64_t e0, uint64_t cap)
{
    uint64_t e1 = e0 + 1;
    while (e1 < n_he && first[e1 + 1] - first[e0] <= cap) ++e1;
    const uint64_t n_r = first[e1] - first[e0];
    return PidxRange{e0, e1, n_r, n_r < (1ull << 32)};
}
// key bits of the sort by edge over n_edges edges
inline uint32_t pidx_key_bits(uint64_t n_edges) { return std::max<uint32_t>(1, ceil_log2(std::max<uint64_t>(2, n_edges))); }
// a range's lists in the file, and whether they go in through a mapping: when the pages were all there (`had`: the bytes the
// file had when it was opened)
struct PidxMap { bool mapped; uint64_t lo, hi; };
inline PidxMap pidx_map(uint64_t had, uint64_t var_tab, uint64_t first_e0, uint64_t n_r)
{
    const uint64_t lo = 24 + 8 * first_e0;
    return PidxMap{had >= var_tab, lo, lo + 8 * n_r};
}

// ---- 5. duplicate marks: as many passes as the free HBM asks for -- a pass's table holds the keys dealt to it at load <= 0.5
// (+25 %: the deal is by hash) in half the free room.  (A table as large as the room allows is not the fastest: at configs[1]
// two passes over 69 GB took 3.0 s where four over 34 GB take 0.3 -- the larger one needed a chunk the driver had to produce first.)
struct DupPlan { uint32_t n_pass; uint64_t slots; };
inline DupPlan plan_dups(uint64_t n_placed, uint64_t free_now, uint32_t min_passes)
{
    uint32_t n_pass = 1;
    while (n_pass < std::min<uint32_t>(1024, min_passes)) n_pass *= 2;
    for (;; n_pass *= 2) {
        const uint64_t slots = 1ull << std::max<uint32_t>(10, ceil_log2(2 * (n_placed / n_pass + n_placed / (4 * n_pass) + 1024)));
        if (16 * slots <= free_now / 2 || n_pass >= 1024) return DupPlan{n_pass, slots};
    }
}

// ---- 6. a sharded run: rank r owns the edges [edge_range_start(r), edge_range_start(r + 1))
inline uint64_t edge_range_start(uint64_t n_he, uint32_t world, uint32_t r) { return (uint64_t)r * n_he / world; }
// entries a rank sends to every owner, from its per-edge counts
inline void shard_send_counts(const uint32_t* counts, uint64_t n_he, uint32_t world, uint64_t* send_counts)
{
    for (uint32_t r = 0; r < world; ++r) {
        uint64_t s = 0;
        for (uint64_t e = edge_range_start(n_he, world, r); e < edge_range_start(n_he, world, r + 1); ++e) s += counts[e];
        send_counts[r] = s;
    }
}
inline std::vector<uint64_t> prefix_sums(const uint64_t* counts, uint64_t n)
{
    std::vector<uint64_t> first(n + 1, 0);
    for (uint64_t e = 0; e < n; ++e) first[e + 1] = first[e] + counts[e];
    return first;
}
// entries of the offset table a rank owning ne edges holds: the last rank also holds the end of the last list
inline uint64_t shard_table_entries(uint64_t ne, uint32_t world, uint32_t rank) { return ne + (rank + 1 == world ? 1 : 0); }
// ... and those entries, edges [e0, e1): where each list starts in the file (one more than a rank writes, but for the last)
inline std::vector<uint64_t> shard_table_slice(const std::vector<uint64_t>& first, uint64_t e0, uint64_t e1)
{
    std::vector<uint64_t> eo(e1 - e0 + 1);
    for (uint64_t e = 0; e <= e1 - e0; ++e) eo[e] = 24 + 8 * first[e0 + e];
    return eo;
}

} // namespace dfk
