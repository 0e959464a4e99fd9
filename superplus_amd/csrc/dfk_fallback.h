// superplus_amd/csrc/dfk_fallback.h -- what the count stage does with a work item that overflowed its LDS table: the
// decisions and the arithmetic between the launches of count_run, count_split and launch_count_big (dfk.hip).
// Host-only: plain functions over instance counts and a handful of constants, so they run on a CPU
// (tests/cpp/test_fallback.cc).  The routes of an overflowed item, in the order they are tried:
//   1. more than one fine bucket: halved by bucket index and counted again (halve_items);
//   2. one fine bucket of 2^SPLIT_FROM sub-buckets or more: partitioned a second time, by k-mer hash, into
//      sub-buckets that fit LDS tables (split_candidates, split_group_end; count_split);
//   3. what is left: 2^p sub-passes of k_count, each taking the k-mers of one selector value (plan_subpasses),
//      a sub-pass that overflows again being cut in two by one more selector bit (refine_subpasses);
//   4. buckets beyond the selector's reach or the switch: HBM tables (size_big_tables; launch_count_big).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace dfk {

// ---- what the host and the kernels share
struct ItemRange { uint32_t b0, b1; };     // a work item: fine buckets [b0,b1) of the current pass

// Where a persistent workgroup is in the chunk of the output buffer it is filling (kept across the launches of
// one pass).  Workgroups take chunks of OUT_CHUNK entries from CountGlobals::part_cursor and fill them item by
// item, an item's entries running over into a fresh chunk when needed; only the last chunk of every workgroup
// is left partly empty, and the host moves entries from the tail into those holes.
struct WgOut { unsigned long long chunk; unsigned int used; unsigned int pad; };

// a hot bucket and its 2^log2p sub-buckets, the first of which is number sub_base of the split (k_hot_pass)
struct HotItem { uint32_t b0, b1; uint32_t sub_base; uint32_t log2p; };

// a bucket and its HBM table: 2^log2s slots from word tab_off of the pool (k_big_*)
struct BigItem { uint32_t b0, b1; uint64_t tab_off; uint32_t log2s; uint32_t pad; };

constexpr int COUNT_CHUNK = 32;                   // records a wave stages at a time

inline uint32_t ceil_log2(uint64_t v) { uint32_t b = 0; while ((1ull << b) < v) ++b; return b; }

// ---- constants of the routes
constexpr uint32_t MAX_SELECTOR_BITS = 8;         // selector bits of a sub-pass word (wave_count_chunk)
constexpr uint64_t SPLIT_SUB_DISTINCT = 700;      // distinct k-mers a sub-bucket of a split bucket is sized for
constexpr uint32_t SPLIT_MAX_LOG2P = 22;          // (a pass's sub-buckets are numbered in 24 bits)
constexpr uint32_t BIG_MIN_LOG2S = 13;            // smallest HBM table

// DFK_SPLIT_FROM_LOG2: buckets of 2^this sub-buckets or more are split; DFK_MAX_SUBPASS_LOG2: buckets beyond 2^this sub-passes
// go to HBM tables.  count_run reads the two once per call.
struct FallbackSwitches { uint32_t split_from_log2 = 2, max_subpass_log2 = 8; };

// ---- 1. halving
// Items that overflowed their table are halved by bucket index; a single fine bucket cannot be: it goes to `singles`.
inline std::vector<ItemRange> halve_items(const std::vector<ItemRange>& overflowed, std::vector<ItemRange>* singles)
{
    std::vector<ItemRange> next;
    for (const ItemRange& r : overflowed) {
        const uint32_t mid = r.b0 + (r.b1 - r.b0) / 2;
        if (r.b1 - r.b0 <= 1) singles->push_back(r); else { next.push_back({r.b0, mid}); next.push_back({mid, r.b1}); }
    }
    return next;
}

// ---- 2., 3. the route of a single bucket
// Distinct k-mers per instance a split or a sub-pass plan assumes: twice what the passes so far have shown (a
// repeat-rich bucket has far fewer distinct k-mers than instances); on the first pass, a guess.
inline double route_distinct_per_inst(double seen) { return seen > 0.0 ? std::min(1.0, 2.0 * seen) : 0.5; }

inline uint64_t distinct_guess(uint64_t inst, double dpi) { return (uint64_t)((double)inst * dpi) + 1; }

// Buckets that would need four sub-passes or more (each sub-pass reads and extracts ALL of the bucket's
// instances again: work quadratic in the bucket's size, 6 s of a 9.5 s step at human scale with a 10 % repeat
// family) are partitioned a second time instead, by k-mer hash (count_split): linear work.
// The candidates: at[i], the bucket's place among the single buckets, and log2p[i], log2 of the sub-buckets its split makes.
// (k_hot_pass keeps a record's place inside its hot bucket in 32 bits: a bucket of 2^32 instances or more -- whatever
// its distinct k-mers -- takes the HBM tables)
struct SplitCandidates { std::vector<uint32_t> at, log2p; };

inline SplitCandidates split_candidates(const std::vector<uint64_t>& inst, double dpi, const FallbackSwitches& sw)
{
    SplitCandidates s;
    for (uint32_t i = 0; i < (uint32_t)inst.size(); ++i) {
        const uint32_t p = ceil_log2((distinct_guess(inst[i], dpi) + SPLIT_SUB_DISTINCT - 1) / SPLIT_SUB_DISTINCT);
        if (p >= sw.split_from_log2 && p <= SPLIT_MAX_LOG2P && inst[i] < (1ull << 32)) { s.at.push_back(i); s.log2p.push_back(p); }
    }
    return s;
}

// The expanded records of the split buckets (32 B per instance: 30 GB for a pass of a human-scale set with a 10 %
// repeat family) must fit one free block of the arena, which the pass plan does not reserve: the buckets are
// split in as many groups as that takes.  (All at once or not at all, three passes in twenty found no block
// and fell back to 250 000 sub-passes and HBM tables: 0.45 s each.)
// instances one group may hold, given the largest block the arena can hand out now (34 bytes each, 512 MiB left alone)
inline uint64_t split_group_cap(uint64_t can) { return can > (512ull << 20) ? (uint64_t)(0.95 * (double)(can - (512ull << 20))) / 34 : 0; }

// end of the group of candidates that starts at i0; == i0: not even the first fits
inline size_t split_group_end(const std::vector<uint64_t>& inst, const std::vector<uint32_t>& at, size_t i0, uint64_t cap_inst)
{
    size_t i1 = i0;
    for (uint64_t sum = 0; i1 < at.size() && sum + inst[at[i1]] <= cap_inst; ++i1) sum += inst[at[i1]];
    return i1;
}

// A fine bucket too rich for one LDS table is counted in 2^p sub-passes of k_count, each taking the k-mers
// of one selector value (all instances of a k-mer share it, so solidity and counts are exact; neighbours in
// another sub-pass are settled with the other cross-item bits).  p is first guessed from the distinct k-mers per
// instance; a sub-pass that overflows anyway is cut in two by one more selector bit and counted again -- its
// siblings are done and stay -- until p = MAX_SELECTOR_BITS, where 2^(log2s-1) *instances* per sub-pass are
// guaranteed: a bucket beyond that gets an HBM table, as does one beyond the switch.
// (The HBM tables are no way out for all of them: k_big_insert runs at 1.8 G instances/s there -- four dependent
// agent-scope atomics per instance, acquire/release fences per probe: 245 ms per pass -- 8.7 s per step at human scale
// with a 10 % repeat family when every bucket beyond four sub-passes goes to them, DFK_MAX_SUBPASS_LOG2=2.)
// one k_count item per sub-pass and its word (p << 8) | selector; huge: the buckets for the HBM tables
struct SubpassPlan { std::vector<ItemRange> items; std::vector<uint32_t> words; std::vector<ItemRange> huge; };

// the buckets no split has taken; log2s: the LDS table's
inline SubpassPlan plan_subpasses(const std::vector<ItemRange>& singles, const std::vector<uint64_t>& inst, const std::vector<uint8_t>& taken, double dpi, uint32_t log2s, const FallbackSwitches& sw)
{
    SubpassPlan s; const uint64_t per_sub = (1ull << log2s) / 2;
    for (size_t i = 0; i < singles.size(); ++i) {
        if (taken[i]) continue;
        const uint32_t p = std::max<uint32_t>(1, ceil_log2((distinct_guess(inst[i], dpi) + per_sub - 1) / per_sub));
        if (ceil_log2((inst[i] + per_sub - 1) / per_sub) > MAX_SELECTOR_BITS || p > sw.max_subpass_log2) { s.huge.push_back(singles[i]); continue; }
        for (uint32_t k = 0; k < (1u << p); ++k) { s.items.push_back(singles[i]); s.words.push_back((p << 8) | k); }
    }
    return s;
}

// Sub-passes that overflowed again come back as {bucket, 0x80000000 | word}: each is replaced by its two halves,
// one more selector bit.  Returns false at an entry that cannot be cut (no marker, or all selector bits in use),
// which is then in *bad.
inline bool refine_subpasses(const std::vector<ItemRange>& again, SubpassPlan* next, ItemRange* bad)
{
    next->items.clear(); next->words.clear();
    for (const ItemRange& r : again) {
        const uint32_t w = r.b1 & 0x7FFFFFFFu, p = w >> 8, k = w & 0xFFu;
        if (!(r.b1 & 0x80000000u) || p >= MAX_SELECTOR_BITS) { *bad = r; return false; }
        next->items.push_back(ItemRange{r.b0, r.b0 + 1}); next->words.push_back(((p + 1) << 8) | k);
        next->items.push_back(ItemRange{r.b0, r.b0 + 1}); next->words.push_back(((p + 1) << 8) | (k + (1u << p)));
    }
    return true;
}

// ---- 4. HBM tables
// A table is sized for the distinct k-mers its bucket is expected to hold -- instances x (distinct k-mers per
// instance seen so far, with a margin) -- at load <= 0.5; 2 x instances is the certain bound and costs 56 bytes
// per instance (42 GB for the hot buckets of one pass of a human-scale set with a 10 % repeat family).  An insert
// that runs out of probe steps says the guess was too low: every table is then rebuilt twice as large.
inline double table_distinct_per_inst(double seen) { return seen > 0.0 ? std::min(1.0, std::max(0.05, 1.5 * seen)) : 1.0; }
inline double table_retry_per_inst(double per_inst) { return std::min(1.0, 2.0 * per_inst); }

// words of a slot: keys, state, contexts, counts, barcode words (BigView)
constexpr uint32_t big_slot_words(int kw, int nbc) { return (uint32_t)(kw + 4 + (nbc > 1 ? nbc - 1 : 0)); }

// items[i].tab_off: the table's first word in the pool; slot_pre: n + 1 prefix sums of the tables' slots; words: of the
// whole pool; certain: every table holds its bucket whatever its k-mers
struct BigTables { std::vector<BigItem> items; std::vector<uint64_t> slot_pre; uint64_t words = 0; bool certain = true; };

inline BigTables size_big_tables(const std::vector<ItemRange>& buckets, const std::vector<uint64_t>& inst, double per_inst, uint32_t slot_words)
{
    BigTables t; t.slot_pre.assign(buckets.size() + 1, 0);
    for (size_t i = 0; i < buckets.size(); ++i) {
        const uint64_t guess = std::min<uint64_t>(inst[i], (uint64_t)((double)inst[i] * per_inst) + 256);
        t.certain = t.certain && guess == inst[i];
        const uint32_t l2 = std::max<uint32_t>(BIG_MIN_LOG2S, ceil_log2(2 * guess + 64));
        t.items.push_back(BigItem{buckets[i].b0, buckets[i].b1, t.words, l2, 0});
        t.words += (uint64_t)slot_words << l2;
        t.slot_pre[i + 1] = t.slot_pre[i] + (1ull << l2);
    }
    return t;
}

// n + 1 prefix sums of the chunks (COUNT_CHUNK records) of every bucket: the tickets k_hot_pass and k_big_insert draw
inline std::vector<uint64_t> chunk_prefixes(const std::vector<uint64_t>& n_records)
{
    std::vector<uint64_t> pre(n_records.size() + 1, 0);
    for (size_t i = 0; i < n_records.size(); ++i) pre[i + 1] = pre[i] + (n_records[i] + COUNT_CHUNK - 1) / COUNT_CHUNK;
    return pre;
}

// ---- the holes of a part
// The holes are the unused end of every workgroup's last chunk (`chunk` entries each).  Entries beyond
// n_lds = claimed - the holes' total move into the holes below n_lds: afterwards [0, n_lds) is dense.  Entry src[i]
// goes to dst[i]; the two sizes disagree when the workgroups' state and the cursor do.
struct HoleMoves { uint64_t n_lds = 0; std::vector<uint64_t> src, dst; };

inline HoleMoves plan_hole_moves(const std::vector<WgOut>& wg, uint64_t chunk, uint64_t claimed)
{
    std::vector<std::pair<uint64_t, uint64_t>> holes; uint64_t n_holes = 0;
    for (const WgOut& w : wg) if (w.chunk != ~0ull && w.used < chunk) { holes.push_back({w.chunk + w.used, w.chunk + chunk}); n_holes += chunk - w.used; }
    std::sort(holes.begin(), holes.end());
    HoleMoves m; m.n_lds = claimed - n_holes;
    for (const auto& h : holes) for (uint64_t i = h.first; i < std::min(h.second, m.n_lds); ++i) m.dst.push_back(i);
    size_t hi = 0;
    for (uint64_t i = m.n_lds; i < claimed && m.src.size() < m.dst.size(); ++i) {
        while (hi < holes.size() && holes[hi].second <= i) ++hi;
        if (hi < holes.size() && holes[hi].first <= i) i = holes[hi].second - 1;   // skip a hole
        else m.src.push_back(i);
    }
    return m;
}

} // namespace dfk
