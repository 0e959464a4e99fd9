// superplus_amd/csrc/dfk_partners.h -- CloseGap2's search for unplaced partners (10X/Closomatic.cc:554-585): for every pair and
// each of its two closer edges, the forward reads on the edge whose mate is not placed on the other, the mate's 32-mers looked up
// among the 32-mers of the other edge's anchors (bod), the mate kept where all hits agree on one position.  The rule over plain
// arrays, the form the device runs and its plan, the layout of a.close.partners.
//
// No HIP call and no device pointer is dereferenced here by the host, so tests/cpp/test_partners.cc compiles this header with a
// plain host compiler (and once more under -fsanitize=address,undefined) and checks it against cases recorded from
// tests/partners_oracle.py.  It is the SECOND restatement of the rule -- written from the reference's text, not from the Python.
//
// The rule (L = 32; a pair (e1, e2), es = { e1, inv[e2] } (:504), e = es[ei], e' = es[1 - ei]; locs and anchors as dfk_closer.h):
//   ids(e) (:556-561)      the ascending distinct ids of the records of locs(e) with fw true.  A record with fw false does not
//                          count, even when the same id has one.
//   bod(e') (:546-551)     for every anchor ( g, add, count ) of e' and every l in 0 .. bases(g) - L: ( the 32-mer of hb.O(g) at
//                          l, add + l ), the sum an int.  An edge of fewer than 32 bases gives nothing.  UniqueSort (:561)
//                          changes no result below.
//   the search (:562-585)  for ei = 0 then 1, for id1 in ids(e) ascending: id2 = id1 ^ 1 (:565); skip if id2 is in ids(e') (:566:
//                          both sets are those made BEFORE this loop); finds = { pos - l } over every l in 0 .. len(id2) - L of
//                          bases[id2] -- the whole read as the .fastb has it -- and every entry of bod(e') whose 32-mer equals
//                          the read's at l (:574-580); finds.solo( ) (:584): push ( id2, finds[0], True ) onto locs[1 - ei].
//   kmer<32> compares all 32 bases (kmers/KmerRecord.h:719-757): the order of bod does not matter, only equality does.
//   "exactly one distinct value" = "at least one hit, and the least hit equals the greatest".
//   The result of a pair and a side depends on ( e, e' ) alone: ids(e), ids(e'), bod(e').
//
// The packing, stated ONCE and used by the table and by the reads alike: bases are 2 bits each, four a byte, base i of a sequence
// at bits 2 (i & 3) of byte i >> 2 (feudal BaseVec, what a.fastb and frag_reads_orig.fastb hold).  The 32-mer at base l is the
// 64 bits from bit 2 l of the sequence's bytes on: base j of it at bits 2 j of the key.  cut32() reads bytes l >> 2 ..
// ( l + 31 ) >> 2 of the sequence and no other -- the ninth byte only when l & 3 -- so with l + 32 <= len it never leaves the
// ceil(len / 4) bytes of a read or an edge.  All A is key 0, all T is all ones.
//
// The form the device runs (dfk_partners_kernels.h, dfk_partners.inc; partners_plan() below is its order of work on the host):
//   sides      element q = 2 pi + ei; its rank k(q) of e in ce, k(q ^ 1) that of e'.
//   forward    the forward part of locs(e) is pass 1 (dfk_closer.h): the leading records of the rank, ascending by id with
//              repeats; fw_n[k] by a binary search per rank (the flags never rise inside a rank).
//   queries    an ITEM is ( q, j ), j a record of the forward part of k(q).  An item is a query when it heads a run of equal
//              ids and id ^ 1 is not found, by binary search, in the forward part of k(q ^ 1).  The items of a range of sides
//              are flagged, the flags scanned, ( q, id2 ) written at the scanned places: the queries in push order.
//   the table  one entry per ( anchor, l ): ( rank of e' relative to the range, key, add + l ), for a RANGE of ranks whose entries
//              fit the room; sorted by ( rank, key ) with stable radix sorts of a permutation (key low word, key high word,
//              rank), the start of every rank known from the counts.
//   the search the queries whose e' lies in the range and has anchors (the others find nothing: they are counted and stay on the
//              host), a BATCH at a time: the host gathers the bases of the batch's reads (only those cross to the device), a wave
//              takes a query, lane i the positions l = i, i + 64, ...; each cuts the key,
//              finds the equal range in the rank's slice, folds pos - l of every hit into a minimum, a maximum and a flag; a wave
//              reduction gives the query's three; kept iff hit and minimum == maximum.  The kept flags are scanned and
//              ( query, pos ) written at the scanned places.
//   Every place in an output comes from a scan or a stable sort; the only atomics add integers (two counters).
//
// The file (dfk_partners_write).  Numbers are little-endian.
//   a.close.partners   "DFKCPRT1" | u64 n = 2 * n_pairs | (n + 1) x u64 starts | starts[n] 16-byte records { i64 id, i32 pos,
//                      u32 fw = 1 } -- the locs record of a.close.locs.  Element 2 pi + ei is what the loop for ei of pair pi
//                      pushes onto locs[1 - ei], in push order; the pairs in the order given.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DFK_PT_HD __host__ __device__ inline
#else
#define DFK_PT_HD inline
#endif

namespace dfk_partners {

constexpr uint32_t L = 32;                         // Closomatic.cc:499
constexpr uint64_t SALT = 0xDDDDull;               // k_digest_seq's, over the records as u64 words, two a record

// the 32-mer at base l of a packed sequence (see the packing above); the caller has l + 32 <= the sequence's bases
DFK_PT_HD uint64_t cut32(const uint8_t* p, uint32_t l)
{
    const uint8_t* b = p + (l >> 2);
    uint64_t x = 0;
    for (int i = 0; i < 8; ++i) x |= (uint64_t)b[i] << (8 * i);
    const uint32_t s = 2 * (l & 3);
    if (s) x = (x >> s) | ((uint64_t)b[8] << (64 - s));
    return x;
}
DFK_PT_HD uint32_t positions(uint32_t len) { return len >= L ? len - L + 1 : 0; }        // the l of a sequence: 0 .. len - L
DFK_PT_HD int32_t find_of(int32_t pos, uint32_t l) { return (int32_t)((uint32_t)pos - l); }   // :580 (unsigned: no trap where an int would wrap)
DFK_PT_HD int32_t entry_pos(int32_t add, uint32_t l) { return (int32_t)((uint32_t)add + l); } // :550
DFK_PT_HD bool loc_fw(const uint64_t* locs, uint64_t i) { return ((locs[2 * i + 1] >> 32) & 1u) != 0; }
DFK_PT_HD uint64_t loc_id(const uint64_t* locs, uint64_t i) { return locs[2 * i]; }

// the first of the sorted keys [lo, hi) that is not below x
DFK_PT_HD uint64_t lower_key(const uint64_t* keys, uint64_t lo, uint64_t hi, uint64_t x)
{
    while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (keys[mid] < x) lo = mid + 1; else hi = mid; }
    return lo;
}
// whether id is among the ids of the records [lo, hi), ascending by id
DFK_PT_HD bool has_id(const uint64_t* locs, uint64_t lo, uint64_t hi, uint64_t id)
{
    const uint64_t end = hi;
    while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (loc_id(locs, mid) < id) lo = mid + 1; else hi = mid; }
    return lo < end && loc_id(locs, lo) == id;
}
// the number of leading records of [lo, hi) with fw true, the flags never rising
DFK_PT_HD uint64_t forward_count(const uint64_t* locs, uint64_t lo, uint64_t hi)
{
    const uint64_t lo0 = lo;
    while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (loc_fw(locs, mid)) lo = mid + 1; else hi = mid; }
    return lo - lo0;
}
// the last i in [0, n) with first[i] <= x, first ascending with first[0] <= x
DFK_PT_HD uint64_t owner_of(const uint64_t* first, uint64_t n, uint64_t x)
{
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) { const uint64_t mid = lo + (hi - lo) / 2; if (first[mid] <= x) lo = mid; else hi = mid; }
    return lo;
}
// one lane's fold of a hit, and two lanes' folds joined
struct Fold { int32_t lo, hi; uint32_t hit; };
DFK_PT_HD void fold_hit(Fold& f, int32_t v) { if (!f.hit) { f.lo = f.hi = v; f.hit = 1; } else { if (v < f.lo) f.lo = v; if (v > f.hi) f.hi = v; } }
DFK_PT_HD Fold fold_join(const Fold& a, const Fold& b)
{
    if (!a.hit) return b;
    if (!b.hit) return a;
    return Fold{a.lo < b.lo ? a.lo : b.lo, a.hi > b.hi ? a.hi : b.hi, 1u};
}
// what one lane of the wave finds of a read against a rank's sorted slice [t0, t1): positions l = lane, lane + 64, ...
DFK_PT_HD Fold search_lane(const uint8_t* read, uint32_t len, uint32_t lane, const uint64_t* keys, const int32_t* pos, uint64_t t0, uint64_t t1)
{
    Fold f{0, 0, 0u};
    for (uint32_t l = lane; l + L <= len; l += 64) {
        const uint64_t x = cut32(read, l);
        for (uint64_t m = lower_key(keys, t0, t1, x); m < t1 && keys[m] == x; ++m) fold_hit(f, find_of(pos[m], l));
    }
    return f;
}
// a query's status from its fold
enum : uint32_t { Q_NONE = 0, Q_KEPT = 1, Q_MULTI = 2 };
DFK_PT_HD uint32_t status_of(const Fold& f) { return !f.hit ? Q_NONE : f.lo == f.hi ? Q_KEPT : Q_MULTI; }

} // namespace dfk_partners

// ---------------------------------------------------------------------------------------------------------------- host only
#include <algorithm>
#include <utility>
#include <vector>
#include "dfk_paths_plan.h"   // pidx_next_range, pidx_key_bits, prefix_sums

namespace dfk_partners {

struct Rec { int64_t id; int32_t pos; uint32_t fw; };
static_assert(sizeof(Rec) == 16, "a.close.partners record");

// everything as plain arrays: the graph, the closer's tables in dfk_closer_fetch's forms, the reads
struct Input {
    uint64_t n_edges; const int32_t* inv;
    const uint8_t* edge_packed; const uint64_t* edge_off /* [E + 1], bytes */; const uint32_t* edge_len /* [E], bases */;
    uint64_t n_ce; const uint64_t* ce; const uint64_t* loc_first; const uint64_t* locs /* two words a record */; const uint64_t* anchor_first; const int32_t* anchors /* three a record */;
    uint64_t n_reads; const uint8_t* read_packed; const uint64_t* read_off /* [N + 1], bytes */; const uint32_t* read_len;
};

struct HostResult {
    std::vector<uint64_t> starts;                  // [2 * n_pairs + 1]
    std::vector<Rec> recs;
    uint64_t queries = 0, positions = 0, entries = 0, any_hit = 0, kept = 0, multi = 0, batches = 0, ranges = 0;
    uint64_t searched = 0;                         // the queries against a bod that is not empty: only those cross to the device
};

// the rank of edge e in ce, or n_ce
inline uint64_t rank_in(const uint64_t* ce, uint64_t n_ce, uint64_t e)
{
    const uint64_t k = (uint64_t)(std::lower_bound(ce, ce + n_ce, e) - ce);
    return k < n_ce && ce[k] == e ? k : n_ce;
}
// the ranks of the sides: side_rank[2 pi + ei] = rank of es[ei].  -1: a pair names an edge outside [0, E); -2: a closer edge of
// a pair is not in ce
inline int side_ranks(const Input& I, const int32_t* pairs, uint64_t n_pairs, std::vector<uint32_t>* side_rank)
{
    side_rank->assign(2 * n_pairs, 0);
    for (uint64_t i = 0; i < 2 * n_pairs; ++i) if (pairs[i] < 0 || (uint64_t)pairs[i] >= I.n_edges) return -1;
    for (uint64_t pi = 0; pi < n_pairs; ++pi) {
        const uint64_t es[2] = {(uint64_t)pairs[2 * pi], (uint64_t)I.inv[pairs[2 * pi + 1]]};    // :504
        for (int ei = 0; ei < 2; ++ei) {
            const uint64_t k = rank_in(I.ce, I.n_ce, es[ei]);
            if (k == I.n_ce) return -2;
            (*side_rank)[2 * pi + ei] = (uint32_t)k;
        }
    }
    return 0;
}
// the entries an anchor gives: the l of its edge
inline uint64_t anchor_entries(const Input& I, uint64_t a) { return positions(I.edge_len[I.anchors[3 * a]]); }

// ---- the literal transcription for one pair: the loops of Closomatic.cc:546-551 and :556-585 as they stand.  out[ei]: what the loop
// for ei pushes onto locs[1 - ei].  The pair's closer edges are in ce (side_ranks).
inline void pair_literal(const Input& I, int32_t e1, int32_t e2, std::vector<Rec> out[2], HostResult* counters)
{
    const uint64_t es[2] = {(uint64_t)e1, (uint64_t)I.inv[e2]};                                  // :504
    std::vector<std::pair<uint64_t, int>> bod[2];                                                // :506
    std::vector<int64_t> ids[2];                                                                 // :556
    for (int ei = 0; ei < 2; ++ei) {
        const uint64_t k = rank_in(I.ce, I.n_ce, es[ei]);
        for (uint64_t a = I.anchor_first[k]; a < I.anchor_first[k + 1]; ++a) {                  // :542-551: the anchors are the kept runs of prec
            const int g = I.anchors[3 * a];
            const uint8_t* E = I.edge_packed + I.edge_off[g];                                    // :546
            for (int l = 0; l <= (int)I.edge_len[g] - (int)L; l++)                               // :547
                bod[ei].emplace_back(cut32(E, (uint32_t)l), entry_pos(I.anchors[3 * a + 1], (uint32_t)l));   // :548-551
        }
        for (uint64_t j = I.loc_first[k]; j < I.loc_first[k + 1]; ++j) {                        // :558
            if (!loc_fw(I.locs, j)) continue;                                                    // :559
            ids[ei].push_back((int64_t)loc_id(I.locs, j));                                       // :560
        }
        std::sort(ids[ei].begin(), ids[ei].end()); ids[ei].erase(std::unique(ids[ei].begin(), ids[ei].end()), ids[ei].end());   // :561
        std::sort(bod[ei].begin(), bod[ei].end()); bod[ei].erase(std::unique(bod[ei].begin(), bod[ei].end()), bod[ei].end());
    }
    for (int ei = 0; ei < 2; ++ei) {                                                             // :562
        for (size_t j = 0; j < ids[ei].size(); ++j) {                                            // :563
            const int64_t id1 = ids[ei][j];
            const int64_t id2 = id1 % 2 == 0 ? id1 + 1 : id1 - 1;                                // :565
            if (std::binary_search(ids[1 - ei].begin(), ids[1 - ei].end(), id2)) continue;       // :566
            const uint8_t* b = I.read_packed + I.read_off[id2];                                  // :572
            const int blen = (int)I.read_len[id2];
            std::vector<int> finds;                                                              // :573
            const auto& B = bod[1 - ei];
            ++counters->queries;
            if (!B.empty()) ++counters->searched;
            for (int l = 0; l <= blen - (int)L; l++) {                                           // :574
                const uint64_t x = cut32(b, (uint32_t)l);                                        // :575-576
                ++counters->positions;
                const auto low = std::lower_bound(B.begin(), B.end(), x, [](const std::pair<uint64_t, int>& p, uint64_t v) { return p.first < v; });       // :577
                const auto high = std::upper_bound(B.begin(), B.end(), x, [](uint64_t v, const std::pair<uint64_t, int>& p) { return v < p.first; });     // :578
                for (auto m = low; m < high; ++m) finds.push_back(find_of(m->second, (uint32_t)l));                                                       // :579-580
            }
            std::sort(finds.begin(), finds.end()); finds.erase(std::unique(finds.begin(), finds.end()), finds.end());   // :581
            if (!finds.empty()) ++counters->any_hit;
            if (finds.size() == 1) { out[ei].push_back(Rec{id2, finds[0], 1u}); ++counters->kept; }                     // :584-585
            else if (!finds.empty()) ++counters->multi;
        }
    }
}

// -1, -2: side_ranks'
inline int partners_literal(const Input& I, const int32_t* pairs, uint64_t n_pairs, HostResult* R)
{
    std::vector<uint32_t> side_rank;
    if (int rc = side_ranks(I, pairs, n_pairs, &side_rank)) return rc;
    R->starts.assign(1, 0);
    for (uint64_t pi = 0; pi < n_pairs; ++pi) {
        std::vector<Rec> out[2];
        pair_literal(I, pairs[2 * pi], pairs[2 * pi + 1], out, R);
        for (int ei = 0; ei < 2; ++ei) { R->recs.insert(R->recs.end(), out[ei].begin(), out[ei].end()); R->starts.push_back(R->recs.size()); }
    }
    for (uint64_t a = 0; a < I.anchor_first[I.n_ce]; ++a) R->entries += anchor_entries(I, a);
    return 0;
}

// ---- the plan
// Queries are found a range of SIDES at a time: as many sides as keep their items (the forward records of their ranks) at the cap;
// an item costs its flag and its place (two u64) and, while they are written, a query's two words.
constexpr uint64_t BYTES_PER_ITEM = 24;
inline uint64_t item_cap(uint64_t free_now, uint64_t forced) { return forced ? forced : std::max<uint64_t>(1ull << 18, free_now / 2 / BYTES_PER_ITEM); }
// The table is built a range of ce RANKS at a time: as many ranks as keep the entries at the cap (DFK_PIDX_RANGE_PAIRS forces small
// ranges).  An entry is at most 64 bytes while its range is sorted: the key's two words, pos and rank, two key and two value
// buffers of the sort, the sorted key and pos.  ok = false: one rank alone has 2^32 entries or more (a table of 64 GB for one
// edge; the sort keeps 32-bit places).
constexpr uint64_t BYTES_PER_ENTRY = 64;
inline uint64_t range_cap(uint64_t free_now, uint64_t range_pairs_switch) { return range_pairs_switch ? range_pairs_switch : std::max<uint64_t>(1ull << 18, free_now / 2 / BYTES_PER_ENTRY); }
inline dfk::PidxRange next_range(const uint64_t* first, uint64_t n, uint64_t k0, uint64_t cap) { return dfk::pidx_next_range(first, n, k0, cap); }
inline uint32_t bits_for(uint64_t n_values) { return dfk::pidx_key_bits(n_values); }
// A batch of queries: a query costs its fixed words (where its bases start, their count, its side, its status, pos, flag, place
// and output: 56 bytes, 64 with slack) and the bytes of its read.  cost_first: the prefix sums of the costs.  A batch holds
// `forced` queries, or with forced == 0 as many as keep the cost at `room`, one at least.
constexpr uint64_t BYTES_PER_QUERY = 64;
inline uint64_t query_cost(uint32_t len) { return BYTES_PER_QUERY + (len + 3) / 4; }
inline uint64_t batch_room(uint64_t free_now) { return std::max<uint64_t>(1ull << 20, free_now / 2); }
inline uint64_t next_batch(const uint64_t* cost_first, uint64_t n, uint64_t b0, uint64_t room, uint64_t forced)
{
    if (forced) return std::min(n, b0 + forced);
    uint64_t b1 = b0 + 1;
    while (b1 < n && cost_first[b1 + 1] - cost_first[b0] <= room) ++b1;
    return b1;
}

struct Query { uint32_t side; uint32_t id2; };

// the queries of the sides [q0, q1) in push order: what the flag kernel, the scan and the emit kernel give together
inline void queries_of(const Input& I, const std::vector<uint32_t>& side_rank, const std::vector<uint64_t>& fw_n, uint64_t q0, uint64_t q1, std::vector<Query>* out)
{
    std::vector<uint64_t> item_first(1, 0);
    for (uint64_t q = q0; q < q1; ++q) item_first.push_back(item_first.back() + fw_n[side_rank[q]]);
    const uint64_t n_items = item_first.back();
    std::vector<uint64_t> flag(n_items + 1, 0);
    for (uint64_t i = 0; i < n_items; ++i) {                                                     // (a thread an item)
        const uint64_t s = owner_of(item_first.data(), q1 - q0, i), q = q0 + s;
        const uint64_t k = side_rank[q], ko = side_rank[q ^ 1], r = I.loc_first[k] + (i - item_first[s]);
        const uint64_t id1 = loc_id(I.locs, r);
        const bool head = r == I.loc_first[k] || loc_id(I.locs, r - 1) != id1;
        flag[i] = head && !has_id(I.locs, I.loc_first[ko], I.loc_first[ko] + fw_n[ko], id1 ^ 1) ? 1u : 0u;
    }
    uint64_t at = out->size();
    std::vector<uint64_t> place(n_items + 1, 0);
    for (uint64_t i = 0; i < n_items; ++i) place[i + 1] = place[i] + flag[i];                    // (the scan)
    out->resize(at + place[n_items]);
    for (uint64_t i = 0; i < n_items; ++i) {
        if (!flag[i]) continue;
        const uint64_t s = owner_of(item_first.data(), q1 - q0, i), q = q0 + s;
        (*out)[at + place[i]] = Query{(uint32_t)q, (uint32_t)(loc_id(I.locs, I.loc_first[side_rank[q]] + (i - item_first[s])) ^ 1)};
    }
}

// The device version's order of work on the host, for the CPU test.  queries_per_batch 0 = what fits `room`; -3: a rank alone has
// 2^32 entries
inline int partners_plan(const Input& I, const int32_t* pairs, uint64_t n_pairs, uint64_t queries_per_batch, uint64_t room, uint64_t table_cap, uint64_t items_cap, HostResult* R)
{
    std::vector<uint32_t> side_rank;
    if (int rc = side_ranks(I, pairs, n_pairs, &side_rank)) return rc;
    const uint64_t n_sides = 2 * n_pairs, n_ce = I.n_ce;
    std::vector<uint64_t> fw_n(n_ce), ent_n(n_ce, 0);
    for (uint64_t k = 0; k < n_ce; ++k) {
        fw_n[k] = forward_count(I.locs, I.loc_first[k], I.loc_first[k + 1]);
        for (uint64_t a = I.anchor_first[k]; a < I.anchor_first[k + 1]; ++a) ent_n[k] += anchor_entries(I, a);
    }
    const std::vector<uint64_t> tfirst = dfk::prefix_sums(ent_n.data(), n_ce);
    R->entries = tfirst[n_ce];
    // the queries, a range of sides at a time
    std::vector<uint64_t> side_items(n_sides);
    for (uint64_t q = 0; q < n_sides; ++q) side_items[q] = fw_n[side_rank[q]];
    const std::vector<uint64_t> ifirst = dfk::prefix_sums(side_items.data(), n_sides);
    std::vector<Query> Q;
    for (uint64_t q0 = 0; q0 < n_sides;) { const uint64_t q1 = next_range(ifirst.data(), n_sides, q0, items_cap).e1; queries_of(I, side_rank, fw_n, q0, q1, &Q); q0 = q1; }
    R->queries = Q.size();
    std::vector<uint32_t> status(Q.size(), Q_NONE); std::vector<int32_t> found(Q.size(), 0);
    // the table a range of ranks at a time; under each the batches of the queries whose e' lies in it
    for (uint64_t k0 = 0; k0 < n_ce;) {
        const dfk::PidxRange range = next_range(tfirst.data(), n_ce, k0, table_cap);
        if (!range.ok) return -3;
        const uint64_t k1 = range.e1, n_t = range.n;
        ++R->ranges;
        struct Ent { uint32_t rank; uint64_t key; int32_t pos; };
        std::vector<Ent> T; T.reserve(n_t);
        for (uint64_t k = k0; k < k1; ++k)
            for (uint64_t a = I.anchor_first[k]; a < I.anchor_first[k + 1]; ++a)
                for (uint32_t l = 0; l < anchor_entries(I, a); ++l)
                    T.push_back(Ent{(uint32_t)(k - k0), cut32(I.edge_packed + I.edge_off[I.anchors[3 * a]], l), entry_pos(I.anchors[3 * a + 1], l)});
        std::stable_sort(T.begin(), T.end(), [](const Ent& a, const Ent& b) { return a.rank != b.rank ? a.rank < b.rank : a.key < b.key; });
        std::vector<uint64_t> keys(T.size() + 1, 0); std::vector<int32_t> pos(T.size() + 1, 0);
        for (size_t i = 0; i < T.size(); ++i) { keys[i] = T[i].key; pos[i] = T[i].pos; }
        std::vector<uint64_t> sel;                                                               // the queries of this range, in query order
        for (uint64_t i = 0; i < Q.size(); ++i) {                                                // (a query against an empty slice finds nothing: it is counted and stays on the host)
            const uint64_t ko = side_rank[Q[i].side ^ 1];
            if (ko < k0 || ko >= k1) continue;
            if (tfirst[ko + 1] == tfirst[ko]) R->positions += positions(I.read_len[Q[i].id2]); else sel.push_back(i);
        }
        R->searched += sel.size();
        std::vector<uint64_t> cost(sel.size());
        for (size_t i = 0; i < sel.size(); ++i) cost[i] = query_cost(I.read_len[Q[sel[i]].id2]);
        const std::vector<uint64_t> cfirst = dfk::prefix_sums(cost.data(), cost.size());
        for (uint64_t b0 = 0; b0 < sel.size();) {
            const uint64_t b1 = next_batch(cfirst.data(), sel.size(), b0, room, queries_per_batch);
            ++R->batches;
            // the gather: the batch's reads one behind the other, the last ending at the buffer's end
            std::vector<uint8_t> bases; std::vector<uint64_t> off;
            for (uint64_t i = b0; i < b1; ++i) {
                const uint64_t id2 = Q[sel[i]].id2, nb = ((uint64_t)I.read_len[id2] + 3) / 4;
                off.push_back(bases.size());
                bases.insert(bases.end(), I.read_packed + I.read_off[id2], I.read_packed + I.read_off[id2] + nb);
            }
            std::vector<uint8_t> exact(bases);                                                  // (capacity == size: a read past the end is the sanitizer's to see)
            exact.shrink_to_fit();
            for (uint64_t i = b0; i < b1; ++i) {                                                 // (a wave a query)
                const Query& q = Q[sel[i]];
                const uint64_t ko = side_rank[q.side ^ 1];
                const uint32_t len = I.read_len[q.id2];
                R->positions += positions(len);
                Fold f{0, 0, 0u};
                for (uint32_t lane = 0; lane < 64; ++lane)
                    f = fold_join(f, search_lane(exact.data() + off[i - b0], len, lane, keys.data(), pos.data(), tfirst[ko] - tfirst[k0], tfirst[ko + 1] - tfirst[k0]));
                status[sel[i]] = status_of(f); found[sel[i]] = f.lo;
            }
            b0 = b1;
        }
        k0 = k1;
    }
    // the records in query order, the starts per side
    R->starts.assign(n_sides + 1, 0);
    for (uint64_t i = 0; i < Q.size(); ++i) {
        R->any_hit += status[i] != Q_NONE; R->multi += status[i] == Q_MULTI;
        if (status[i] != Q_KEPT) continue;
        R->recs.push_back(Rec{(int64_t)Q[i].id2, found[i], 1u}); ++R->starts[Q[i].side + 1];
    }
    for (uint64_t q = 0; q < n_sides; ++q) R->starts[q + 1] += R->starts[q];
    R->kept = R->recs.size();
    return 0;
}

// ---- the file's fixed parts
constexpr const char* MAGIC = "DFKCPRT1";
inline uint64_t records_at(uint64_t n) { return 16 + 8 * (n + 1); }
inline uint64_t file_size(uint64_t n, uint64_t n_records) { return records_at(n) + 16 * n_records; }

} // namespace dfk_partners
