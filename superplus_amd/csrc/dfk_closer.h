// superplus_amd/csrc/dfk_closer.h -- the front end the two gap closers share (CloseGap2, 10X/Closomatic.cc:503-552; Stackster,
// 10X/Stackster.cc:289-324): per closer edge, where the reads lie (locs), which edges follow often enough (anchors), and which
// reads the stacks will want (reads).  The rule over plain arrays, the plan of the device version, the layouts of a.close.*.
//
// No HIP call and no device pointer is dereferenced here by the host, so tests/cpp/test_closer.cc compiles this header with a
// plain host compiler (and once more under -fsanitize=address,undefined) and checks it against cases recorded from
// tests/closer_oracle.py.  It is the SECOND restatement of the rule -- written from the reference's text, not from the Python.
//
// The rule (E edges, N reads, N even, the mate of id = id ^ 1, kmers(x) the edge's k-mer count, off(id) the path's offset word,
// list(f) = a.paths.inv's element of f: read ids ascending, a read that holds f m times listed m times):
//   closer edges           ce = the ascending distinct values of {p.first, inv[p.second]} over the pairs p: CloseGap2 works
//                          es = { e1, inv[e2] } (Closomatic.cc:503-504), Stackster e = ( spass == 1 ? e1 : inv[e2] ) (Stackster.cc:296)
//   locs(e) (:507-535)     for pass 1 then 2, f = ( pass == 1 ? e : inv[e] ) (:512); for i over list(f) (:513); for j ascending with
//                          p[j] == f (:517-518): ( id, pos, pass == 1 ) (:534-535) with pos = off(id) - sum_{l<j} kmers(p[l])
//                          (:531-533), an int.  No duplicate filter.  A read on f m times is listed m times and gives its m
//                          occurrences each time: m x m records.  A self-inverse e has f = e in both passes: every read twice.
//   anchors(e) (:509-552)  prec is filled beside every record above.  Pass 1 (:520-524): for l = j + 1 .. n - 1 the pair
//                          ( p[l], sum_{t=j}^{l-1} kmers(p[t]) ); pass 2 (:526-530): for l = j - 1 .. 0 the pair
//                          ( inv[p[l]], sum_{t=l+1}^{j} kmers(p[t]) ).  Sort(prec) (:536); a run of equal pairs of length
//                          j - i >= MIN_EDGE_COUNT = 5 (:498, :542) is an anchor ( g, add, count ), ascending by g then add.  The
//                          32-mers of bod (:546-551) follow from hb.O(g) and are the consumer's.
//   reads(e) (Stackster.cc:289-324, ALT = False)   Stackster's idsfw for spass == 1 with e1 = e:
//                          ( id, true ) for id in list(e), ( id, false ) for id in list(inv[e]) (:298-309: spass == 1 ^ pass == 2);
//                          for id1 in list(e), each j with p1[j] == e (:316-317) and kmers[e] + K - 1 - pos1 <= MAX_DIST = 800
//                          (:321; pos1 by :318-320, the pos above): ( id1 ^ 1, false ) (:314, :322: spass == 2 is false).  dup[id/2]
//                          and dup[id1/2] skip (:302, :313).  The mate's own path is never read: an unplaced mate enters.
//                          Sorted and distinct (:324 UniqueSort), ( id, false ) < ( id, true ).
//   a pair                 for spass == 2, e = inv[e2], :309 pushes spass == 1 ^ pass == 2 = ( pass == 2 ): true for list(inv[e]),
//                          false for list(e) -- the flags of reads(inv[e2]) negated -- and :322 pushes ( id2, spass == 2 ) =
//                          ( id2, true ), the negation again.  So idsfw( e1, e2 ) = reads(e1) U { ( id, !fw ) : ( id, fw ) in
//                          reads(inv[e2]) }, and locs / bod of a pair are those of es[0] = e1 and es[1] = inv[e2].
//
// The files (dfk_closer_write).  Numbers are little-endian.
//   a.close.edges    "BINWRITE" | u64 n | n x u64: ce
//   the three tables share one format: magic[8] | u64 n | (n + 1) x u64 starts | starts[n] records.  Element k (the records
//   [starts[k], starts[k + 1])) belongs to ce[k].
//   a.close.locs     magic "DFKCLOC1", 16-byte records { i64 id, i32 pos, u32 fw }
//   a.close.anchors  magic "DFKCANC1", 12-byte records { i32 g, i32 add, i32 count }
//   a.close.reads    magic "DFKCRDS1",  8-byte records u64 id << 1 | fw
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DFK_CLOSER_HD __host__ __device__ inline
#else
#define DFK_CLOSER_HD inline
#endif

namespace dfk_closer {

constexpr int32_t MIN_EDGE_COUNT = 5;             // Closomatic.cc:498
constexpr int32_t MAX_DIST = 800;                 // Stackster.cc:292
constexpr uint32_t MARK_WORD_BITS = 32;           // the marks are dfk_subset's bit set
constexpr uint64_t SALT_EDGES = 0x9999ull, SALT_LOCS = 0xAAAAull, SALT_ANCHORS = 0xBBBBull, SALT_READS = 0xCCCCull;   // k_digest_seq's

DFK_CLOSER_HD bool marked(const uint32_t* marks, uint32_t e) { return (marks[e / MARK_WORD_BITS] >> (e % MARK_WORD_BITS)) & 1u; }

// the packed words
DFK_CLOSER_HD uint32_t loc_key(uint32_t k_rel, uint32_t pass /* 0, 1 */) { return 2 * k_rel + pass; }    // the sort key of a record: rank, then pass
DFK_CLOSER_HD uint64_t loc_word1(int32_t pos, bool fw) { return (uint64_t)(uint32_t)pos | ((uint64_t)(fw ? 1u : 0u) << 32); }   // bytes 8..15 of a locs record
DFK_CLOSER_HD uint32_t read_word(uint64_t id, bool fw) { return (uint32_t)(id << 1) | (fw ? 1u : 0u); }  // id < 2^31: the sort key of a set entry
DFK_CLOSER_HD bool mate_within(int32_t kmers_e, int32_t K, int32_t pos1) { return !((int64_t)kmers_e + K - 1 - pos1 > MAX_DIST); }  // :321 (64-bit: no wrap)

// what the sweep reads of the graph and of the closer edges
struct Tables { const uint32_t* marks; const uint32_t* rank_of; const int32_t* inv; const int32_t* kmers; };

// One read against the closer edges of ranks [k0, k1), in the order the device emits: path positions t ascending -- the t-th
// entry of the read in list(p[t]) -- then pass, then the occurrences j of p[t] ascending.  For one (rank, pass) the edge f is
// fixed, so a read's records come as its m list entries, each with all m occurrences: the reference's order inside a read.
// Reads ascending and a stable sort by (rank, pass) then give the reference's order overall.
//   s.entry(k, pass, dup)      a list entry of list(f), f = (pass ? inv[ce[k]] : ce[k])
//   s.loc(k, pass, pos)        a locs record
//   s.prec(k, g, add)          a prec tuple
//   s.mate(k, taken)           a mate tested against MAX_DIST (pass 0 only, never for a duplicate)
template <class Sink>
DFK_CLOSER_HD void walk_read(const uint32_t* path, uint32_t n, int32_t off, bool dup, const Tables& T, uint32_t k0, uint32_t k1, int32_t K, Sink& s)
{
    for (uint32_t t = 0; t < n; ++t) {
        const uint32_t f = path[t];
        for (uint32_t pass = 0; pass < 2; ++pass) {
            const uint32_t x = pass ? (uint32_t)T.inv[f] : f;
            if (!marked(T.marks, x)) continue;
            const uint32_t k = T.rank_of[x];
            if (k < k0 || k >= k1) continue;
            s.entry(k, pass, dup);
            uint32_t pos = (uint32_t)off;                                       // (unsigned: the reference's int may wrap, this must not trap)
            for (uint32_t j = 0; j < n; pos -= (uint32_t)T.kmers[path[j]], ++j) {
                if (path[j] != f) continue;
                s.loc(k, pass, (int32_t)pos);
                uint32_t add = 0;
                if (!pass) for (uint32_t l = j + 1; l < n; ++l) { add += (uint32_t)T.kmers[path[l - 1]]; s.prec(k, (int32_t)path[l], (int32_t)add); }
                else for (uint32_t l = j; l-- > 0;) { add += (uint32_t)T.kmers[path[l + 1]]; s.prec(k, T.inv[path[l]], (int32_t)add); }
                if (!pass && !dup) s.mate(k, mate_within(T.kmers[f], K, (int32_t)pos));
            }
        }
    }
}

} // namespace dfk_closer

// ---------------------------------------------------------------------------------------------------------------- host only
#include <algorithm>
#include <utility>
#include <vector>
#include "dfk_paths_plan.h"   // pidx_range_cap / pidx_next_range, grid_256, prefix_sums

namespace dfk_closer {

struct Loc { int64_t id; int32_t pos; uint32_t fw; };
struct Anchor { int32_t g, add, count; };
static_assert(sizeof(Loc) == 16 && sizeof(Anchor) == 12, "a.close.* records");

struct EdgeResult {
    std::vector<Loc> locs; std::vector<Anchor> anchors; std::vector<uint64_t> reads;    // reads: id << 1 | fw, ascending
    uint64_t prec = 0, mates_in = 0, mates_out = 0, dup_skipped = 0;
};

// the graph and the paths as the literal transcription reads them: paths as a CSR, the index as a CSR of read ids per edge
struct Input {
    uint64_t n_edges; const int32_t* inv; const int32_t* kmers; int32_t K;
    uint64_t n_reads; const uint64_t* first; const int32_t* edges; const int32_t* offsets; const uint8_t* dup;
    const uint64_t* idx_first; const uint64_t* idx_ids;
};

// the index (writePathsIndex: (edge, read) pairs sorted, duplicates kept)
inline void build_index(uint64_t n_edges, uint64_t n_reads, const uint64_t* first, const int32_t* edges, std::vector<uint64_t>* idx_first, std::vector<uint64_t>* idx_ids)
{
    std::vector<uint64_t> counts(n_edges, 0);
    for (uint64_t k = 0; k < first[n_reads]; ++k) ++counts[edges[k]];
    *idx_first = dfk::prefix_sums(counts.data(), n_edges);
    idx_ids->assign(first[n_reads], 0);
    std::vector<uint64_t> at(idx_first->begin(), idx_first->end() - 1);
    for (uint64_t id = 0; id < n_reads; ++id) for (uint64_t k = first[id]; k < first[id + 1]; ++k) (*idx_ids)[at[edges[k]]++] = id;
}

// ce (:503-504 / Stackster.cc:296).  -1: a pair names an edge outside [0, E)
inline int closer_edges(const int32_t* pairs, uint64_t n_pairs, const int32_t* inv, uint64_t n_edges, std::vector<uint64_t>* ce)
{
    for (uint64_t i = 0; i < 2 * n_pairs; ++i) if (pairs[i] < 0 || (uint64_t)pairs[i] >= n_edges) return -1;
    for (uint64_t i = 0; i < n_pairs; ++i) { ce->push_back((uint64_t)pairs[2 * i]); ce->push_back((uint64_t)inv[pairs[2 * i + 1]]); }
    std::sort(ce->begin(), ce->end());
    ce->erase(std::unique(ce->begin(), ce->end()), ce->end());
    return 0;
}

// the literal transcription for one edge: the loops of Closomatic.cc:509-552 and Stackster.cc:298-322 as they stand
inline EdgeResult edge_literal(const Input& I, int32_t e)
{
    EdgeResult R;
    std::vector<std::pair<int32_t, int32_t>> prec;                              // :509
    auto path_of = [&](uint64_t id) { return I.edges + I.first[id]; };
    auto len_of = [&](uint64_t id) { return (int)(I.first[id + 1] - I.first[id]); };
    for (int pass = 1; pass <= 2; ++pass) {                                     // :511
        const int32_t f = pass == 1 ? e : I.inv[e];                             // :512
        for (uint64_t i = I.idx_first[f]; i < I.idx_first[f + 1]; ++i) {        // :513
            const int64_t id = (int64_t)I.idx_ids[i];
            const int32_t* p = path_of((uint64_t)id);
            const int n = len_of((uint64_t)id);
            for (int j = 0; j < n; ++j) {
                if (p[j] != f) continue;                                        // :518
                if (pass == 1) { uint32_t add = 0; for (int l = j + 1; l < n; ++l) { add += (uint32_t)I.kmers[p[l - 1]]; prec.emplace_back(p[l], (int32_t)add); } }
                else { uint32_t add = 0; for (int l = j - 1; l >= 0; --l) { add += (uint32_t)I.kmers[p[l + 1]]; prec.emplace_back(I.inv[p[l]], (int32_t)add); } }
                uint32_t pos = (uint32_t)I.offsets[id];                         // :531
                for (int l = 0; l < j; ++l) pos -= (uint32_t)I.kmers[p[l]];
                R.locs.push_back(Loc{id, (int32_t)pos, pass == 1 ? 1u : 0u});   // :534-535
            }
        }
    }
    R.prec = prec.size();
    std::sort(prec.begin(), prec.end());                                        // :536
    for (size_t i = 0; i < prec.size();) {
        size_t j = i + 1;
        while (j < prec.size() && prec[j] == prec[i]) ++j;
        if ((int64_t)(j - i) >= MIN_EDGE_COUNT) R.anchors.push_back(Anchor{prec[i].first, prec[i].second, (int32_t)(j - i)});   // :542
        i = j;
    }
    // Stackster.cc:298-322 with spass == 1, e1 = e
    std::vector<uint64_t> idsfw;
    for (int pass = 1; pass <= 2; ++pass) {
        const int32_t f = pass == 1 ? e : I.inv[e];
        for (uint64_t i = I.idx_first[f]; i < I.idx_first[f + 1]; ++i) {
            const uint64_t id = I.idx_ids[i];
            if (I.dup[id / 2]) { ++R.dup_skipped; continue; }                   // :302
            idsfw.push_back(id << 1 | (uint64_t)((1 == 1) ^ (pass == 2)));      // :309
        }
    }
    for (uint64_t i = I.idx_first[e]; i < I.idx_first[e + 1]; ++i) {            // :310
        const uint64_t id1 = I.idx_ids[i];
        if (I.dup[id1 / 2]) continue;                                           // :313
        const uint64_t id2 = id1 % 2 == 0 ? id1 + 1 : id1 - 1;                  // :314
        const int32_t* p1 = path_of(id1);
        for (int j = 0; j < len_of(id1); ++j) {
            if (p1[j] != e) continue;
            uint32_t pos1 = (uint32_t)I.offsets[id1];
            for (int l = 0; l < j; ++l) pos1 -= (uint32_t)I.kmers[p1[l]];
            if (!mate_within(I.kmers[e], I.K, (int32_t)pos1)) { ++R.mates_out; continue; }      // :321
            ++R.mates_in;
            idsfw.push_back(id2 << 1);                                          // :322 (spass == 2 is false)
        }
    }
    std::sort(idsfw.begin(), idsfw.end());                                      // :324
    idsfw.erase(std::unique(idsfw.begin(), idsfw.end()), idsfw.end());
    R.reads = idsfw;
    return R;
}

// Stackster.cc:295-324 for a pair as it stands, both spasses: the sorted distinct ( id << 1 | fw )
inline std::vector<uint64_t> pair_literal(const Input& I, int32_t e1, int32_t e2)
{
    std::vector<uint64_t> idsfw;
    for (int spass = 1; spass <= 2; ++spass) {
        const int32_t e = spass == 1 ? e1 : I.inv[e2];
        for (int pass = 1; pass <= 2; ++pass) {
            const int32_t f = pass == 1 ? e : I.inv[e];
            for (uint64_t i = I.idx_first[f]; i < I.idx_first[f + 1]; ++i) {
                const uint64_t id = I.idx_ids[i];
                if (I.dup[id / 2]) continue;
                idsfw.push_back(id << 1 | (uint64_t)((spass == 1) ^ (pass == 2)));
            }
        }
        for (uint64_t i = I.idx_first[e]; i < I.idx_first[e + 1]; ++i) {
            const uint64_t id1 = I.idx_ids[i];
            if (I.dup[id1 / 2]) continue;
            const uint64_t id2 = id1 ^ 1;
            const int32_t* p1 = I.edges + I.first[id1];
            const int n = (int)(I.first[id1 + 1] - I.first[id1]);
            for (int j = 0; j < n; ++j) {
                if (p1[j] != e) continue;
                uint32_t pos1 = (uint32_t)I.offsets[id1];
                for (int l = 0; l < j; ++l) pos1 -= (uint32_t)I.kmers[p1[l]];
                if (!mate_within(I.kmers[e], I.K, (int32_t)pos1)) continue;
                idsfw.push_back(id2 << 1 | (uint64_t)(spass == 2));
            }
        }
    }
    std::sort(idsfw.begin(), idsfw.end());
    idsfw.erase(std::unique(idsfw.begin(), idsfw.end()), idsfw.end());
    return idsfw;
}
// ... and from the per-edge sets: reads(e1) U { ( id, !fw ) : ( id, fw ) in reads(inv[e2]) }
inline std::vector<uint64_t> pair_composed(const std::vector<uint64_t>& reads_e1, const std::vector<uint64_t>& reads_inv_e2)
{
    std::vector<uint64_t> u(reads_e1);
    for (uint64_t w : reads_inv_e2) u.push_back(w ^ 1);
    std::sort(u.begin(), u.end());
    u.erase(std::unique(u.begin(), u.end()), u.end());
    return u;
}

// the whole result, as the files hold it
struct HostResult {
    std::vector<uint64_t> ce, loc_first, anchor_first, read_first;
    std::vector<Loc> locs; std::vector<Anchor> anchors; std::vector<uint64_t> reads;
    std::vector<uint64_t> weight;                                              // per rank: what the plan sizes ranges by
    uint64_t prec = 0, mates_in = 0, mates_out = 0, dup_skipped = 0;
};

// -1: an edge out of range, -2: N odd, -3: a read id of 2^31 or more
inline int closer_literal(const Input& I, const int32_t* pairs, uint64_t n_pairs, HostResult* R)
{
    if (I.n_reads % 2) return -2;
    if (I.n_reads > (1ull << 31)) return -3;
    if (closer_edges(pairs, n_pairs, I.inv, I.n_edges, &R->ce)) return -1;
    R->loc_first.push_back(0); R->anchor_first.push_back(0); R->read_first.push_back(0);
    for (uint64_t e : R->ce) {
        const EdgeResult r = edge_literal(I, (int32_t)e);
        R->locs.insert(R->locs.end(), r.locs.begin(), r.locs.end());
        R->anchors.insert(R->anchors.end(), r.anchors.begin(), r.anchors.end());
        R->reads.insert(R->reads.end(), r.reads.begin(), r.reads.end());
        R->loc_first.push_back(R->locs.size()); R->anchor_first.push_back(R->anchors.size()); R->read_first.push_back(R->reads.size());
        R->prec += r.prec; R->mates_in += r.mates_in; R->mates_out += r.mates_out; R->dup_skipped += r.dup_skipped;
    }
    return 0;
}

// ---- the plan
// The tables are built a range of ce RANKS at a time.  A rank's weight is everything the sweep emits for it before anything is
// dropped: its locs records, its prec tuples and its set entries (list entries kept plus mates let in).  A range is as many ranks
// as keep the weight at the cap pidx_range_cap gives (DFK_PIDX_RANGE_PAIRS forces small ranges), a quarter of it: a unit of
// weight is at most 80 bytes while its range is sorted (two key and two value buffers, the fields beside them, the records
// formed from them), where an entry of the paths index is 24.  ok = false: one edge alone weighs 2^32 or more.
constexpr uint64_t BYTES_PER_WEIGHT = 80;
inline uint64_t range_cap(uint64_t free_now, uint64_t range_pairs_switch) { return range_pairs_switch ? range_pairs_switch : std::max<uint64_t>(1ull << 18, dfk::pidx_range_cap(free_now, 0) / 4); }
inline dfk::PidxRange next_range(const uint64_t* first, uint64_t n_ce, uint64_t k0, uint64_t cap) { return dfk::pidx_next_range(first, n_ce, k0, cap); }
inline uint64_t count_ranges(const uint64_t* first, uint64_t n_ce, uint64_t cap)
{
    uint64_t n = 0;
    for (uint64_t k0 = 0; k0 < n_ce; ++n) k0 = next_range(first, n_ce, k0, cap).e1;
    return n;
}
inline uint32_t bits_for(uint64_t n_values) { return dfk::pidx_key_bits(n_values); }       // key bits of a sort over values [0, n_values)
inline uint32_t loc_key_bits(uint64_t n_ranks) { return bits_for(2 * n_ranks); }

// The device version's order of work on the host, for the CPU test: reads ascending through walk_read, a stable sort of the
// records by (rank, pass), prec tuples sorted and counted, set entries sorted and made distinct -- a range of ranks at a time.
inline int closer_sweep(const Input& I, const int32_t* pairs, uint64_t n_pairs, uint64_t cap, HostResult* R, uint64_t* n_ranges)
{
    if (I.n_reads % 2) return -2;
    if (I.n_reads > (1ull << 31)) return -3;
    if (closer_edges(pairs, n_pairs, I.inv, I.n_edges, &R->ce)) return -1;
    const uint64_t n_ce = R->ce.size();
    std::vector<uint32_t> marks(std::max<uint64_t>(1, (I.n_edges + 31) / 32), 0u), rank_of(std::max<uint64_t>(1, I.n_edges), 0u);
    for (uint64_t k = 0; k < n_ce; ++k) { marks[R->ce[k] / 32] |= 1u << (R->ce[k] % 32); rank_of[R->ce[k]] = (uint32_t)k; }
    const Tables T{marks.data(), rank_of.data(), I.inv, I.kmers};
    struct WeightSink {
        std::vector<uint64_t>* w;
        void entry(uint32_t k, uint32_t, bool dup) { if (!dup) ++(*w)[k]; }
        void loc(uint32_t k, uint32_t, int32_t) { ++(*w)[k]; }
        void prec(uint32_t k, int32_t, int32_t) { ++(*w)[k]; }
        void mate(uint32_t k, bool taken) { if (taken) ++(*w)[k]; }
    };
    R->weight.assign(n_ce, 0);
    WeightSink ws{&R->weight};
    for (uint64_t id = 0; id < I.n_reads; ++id)
        walk_read((const uint32_t*)I.edges + I.first[id], (uint32_t)(I.first[id + 1] - I.first[id]), I.offsets[id], I.dup[id / 2] != 0, T, 0, (uint32_t)n_ce, I.K, ws);
    const std::vector<uint64_t> wfirst = dfk::prefix_sums(R->weight.data(), n_ce);
    R->loc_first.assign(1, 0); R->anchor_first.assign(1, 0); R->read_first.assign(1, 0);
    *n_ranges = 0;
    struct Rec { uint32_t key; Loc l; };
    struct EmitSink {
        uint32_t k0; uint64_t id; std::vector<Rec>* recs; std::vector<std::pair<uint32_t, std::pair<int32_t, int32_t>>>* pv; std::vector<std::pair<uint32_t, uint32_t>>* ent;
        uint64_t mates_in = 0, mates_out = 0, dup_skipped = 0;
        void entry(uint32_t k, uint32_t pass, bool dup) { if (dup) ++dup_skipped; else ent->emplace_back(k - k0, read_word(id, pass == 0)); }
        void loc(uint32_t k, uint32_t pass, int32_t pos) { recs->push_back(Rec{loc_key(k - k0, pass), Loc{(int64_t)id, pos, pass == 0 ? 1u : 0u}}); }
        void prec(uint32_t k, int32_t g, int32_t add) { pv->push_back({k - k0, {g, add}}); }
        void mate(uint32_t k, bool taken) { if (taken) { ++mates_in; ent->emplace_back(k - k0, read_word(id ^ 1, false)); } else ++mates_out; }
    };
    for (uint64_t k0 = 0; k0 < n_ce;) {
        const dfk::PidxRange range = next_range(wfirst.data(), n_ce, k0, cap);
        if (!range.ok) return -4;
        const uint64_t k1 = range.e1;
        ++*n_ranges;
        std::vector<Rec> recs; std::vector<std::pair<uint32_t, std::pair<int32_t, int32_t>>> prec; std::vector<std::pair<uint32_t, uint32_t>> ent;
        EmitSink es; es.k0 = (uint32_t)k0; es.recs = &recs; es.pv = &prec; es.ent = &ent;
        for (uint64_t id = 0; id < I.n_reads; ++id) {
            es.id = id;
            walk_read((const uint32_t*)I.edges + I.first[id], (uint32_t)(I.first[id + 1] - I.first[id]), I.offsets[id], I.dup[id / 2] != 0, T, (uint32_t)k0, (uint32_t)k1, I.K, es);
        }
        R->prec += prec.size(); R->mates_in += es.mates_in; R->mates_out += es.mates_out; R->dup_skipped += es.dup_skipped;
        std::stable_sort(recs.begin(), recs.end(), [](const Rec& a, const Rec& b) { return a.key < b.key; });
        std::sort(prec.begin(), prec.end());
        std::sort(ent.begin(), ent.end());
        ent.erase(std::unique(ent.begin(), ent.end()), ent.end());
        std::vector<uint64_t> nl(k1 - k0, 0), na(k1 - k0, 0), nr(k1 - k0, 0);
        for (const Rec& r : recs) { R->locs.push_back(r.l); ++nl[r.key / 2]; }
        for (size_t i = 0; i < prec.size();) {
            size_t j = i + 1;
            while (j < prec.size() && prec[j] == prec[i]) ++j;
            if ((int64_t)(j - i) >= MIN_EDGE_COUNT) { R->anchors.push_back(Anchor{prec[i].second.first, prec[i].second.second, (int32_t)(j - i)}); ++na[prec[i].first]; }
            i = j;
        }
        for (const auto& en : ent) { R->reads.push_back(en.second); ++nr[en.first]; }
        for (uint64_t k = 0; k < k1 - k0; ++k) {
            R->loc_first.push_back(R->loc_first.back() + nl[k]); R->anchor_first.push_back(R->anchor_first.back() + na[k]); R->read_first.push_back(R->read_first.back() + nr[k]);
        }
        k0 = k1;
    }
    return 0;
}

inline unsigned grid_reads(uint64_t n, unsigned cus) { return dfk::grid_256(n + 1, cus); }  // (n + 1: the kernels that fill a scan's input write its last word too)

// ---- the files' fixed parts
struct BinHead { char magic[8]; uint64_t n; };
static_assert(sizeof(BinHead) == 16, "BINWRITE header");
inline BinHead head_of(const char* magic8, uint64_t n) { BinHead h; for (int i = 0; i < 8; ++i) h.magic[i] = magic8[i]; h.n = n; return h; }
constexpr const char* MAGIC_EDGES = "BINWRITE";
constexpr const char* MAGIC_LOCS = "DFKCLOC1";
constexpr const char* MAGIC_ANCHORS = "DFKCANC1";
constexpr const char* MAGIC_READS = "DFKCRDS1";
inline uint64_t edges_file_size(uint64_t n) { return 16 + 8 * n; }
inline uint64_t table_records_at(uint64_t n) { return 16 + 8 * (n + 1); }                  // where a table's records start
inline uint64_t table_file_size(uint64_t n, uint64_t n_records, uint64_t record_bytes) { return table_records_at(n) + n_records * record_bytes; }

} // namespace dfk_closer
