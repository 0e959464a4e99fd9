// superplus_amd/csrc/dfk_patch.h -- the patched graph from edges and closures (10X/runstages/RunStages.cc:330-360): the rule stated
// literally, the pieces host and kernels share, the order of work the device runs (on the host, for tests/cpp/test_patch.cc) and the
// layout of a.patch.to3.  Host code compiles with any C++17 compiler; nothing here needs HIP.
//
// ---- The rule (reference paths relative to lib/assembly/src)
// 1. BuildAll (paths/long/large/GapToyTools4.cc:132-159) and RunStages.cc:342.  allx, in this order:
//      allx[e] = hb.EdgeObject(e) for every e < hb.E(), both orientations of every edge (:142-143);
//      for v in vertices, for i1 over To(v), for i2 over From(v) (:150-159): the last K bases of e1 followed by e2[K-1], skipped where
//      either edge is empty;
//      the closures, in the combined list's order (RunStages.cc:323-324, :342).
// 2. BigKMerizer::kmerize (kmers/BigKPather.cc:40-55, add / canonicalAdd :97-106).  A sequence shorter than K gives nothing; one of
//    exactly K bases one K-mer with an empty context; otherwise the first K-mer has initialContext(bv[K]) (one successor), the inner ones
//    KMerContext(itr[-1], itr[K]), the last finalContext(itr[-1]) (one predecessor).  A K-mer is stored canonical (isRev() ? rc() : kmer:
//    a palindrome as it is), its context reverse-complemented with it (KMerContext::rc = the byte's bits reversed); the contexts of equal
//    K-mers are OR-ed.  No count, no quality, no recomputeAdjacencies: a context bit exists only where a member of allx shows two K-mers
//    side by side.
// 3. BigKEdgeBuilder (:112-307), then buildHBVFromEdges.  Beside BuildReadQGraph48.cc's EdgeBuilder (:320-503), which k_graph_classify and
//    the walks of dfk_graph_kernels.h restate, statement by statement:
//      isPalindrome (:207-213 | :421-427)       for even K both are CF<K>::isPalindrome of the K-mer.  Odd K differs and is out of scope.
//      upstreamExtensionPossible (:215-225 | :399-408), downstreamExtensionPossible (:227-237 | :410-419)
//                                               the same: one predecessor (successor), the neighbour not a palindrome, and the neighbour's
//                                               context turned to this orientation shows one successor (predecessor).
//      buildEdge (:144-159 | :326-336)          the same four cases in the same order.
//      extend (:244-266 | :436-465)             the same breaks: several successors, a palindromic next K-mer (popped), a next K-mer with
//                                               several predecessors (popped); then getCanonicalForm of the whole sequence: PALINDROME
//                                               (asserted to be K long) and FWD are added, REV is dropped (its mirror image is built from
//                                               the other end).
//      addEdge (:280-301 | :480-491)            both reverse-complement a REV sequence before storing it.  The order of mEdges is a thread
//                                               race in both; buildHBVFromEdges sorts (HBVFromEdges.cc:106-111), so hb3's numbering is
//                                               defined.
//      simpleCircle (:162-188 | :338-365)       the same walk over single successors until the first entry comes back.
//      canonicalizeCircle (:190-205 | :367-392) worded differently.  Here: the minimal entry by BigKMer's operator< (bases in the entry's
//                                               own, canonical, orientation); if the sequence at that entry's index does not std::equal
//                                               the entry's bases, the whole circle is reverse-complemented and idx = size - idx - K.
//                                               There: the minimal entry by KMer's operator< and CF<K>::getForm of the sequence at idx ==
//                                               REV decides.  An entry is stored canonical and, K even, a K-mer of a circle is no
//                                               palindrome (palindromes are edges of their own), so "the sequence there is not the
//                                               canonical K-mer" and "the sequence there is REV" say the same, and both orders are the
//                                               lexical order of the canonical bases.  literal_edges() below is the wording of :190-205;
//                                               tests/patch_oracle.py goes through oracle/graph_oracle.py, the wording of :367-392; the
//                                               cycle cases of tests/patch_cases.py hold them to each other.
//    buildHBVFromEdges is restated by build_hbv (dfk_graph.inc) and by oracle/graph_oracle.py's build_hbv; this header stops at the
//    canonical edges in HBVFromEdges' order (sorted_edges(): length descending, then lexical) and names an hb3 edge as
//    2 * (place in that order) + (reverse complement ? 1 : 0), a palindrome as 2 * place.
// 4. Pather (:310-353) for allx[i], i < hb.E() only (RunStages.cc:355-358).  updateDict (:86-94) leaves in every entry where its K-mer
//    lies on its edge and whether the edge shows its reverse complement; lookup (:356-363) turns that round for a read K-mer that
//    isRev().  So the first K-mer gives (edge, offset in the read's direction, isRC): left3[i] = getFirstSkip() = that offset, the first id
//    = isRC ? revXlat : fwdXlat.  Then (:333-345) while readLenRemaining > edgeLenRemaining: readLenRemaining -= edgeLenRemaining - (K-1),
//    the K-mer at read.size() - readLenRemaining is looked up, ForceAssertEq(offset, 0), its id appended, edgeLenRemaining = its edge's
//    size.  to3[i] = the ids.  An old edge shorter than K has an empty path (the graph has none).  The paths of the crossings and of the
//    closures are computed by the reference and thrown away; nothing here computes them.
//
// ---- The form the device runs (dfk_patch_kernels.h, dfk_patch.inc; device_order() below is the same order of work on the host)
//  * Base entries.  In a unipath graph every K-mer lies on exactly one canonical edge (e <= inv[e]): a self-inverse edge is one
//    palindromic K-mer.  The canonical edges in ascending e get first[c] = the K-mers before them; entry slot = first[c] + pos, and back by
//    the largest c with first[c] <= slot (slot_edge()).  entry_context() gives the context: the neighbouring bases inside the edge; at its
//    two ends the crossings' bits, the OR over To(to_left[e]) of the base before the last K, the OR over From(to_right[e]) of base K-1.
//    inv[e] is in allx too and shows the same K-mers reverse-complemented: inside the edge that adds nothing, at the ends it adds the
//    crossings of inv[e]'s vertices, turned round -- entry_context() takes both and is the one place that says how; an edge that is its own
//    inverse is in allx once and gets its own bits alone.  The host checks that the ends of the edges at a vertex agree in their K-1
//    bases (a crossing's second K-mer is then the first K-mer of e2: crossings add no K-mer).
//  * A K-mer on two canonical edges (arrays form only) is found by looking every base entry up and comparing the id found: DFK_E_ARG.
//  * Closure K-mers: a lane a position; found -> atomicOr of the context into the entry (order-free, exact), not found -> appended.  The
//    list is sorted and its equal keys OR-ed on the host (it is small), the survivors are the dictionary's second part.
//  * The graph kernels, unchanged, over the two parts; build_hbv.
//  * to3 / left3: after k_graph_bases an entry holds (edge3, offset3).  Walking a canonical old edge forwards, position j reads its hb3
//    edge forwards or backwards (walk_dir()), its offset in walking direction is offset3 or n3 - 1 - offset3, and it starts a new id
//    where j == 0 or that offset is 0 (is_head()).  The ids of a canonical edge are its heads' in order; left3 the first entry's offset
//    in walking direction.  inv[e]'s path is e's reversed through hb3's involution, its left3 = n3 - 1 - (the last entry's offset in
//    walking direction) (inv_route(), inv_left3()).
//
// ---- a.patch.to3 (little-endian, no byte undefined)
//   0   char[8] "DFKPTO31"      8  u64 n_edges      16  u64 n_to3
//   24  u64 to3_first[n_edges + 1]        then i32 to3[n_to3]        then i32 left3[n_edges]
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define DFK_PATCH_HD __host__ __device__ inline
#else
#define DFK_PATCH_HD inline
#endif

namespace dfk_patch {

constexpr char MAGIC[9] = "DFKPTO31";
constexpr uint64_t SALT = 0x9A7C;
constexpr uint64_t to3_first_at() { return 24; }
constexpr uint64_t to3_at(uint64_t n_edges) { return 24 + 8 * (n_edges + 1); }
constexpr uint64_t left3_at(uint64_t n_edges, uint64_t n_to3) { return to3_at(n_edges) + 4 * n_to3; }
constexpr uint64_t file_bytes(uint64_t n_edges, uint64_t n_to3) { return left3_at(n_edges, n_to3) + 4 * n_edges; }

// ---- shared by host and kernels
DFK_PATCH_HD uint32_t ctx_rc8(uint32_t c)                              // KMerContext::rc: the byte's bits in reverse order
{
    c = ((c & 0xF0u) >> 4) | ((c & 0x0Fu) << 4);
    c = ((c & 0xCCu) >> 2) | ((c & 0x33u) << 2);
    return ((c & 0xAAu) >> 1) | ((c & 0x55u) << 1);
}
// The context of the canonical entry of a K-mer of old edge e.  pred, succ: the nibbles e itself shows at this position -- 1 << the
// neighbouring base inside the edge, at an end the crossings of that end's vertex.  inv_pred, inv_succ: the nibbles inv[e] shows at the
// mirrored position IN ITS OWN ORIENTATION where they say more than e's: at an end of inv[e] the crossings of ITS vertex, otherwise 0;
// both 0 where e is its own inverse.  rev: the K-mer as e reads it isRev(), the entry holds its reverse complement.
DFK_PATCH_HD uint32_t entry_context(uint32_t pred, uint32_t succ, uint32_t inv_pred, uint32_t inv_succ, bool rev)
{
    const uint32_t c = (pred << 4 | succ) | ctx_rc8(inv_pred << 4 | inv_succ);
    return rev ? ctx_rc8(c) : c;
}
// the crossings of a canonical edge's four ends in one word: bits 0-3 pred at to_left[e], 4-7 succ at to_right[e], 8-11 pred at
// to_left[inv e], 12-15 succ at to_right[inv e] (8-15 zero where inv[e] == e)
DFK_PATCH_HD uint32_t position_context(uint32_t ends, uint32_t pos, uint32_t n, uint32_t base_before, uint32_t base_after, bool rev)
{
    const bool first = pos == 0, last = pos + 1 == n;
    return entry_context(first ? ends & 15u : 1u << base_before, last ? (ends >> 4) & 15u : 1u << base_after,
                         last ? (ends >> 8) & 15u : 0u, first ? (ends >> 12) & 15u : 0u, rev);
}
// the canonical edge of a slot: the largest c with first[c] <= slot (first[n_canon] = the number of slots)
DFK_PATCH_HD uint32_t slot_edge(const uint64_t* first, uint32_t n_canon, uint64_t slot)
{
    uint32_t lo = 0, hi = n_canon;
    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (first[mid] <= slot) lo = mid; else hi = mid; }
    return lo;
}
// An old edge read forwards meets an entry whose canonical K-mer it reads reversed (`read_rev`) and which its hb3 edge shows forwards
// (`stored_fwd`): does the walk read the hb3 edge forwards?  (A palindrome: read_rev false, stored_fwd true.)
DFK_PATCH_HD bool walk_dir(bool read_rev, bool stored_fwd) { return read_rev != stored_fwd; }
DFK_PATCH_HD uint32_t walk_offset(bool fwd, uint32_t off3, uint32_t n3) { return fwd ? off3 : n3 - 1 - off3; }
DFK_PATCH_HD bool is_head(uint32_t pos, uint32_t walk_off) { return pos == 0 || walk_off == 0; }
// The inv route.  inv[e] reads e's K-mers backwards: its first K-mer is e's last, n3 - 1 - (that entry's offset in e's walking direction) from
// the start of the hb3 edge as inv[e] walks it; its ids are e's in reverse order, each through hb3's involution (`inv_id`).
DFK_PATCH_HD int32_t inv_left3(uint32_t last_n3, uint32_t last_walk_off) { return (int32_t)(last_n3 - 1 - last_walk_off); }
template <class Inv> inline void inv_route(const int32_t* ids, uint64_t n, Inv inv_id, int32_t* out) { for (uint64_t j = 0; j < n; ++j) out[j] = inv_id(ids[n - 1 - j]); }

// ================================================================================================ host
typedef std::vector<uint8_t> Seq;                                     // base codes 0-3

struct Graph {
    uint32_t K = 0, n_vertices = 0;
    std::vector<Seq> edges;
    std::vector<int32_t> inv, to_left, to_right;
};
struct Result {
    std::vector<Seq> edges3;                                           // canonical, in HBVFromEdges' order
    std::vector<uint64_t> to3_first;
    std::vector<int32_t> to3, left3;                                   // ids as 2 * place + rc
    uint64_t crossings = 0, shorter = 0, positions = 0, found = 0, fresh = 0, fresh_unique = 0, bits_added = 0, kmers3 = 0, single3 = 0, batches = 0;
    bool operator==(const Result& o) const
    {
        return edges3 == o.edges3 && to3_first == o.to3_first && to3 == o.to3 && left3 == o.left3 && crossings == o.crossings && shorter == o.shorter && positions == o.positions &&
               found == o.found && fresh == o.fresh && fresh_unique == o.fresh_unique && bits_added == o.bits_added && kmers3 == o.kmers3 && single3 == o.single3;
    }
};

inline Seq rc_seq(const Seq& s) { Seq r(s.rbegin(), s.rend()); for (uint8_t& b : r) b ^= 3; return r; }
enum Form { FWD, REV, PALINDROME };
inline Form canonical_form(const uint8_t* beg, size_t len)            // getCanonicalForm, dna/CanonicalForm.h:34-46
{
    if (len & 1) return beg[len / 2] & 2 ? REV : FWD;
    const uint8_t* end = beg + len;
    while (beg != end) { const uint8_t f = *beg, r = *--end ^ 3; if (f < r) return FWD; if (r < f) return REV; ++beg; }
    return PALINDROME;
}
inline uint32_t popcount8(uint32_t x) { return (uint32_t)__builtin_popcount(x & 0xFFu); }

// what does not hold together: "" or the reason (the arrays form's DFK_E_ARG)
inline std::string check_graph(const Graph& G)
{
    const size_t E = G.edges.size();
    const uint32_t K = G.K;
    if (K < 4 || (K & 1)) return "K must be even";
    if (G.inv.size() != E || G.to_left.size() != E || G.to_right.size() != E) return "the tables are not n_edges long";
    for (size_t e = 0; e < E; ++e) {
        if (G.inv[e] < 0 || (size_t)G.inv[e] >= E || (size_t)G.inv[G.inv[e]] != e) return "inv is not an involution at edge " + std::to_string(e);
        if (G.to_left[e] < 0 || (uint32_t)G.to_left[e] >= G.n_vertices || G.to_right[e] < 0 || (uint32_t)G.to_right[e] >= G.n_vertices) return "an end of edge " + std::to_string(e) + " is no vertex";
        if (G.edges[e].size() < K) return "edge " + std::to_string(e) + " is shorter than K";
        for (uint8_t b : G.edges[e]) if (b > 3) return "edge " + std::to_string(e) + " has a base above 3";
    }
    for (size_t e = 0; e < E; ++e) if (G.edges[G.inv[e]] != rc_seq(G.edges[e])) return "edge inv[" + std::to_string(e) + "] is not its reverse complement";
    // the K-1 bases of a vertex: every edge that ends there ends with them, every edge that starts there starts with them
    std::vector<int64_t> owner(G.n_vertices, -1);                      // edge << 1 | (its end, not its start)
    auto key = [&](int64_t o) { const Seq& s = G.edges[o >> 1]; return (o & 1) ? s.data() + s.size() - (K - 1) : s.data(); };
    for (size_t e = 0; e < E; ++e)
        for (int end = 0; end < 2; ++end) {
            const int32_t v = end ? G.to_right[e] : G.to_left[e];
            const int64_t me = (int64_t)(e << 1) | end;
            if (owner[v] < 0) owner[v] = me;
            else if (memcmp(key(owner[v]), key(me), K - 1) != 0) return "the edges at vertex " + std::to_string(v) + " do not share its K-1 bases";
        }
    return "";
}

// ---- 1. BuildAll
inline std::vector<Seq> build_all(const Graph& G, const std::vector<Seq>& closures, uint64_t* n_cross)
{
    const uint32_t K = G.K;
    std::vector<Seq> allx(G.edges.begin(), G.edges.end());
    // digraphE keeps To(v) / From(v) by neighbouring vertex, equal neighbours by edge number
    std::vector<std::vector<std::pair<int32_t, int32_t>>> to(G.n_vertices), from(G.n_vertices);
    for (size_t e = 0; e < G.edges.size(); ++e) { from[G.to_left[e]].push_back({G.to_right[e], (int32_t)e}); to[G.to_right[e]].push_back({G.to_left[e], (int32_t)e}); }
    for (uint32_t v = 0; v < G.n_vertices; ++v) {
        std::sort(to[v].begin(), to[v].end()); std::sort(from[v].begin(), from[v].end());
        for (const auto& i1 : to[v])
            for (const auto& i2 : from[v]) {
                const Seq& x1 = G.edges[i1.second]; const Seq& x2 = G.edges[i2.second];
                if (x1.empty() || x2.empty()) continue;
                Seq tmp(x1.end() - K, x1.end());
                tmp.push_back(x2[K - 1]);
                allx.push_back(tmp);
            }
    }
    *n_cross = allx.size() - G.edges.size();
    allx.insert(allx.end(), closures.begin(), closures.end());
    return allx;
}

// ---- 2. kmerize
struct Ent { uint8_t ctx = 0; bool assigned = false; int32_t edge = -1; uint32_t off = 0; bool rc = false; };
typedef std::map<Seq, Ent> Dict;                                       // canonical K-mer -> entry; the map's order is BigKMer's operator<
inline void kmerize(const Seq& bv, uint32_t K, Dict& d)
{
    if (bv.size() < K) return;
    const size_t n = bv.size() - K + 1;
    for (size_t p = 0; p < n; ++p) {
        uint32_t ctx = 0;
        if (bv.size() > K) {
            if (p > 0) ctx |= 16u << bv[p - 1];
            if (p + 1 < n) ctx |= 1u << bv[p + K];
        }
        Seq k(bv.begin() + p, bv.begin() + p + K);
        if (canonical_form(k.data(), K) == REV) { k = rc_seq(k); ctx = ctx_rc8(ctx); }
        d[k].ctx |= (uint8_t)ctx;
    }
}

// ---- 3. BigKEdgeBuilder, as written
struct EdgeBuilder {
    uint32_t K; Dict& d; std::vector<Seq>& edges;
    std::vector<Ent*> ents; Seq seq;
    static uint32_t preds(uint32_t c) { return popcount8(c >> 4); }
    static uint32_t succs(uint32_t c) { return popcount8(c & 15u); }
    static uint8_t single(uint32_t nib) { return (uint8_t)__builtin_ctz(nib); }
    bool is_pal(const uint8_t* k) const { return canonical_form(k, K) == PALINDROME; }             // :207-213, K even
    Ent* lookup(const uint8_t* k, uint32_t* ctx)                                                  // :268-278
    {
        Seq s(k, k + K);
        const bool rev = canonical_form(k, K) == REV;
        if (rev) s = rc_seq(s);
        auto it = d.find(s);
        if (it == d.end()) throw std::runtime_error("patch: a context names a K-mer that is not in the dictionary");
        *ctx = rev ? ctx_rc8(it->second.ctx) : it->second.ctx;
        return &it->second;
    }
    bool up_ok(const Seq& k, uint32_t ctx)                                                        // :215-225
    {
        if (preds(ctx) != 1) return false;
        Seq p(1, single(ctx >> 4)); p.insert(p.end(), k.begin(), k.end() - 1);
        if (is_pal(p.data())) return false;
        uint32_t c; lookup(p.data(), &c);
        return succs(c) == 1;
    }
    bool down_ok(const Seq& k, uint32_t ctx)                                                      // :227-237
    {
        if (succs(ctx) != 1) return false;
        Seq s(k.begin() + 1, k.end()); s.push_back(single(ctx & 15u));
        if (is_pal(s.data())) return false;
        uint32_t c; lookup(s.data(), &c);
        return preds(c) == 1;
    }
    void add_edge()                                                                               // :280-301
    {
        if (canonical_form(seq.data(), seq.size()) == REV) seq = rc_seq(seq);
        edges.push_back(seq);
        for (Ent* e : ents) { if (e->assigned) throw std::runtime_error("patch: a K-mer on two edges"); e->assigned = true; }
        seq.clear(); ents.clear();
    }
    void extend(uint32_t ctx)                                                                     // :244-266
    {
        while (succs(ctx) == 1) {
            seq.push_back(single(ctx & 15u));
            const uint8_t* k = seq.data() + seq.size() - K;
            if (is_pal(k)) { seq.pop_back(); break; }
            Ent* e = lookup(k, &ctx);
            if (preds(ctx) != 1) { seq.pop_back(); break; }
            ents.push_back(e);
        }
        switch (canonical_form(seq.data(), seq.size())) {
        case PALINDROME: if (seq.size() != K) throw std::runtime_error("patch: a palindromic edge longer than K");   // falls through
        case FWD: add_edge(); break;
        case REV: seq.clear(); ents.clear(); break;
        }
    }
    void build_edge(const Seq& k, Ent& e)                                                         // :144-159
    {
        if (is_pal(k.data())) { seq = k; ents.push_back(&e); add_edge(); }
        else if (up_ok(k, e.ctx)) {
            if (down_ok(k, e.ctx)) return;
            seq = rc_seq(k); ents.push_back(&e); extend(ctx_rc8(e.ctx));
        } else if (down_ok(k, e.ctx)) { seq = k; ents.push_back(&e); extend(e.ctx); }
        else { seq = k; ents.push_back(&e); add_edge(); }
    }
    void simple_circle(const Seq& k, Ent& first)                                                  // :162-188
    {
        seq = k; ents.push_back(&first);
        uint32_t ctx = first.ctx;
        for (;;) {
            if (preds(ctx) != 1 || succs(ctx) != 1) throw std::runtime_error("patch: a circle with a branch");
            seq.push_back(single(ctx & 15u));
            Ent* e = lookup(seq.data() + seq.size() - K, &ctx);
            if (e == &first) { seq.pop_back(); break; }
            if (e->assigned) throw std::runtime_error("patch: failed to close circle");
            ents.push_back(e);
        }
        // canonicalizeCircle, :190-205: the minimal entry by its own (canonical) bases
        size_t idx = 0; Seq best;
        for (size_t i = 0; i < ents.size(); ++i) {
            Seq c(seq.begin() + i, seq.begin() + i + K);
            if (canonical_form(c.data(), K) == REV) c = rc_seq(c);
            if (i == 0 || c < best) { best = c; idx = i; }
        }
        if (!std::equal(best.begin(), best.end(), seq.begin() + idx)) { seq = rc_seq(seq); idx = seq.size() - idx - K; }
        Seq bv(seq.begin() + idx, seq.end());
        bv.insert(bv.end(), seq.begin() + (K - 1), seq.begin() + (K - 1 + idx));
        seq = bv;
        add_edge();
    }
};
inline std::vector<Seq> literal_edges(Dict& d, uint32_t K)                                        // buildEdges, :119-138
{
    std::vector<Seq> edges;
    EdgeBuilder eb{K, d, edges, {}, {}};
    for (auto& kv : d) if (!kv.second.assigned) eb.build_edge(kv.first, kv.second);
    for (auto& kv : d) if (!kv.second.assigned) eb.simple_circle(kv.first, kv.second);
    return edges;
}
inline std::vector<Seq> sorted_edges(std::vector<Seq> e)                                          // HBVFromEdges.cc:106-111
{
    std::sort(e.begin(), e.end(), [](const Seq& a, const Seq& b) { return a.size() != b.size() ? a.size() > b.size() : a < b; });
    return e;
}
inline void update_dict(Dict& d, const std::vector<Seq>& edges, uint32_t K)                       // :86-94
{
    for (size_t i = 0; i < edges.size(); ++i)
        for (size_t o = 0; o + K <= edges[i].size(); ++o) {
            Seq k(edges[i].begin() + o, edges[i].begin() + o + K);
            const bool rev = canonical_form(k.data(), K) == REV;
            Ent& e = d.at(rev ? rc_seq(k) : k);
            e.edge = (int32_t)i; e.rc = rev; e.off = (uint32_t)(rev ? edges[i].size() - o - K : o);
        }
}
// ---- 4. Pather
inline void pather(const Seq& read, uint32_t K, const Dict& d, const std::vector<Seq>& edges, std::vector<int32_t>* ids, int32_t* first_skip)
{
    ids->clear(); *first_skip = 0;
    if (read.size() < K) return;
    auto lookup = [&](size_t pos) {                                                                // :356-363
        Seq k(read.begin() + pos, read.begin() + pos + K);
        if (canonical_form(k.data(), K) == REV) { Ent e = d.at(rc_seq(k)); e.off = (uint32_t)(edges[e.edge].size() - e.off - K); e.rc = !e.rc; return e; }
        return d.at(k);
    };
    auto id_of = [&](const Ent& e) { return 2 * e.edge + (e.rc && canonical_form(edges[e.edge].data(), edges[e.edge].size()) != PALINDROME ? 1 : 0); };
    Ent e = lookup(0);
    *first_skip = (int32_t)e.off;
    ids->push_back(id_of(e));
    size_t read_left = read.size(), edge_left = edges[e.edge].size() - e.off;
    while (read_left > edge_left) {
        read_left = read_left - edge_left + K - 1;
        e = lookup(read.size() - read_left);
        if (e.off != 0) throw std::runtime_error("patch: ForceAssertEq(offset, 0)");
        ids->push_back(id_of(e));
        edge_left = edges[e.edge].size();
    }
}

// the literal form: BuildAll, kmerize, the edges, the old edges' paths
inline Result literal(const Graph& G, const std::vector<Seq>& closures)
{
    Result R;
    const uint32_t K = G.K;
    const size_t E = G.edges.size();
    const std::vector<Seq> allx = build_all(G, closures, &R.crossings);
    Dict d;
    for (size_t i = 0; i < E + R.crossings; ++i) kmerize(allx[i], K, d);
    const Dict base = d;
    for (size_t i = E + R.crossings; i < allx.size(); ++i) {
        const Seq& s = allx[i];
        R.shorter += s.size() < K;
        for (size_t p = 0; p + K <= s.size(); ++p) {
            Seq k(s.begin() + p, s.begin() + p + K);
            if (canonical_form(k.data(), K) == REV) k = rc_seq(k);
            ++R.positions; R.found += base.count(k);
        }
        kmerize(s, K, d);
    }
    R.fresh = R.positions - R.found; R.fresh_unique = d.size() - base.size(); R.kmers3 = d.size();
    for (const auto& kv : base) R.bits_added += popcount8(d.at(kv.first).ctx & ~kv.second.ctx);
    R.edges3 = sorted_edges(literal_edges(d, K));
    for (const Seq& s : R.edges3) R.single3 += s.size() == K;
    update_dict(d, R.edges3, K);
    R.to3_first.assign(1, 0); R.left3.resize(E);
    std::vector<int32_t> ids;
    for (size_t e = 0; e < E; ++e) {
        pather(allx[e], K, d, R.edges3, &ids, &R.left3[e]);
        R.to3.insert(R.to3.end(), ids.begin(), ids.end());
        R.to3_first.push_back(R.to3.size());
    }
    return R;
}

// ---- the device's order of work, on the host
struct Plan {
    std::vector<uint32_t> canon;                                       // the canonical edges, ascending
    std::vector<uint64_t> first;                                       // [n_canon + 1]
    std::vector<uint16_t> ends;                                        // position_context()'s word per canonical edge
};
inline Plan plan_of(const Graph& G)
{
    Plan P;
    const uint32_t K = G.K;
    std::vector<uint8_t> vpred(G.n_vertices, 0), vsucc(G.n_vertices, 0);
    for (size_t e = 0; e < G.edges.size(); ++e) {
        const Seq& s = G.edges[e];
        vpred[G.to_right[e]] |= (uint8_t)(1u << s[s.size() - K]);                        // e in To(v): the base before its last K-1
        vsucc[G.to_left[e]] |= (uint8_t)(1u << s[K - 1]);                                // e in From(v)
    }
    P.first.assign(1, 0);
    for (size_t e = 0; e < G.edges.size(); ++e) {
        if ((size_t)G.inv[e] < e) continue;
        const int32_t i = G.inv[e];
        uint32_t w = vpred[G.to_left[e]] | (uint32_t)vsucc[G.to_right[e]] << 4;
        if ((size_t)i != e) w |= (uint32_t)vpred[G.to_left[i]] << 8 | (uint32_t)vsucc[G.to_right[i]] << 12;
        P.canon.push_back((uint32_t)e); P.ends.push_back((uint16_t)w);
        P.first.push_back(P.first.back() + G.edges[e].size() - K + 1);
    }
    return P;
}
struct HostEntry { Seq k; uint8_t ctx; };
// the head flags of a canonical edge and the inv route: the ids and left3 of e and of inv[e] from e's entries alone
struct Step { int32_t id; uint32_t walk_off; };
// the whole of it: base entries by slot, the closures' K-mers in batches against them, the list sorted and merged, the edges (through
// literal_edges: the graph kernels are restated elsewhere), then heads / emit and the inv route.  Throws where a K-mer has two slots.
inline Result device_order(const Graph& G, const std::vector<Seq>& closures, uint64_t kmers_per_batch)
{
    Result R;
    const uint32_t K = G.K;
    const size_t E = G.edges.size();
    const Plan P = plan_of(G);
    const uint32_t nc = (uint32_t)P.canon.size();
    const uint64_t n_base = P.first[nc];
    { std::vector<uint32_t> nt(G.n_vertices, 0), nf(G.n_vertices, 0);
      for (size_t e = 0; e < E; ++e) { ++nf[G.to_left[e]]; ++nt[G.to_right[e]]; }
      for (uint32_t v = 0; v < G.n_vertices; ++v) R.crossings += (uint64_t)nt[v] * nf[v]; }
    std::vector<HostEntry> ent(n_base);
    std::vector<uint8_t> read_rev(n_base);
    std::map<Seq, uint64_t> index;
    for (uint64_t slot = 0; slot < n_base; ++slot) {
        const uint32_t c = slot_edge(P.first.data(), nc, slot), pos = (uint32_t)(slot - P.first[c]);
        const Seq& s = G.edges[P.canon[c]];
        const uint32_t n = (uint32_t)(s.size() - K + 1);
        Seq k(s.begin() + pos, s.begin() + pos + K);
        const bool rev = canonical_form(k.data(), K) == REV;
        const uint32_t ctx = position_context(P.ends[c], pos, n, pos ? s[pos - 1] : 0u, pos + 1 < n ? s[pos + K] : 0u, rev);
        ent[slot] = HostEntry{rev ? rc_seq(k) : k, (uint8_t)ctx}; read_rev[slot] = rev;
        if (!index.emplace(ent[slot].k, slot).second) throw std::invalid_argument("a K-mer lies on two canonical edges");
    }
    // closure positions, a batch at a time
    std::vector<uint64_t> cfirst(1, 0);
    for (const Seq& s : closures) { R.shorter += s.size() < K; cfirst.push_back(cfirst.back() + (s.size() >= K ? s.size() - K + 1 : 0)); }
    R.positions = cfirst.back();
    const uint64_t per = kmers_per_batch ? kmers_per_batch : std::max<uint64_t>(1, R.positions);
    std::vector<HostEntry> list;
    for (uint64_t q0 = 0; q0 < R.positions; q0 += per) {
        ++R.batches;
        for (uint64_t q = q0; q < std::min(R.positions, q0 + per); ++q) {
            const size_t i = (size_t)(std::upper_bound(cfirst.begin(), cfirst.end(), q) - cfirst.begin() - 1);
            const Seq& s = closures[i];
            const uint32_t p = (uint32_t)(q - cfirst[i]), n = (uint32_t)(s.size() - K + 1);
            Seq k(s.begin() + p, s.begin() + p + K);
            const bool rev = canonical_form(k.data(), K) == REV;
            const uint32_t ctx = entry_context(p ? 1u << s[p - 1] : 0u, p + 1 < n ? 1u << s[p + K] : 0u, 0, 0, rev);
            if (rev) k = rc_seq(k);
            auto it = index.find(k);
            if (it != index.end()) { ++R.found; R.bits_added += popcount8(ctx & ~ent[it->second].ctx); ent[it->second].ctx |= (uint8_t)ctx; }
            else list.push_back(HostEntry{k, (uint8_t)ctx});
        }
    }
    R.fresh = list.size();
    std::stable_sort(list.begin(), list.end(), [](const HostEntry& a, const HostEntry& b) { return a.k < b.k; });
    std::vector<HostEntry> part2;
    for (const HostEntry& h : list) { if (!part2.empty() && part2.back().k == h.k) part2.back().ctx |= h.ctx; else part2.push_back(h); }
    R.fresh_unique = part2.size(); R.kmers3 = n_base + part2.size();
    Dict d;
    for (const HostEntry& h : ent) d[h.k].ctx = h.ctx;
    for (const HostEntry& h : part2) d[h.k].ctx = h.ctx;
    R.edges3 = sorted_edges(literal_edges(d, K));
    std::vector<uint8_t> pal(R.edges3.size());
    for (size_t i = 0; i < R.edges3.size(); ++i) { R.single3 += R.edges3[i].size() == K; pal[i] = canonical_form(R.edges3[i].data(), R.edges3[i].size()) == PALINDROME; }
    // what k_graph_bases leaves in an entry: its canonical edge and the offset of the K-mer on it; whether the edge shows the canonical K-mer
    // is read off the edge's bases
    std::map<Seq, std::pair<uint32_t, uint32_t>> where;
    for (size_t i = 0; i < R.edges3.size(); ++i)
        for (size_t o = 0; o + K <= R.edges3[i].size(); ++o) {
            Seq k(R.edges3[i].begin() + o, R.edges3[i].begin() + o + K);
            if (canonical_form(k.data(), K) == REV) k = rc_seq(k);
            where[k] = {(uint32_t)i, (uint32_t)o};
        }
    auto step = [&](uint64_t slot) {
        const auto w = where.at(ent[slot].k);
        const Seq& s3 = R.edges3[w.first];
        const bool stored_fwd = std::equal(ent[slot].k.begin(), ent[slot].k.end(), s3.begin() + w.second);
        const bool fwd = walk_dir(read_rev[slot] != 0, stored_fwd);
        return Step{(int32_t)(2 * w.first + (fwd || pal[w.first] ? 0 : 1)), walk_offset(fwd, w.second, (uint32_t)(s3.size() - K + 1))};
    };
    std::vector<std::vector<int32_t>> paths(E);
    R.left3.assign(E, 0);
    for (uint32_t c = 0; c < nc; ++c) {
        const uint32_t e = P.canon[c];
        std::vector<int32_t>& ids = paths[e];
        Step last{0, 0};
        for (uint64_t slot = P.first[c]; slot < P.first[c + 1]; ++slot) {
            last = step(slot);
            const uint32_t pos = (uint32_t)(slot - P.first[c]);
            if (is_head(pos, last.walk_off)) ids.push_back(last.id);
            if (pos == 0) R.left3[e] = (int32_t)last.walk_off;
        }
        if ((uint32_t)G.inv[e] != e) {
            const uint32_t n3 = (uint32_t)(R.edges3[last.id >> 1].size() - K + 1);
            paths[G.inv[e]].resize(ids.size());
            inv_route(ids.data(), ids.size(), [&](int32_t id) { return pal[id >> 1] ? id : id ^ 1; }, paths[G.inv[e]].data());      // (hb3's involution on these ids)
            R.left3[G.inv[e]] = inv_left3(n3, last.walk_off);
        }
    }
    R.to3_first.assign(1, 0);
    for (size_t e = 0; e < E; ++e) { R.to3.insert(R.to3.end(), paths[e].begin(), paths[e].end()); R.to3_first.push_back(R.to3.size()); }
    return R;
}

// ---- the digest of to3 / left3 and the file
inline uint64_t mix64(uint64_t x) { x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; return x ^ (x >> 31); }
// k_digest_seq's sum and xor over to3_first, then to3, then left3 as one sequence of values
inline void digest(const std::vector<uint64_t>& to3_first, const std::vector<int32_t>& to3, const std::vector<int32_t>& left3, uint64_t* sum, uint64_t* xr)
{
    uint64_t i = 0; *sum = 0; *xr = 0;
    auto one = [&](uint64_t v) { const uint64_t h = mix64(mix64(i++ + SALT) ^ v); *sum += h; *xr ^= mix64(h + 0xD1B54A32D192ED03ull); };
    for (uint64_t v : to3_first) one(v);
    for (int32_t v : to3) one((uint64_t)(uint32_t)v);
    for (int32_t v : left3) one((uint64_t)(uint32_t)v);
}
inline std::vector<uint8_t> to3_file(const std::vector<uint64_t>& to3_first, const std::vector<int32_t>& to3, const std::vector<int32_t>& left3)
{
    const uint64_t E = left3.size(), n = to3.size();
    std::vector<uint8_t> f(file_bytes(E, n));
    memcpy(f.data(), MAGIC, 8); memcpy(f.data() + 8, &E, 8); memcpy(f.data() + 16, &n, 8);
    memcpy(f.data() + to3_first_at(), to3_first.data(), 8 * (E + 1));
    if (n) memcpy(f.data() + to3_at(E), to3.data(), 4 * n);
    if (E) memcpy(f.data() + left3_at(E, n), left3.data(), 4 * E);
    return f;
}
} // namespace dfk_patch
