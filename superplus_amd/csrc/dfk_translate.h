// superplus_amd/csrc/dfk_translate.h -- the read paths moved onto the patched graph (TranslatePaths and the Validate behind it, the end of
// StagePatch, 10X/runstages/RunStages.cc:364-371): the rule stated literally, the pieces host and kernels share, the bound that lets the
// device decide every path the pather can produce, the plan and the layout of the result.  Host code compiles with any C++17 compiler;
// nothing here needs HIP.
//
// ---- The rule (reference paths relative to lib/assembly/src; paths/long/large/GapToyTools4.cc:163-196), per read i whose path is not
// empty, with e0 = path[0] and start = offset + left3[e0] in int (:169):
//   1. to3[e0] empty (:171-173)                         the path is cleared.
//   2. start < hb3.Bases(to3[e0][0]) (:175-179)         the path becomes [to3[e0][0]] with offset start.  A negative start lands here.
//   3. otherwise (:181-196)                             p = OverlapAppend(p, to3[path[j]]) for j = 0, 1, ..., stopping at the first j whose
//                                                       to3 is empty (:182-184).  OverlapAppend (Vec.h:593-606) drops from the appended
//                                                       list its longest prefix that is a suffix of p.  Then (:185-189)
//                                                         while (start >= Bases(p[trim])) { start -= Kmers(p[trim]); trim++; if (trim == |p|) break; }
//                                                       trim == |p| (:191-193): cleared.  Else the path becomes [p[trim]] with offset start.
// Three things decide the bytes:
//   * The test is against Bases = Kmers + K - 1, the subtraction is Kmers: a start in the last K - 1 bases of an hb3 edge stays on it.
//   * clear() and resize(1) touch neither mOffset nor mLastSkip (paths/long/ReadPath.h:24-88): a cleared path keeps its OLD offset and is
//     the 8 bytes {old offset, 0} of a feudal file; a translated one the 12 bytes {start, 0, edge}; a path empty before is left alone.
//   * Validate -> ValidateAllReadPaths -> ValidateReadPath (paths/long/ReadPathTools.cc:35-105, read_length = 0).  For a path of one edge
//     it tests edge_id >= edge_count (:44-48, signed: a negative id passes) and nothing else: there is no next edge to connect to (:51-59),
//     the negative-offset test needs a read length (:62), and the "positive offset" test reads offset < 0 && offset >= len (:70), which
//     no offset satisfies.  valid_id() below is that one test; DFK_TRANSLATE_INVALID counts the placed reads that fail it.
//
// ---- The bound (inside_bound(), checked by tests/cpp/test_translate.cc)
// Let S = the sum of Kmers over to3[e0].  If start < S, the loop of step 3 stops INSIDE to3[e0]: take the least t with
// start < Kmers(to3[e0][0]) + ... + Kmers(to3[e0][t]); when the loop reaches trim = t (if it has not stopped before) what is left of start is
// below Kmers(p[t]) < Bases(p[t]), and it stops.  The first |to3[e0]| entries of p ARE to3[e0], whatever is appended behind them (the
// first OverlapAppend meets an empty p).  So for start < S the answer needs no OverlapAppend and no edge of the path but the first.
// k_path_verify counts offset >= kmers(e0) as a broken path (dfk_check_kernels.h), and dfk_patch.h's check_invariants holds that to3[e0]
// spells e0 from left3[e0], so S >= left3[e0] + kmers(e0) > start for every path the pather makes.  Those are all decided on the device.
// A read whose walk over to3[e0] alone runs off its end (walk_first() says so; only hand-made inputs have them) is flagged, its path comes
// back and literal() decides it on the host; DFK_TRANSLATE_HOST counts them and is 0 on a context's own paths.
//
// ---- The plan (dfk_translate_kernels.h, dfk_translate.inc)
// The batches are those of the paths, one result batch beside each.  Per batch, two passes over units of 256 reads (UNIT; unit u is the
// reads [256 u, 256 u + 256) of the batch; a workgroup of 256 lanes takes the units u = blockIdx.x, + gridDim.x, ...: grid_256 of
// dfk_paths_plan.h):
//   decide    a lane a read: the element's two bounds, its offset and first edge id, the gathers into to3_first / left3 / to3 / kmers3;
//             an 8-byte record {new offset, new edge or -1}; the unit's word count (record_words()) in words[u]; flagged reads' numbers
//             appended to a list.
//   (host)    flagged reads settled by literal(), k_tp_override writes their records and adds to their units' word counts.
//   layout    the project's exclusive scan over words[0 .. n_units].
//   emit      the unit's elements laid out in LDS and stored from there; elem_off; the content digest; Validate's count.
// The tables cross once a call.  records, words, the scan, the list and the counters are scratch of the largest batch, from the arena and
// back on return; the result's var / elem_off blocks stay until dfk_translate_drop, the next build or the paths' release.
//
// ---- The result: a second list of batches in the layout k_path_emit leaves (dfk_paths.inc): per read the words {offset, lastSkip = 0}
// and, where placed, one edge id; elem_off[i] the byte offset of read i's element in the batch's data.  a.patch.paths is the feudal file
// of it, written by the code that writes a.paths.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define DFK_TP_HD __host__ __device__ inline
#else
#define DFK_TP_HD inline
#endif

namespace dfk_translate {

constexpr uint32_t UNIT = 256;                                        // reads a unit: one pass of a 256-lane workgroup
constexpr int32_t LIMIT = 1 << 30;                                    // |offset| and left3 stay below it: start is an int
constexpr uint64_t DIGEST_SEED = 0x9E3779B97F4A7C15ull;               // k_paths_digest's (dfk_check_kernels.h)
constexpr uint64_t DIGEST_XOR = 0xD1B54A32D192ED03ull;

// ---- shared by host and kernels
DFK_TP_HD int32_t start_of(int32_t offset, int32_t left3) { return offset + left3; }                                    // :169
DFK_TP_HD int32_t bases_of(int32_t kmers, int32_t K) { return kmers + K - 1; }
DFK_TP_HD bool first_edge_takes(int32_t start, int32_t kmers_first, int32_t K) { return start < bases_of(kmers_first, K); }   // :175
struct Walk { int32_t edge, offset; };                                // edge -1: ran off the list
// the loop of :185-189 over to3[e0] alone (n >= 1 ids)
DFK_TP_HD Walk walk_first(const int32_t* ids, uint64_t n, const int32_t* kmers3, int32_t K, int32_t start)
{
    uint64_t trim = 0;
    while (start >= bases_of(kmers3[ids[trim]], K)) {
        start -= kmers3[ids[trim]];
        if (++trim == n) return Walk{-1, start};
    }
    return Walk{ids[trim], start};
}
DFK_TP_HD uint32_t record_words(int32_t edge) { return edge < 0 ? 2u : 3u; }
DFK_TP_HD bool valid_id(int32_t edge, int64_t n_edges3) { return !((int64_t)edge >= n_edges3); }                       // ReadPathTools.cc:44-48
DFK_TP_HD uint64_t mix64(uint64_t x)                                  // digest_mix (dfk_kernels.h)
{
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// the content digest of one read as k_paths_digest forms it: h(r, offset, lastSkip = 0, the edge if there is one)
DFK_TP_HD uint64_t read_digest(uint64_t r, int32_t offset, int32_t edge)
{
    uint64_t h = mix64(r + DIGEST_SEED);
    h = mix64(h ^ (uint64_t)(uint32_t)offset);
    h = mix64(h ^ 0ull);
    if (edge >= 0) h = mix64(h ^ (uint64_t)(uint32_t)edge);
    return h;
}
// start < inside_bound(to3[e0]) => walk_first() does not run off (the proof is above)
DFK_TP_HD int64_t inside_bound(const int32_t* ids, uint64_t n, const int32_t* kmers3)
{
    int64_t s = 0;
    for (uint64_t j = 0; j < n; ++j) s += kmers3[ids[j]];
    return s;
}

// ================================================================================================ host
struct Tables {                                                        // to3 / left3 of the old edges, Kmers of hb3's
    int32_t K = 0;
    std::vector<uint64_t> to3_first;                                   // [n_edges + 1]
    std::vector<int32_t> to3, left3, kmers3;
    uint64_t n_edges() const { return left3.size(); }
};
struct Path { int32_t offset = 0; std::vector<int32_t> edges; };
struct Outcome { int32_t offset, edge; };                              // edge -1: no path (cleared, or empty before)
enum Kind { EMPTY_BEFORE, CLEARED_EMPTY, STEP2, WALK, CLEARED_RANOFF };

// what does not hold together: "" or the reason (DFK_E_ARG)
inline std::string check_tables(const Tables& T)
{
    const uint64_t E = T.n_edges(), E3 = T.kmers3.size();
    if (T.K < 2) return "K is below 2";
    if (T.to3_first.size() != E + 1) return "to3_first is not n_edges + 1 long";
    if (T.to3_first[0] != 0) return "to3_first does not start at 0";
    for (uint64_t e = 0; e < E; ++e) if (T.to3_first[e + 1] < T.to3_first[e]) return "to3_first falls at edge " + std::to_string(e);
    if (T.to3_first[E] != T.to3.size()) return "to3_first does not end at the number of to3 entries";
    for (int32_t id : T.to3) if (id < 0 || (uint64_t)id >= E3) return "to3 holds " + std::to_string(id) + ": hb3 has " + std::to_string(E3) + " edges";
    for (int32_t k : T.kmers3) if (k < 1 || k >= LIMIT) return "an hb3 edge of " + std::to_string(k) + " K-mers";
    for (int32_t l : T.left3) if (l <= -LIMIT || l >= LIMIT) return "left3 of " + std::to_string(l) + ": below 2^30 in size";
    return "";
}
inline std::string check_path(const Tables& T, const Path& p)
{
    if (p.offset <= -LIMIT || p.offset >= LIMIT) return "an offset of " + std::to_string(p.offset) + ": below 2^30 in size";
    for (int32_t e : p.edges) if (e < 0 || (uint64_t)e >= T.n_edges()) return "a path holds edge " + std::to_string(e) + ": the graph has " + std::to_string(T.n_edges());
    return "";
}

// Vec.h:593-606 as written
inline size_t overlap_append(std::vector<int32_t>& v1, const int32_t* v2, size_t v2_size)
{
    size_t best = 0;
    const size_t v1_size = v1.size(), max_overl = std::min(v1_size, v2_size);
    for (size_t overl = max_overl; overl; --overl)
        if (std::equal(v1.end() - overl, v1.end(), v2)) { best = overl; break; }
    v1.insert(v1.end(), v2 + best, v2 + v2_size);
    return best;
}

// GapToyTools4.cc:167-196 for one read, as written
inline Outcome literal(const Tables& T, const Path& path, Kind* kind = nullptr)
{
    Kind k_; Kind& k = kind ? *kind : k_;
    if (path.edges.empty()) { k = EMPTY_BEFORE; return Outcome{path.offset, -1}; }                                      // :168
    const int32_t e0 = path.edges[0];
    int start = path.offset + T.left3[e0];                                                                              // :169
    const int32_t* first = T.to3.data() + T.to3_first[e0];
    if (T.to3_first[e0 + 1] == T.to3_first[e0]) { k = CLEARED_EMPTY; return Outcome{path.offset, -1}; }                 // :171-173
    if (start < T.kmers3[first[0]] + T.K - 1) { k = STEP2; return Outcome{start, first[0]}; }                           // :175-179
    std::vector<int32_t> p;                                                                                             // :181
    for (int j = 0; j < (int)path.edges.size(); ++j) {                                                                  // :182
        const int32_t e = path.edges[j];
        if (T.to3_first[e + 1] == T.to3_first[e]) break;                                                                // :183
        overlap_append(p, T.to3.data() + T.to3_first[e], (size_t)(T.to3_first[e + 1] - T.to3_first[e]));               // :184
    }
    int trim = 0;                                                                                                       // :185
    while (start >= T.kmers3[p[trim]] + T.K - 1) {                                                                      // :186
        start -= T.kmers3[p[trim]];                                                                                     // :187
        trim++;                                                                                                         // :188
        if (trim == (int)p.size()) break;                                                                               // :189
    }
    if (trim == (int)p.size()) { k = CLEARED_RANOFF; return Outcome{path.offset, -1}; }                                 // :191-193
    k = WALK;
    return Outcome{start, p[trim]};                                                                                     // :194-196
}

// The device's order of work on the host: the shared pieces decide; *flagged = the host route is needed (the outcome is then unset)
inline Outcome decide(const Tables& T, int32_t offset, bool has_path, int32_t e0, bool* flagged, Kind* kind)
{
    *flagged = false;
    if (!has_path) { *kind = EMPTY_BEFORE; return Outcome{offset, -1}; }
    const uint64_t t0 = T.to3_first[e0], t1 = T.to3_first[e0 + 1];
    if (t1 == t0) { *kind = CLEARED_EMPTY; return Outcome{offset, -1}; }
    const int32_t start = start_of(offset, T.left3[e0]);
    if (first_edge_takes(start, T.kmers3[T.to3[t0]], T.K)) { *kind = STEP2; return Outcome{start, T.to3[t0]}; }
    const Walk w = walk_first(T.to3.data() + t0, t1 - t0, T.kmers3.data(), T.K, start);
    if (w.edge < 0) { *flagged = true; *kind = CLEARED_RANOFF; return Outcome{offset, -1}; }
    *kind = WALK;
    return Outcome{w.offset, w.edge};
}
// decide(), and literal() where it flags: what the library computes
inline Outcome translate_one(const Tables& T, const Path& p, Kind* kind, bool* host_route)
{
    const Outcome o = decide(T, p.offset, !p.edges.empty(), p.edges.empty() ? 0 : p.edges[0], host_route, kind);
    return *host_route ? literal(T, p, kind) : o;
}

// ---- the plan
struct Plan { uint64_t n_units, scan_words; };                        // of a batch of n reads: its units, and the scan's input (a total behind them)
inline Plan plan_of(uint64_t n_reads_in_batch) { const uint64_t u = (n_reads_in_batch + UNIT - 1) / UNIT; return Plan{u, u + 1}; }
// the host route's part of the layout: a flagged read was counted with 2 words; its unit gets one more where literal() placed it
inline uint64_t unit_of(uint64_t read_in_batch) { return read_in_batch / UNIT; }

} // namespace dfk_translate
