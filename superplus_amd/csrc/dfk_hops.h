// superplus_amd/csrc/dfk_hops.h -- FindEdgePairs (lib/assembly/src/10X/Closomatic.cc:17-358) as functions of plain arrays.
//
// No HIP call and no device pointer is dereferenced here by the host, so tests/cpp/test_hops.cc compiles this header with a
// plain host compiler (and once more under -fsanitize=address,undefined) and checks it against cases recorded from
// tests/hops_oracle.py.  It is the SECOND restatement of the rule -- written from the reference's text, not from the Python --
// and it serves three ends:
//   * the per-edge part of method 3 (build X, the search, too_easy / can / rights) is ONE function, edge_pairs(), written
//     against an executor: HostExec runs it on one thread, the kernel k_hops_edges (dfk_hops_kernels.h) runs the same text
//     on a wave of 64 lanes with its sets in LDS.  The control flow is the same for every lane; the lanes share the
//     membership tests and the copies.  What the sanitizer sees here is therefore what the wave executes;
//   * an edge whose sets do not fit the capacities is never truncated: edge_pairs() says HOPS_OVERFLOW before it emits
//     anything, and the host decides that edge with edge_pairs_exact() -- the same function, the capacity it met doubled until it fits;
//   * find_edge_pairs_host(): all three methods on the host, for the CPU test.
//
// The rule (N reads, mate of id = id ^ 1, kmers(e) = length - K + 1, bid[id] = N + bc[id]: only equality matters, so bc
// itself stands for it):
//   sink test of e1 (:63-74)     every edge e in From(ToRight(e1)), far vertex w: From(w) empty, |To(w)| <= 1, kmers(e) <= 120
//   source test of e2 (:101-111) every edge e in To(ToLeft(e2)), far vertex w: To(w) empty, |From(w)| <= 1, kmers(e) <= 120
//   mate set of e1 (:77-91)      over the reads on e1 with a placed mate: (e2 = inv[last edge of the mate's path], bid), e2 != e1
//   method 1 (:54-120)           e1 passes the sink test, e2 seen with >= 2 distinct bid, ONE_GOOD or e2 passes the source test
//   method 2 (:126-179)          e1 passes the sink test and got nothing from method 1; e2 seen with >= 2 distinct bid,
//                                kmers(e2) >= 100, ToRight(e1) != ToLeft(e2)
//   method 3 (:191-341)          edge_pairs() below
//   pairs = the sorted set union (:345)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DFK_HOPS_HD __host__ __device__ inline
#else
#define DFK_HOPS_HD inline
#endif

namespace dfk_hops {

constexpr int MAX_DIST_TO_END = 120;    // :51
constexpr int MIN_LANDING = 100;        // :52
constexpr int GOOD_EXT = 100;           // :199
constexpr int MIN_RIGHT = 40;           // :200
constexpr int MAX_ROUNDS = 100;         // a sequence grows by an edge of at least one k-mer a round: GOOD_EXT is reached by then

// the graph as the paths tables hold it: per edge kmers / inv / to_left / to_right, per vertex the rows From / To (far vertex,
// edge), from_start[v] .. from_start[v + 1]
struct Graph {
    const int32_t* kmers; const int32_t* inv; const int32_t* to_left; const int32_t* to_right;
    const uint32_t* from_start; const int32_t* from_vtx; const int32_t* from_edge;
    const uint32_t* to_start; const int32_t* to_vtx; const int32_t* to_edge;
};

DFK_HOPS_HD bool sink_ok(const Graph& g, int32_t e1)
{
    const int32_t v = g.to_right[e1];
    for (uint32_t j = g.from_start[v]; j < g.from_start[v + 1]; ++j) {
        const int32_t w = g.from_vtx[j];
        if (g.from_start[w + 1] - g.from_start[w] > 0 || g.to_start[w + 1] - g.to_start[w] > 1) return false;
        if (g.kmers[g.from_edge[j]] > MAX_DIST_TO_END) return false;
    }
    return true;
}

DFK_HOPS_HD bool source_ok(const Graph& g, int32_t e2)
{
    const int32_t v = g.to_left[e2];
    for (uint32_t j = g.to_start[v]; j < g.to_start[v + 1]; ++j) {
        const int32_t w = g.to_vtx[j];
        if (g.to_start[w + 1] - g.to_start[w] > 0 || g.from_start[w + 1] - g.from_start[w] > 1) return false;
        if (g.kmers[g.to_edge[j]] > MAX_DIST_TO_END) return false;
    }
    return true;
}

// ---- method 3 on one edge
// Capacities, in slots: a set of sequences keeps one slot for the sequence being tried, so it HOLDS one fewer.
struct Caps {
    int x_slots, x_len;          // X: sequences, edges a sequence          (DFK_HOPS_MAX_SEQS, DFK_HOPS_MAX_LEN)
    int ext_slots, ext_len;      // exts / exts2
    int can, easy;               // distinct f of can, members of too_easy
    DFK_HOPS_HD uint64_t words() const
    {
        return (uint64_t)x_slots * x_len + x_slots + 2ull * ((uint64_t)ext_slots * ext_len + ext_slots) + 3ull * can + easy;
    }
};
DFK_HOPS_HD Caps caps_of(int max_seqs, int max_len)
{
    Caps c;
    c.x_slots = max_seqs < 1 ? 1 : max_seqs; c.x_len = max_len < 1 ? 1 : max_len;
    c.ext_slots = 32; c.ext_len = 2 * c.x_len < 32 ? 32 : 2 * c.x_len;
    c.can = 128; c.easy = 128;
    return c;
}

// the sets of one edge, carved out of words() 32-bit words (LDS on the device)
struct Work {
    int32_t *x, *x_n, *a, *a_n, *b, *b_n, *can_f, *can_b, *can_m, *easy;
    DFK_HOPS_HD Work(int32_t* p, const Caps& c)
    {
        x = p; p += (uint64_t)c.x_slots * c.x_len; x_n = p; p += c.x_slots;
        a = p; p += (uint64_t)c.ext_slots * c.ext_len; a_n = p; p += c.ext_slots;
        b = p; p += (uint64_t)c.ext_slots * c.ext_len; b_n = p; p += c.ext_slots;
        can_f = p; p += c.can; can_b = p; p += c.can; can_m = p; p += c.can; easy = p;
    }
};

struct HostExec {
    static constexpr int lanes = 1;
    int lane() const { return 0; }
    bool any(bool b) const { return b; }
    void sync() const {}
};

enum { HOPS_SKIP = 0, HOPS_EXTENDED = 1, HOPS_NOT_EXTENDED = 2, HOPS_OVERFLOW = -1, HOPS_INTERNAL = -2 };
enum { OVER_X_SLOTS = 1, OVER_X_LEN, OVER_EXT_SLOTS, OVER_EXT_LEN, OVER_CAN, OVER_EASY };    // EdgeStat::over: which capacity HOPS_OVERFLOW met
struct EdgeStat { int n_x = 0, longest_x = 0, rounds = 0, most_exts = 0, longest_ext = 0, over = 0; };

// the sequence staged in slot n of a set of n members: 1 = new (n grows), 0 = already a member, -1 = new and no slot left
template <class Ex>
DFK_HOPS_HD int commit_seq(const Ex& ex, const int32_t* buf, const int32_t* len, int& n, int slots, int stride)
{
    const int32_t* c = buf + (uint64_t)n * stride;
    const int cl = len[n];
    bool dup = false;
    for (int i = ex.lane(); i < n; i += Ex::lanes) {
        if (len[i] != cl) continue;
        const int32_t* o = buf + (uint64_t)i * stride;
        bool eq = true;
        for (int k = 0; k < cl; ++k) if (o[k] != c[k]) { eq = false; break; }
        if (eq) dup = true;
    }
    if (ex.any(dup)) return 0;
    if (n + 1 >= slots) return -1;
    ++n;
    return 1;
}

// Paths: int len(uint32_t id, const int32_t** edges) -- a read's path.  Bad: bool operator()(uint32_t pair).
// list: the reads on e (entry = id << 1) and the reads on inv[e] (entry = id << 1 | 1), in any order, a read once or more per
// crossing: everything below is a set.  emit(e, f) is called by lane 0, and only when the edge is decided (never before an overflow).
template <class Ex, class Paths, class Bad, class Emit>
DFK_HOPS_HD int edge_pairs(const Ex& ex, const Graph& g, int K, int32_t e, const uint32_t* list, uint64_t n_list, const Paths& paths,
                           const int32_t* bc, const Bad& bad, const Caps& cp, const Work& w, Emit& emit, EdgeStat* st)
{
    if (g.kmers[e] < K + 1) return HOPS_SKIP;                                 // :198, :204  MIN_CAND
    auto over = [&](int which) { if (st) st->over = which; return (int)HOPS_OVERFLOW; };
    const int32_t re = g.inv[e];
    {   // :250-251  at least two barcodes among the reads on e and on re
        bool two = false;
        const int32_t first = n_list ? bc[list[0] >> 1] : 0;
        for (uint64_t i = 1; i < n_list && !two; ++i) two = bc[list[i] >> 1] != first;
        if (!two) return HOPS_SKIP;
    }
    // ---- X (:217-246)
    int nx = 0, longest = 0, sx;
    auto over_x = [&](int r) { return over(r == -2 ? OVER_X_LEN : OVER_X_SLOTS); };
    auto stage_x = [&](const int32_t* p, int from, int n, int step, bool invert) -> int {     // p[from], p[from + step], ... n of them
        if (n > cp.x_len) return -2;
        int32_t* s = w.x + (uint64_t)nx * cp.x_len;
        ex.sync();
        for (int k = ex.lane(); k < n; k += Ex::lanes) { const int32_t f = p[from + k * step]; s[k] = invert ? g.inv[f] : f; }
        if (ex.lane() == 0) w.x_n[nx] = n;
        ex.sync();
        const int r = commit_seq(ex, w.x, w.x_n, nx, cp.x_slots, cp.x_len);
        if (r > 0 && n > longest) longest = n;
        return r;
    };
    for (uint64_t i = 0; i < n_list; ++i) {
        const uint32_t id = list[i] >> 1;
        const int32_t* p; const int np = paths.len(id, &p);
        if (!(list[i] & 1u)) {
            for (int j = 0; j < np; ++j)
                if (p[j] == e && (sx = stage_x(p, j, np - j, 1, false)) < 0) return over_x(sx);
            const int32_t* p2; const int n2 = paths.len(id ^ 1u, &p2);
            if (n2 > 0 && (sx = stage_x(p2, n2 - 1, n2, -1, true)) < 0) return over_x(sx);
        } else {
            for (int j = 0; j < np; ++j)
                if (p[j] == re && (sx = stage_x(p, j, j + 1, -1, true)) < 0) return over_x(sx);
        }
    }
    if (st) { st->n_x = nx; st->longest_x = longest; }
    // ---- the search (:256-292)
    int32_t *A = w.a, *An = w.a_n, *B = w.b, *Bn = w.b_n;
    int na = 0;
    ex.sync();
    for (int i = 0; i < nx; ++i) {
        const int32_t* x = w.x + (uint64_t)i * cp.x_len;
        if (x[0] != e) continue;
        if (na + 1 >= cp.ext_slots) return over(OVER_EXT_SLOTS);
        if (w.x_n[i] > cp.ext_len) return over(OVER_EXT_LEN);
        for (int k = ex.lane(); k < w.x_n[i]; k += Ex::lanes) A[(uint64_t)na * cp.ext_len + k] = x[k];
        if (ex.lane() == 0) An[na] = w.x_n[i];
        ++na;
    }
    ex.sync();
    bool extended = false;
    int rounds = 0, most = na, longest_ext = 0;
    for (int i = 0; i < na; ++i) if (An[i] > longest_ext) longest_ext = An[i];
    for (;;) {
        bool good = false;
        for (int i = ex.lane(); i < na; i += Ex::lanes) {
            const int32_t* x = A + (uint64_t)i * cp.ext_len;
            int n = 0;
            for (int j = 1; j < An[i]; ++j) n += g.kmers[x[j]];
            if (n >= GOOD_EXT) good = true;
        }
        if (ex.any(good)) { extended = true; break; }
        int nb = 0;
        for (int i = 0; i < na; ++i) {
            const int32_t* x = A + (uint64_t)i * cp.ext_len;
            const int xl = An[i];
            const int32_t f = x[xl - 1];
            for (int j = 0; j < nx; ++j) {
                const int32_t* y = w.x + (uint64_t)j * cp.x_len;
                const int yl = w.x_n[j];
                for (int l = 0; l < yl - 1; ++l) {
                    if (y[l] != f) continue;
                    bool mismatch = false;
                    for (int m = 0; m < yl; ++m) {                            // :279-285
                        const int n = m + xl - 1 - l;
                        if (n < 0 || n >= xl) continue;
                        if (x[n] != y[m]) { mismatch = true; break; }
                    }
                    if (mismatch) continue;
                    const int nl = xl + yl - 1 - l;
                    if (nl > cp.ext_len) return over(OVER_EXT_LEN);
                    int32_t* s = B + (uint64_t)nb * cp.ext_len;
                    ex.sync();
                    for (int k = ex.lane(); k < nl; k += Ex::lanes) s[k] = k < xl ? x[k] : y[l + 1 + (k - xl)];
                    if (ex.lane() == 0) Bn[nb] = nl;
                    ex.sync();
                    const int r = commit_seq(ex, B, Bn, nb, cp.ext_slots, cp.ext_len);
                    if (r < 0) return over(OVER_EXT_SLOTS);
                    if (r > 0 && nl > longest_ext) longest_ext = nl;
                }
            }
        }
        if (!nb) break;
        int32_t* t = A; A = B; B = t; t = An; An = Bn; Bn = t;
        na = nb;
        if (na > most) most = na;
        if (++rounds > MAX_ROUNDS) return HOPS_INTERNAL;
    }
    if (st) { st->rounds = rounds; st->most_exts = most; st->longest_ext = longest_ext; }
    if (extended) return HOPS_EXTENDED;
    // ---- possible rights (:297-338): only reads whose pair is not bad count from here on
    int n_can = 0, n_easy = 0;
    auto wanted = [&](int32_t f) { return g.kmers[f] >= MIN_RIGHT && f != e && f != re; };
    auto add_easy = [&](int32_t f) -> bool {
        ex.sync();
        bool have = false;
        for (int i = ex.lane(); i < n_easy; i += Ex::lanes) if (w.easy[i] == f) have = true;
        if (ex.any(have)) return true;
        if (n_easy >= cp.easy) return false;
        if (ex.lane() == 0) w.easy[n_easy] = f;
        ++n_easy;
        return true;
    };
    auto add_can = [&](int32_t f, int32_t b) -> bool {
        ex.sync();
        bool have = false;
        for (int i = ex.lane(); i < n_can; i += Ex::lanes)
            if (w.can_f[i] == f) { have = true; if (w.can_b[i] != b) w.can_m[i] = 1; }
        if (ex.any(have)) return true;
        if (n_can >= cp.can) return false;
        if (ex.lane() == 0) { w.can_f[n_can] = f; w.can_b[n_can] = b; w.can_m[n_can] = 0; }
        ++n_can;
        return true;
    };
    for (uint64_t i = 0; i < n_list; ++i) {
        const uint32_t id = list[i] >> 1;
        if (bad(id >> 1)) continue;
        const int32_t* p; const int np = paths.len(id, &p);
        if (!(list[i] & 1u)) {
            for (int j = 0; j < np; ++j) {
                if (p[j] != e) continue;
                for (int l = j + 1; l < np; ++l) if (wanted(p[l]) && !add_easy(p[l])) return over(OVER_EASY);
            }
            const int32_t* p2; const int n2 = paths.len(id ^ 1u, &p2);
            for (int l = n2 - 1; l >= 0; --l) { const int32_t f = g.inv[p2[l]]; if (wanted(f) && !add_can(f, bc[id])) return over(OVER_CAN); }
        } else {
            for (int j = 0; j < np; ++j) {
                if (p[j] != re) continue;
                for (int l = j; l >= 0; --l) { const int32_t f = g.inv[p[l]]; if (wanted(f) && !add_can(f, bc[id])) return over(OVER_CAN); }
            }
        }
    }
    ex.sync();
    for (int i = 0; i < n_can; ++i) {
        if (!w.can_m[i]) continue;
        const int32_t f = w.can_f[i];
        bool easy = false;
        for (int k = ex.lane(); k < n_easy; k += Ex::lanes) if (w.easy[k] == f) easy = true;
        if (ex.any(easy)) continue;
        if (ex.lane() == 0) emit(e, f);
    }
    return HOPS_NOT_EXTENDED;
}

} // namespace dfk_hops

// ---------------------------------------------------------------------------------------------------------------- host only
#include <algorithm>
#include <map>
#include <set>
#include <utility>
#include <vector>

namespace dfk_hops {

// edge_pairs() again with the capacity that overflowed doubled (EdgeStat::over names it; the others keep their size), until the
// edge fits: the exact route for an edge the device could not hold.  The sets stay arrays searched in full, so an edge costs
// about |list| x |X| comparisons of sequences to build X and |exts| x |X| x length a round: fine for the hundreds to thousands of
// sequences a repeat edge of a fixture-sized or bacterial graph gives, minutes for 1e5.  EXACT_MAX_WORDS (1 GiB of sets) is
// where it gives up and says so (HOPS_INTERNAL) rather than run out of memory: that is 4 million sequences of 64 edges in X,
// or 5e5 of 512.
constexpr uint64_t EXACT_MAX_WORDS = 1ull << 28;
template <class Paths, class Bad>
int edge_pairs_exact(const Graph& g, int K, int32_t e, const uint32_t* list, uint64_t n_list, const Paths& paths, const int32_t* bc, const Bad& bad,
                     std::vector<std::pair<int32_t, int32_t>>* out, EdgeStat* st, Caps* fitted = nullptr /* the capacities it fitted */)
{
    Caps cp = caps_of(256, 64);
    EdgeStat mine;
    if (!st) st = &mine;
    while (cp.words() <= EXACT_MAX_WORDS) {
        std::vector<int32_t> room(cp.words());
        const Work w(room.data(), cp);
        std::vector<std::pair<int32_t, int32_t>> got;
        auto emit = [&](int32_t a, int32_t b) { got.emplace_back(a, b); };
        *st = EdgeStat();
        const int r = edge_pairs(HostExec{}, g, K, e, list, n_list, paths, bc, bad, cp, w, emit, st);
        if (r != HOPS_OVERFLOW) { out->insert(out->end(), got.begin(), got.end()); if (fitted) *fitted = cp; return r; }
        int* grow = st->over == OVER_X_SLOTS ? &cp.x_slots : st->over == OVER_X_LEN ? &cp.x_len : st->over == OVER_EXT_SLOTS ? &cp.ext_slots :
                    st->over == OVER_EXT_LEN ? &cp.ext_len : st->over == OVER_CAN ? &cp.can : st->over == OVER_EASY ? &cp.easy : nullptr;
        if (!grow || *grow > (1 << 29)) return HOPS_INTERNAL;
        *grow *= 2;
    }
    return HOPS_INTERNAL;
}

struct CsrPaths {                                   // every path in host memory: first[id] .. first[id + 1] of edges
    const uint64_t* first; const int32_t* edges;
    int len(uint32_t id, const int32_t** p) const { *p = edges + first[id]; return (int)(first[id + 1] - first[id]); }
};

struct HostResult {
    std::vector<std::pair<int32_t, int32_t>> m1, m2, m3, pairs;
    uint64_t searched = 0, extended = 0, most_rounds = 0, largest_x = 0, largest_exts = 0, longest = 0, host_edges = 0;
};

// All three methods on the host.  max_seqs / max_len: the capacities an edge is tried with first (as the device would); an
// edge that overflows them is counted in host_edges and decided by edge_pairs_exact.
inline int find_edge_pairs_host(const Graph& g, int32_t n_edges, int K, const CsrPaths& paths, uint64_t n_reads, const int32_t* bc, const uint8_t* bad_pairs,
                                bool one_good, int max_seqs, int max_len, HostResult* R)
{
    // the combined index: per edge the reads on it (<< 1) and the reads on its involution (<< 1 | 1)
    std::vector<std::vector<uint32_t>> idx((size_t)n_edges);
    for (uint64_t id = 0; id < n_reads; ++id) {
        const int32_t* p; const int n = paths.len((uint32_t)id, &p);
        for (int j = 0; j < n; ++j) { idx[(size_t)p[j]].push_back((uint32_t)id << 1); idx[(size_t)g.inv[p[j]]].push_back((uint32_t)id << 1 | 1u); }
    }
    auto bad = [&](uint32_t pair) { return bad_pairs[pair] != 0; };
    std::vector<uint8_t> seen((size_t)n_edges, 0);
    std::vector<std::vector<int32_t>> supported((size_t)n_edges);
    for (int32_t e1 = 0; e1 < n_edges; ++e1) {
        if (!sink_ok(g, e1)) continue;
        std::set<std::pair<int32_t, int32_t>> e2s;                                       // :77-91
        for (uint32_t v : idx[(size_t)e1]) {
            if (v & 1u) continue;
            const int32_t* p2; const int n2 = paths.len((v >> 1) ^ 1u, &p2);
            if (n2 > 0) { const int32_t e2 = g.inv[p2[n2 - 1]]; if (e2 != e1) e2s.insert({e2, bc[v >> 1]}); }
        }
        std::map<int32_t, int> n_of;
        for (const auto& x : e2s) ++n_of[x.first];
        for (const auto& x : n_of) if (x.second >= 2) supported[(size_t)e1].push_back(x.first);
        for (int32_t e2 : supported[(size_t)e1])
            if (one_good || source_ok(g, e2)) { R->m1.emplace_back(e1, e2); seen[(size_t)e1] = 1; }
    }
    for (int32_t e1 = 0; e1 < n_edges; ++e1) {                                           // :126-179 (the sink test was the filter above)
        if (seen[(size_t)e1]) continue;
        for (int32_t e2 : supported[(size_t)e1])
            if (g.kmers[e2] >= MIN_LANDING && e2 != e1 && g.to_right[e1] != g.to_left[e2]) R->m2.emplace_back(e1, e2);
    }
    const Caps cp = caps_of(max_seqs, max_len);
    std::vector<int32_t> room(cp.words());
    const Work w(room.data(), cp);
    for (int32_t e = 0; e < n_edges; ++e) {
        const std::vector<uint32_t>& l = idx[(size_t)e];
        EdgeStat st;
        std::vector<std::pair<int32_t, int32_t>> got;
        auto emit = [&](int32_t a, int32_t b) { got.emplace_back(a, b); };
        int r = edge_pairs(HostExec{}, g, K, e, l.data(), l.size(), paths, bc, bad, cp, w, emit, &st);
        if (r == HOPS_OVERFLOW) { ++R->host_edges; got.clear(); st = EdgeStat(); r = edge_pairs_exact(g, K, e, l.data(), l.size(), paths, bc, bad, &got, &st); }
        if (r < 0) return r;
        if (r == HOPS_SKIP) continue;
        ++R->searched; R->extended += r == HOPS_EXTENDED;
        R->most_rounds = std::max<uint64_t>(R->most_rounds, (uint64_t)st.rounds); R->largest_x = std::max<uint64_t>(R->largest_x, (uint64_t)st.n_x);
        R->largest_exts = std::max<uint64_t>(R->largest_exts, (uint64_t)st.most_exts); R->longest = std::max<uint64_t>(R->longest, (uint64_t)st.longest_x);
        R->m3.insert(R->m3.end(), got.begin(), got.end());
    }
    std::sort(R->m3.begin(), R->m3.end());
    R->pairs = R->m1; R->pairs.insert(R->pairs.end(), R->m2.begin(), R->m2.end()); R->pairs.insert(R->pairs.end(), R->m3.begin(), R->m3.end());
    std::sort(R->pairs.begin(), R->pairs.end());
    R->pairs.erase(std::unique(R->pairs.begin(), R->pairs.end()), R->pairs.end());
    return 0;
}

// the digest of a pair list: (sum, xor) over the pairs of a 64-bit mix -- order-independent, disjoint sets add / xor
inline uint64_t mix64(uint64_t x)
{
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; return x ^ (x >> 31);
}
inline void pairs_digest(const std::vector<std::pair<int32_t, int32_t>>& pairs, uint64_t out[2])
{
    out[0] = out[1] = 0;
    for (const auto& p : pairs) {
        const uint64_t h = mix64((((uint64_t)(uint32_t)p.first << 32) | (uint32_t)p.second) + 0x9E3779B97F4A7C15ull);
        out[0] += h; out[1] ^= mix64(h + 0xD1B54A32D192ED03ull);
    }
}

} // namespace dfk_hops
