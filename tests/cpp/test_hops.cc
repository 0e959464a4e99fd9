// tests/cpp/test_hops.cc -- superplus_amd/csrc/dfk_hops.h (FindEdgePairs, 10X/Closomatic.cc:17-358, restated in C++) on the host:
// a graph and three searches worked out by hand, then the seeded graphs of tests/hops_cases.py (dense random ones, gapped chains) against what tests/hops_oracle.py said about them
// (tests/cpp/hops_cases.txt).  Built plain and under -fsanitize=address,undefined by tests/test_hops_cpu.py.
//   g++ -std=c++17 -O1 -g -I superplus_amd/csrc -o test_hops tests/cpp/test_hops.cc && ./test_hops tests/cpp/hops_cases.txt
#include "dfk_hops.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

using namespace dfk_hops;
using Pairs = std::vector<std::pair<int32_t, int32_t>>;

static int g_failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_failed; fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } while (0)

struct Case {
    int K = 0, one_good = 0, max_seqs = 0, max_len = 0;
    std::vector<int32_t> kmers, inv, to_left, to_right, bc;
    std::vector<uint8_t> bad;
    std::vector<uint64_t> first; std::vector<int32_t> edges;
    std::vector<uint32_t> from_start, to_start; std::vector<int32_t> from_vtx, from_edge, to_vtx, to_edge;
    int n_vertices = 0;

    void set_paths(const std::vector<std::vector<int32_t>>& paths)
    {
        first.assign(1, 0); edges.clear();
        for (const auto& p : paths) { edges.insert(edges.end(), p.begin(), p.end()); first.push_back(edges.size()); }
        edges.push_back(0);                                   // (so that an empty set of paths still has an address)
    }
    void rows()
    {
        const size_t E = kmers.size(), V = (size_t)n_vertices;
        from_start.assign(V + 1, 0); to_start.assign(V + 1, 0);
        for (size_t e = 0; e < E; ++e) { ++from_start[(size_t)to_left[e] + 1]; ++to_start[(size_t)to_right[e] + 1]; }
        for (size_t v = 0; v < V; ++v) { from_start[v + 1] += from_start[v]; to_start[v + 1] += to_start[v]; }
        from_vtx.assign(E + 1, 0); from_edge.assign(E + 1, 0); to_vtx.assign(E + 1, 0); to_edge.assign(E + 1, 0);
        std::vector<uint32_t> fa(from_start.begin(), from_start.end() - 1), ta(to_start.begin(), to_start.end() - 1);
        for (size_t e = 0; e < E; ++e) {
            const uint32_t f = fa[(size_t)to_left[e]]++, t = ta[(size_t)to_right[e]]++;
            from_vtx[f] = to_right[e]; from_edge[f] = (int32_t)e; to_vtx[t] = to_left[e]; to_edge[t] = (int32_t)e;
        }
    }
    Graph graph() const
    {
        return Graph{kmers.data(), inv.data(), to_left.data(), to_right.data(), from_start.data(), from_vtx.data(), from_edge.data(), to_start.data(), to_vtx.data(), to_edge.data()};
    }
    int run(HostResult* R) const
    {
        const CsrPaths P{first.data(), edges.data()};
        return find_edge_pairs_host(graph(), (int32_t)kmers.size(), K, P, first.size() - 1, bc.data(), bad.data(), one_good != 0, max_seqs, max_len, R);
    }
};

static std::string show(const Pairs& p)
{
    std::string s;
    for (size_t i = 0; i < p.size() && i < 12; ++i) s += "(" + std::to_string(p[i].first) + "," + std::to_string(p[i].second) + ")";
    return s + " [" + std::to_string(p.size()) + "]";
}

// A chain worked out by hand.  K = 4 (MIN_CAND = 5).  Vertices 0..7, every edge with its involution:
//   e0: 0 -> 1, 50 k-mers      e1 = inv: 6 -> 7
//   e2: 1 -> 2, 60 k-mers      e3 = inv: 5 -> 6        (e2 follows e0)
//   e4: 3 -> 4, 110 k-mers     e5 = inv: 4' .. kept apart: 8 -> 9
// Reads (pairs (0,1), (2,3), (4,5), (6,7)), barcodes 1, 1, 2, 2, 3, 3, 0, 0:
//   r0 = [e0, e2]   r1 = [e5]          the mate lies on inv[e4]: seen from r0 the far edge is inv[e5] = e4
//   r2 = [e0]       r3 = [e5]
//   r4 = [e2]       r5 = []
//   r6 = [e0, e2]   r7 = []
// Method 1, e1 = e2: ToRight(e2) = vertex 2 has nothing after it: the sink test passes.  Reads on e2: r0 (mate r1, e2' = inv[e5] = e4,
//   barcode 1), r4 (mate unplaced), r6 (mate unplaced): e4 is seen with one barcode only: not supported.  Nothing.
// Method 1, e1 = e0: From(ToRight(e0)) = {e2}, its far vertex 2 has no edge leaving and one entering, kmers(e2) = 60 <= 120: passes.
//   Reads on e0: r0 (e4, bc 1), r2 (e4, bc 2), r6 (unplaced mate): e4 supported by two barcodes.  Source test of e4: nothing enters
//   vertex 3: passes.  Method 1 emits (e0, e4); method 2 has nothing left for e0.
// Method 3, e = e0 (50 k-mers >= 5): reads on e0: r0, r2, r6 (barcodes 1, 2, 0); on inv[e0] = e1: none.
//   X = {[e0, e2], [e0], [e4]} ([e4] = r1 and r3 reversed and involuted).  exts = {[e0, e2], [e0]}: [e0, e2] has 60 k-mers behind
//   e0: short of 100.  Round 1: [e0, e2] ends in e2, which no member of X holds before its last place; [e0] ends in e0: y = [e0, e2]
//   at l = 0 agrees: exts2 = {[e0, e2]}, which replaces exts (one round).  Then nothing can be made from [e0, e2]: exts2 = {}: not
//   extended.  too_easy = {e2} (kmers 60 >= 40, behind e0 in r0 and r6).  can = {(e4, 1), (e4, 2)}: e4 has two barcodes and
//   is not too easy: method 3 emits (e0, e4).
// Method 3, e = e4 (110 k-mers): reads on e4: none; on inv[e4] = e5: r1, r3 (barcodes 1, 2).  X = {[e4]} (inv of [e5] read backwards
//   from the occurrence).  exts = {[e4]}: nothing behind it, no member of X goes on: not extended, no round.  can: from the reads
//   on e5 only inv[e5] = e4 itself, which is excluded: nothing.
// Method 3, e = e2: reads r0, r4, r6, barcodes 1, 3, 0.  X = {[e2], [e4]}; exts = {[e2]}; no extension; can = {(e4, 1)}: one barcode.
// Method 3, e = e5 / e1 / e3: e5 has reads r1, r3 on it; X = {[e5], inv-reversed mates: r0 -> [e3, e1], r2 -> [e1]}; exts = {[e5]};
//   not extended; can = {(e3, 1), (e1, 1), (e1, 2)}: e1 (50 k-mers >= 40) has two barcodes: emits (e5, e1).  e3 (60) has one.
//   e1 and e3 carry no reads themselves but inv[e1] = e0 does: for e = e1: reads on re = e0: r0, r2, r6; X = {[e1] (from r2, r0 at j = 0;
//   r6 too)}, can = {(e1 itself excluded)} -> nothing.  For e = e3: reads on re = e2: r0 (j = 1: [e3, e1]), r4 ([e3]), r6 ([e3, e1]);
//   X = {[e3, e1], [e3]}; [e3, e1] has 50 k-mers behind e3: short; one round: [e3] + y = [e3, e1] -> {[e3, e1]}, then nothing;
//   not extended; can: (e1, 1), (e1, 0) -- r4 contributes only e3 itself -- two barcodes (one of them the shared id of the
//   unbarcoded reads): emits (e3, e1).
// Pair (2, 3) is then marked bad: r2 no longer counts for can.  (e0, e4) of method 3 loses barcode 2 and goes; method 1 keeps
// (e0, e4), which does not look at the marks; (e5, e1) loses (e1, 2) -- r3 is in the bad pair -- and goes; (e3, e1) stays.
static void hand_case()
{
    Case c;
    c.K = 4; c.max_seqs = 96; c.max_len = 24; c.n_vertices = 10;
    c.kmers = {50, 50, 60, 60, 110, 110};
    c.inv = {1, 0, 3, 2, 5, 4};
    c.to_left = {0, 6, 1, 5, 3, 8};
    c.to_right = {1, 7, 2, 6, 4, 9};
    c.bc = {1, 1, 2, 2, 3, 3, 0, 0};
    c.bad = {0, 0, 0, 0};
    c.set_paths({{0, 2}, {5}, {0}, {5}, {2}, {}, {0, 2}, {}});
    c.rows();
    const Graph g = c.graph();
    CHECK(sink_ok(g, 0) && sink_ok(g, 2) && source_ok(g, 4), "the tests of the chain");
    HostResult R;
    CHECK(c.run(&R) == 0, "run");
    CHECK(R.m1 == Pairs({{0, 4}}), "method 1: %s", show(R.m1).c_str());
    CHECK(R.m2.empty(), "method 2: %s", show(R.m2).c_str());
    CHECK(R.m3 == Pairs({{0, 4}, {3, 1}, {5, 1}}), "method 3: %s", show(R.m3).c_str());
    CHECK(R.pairs == Pairs({{0, 4}, {3, 1}, {5, 1}}), "union: %s", show(R.pairs).c_str());
    CHECK(R.most_rounds == 1 && R.extended == 0, "rounds %llu extended %llu", (unsigned long long)R.most_rounds, (unsigned long long)R.extended);
    // kmers(e2) = 121: e0 fails the sink test through that clause alone; method 1 is gone, method 3 does not look at it
    Case d = c; d.kmers[2] = d.kmers[3] = 121;
    CHECK(!sink_ok(d.graph(), 0), "the k-mers clause of the sink test");
    HostResult R2; CHECK(d.run(&R2) == 0, "run");
    CHECK(R2.m1.empty() && R2.m2.empty(), "no sink, no pair: %s", show(R2.m1).c_str());
    // [e0, e2] is now an extension of 121 k-mers: e0 is extended and emits nothing; the others as before
    CHECK(R2.m3 == Pairs({{3, 1}, {5, 1}}) && R2.extended == 1, "method 3: %s, %llu extended", show(R2.m3).c_str(), (unsigned long long)R2.extended);
    // the bad pair
    Case b = c; b.bad[1] = 1;
    HostResult R3; CHECK(b.run(&R3) == 0, "run");
    CHECK(R3.m1 == Pairs({{0, 4}}) && R3.m3 == Pairs({{3, 1}}), "with pair 1 bad: %s / %s", show(R3.m1).c_str(), show(R3.m3).c_str());
    // capacities of one slot: every edge that reaches the search overflows and is decided exactly: the same answer
    Case s = c; s.max_seqs = 1;
    HostResult R4; CHECK(s.run(&R4) == 0, "run");
    CHECK(R4.pairs == R.pairs && R4.host_edges == R4.searched && R4.searched == R.searched && R.host_edges == 0, "one slot: %s, %llu of %llu on the exact route",
          show(R4.pairs).c_str(), (unsigned long long)R4.host_edges, (unsigned long long)R4.searched);
}

// one edge of a case on the exact route, as the host decides an edge the device could not hold
static int one_edge(const Case& c, int32_t e, Pairs* out, EdgeStat* st, Caps* fitted = nullptr)
{
    const CsrPaths P{c.first.data(), c.edges.data()};
    std::vector<uint32_t> list;
    for (uint32_t id = 0; id + 1 < c.first.size(); ++id) {
        const int32_t* p; const int n = P.len(id, &p);
        for (int j = 0; j < n; ++j) { if (p[j] == e) list.push_back(id << 1); if (c.inv[(size_t)p[j]] == e) list.push_back(id << 1 | 1u); }
    }
    auto bad = [&](uint32_t pair) { return c.bad[pair] != 0; };
    return edge_pairs_exact(c.graph(), c.K, e, list.data(), list.size(), P, c.bc.data(), bad, out, st, fitted);
}

// The search, by hand.  K = 4.  A chain E0 .. E4 of forward edges 0, 2, 4, 6, 8 (inv = odd neighbour, laid out as a chain of its
// own); kmers(E0) = 10, the others 40, so 100 k-mers behind E0 take three edges.  Two pairs, barcodes 1 and 2, both with their
// first read on [E0, E1]; the mates decide what else X of E0 holds (a mate's path, reversed and involuted, joins X as it is):
//   two rounds:  mates [inv E2, inv E1] and [inv E3, inv E2]: X = {[E0, E1], [E1, E2], [E2, E3]}.  exts = {[E0, E1]} (40).
//       Round 1: [E1, E2] holds E1 at l = 0: [E0, E1, E2] (80).  Round 2: [E2, E3] at l = 0: [E0, E1, E2, E3] (120): extended.
//   a mismatch before l:  the first mate is [inv E2, inv E1, inv E4] instead: X = {[E0, E1], [E4, E1, E2], [E2, E3]}.  y = [E4, E1, E2]
//       holds E1 at l = 1, but laid on x = [E0, E1] its E4 (m = 0 < l) falls on E0: not laid on.  Nothing else holds E1 before its
//       end: exts2 is empty at once: not extended, no round.  too_easy = {E1}; can = {(E4, 1), (E1, 1), (E2, 1), (E2, 2), (E3, 2)}:
//       E2 has two barcodes and is not too easy: (E0, E2).
//   ... and with E0 in E4's place (mate [inv E2, inv E1, inv E0]) y = [E0, E1, E2] is a member of exts from the start (80 behind
//       E0); one round adds [E2, E3]: extended.
static void search_cases()
{
    Case c;
    c.K = 4; c.max_seqs = 96; c.max_len = 24; c.n_vertices = 12;
    c.kmers = {10, 10, 40, 40, 40, 40, 40, 40, 40, 40};
    c.inv = {1, 0, 3, 2, 5, 4, 7, 6, 9, 8};
    c.to_left = {0, 10, 1, 9, 2, 8, 3, 7, 4, 6};                 // E_i: i -> i + 1; inv E_i: 10 - i -> 11 - i
    c.to_right = {1, 11, 2, 10, 3, 9, 4, 8, 5, 7};
    c.bc = {1, 1, 2, 2};
    c.bad = {0, 0};
    c.rows();
    struct { std::vector<int32_t> mate; int want, rounds; Pairs pairs; } t[3] = {
        {{5, 3}, HOPS_EXTENDED, 2, {}}, {{5, 3, 9}, HOPS_NOT_EXTENDED, 0, {{0, 4}}}, {{5, 3, 1}, HOPS_EXTENDED, 1, {}}};
    for (const auto& x : t) {
        c.set_paths({{0, 2}, x.mate, {0, 2}, {7, 5}});
        Pairs got; EdgeStat st;
        const int r = one_edge(c, 0, &got, &st);
        CHECK(r == x.want && st.rounds == x.rounds && st.n_x == 3 && got == x.pairs, "mate of %zu edges: %d after %d round(s), |X| = %d, %s", x.mate.size(), r, st.rounds, st.n_x,
              show(got).c_str());
    }
    // the exact route grows the capacity it met and no other: 300 distinct sequences of 2 edges cannot be 300 x 64 x 2^k words
    Case big = c;
    big.kmers.assign(2 * 301, 10); big.inv.resize(2 * 301); big.to_left.assign(2 * 301, 0); big.to_right.assign(2 * 301, 1);
    for (int32_t e = 0; e < 2 * 301; ++e) big.inv[(size_t)e] = e ^ 1;
    big.n_vertices = 2; big.rows();
    std::vector<std::vector<int32_t>> paths;
    big.bc.clear(); big.bad.clear();
    for (int32_t i = 1; i <= 300; ++i) { paths.push_back({0, 2 * i}); paths.push_back({}); big.bc.push_back(i); big.bc.push_back(i); big.bad.push_back(0); }
    big.set_paths(paths);
    Pairs got; EdgeStat st; Caps cp = caps_of(1, 1);
    const Caps start = caps_of(256, 64);
    CHECK(one_edge(big, 0, &got, &st, &cp) == HOPS_NOT_EXTENDED && st.n_x == 300 && st.longest_x == 2 && got.empty(), "300 sequences: |X| = %d, longest %d, %s", st.n_x, st.longest_x,
          show(got).c_str());
    CHECK(cp.x_slots == 512 && cp.ext_slots == 512 && cp.x_len == start.x_len && cp.ext_len == start.ext_len && cp.can == start.can && cp.easy == start.easy,
          "fitted with %d x %d, %d x %d, %d, %d", cp.x_slots, cp.x_len, cp.ext_slots, cp.ext_len, cp.can, cp.easy);
}

static bool ints(std::ifstream& f, std::vector<long long>* v)
{
    std::string line;
    if (!std::getline(f, line)) return false;
    std::istringstream s(line);
    v->clear();
    for (long long x; s >> x;) v->push_back(x);
    return true;
}

static Pairs pairs_of(const std::vector<long long>& v)
{
    Pairs p;
    for (size_t i = 1; i + 1 < v.size(); i += 2) p.emplace_back((int32_t)v[i], (int32_t)v[i + 1]);
    return p;
}

// graph NAME K / E V N / kmers / inv / to_left / to_right / bc / bad / N paths, then per variant of it:
// variant ONE_GOOD MAX_SEQS MAX_LEN / m1 / m2 / m3 / union / counters / digest
static int recorded_cases(const char* path)
{
    std::ifstream f(path);
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return -1; }
    int n_cases = 0;
    std::string line, name;
    Case c;
    bool have_graph = false;
    while (std::getline(f, line)) {
        std::istringstream hd(line);
        std::string word;
        hd >> word;
        std::vector<long long> v;
        if (word == "graph") {
            c = Case();
            hd >> name >> c.K;
            if (!ints(f, &v) || v.size() != 3) return -1;
            const size_t E = (size_t)v[0], N = (size_t)v[2];
            c.n_vertices = (int)v[1];
            auto take = [&](std::vector<int32_t>* d, size_t n) { if (!ints(f, &v) || v.size() != n) return false; d->assign(v.begin(), v.end()); return true; };
            std::vector<int32_t> bad;
            if (!take(&c.kmers, E) || !take(&c.inv, E) || !take(&c.to_left, E) || !take(&c.to_right, E) || !take(&c.bc, N) || !take(&bad, N / 2)) return -1;
            c.bad.assign(bad.begin(), bad.end());
            std::vector<std::vector<int32_t>> paths(N);
            for (size_t i = 0; i < N; ++i) { if (!ints(f, &v) || v.empty() || v.size() != (size_t)v[0] + 1) return -1; paths[i].assign(v.begin() + 1, v.end()); }
            c.set_paths(paths);
            c.rows();
            have_graph = true;
            continue;
        }
        if (word != "variant" || !have_graph) { fprintf(stderr, "neither a graph nor a variant of one: %s\n", line.c_str()); return -1; }
        hd >> c.one_good >> c.max_seqs >> c.max_len;
        Pairs want[4];
        for (Pairs& w : want) { if (!ints(f, &v)) return -1; w = pairs_of(v); }
        std::vector<long long> ctr;
        if (!ints(f, &ctr) || ctr.size() != 7) return -1;
        std::string dline;
        if (!std::getline(f, dline)) return -1;
        unsigned long long d0 = 0, d1 = 0;
        if (sscanf(dline.c_str(), "%llu %llu", &d0, &d1) != 2) return -1;
        HostResult R;
        const int rc = c.run(&R);
        const std::string what = name + " one_good " + std::to_string(c.one_good) + " caps " + std::to_string(c.max_seqs) + "x" + std::to_string(c.max_len);
        CHECK(rc == 0, "%s: %d", what.c_str(), rc);
        CHECK(R.m1 == want[0], "%s method 1: %s want %s", what.c_str(), show(R.m1).c_str(), show(want[0]).c_str());
        CHECK(R.m2 == want[1], "%s method 2: %s want %s", what.c_str(), show(R.m2).c_str(), show(want[1]).c_str());
        CHECK(R.m3 == want[2], "%s method 3: %s want %s", what.c_str(), show(R.m3).c_str(), show(want[2]).c_str());
        CHECK(R.pairs == want[3], "%s union: %s want %s", what.c_str(), show(R.pairs).c_str(), show(want[3]).c_str());
        const unsigned long long got[7] = {R.searched, R.extended, R.most_rounds, R.largest_x, R.largest_exts, R.longest, R.host_edges};
        for (int i = 0; i < 7; ++i) CHECK(got[i] == (unsigned long long)ctr[i], "%s counter %d: %llu want %lld", what.c_str(), i, got[i], ctr[i]);
        uint64_t h[2]; pairs_digest(R.pairs, h);
        CHECK(h[0] == d0 && h[1] == d1, "%s digest", what.c_str());
        ++n_cases;
    }
    return n_cases;
}

int main(int argc, char** argv)
{
    hand_case();
    search_cases();
    int n = 0;
    if (argc > 1) { n = recorded_cases(argv[1]); if (n <= 0) { fprintf(stderr, "no recorded case could be read from %s\n", argv[1]); return 2; } }
    if (g_failed) { fprintf(stderr, "%d check(s) failed\n", g_failed); return 1; }
    printf("test_hops: the hand cases and %d recorded cases agree\n", n);
    return 0;
}
