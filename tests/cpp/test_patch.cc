// tests/cpp/test_patch.cc -- superplus_amd/csrc/dfk_patch.h on the host: the literal form (BuildAll, kmerize, BigKEdgeBuilder as written,
// the Pather loop) against the cases recorded from tests/patch_oracle.py (tests/cpp/patch_cases.txt); the device's order of work
// (slot formula, entry_context(), batches of closure positions, heads / emit and the inv route) against the literal form under
// kmers_per_batch 1, 37 and 0; check_graph() and the two-slots refusal on the recorded refusals; the file and the digest's parts.  Its own
// main; built plain and under -fsanitize=address,undefined by tests/test_patch_cpu.py.
//   test_patch <cases file>
// A block "time NAME" (head K, vertices, edges, closures; the tables; the edges; the closures -- no expectations) is what tools/patch_cost.py
// writes: the literal form is run on it once, on this one thread, and its wall time printed.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include "dfk_patch.h"

static int g_failed = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++g_failed; } } while (0)

using dfk_patch::Seq;

template <class T> static std::vector<T> row(std::ifstream& in)
{
    std::string line;
    std::getline(in, line);
    std::vector<T> v;
    if (line == "-") return v;
    std::istringstream s(line);
    long long x;
    while (s >> x) v.push_back((T)x);
    return v;
}
static Seq seq_row(std::ifstream& in)
{
    std::string line;
    std::getline(in, line);
    Seq s;
    if (line == "-") return s;
    for (char c : line) s.push_back((uint8_t)(c - '0'));
    return s;
}
static dfk_patch::Graph graph_rows(std::ifstream& in, const std::vector<uint64_t>& head)
{
    dfk_patch::Graph G;
    G.K = (uint32_t)head[0]; G.n_vertices = (uint32_t)head[1];
    G.inv = row<int32_t>(in); G.to_left = row<int32_t>(in); G.to_right = row<int32_t>(in);
    for (uint64_t e = 0; e < head[2]; ++e) G.edges.push_back(seq_row(in));
    return G;
}

int main(int argc, char** argv)
{
    if (argc < 2) { printf("usage: test_patch <cases file>\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { printf("cannot read %s\n", argv[1]); return 2; }
    int n_cases = 0, n_refused = 0;
    std::string line;
    while (std::getline(in, line)) {
        if (line.rfind("refuse ", 0) == 0) {
            const std::string name = line.substr(7);
            const dfk_patch::Graph G = graph_rows(in, row<uint64_t>(in));
            const std::string why = dfk_patch::check_graph(G);
            if (name == "twice") {                                     // holds together; the slot check finds it
                CHECK(why.empty());
                bool threw = false;
                try { (void)dfk_patch::device_order(G, {}, 0); } catch (const std::invalid_argument&) { threw = true; }
                CHECK(threw);
            } else CHECK(!why.empty());
            ++n_refused;
            continue;
        }
        if (line.rfind("time ", 0) == 0) {
            const std::vector<uint64_t> head = row<uint64_t>(in);
            const dfk_patch::Graph G = graph_rows(in, head);
            std::vector<Seq> closures;
            for (uint64_t i = 0; i < head[3]; ++i) closures.push_back(seq_row(in));
            CHECK(dfk_patch::check_graph(G).empty());
            const auto t0 = std::chrono::steady_clock::now();
            const dfk_patch::Result L = dfk_patch::literal(G, closures);
            const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
            printf("LITERAL %s {\"us\": %.0f, \"kmers3\": %llu, \"new_unique\": %llu, \"bits_added\": %llu, \"canonical3\": %zu, \"to3\": %zu}\n", line.substr(5).c_str(), us, (unsigned long long)L.kmers3,
                   (unsigned long long)L.fresh_unique, (unsigned long long)L.bits_added, L.edges3.size(), L.to3.size());
            continue;
        }
        if (line.rfind("case ", 0) != 0) { printf("unexpected line: %s\n", line.c_str()); return 2; }
        const std::string name = line.substr(5);
        const std::vector<uint64_t> head = row<uint64_t>(in);
        const dfk_patch::Graph G = graph_rows(in, head);
        std::vector<Seq> closures, want_edges;
        for (uint64_t i = 0; i < head[3]; ++i) closures.push_back(seq_row(in));
        for (uint64_t i = 0; i < head[4]; ++i) want_edges.push_back(seq_row(in));
        const std::vector<uint64_t> first = row<uint64_t>(in);
        const std::vector<int32_t> to3 = row<int32_t>(in), left3 = row<int32_t>(in);
        const std::vector<uint64_t> k = row<uint64_t>(in);          // crossings short positions found new new_unique bits_added kmers3 single3
        CHECK(dfk_patch::check_graph(G).empty());
        const dfk_patch::Result L = dfk_patch::literal(G, closures);
        const bool lit = L.edges3 == want_edges && L.to3_first == first && L.to3 == to3 && L.left3 == left3 && k.size() == 9 && L.crossings == k[0] && L.shorter == k[1] && L.positions == k[2] &&
                         L.found == k[3] && L.fresh == k[4] && L.fresh_unique == k[5] && L.bits_added == k[6] && L.kmers3 == k[7] && L.single3 == k[8];
        if (!lit) { printf("FAILED case %s: the literal form is not what was recorded\n", name.c_str()); ++g_failed; }
        for (uint64_t per : {1ull, 37ull, 0ull}) {
            const dfk_patch::Result D = dfk_patch::device_order(G, closures, per);
            if (!(D == L)) { printf("FAILED case %s: the device's order of work with %llu K-mers a batch\n", name.c_str(), (unsigned long long)per); ++g_failed; }
            const uint64_t want_batches = per ? (L.positions + per - 1) / per : (L.positions ? 1 : 0);
            CHECK(D.batches == want_batches);
        }
        // every slot goes to its edge and back
        const dfk_patch::Plan P = dfk_patch::plan_of(G);
        for (uint32_t c = 0; c < P.canon.size(); ++c)
            for (uint64_t s = P.first[c]; s < P.first[c + 1]; ++s) CHECK(dfk_patch::slot_edge(P.first.data(), (uint32_t)P.canon.size(), s) == c);
        // the file: its parts where the layout says
        const std::vector<uint8_t> f = dfk_patch::to3_file(L.to3_first, L.to3, L.left3);
        CHECK(f.size() == dfk_patch::file_bytes(L.left3.size(), L.to3.size()) && memcmp(f.data(), "DFKPTO31", 8) == 0);
        if (!L.left3.empty()) CHECK(memcmp(f.data() + dfk_patch::left3_at(L.left3.size(), L.to3.size()), L.left3.data(), 4 * L.left3.size()) == 0);
        ++n_cases;
    }
    for (uint32_t c = 0; c < 256; ++c) CHECK(dfk_patch::ctx_rc8(dfk_patch::ctx_rc8(c)) == c && (dfk_patch::ctx_rc8(c) & 1u) == (c >> 7));
    if (g_failed) { printf("%d checks FAILED\n", g_failed); return 1; }
    printf("%d recorded cases agree, %d refusals refused\n", n_cases, n_refused);
    return 0;
}
