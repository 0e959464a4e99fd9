// tests/cpp/test_subset.cc -- superplus_amd/csrc/dfk_subset.h on the host: the rule on the graph worked out by hand in
// tests/test_subset_oracle.py, on the seeded cases recorded from tests/subset_oracle.py (tests/cpp/subset_cases.txt), the range plan
// on random sizes, the packed words of the gather's scan, the files' fixed parts.  Its own main; built plain and under
// -fsanitize=address,undefined by tests/test_subset_cpu.py.
//   test_subset <cases file>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include "dfk_subset.h"

static int g_failed = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++g_failed; } } while (0)

struct Case {
    std::string name;
    std::vector<int32_t> inv, edges, pairs;
    std::vector<uint64_t> first, eoi, ids, index_first;
    uint64_t path_entries = 0, index_entries = 0, one = 0, unplaced = 0;
};

template <class T> static std::vector<T> row(const std::string& line, bool counted = false)
{
    std::istringstream in(line);
    std::vector<T> v;
    long long x;
    if (counted) { in >> x; }
    while (in >> x) v.push_back((T)x);
    return v;
}

static void run_case(const Case& c)
{
    dfk_subset::HostResult r;
    const uint64_t E = c.inv.size(), N = c.first.size() - 1;
    const int rc = dfk_subset::subset_host(E, c.inv.data(), N, c.first.data(), c.edges.data(), c.pairs.data(), c.pairs.size() / 2, &r);
    CHECK(rc == 0);
    if (rc) return;
    if (!(r.eoi == c.eoi && r.ids == c.ids)) printf("case %s: eoi or ids differ\n", c.name.c_str());
    CHECK(r.eoi == c.eoi); CHECK(r.ids == c.ids); CHECK(r.index_first == c.index_first);
    CHECK(r.path_entries == c.path_entries); CHECK(r.index_first.back() == c.index_entries); CHECK(r.one_read_only == c.one); CHECK(r.unplaced == c.unplaced);
    // the gather's packed scan gives every id its rank and every element its byte, whatever the batches
    for (uint64_t per : {(uint64_t)1, (uint64_t)7, N ? N : (uint64_t)1}) {
        std::vector<unsigned long long> bits(std::max<uint64_t>(1, dfk_subset::pair_words(N / 2)), 0ull);
        for (uint64_t id : r.ids) bits[(id >> 1) / 64] |= 1ull << ((id >> 1) % 64);
        uint64_t ids_done = 0, bytes_done = 0;
        for (uint64_t r0 = 0; r0 < N; r0 += per) {
            uint64_t acc = 0;
            for (uint64_t i = r0; i < std::min(N, r0 + per); ++i) {
                if (!dfk_subset::pair_bit(bits.data(), i >> 1)) continue;
                CHECK(ids_done + dfk_subset::gather_rank(acc) < r.ids.size() && r.ids[ids_done + dfk_subset::gather_rank(acc)] == i);
                acc += dfk_subset::gather_word(dfk_subset::path_elem_bytes(c.first[i + 1] - c.first[i]));
            }
            ids_done += dfk_subset::gather_rank(acc); bytes_done += dfk_subset::gather_byte(acc);
        }
        CHECK(ids_done == r.ids.size() && bytes_done == 8 * r.ids.size() + 4 * r.path_entries);
    }
    // the layouts
    const dfk::FeudalLayout lp = dfk_subset::paths_layout(r.ids.size(), r.path_entries), lx = dfk_subset::index_layout(r.eoi.size(), r.index_first.back());
    CHECK(lp.head.n == r.ids.size() && lp.head.szX == 24 && lp.head.szA == 4 && lp.var_tab == 24 + 8 * r.ids.size() + 4 * r.path_entries && lp.file_size == lp.var_tab + 8 * (r.ids.size() + 1));
    CHECK(lx.head.n == r.eoi.size() && lx.head.szX == 16 && lx.head.szA == 8 && lx.var_tab == 24 + 8 * r.index_first.back() && lx.file_size == lx.var_tab + 8 * (r.eoi.size() + 1));
    // ranges of ranks: they tile [0, n_eoi), hold at most cap entries unless a single edge holds more
    for (uint64_t cap : {(uint64_t)1, (uint64_t)3, (uint64_t)50, (uint64_t)1 << 20}) {
        uint64_t k0 = 0, n = 0, total = 0;
        while (k0 < r.eoi.size()) {
            const dfk::PidxRange g = dfk_subset::next_range(r.index_first.data(), r.eoi.size(), k0, cap);
            CHECK(g.e0 == k0 && g.e1 > k0 && g.e1 <= r.eoi.size() && g.ok);
            CHECK(g.n == r.index_first[g.e1] - r.index_first[k0]);
            CHECK(g.n <= cap || g.e1 == k0 + 1);
            total += g.n; k0 = g.e1; ++n;
        }
        CHECK(total == r.index_first.back() && n == dfk_subset::count_ranges(r.index_first.data(), r.eoi.size(), cap));
    }
}

static Case hand()
{
    Case c;
    c.name = "hand";
    c.inv = {1, 0, 3, 2, 5, 4, 7, 6, 9, 8, 11, 10, 12, 13};
    c.pairs = {0, 4, 12, 6};
    const std::vector<std::vector<int32_t>> paths = {{0, 2}, {9}, {8}, {3, 5}, {}, {4}, {}, {}, {2, 8}, {10}, {6, 12, 6}, {7}, {12, 12, 12}, {13}, {10, 11}, {3}};
    c.first.push_back(0);
    for (const auto& p : paths) { c.edges.insert(c.edges.end(), p.begin(), p.end()); c.first.push_back(c.edges.size()); }
    c.eoi = {0, 1, 4, 5, 6, 7, 12};
    c.ids = {0, 1, 2, 3, 4, 5, 10, 11, 12, 13};
    c.index_first = {0, 1, 1, 2, 3, 5, 6, 10};
    c.path_entries = 15; c.index_entries = 10; c.one = 4; c.unplaced = 1;
    return c;
}

static void refusals()
{
    const std::vector<int32_t> inv = {1, 0, 2};
    const std::vector<uint64_t> first = {0, 1, 2};
    const std::vector<int32_t> edges = {0, 2};
    dfk_subset::HostResult r;
    const int32_t past[2] = {0, 3}, neg[2] = {-1, 0}, fine[2] = {2, 2};
    CHECK(dfk_subset::subset_host(3, inv.data(), 2, first.data(), edges.data(), past, 1, &r) == -1);
    CHECK(dfk_subset::subset_host(3, inv.data(), 2, first.data(), edges.data(), neg, 1, &r) == -1);
    CHECK(dfk_subset::subset_host(3, inv.data(), 1, first.data(), edges.data(), fine, 1, &r) == -2);
    CHECK(r.eoi.empty() && r.ids.empty());
    CHECK(dfk_subset::subset_host(3, inv.data(), 2, first.data(), edges.data(), fine, 1, &r) == 0);
    CHECK(r.eoi == std::vector<uint64_t>{2} && (r.ids == std::vector<uint64_t>{0, 1}) && r.one_read_only == 1);
    // a single edge with 2^32 entries: the range is refused
    const uint64_t big[3] = {0, 5, 5 + (1ull << 32)};
    CHECK(dfk_subset::next_range(big, 2, 0, 10).ok && !dfk_subset::next_range(big, 2, 1, 10).ok);
    // the files' fixed parts
    const dfk_subset::BinHead h = dfk_subset::bin_head(7);
    CHECK(memcmp(&h, "BINWRITE\7\0\0\0\0\0\0\0", 16) == 0 && dfk_subset::ids_file_size(7) == 72);
    CHECK(dfk_subset::paths_layout(0, 0).file_size == 32 && dfk_subset::index_layout(0, 0).file_size == 32);
    CHECK(dfk_subset::mark_words(0) == 0 && dfk_subset::mark_words(32) == 1 && dfk_subset::mark_words(33) == 2 && dfk_subset::pair_words(65) == 2);
    CHECK(dfk_subset::gather_rank(3 * dfk_subset::gather_word(12)) == 3 && dfk_subset::gather_byte(3 * dfk_subset::gather_word(12)) == 36);
}

static void range_plan_on_random_sizes()
{
    srand(12345);
    for (int t = 0; t < 200; ++t) {
        const uint64_t n = (uint64_t)(rand() % 40);
        std::vector<uint64_t> first(n + 1, 0);
        for (uint64_t k = 0; k < n; ++k) first[k + 1] = first[k] + (uint64_t)(rand() % 5 == 0 ? 0 : rand() % 1000);
        const uint64_t cap = 1 + (uint64_t)(rand() % 2000);
        uint64_t k0 = 0, ranges = 0;
        while (k0 < n) {
            const dfk::PidxRange g = dfk_subset::next_range(first.data(), n, k0, cap);
            CHECK(g.e1 > k0 && g.e1 <= n && (g.n <= cap || g.e1 == k0 + 1));
            if (g.e1 < n) CHECK(first[g.e1 + 1] - first[k0] > cap);                 // greedy: the next edge would not have fitted
            k0 = g.e1; ++ranges;
        }
        CHECK(ranges == dfk_subset::count_ranges(first.data(), n, cap));
        CHECK(dfk_subset::range_cap(1ull << 40, cap) == cap && dfk_subset::range_cap(0, 0) == (1ull << 20));
    }
}

int main(int argc, char** argv)
{
    if (argc != 2) { printf("usage: test_subset <cases file>\n"); return 2; }
    run_case(hand());
    refusals();
    range_plan_on_random_sizes();
    std::ifstream in(argv[1]);
    if (!in) { printf("cannot read %s\n", argv[1]); return 2; }
    std::string line;
    int n_cases = 0;
    while (std::getline(in, line)) {
        if (line.rfind("case ", 0) != 0) { printf("unexpected line: %s\n", line.c_str()); return 2; }
        Case c;
        { std::istringstream h(line.substr(5)); h >> c.name; }
        std::string l[8];
        for (auto& s : l) if (!std::getline(in, s)) { printf("case %s is cut short\n", c.name.c_str()); return 2; }
        c.inv = row<int32_t>(l[0]); c.first = row<uint64_t>(l[1]); c.edges = row<int32_t>(l[2]); c.pairs = row<int32_t>(l[3]);
        c.eoi = row<uint64_t>(l[4], true); c.ids = row<uint64_t>(l[5], true);
        const std::vector<uint64_t> k = row<uint64_t>(l[6]);
        if (k.size() != 4 || c.first.empty()) { printf("case %s is malformed\n", c.name.c_str()); return 2; }
        c.path_entries = k[0]; c.index_entries = k[1]; c.one = k[2]; c.unplaced = k[3];
        c.index_first = row<uint64_t>(l[7]);
        if (c.edges.empty()) c.edges.push_back(0);
        run_case(c);
        ++n_cases;
    }
    if (g_failed) { printf("%d check(s) failed\n", g_failed); return 1; }
    printf("the hand case and %d recorded cases agree\n", n_cases);
    return 0;
}
