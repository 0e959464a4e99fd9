// tests/cpp/test_closer.cc -- superplus_amd/csrc/dfk_closer.h on the host: the literal per-edge transcription against the cases
// recorded from tests/closer_oracle.py (tests/cpp/closer_cases.txt, and fixtures written out in the same form), the per-pair
// composition identity against Stackster's loops run for the pair as they stand, the device version's order of work
// (closer_sweep: walk_read, stable sort, ranges of ranks) against the literal one under several range caps, the range plan on
// random sizes, the packed words and the files' fixed parts.  Its own main; built plain and under -fsanitize=address,undefined by
// tests/test_closer_cpu.py.
//   test_closer <cases file>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include "dfk_closer.h"

static int g_failed = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++g_failed; } } while (0)

struct Case {
    std::string name;
    int32_t K = 0;
    std::vector<int32_t> inv, kmers, edges, offsets, pairs;
    std::vector<uint8_t> dup;
    std::vector<uint64_t> first, ce, loc_first, anchor_first, read_first, reads;
    std::vector<int64_t> locs, anchors;                                        // flat: (id, pos, fw), (g, add, count)
    uint64_t prec = 0, mates_in = 0, mates_out = 0, dup_skipped = 0;
};

template <class T> static std::vector<T> row(const std::string& line)
{
    std::istringstream in(line);
    std::vector<T> v;
    long long x;
    while (in >> x) v.push_back((T)x);
    return v;
}

static bool same_tables(const dfk_closer::HostResult& a, const dfk_closer::HostResult& b)
{
    if (!(a.ce == b.ce && a.loc_first == b.loc_first && a.anchor_first == b.anchor_first && a.read_first == b.read_first && a.reads == b.reads)) return false;
    if (a.locs.size() != b.locs.size() || a.anchors.size() != b.anchors.size()) return false;
    for (size_t i = 0; i < a.locs.size(); ++i) if (a.locs[i].id != b.locs[i].id || a.locs[i].pos != b.locs[i].pos || a.locs[i].fw != b.locs[i].fw) return false;
    for (size_t i = 0; i < a.anchors.size(); ++i) if (a.anchors[i].g != b.anchors[i].g || a.anchors[i].add != b.anchors[i].add || a.anchors[i].count != b.anchors[i].count) return false;
    return a.prec == b.prec && a.mates_in == b.mates_in && a.mates_out == b.mates_out && a.dup_skipped == b.dup_skipped;
}

static void run_case(const Case& c)
{
    using namespace dfk_closer;
    const uint64_t E = c.inv.size(), N = c.first.size() - 1;
    std::vector<uint64_t> idx_first, idx_ids;
    std::vector<int32_t> edges(c.edges), offsets(c.offsets);
    if (edges.empty()) edges.push_back(0);
    if (offsets.empty()) offsets.push_back(0);
    std::vector<uint8_t> dup(c.dup);
    if (dup.empty()) dup.push_back(0);
    build_index(E, N, c.first.data(), edges.data(), &idx_first, &idx_ids);
    if (idx_ids.empty()) idx_ids.push_back(0);
    const Input I{E, c.inv.data(), c.kmers.data(), c.K, N, c.first.data(), edges.data(), offsets.data(), dup.data(), idx_first.data(), idx_ids.data()};
    HostResult r;
    const int rc = closer_literal(I, c.pairs.data(), c.pairs.size() / 2, &r);
    CHECK(rc == 0);
    if (rc) return;
    // ---- the literal transcription against the Python restatement
    bool ok = r.ce == c.ce && r.loc_first == c.loc_first && r.anchor_first == c.anchor_first && r.read_first == c.read_first && r.reads == c.reads;
    ok = ok && r.locs.size() * 3 == c.locs.size() && r.anchors.size() * 3 == c.anchors.size();
    for (size_t i = 0; ok && i < r.locs.size(); ++i) ok = r.locs[i].id == c.locs[3 * i] && r.locs[i].pos == c.locs[3 * i + 1] && (int64_t)r.locs[i].fw == c.locs[3 * i + 2];
    for (size_t i = 0; ok && i < r.anchors.size(); ++i) ok = r.anchors[i].g == c.anchors[3 * i] && r.anchors[i].add == c.anchors[3 * i + 1] && r.anchors[i].count == c.anchors[3 * i + 2];
    if (!ok) printf("case %s: the tables differ from the recorded ones\n", c.name.c_str());
    CHECK(ok);
    CHECK(r.prec == c.prec && r.mates_in == c.mates_in && r.mates_out == c.mates_out && r.dup_skipped == c.dup_skipped);
    // ---- the per-pair composition: Stackster's loops for the pair as they stand = reads(e1) U flipped reads(inv[e2])
    for (uint64_t p = 0; p < c.pairs.size() / 2; ++p) {
        const int32_t e1 = c.pairs[2 * p], e2 = c.pairs[2 * p + 1];
        const uint64_t k1 = (uint64_t)(std::lower_bound(r.ce.begin(), r.ce.end(), (uint64_t)e1) - r.ce.begin());
        const uint64_t k2 = (uint64_t)(std::lower_bound(r.ce.begin(), r.ce.end(), (uint64_t)c.inv[e2]) - r.ce.begin());
        CHECK(k1 < r.ce.size() && r.ce[k1] == (uint64_t)e1 && k2 < r.ce.size() && r.ce[k2] == (uint64_t)c.inv[e2]);
        const std::vector<uint64_t> a(r.reads.begin() + r.read_first[k1], r.reads.begin() + r.read_first[k1 + 1]), b(r.reads.begin() + r.read_first[k2], r.reads.begin() + r.read_first[k2 + 1]);
        CHECK(pair_composed(a, b) == pair_literal(I, e1, e2));
    }
    // ---- the device version's order of work gives the same tables, whatever the ranges
    uint64_t total_weight = 0;
    for (uint64_t cap : {(uint64_t)1, (uint64_t)37, (uint64_t)1000, (uint64_t)1 << 30}) {
        HostResult s;
        uint64_t n_ranges = 0;
        CHECK(closer_sweep(I, c.pairs.data(), c.pairs.size() / 2, cap, &s, &n_ranges) == 0);
        CHECK(same_tables(r, s));
        total_weight = 0;
        for (uint64_t w : s.weight) total_weight += w;
        const std::vector<uint64_t> wfirst = dfk::prefix_sums(s.weight.data(), s.weight.size());
        CHECK(n_ranges == count_ranges(wfirst.data(), s.weight.size(), cap));
        uint64_t heavy = 0;                                                     // (a range starts at one rank and goes on only while it stays within the cap)
        for (uint64_t w : s.weight) heavy += w >= 2;
        if (cap == 1) CHECK(n_ranges <= s.ce.size() && n_ranges >= heavy);
        if (cap == (1ull << 30)) CHECK(n_ranges == (s.ce.empty() ? 0u : 1u));
        // a rank's weight bounds what it leaves in each table
        for (uint64_t k = 0; k < s.ce.size(); ++k)
            CHECK(s.weight[k] >= (s.loc_first[k + 1] - s.loc_first[k]) + (s.read_first[k + 1] - s.read_first[k]) && (s.anchor_first[k + 1] - s.anchor_first[k]) * MIN_EDGE_COUNT <= s.weight[k]);
    }
    CHECK(total_weight >= r.locs.size() + r.prec);
    // ---- the files' sizes
    CHECK(table_file_size(r.ce.size(), r.locs.size(), sizeof(Loc)) == 16 + 8 * (r.ce.size() + 1) + 16 * r.locs.size());
}

static void refusals_and_words()
{
    using namespace dfk_closer;
    const std::vector<int32_t> inv = {1, 0, 2}, kmers = {5, 5, 9}, edges = {0, 2}, offsets = {0, 0};
    const std::vector<uint64_t> first = {0, 1, 2};
    const std::vector<uint8_t> dup = {0};
    std::vector<uint64_t> xf, xi;
    build_index(3, 2, first.data(), edges.data(), &xf, &xi);
    const Input I{3, inv.data(), kmers.data(), 4, 2, first.data(), edges.data(), offsets.data(), dup.data(), xf.data(), xi.data()};
    Input odd = I; odd.n_reads = 1;
    HostResult r;
    const int32_t past[2] = {0, 3}, neg[2] = {-1, 0}, fine[2] = {0, 2};
    CHECK(closer_literal(I, past, 1, &r) == -1 && r.ce.empty());
    CHECK(closer_literal(I, neg, 1, &r) == -1);
    CHECK(closer_literal(odd, fine, 1, &r) == -2);
    Input many = I; many.n_reads = (1ull << 31) + 2;
    CHECK(closer_literal(many, fine, 1, &r) == -3);
    CHECK(closer_literal(I, fine, 1, &r) == 0);
    // ce = {0, inv[2] = 2}; edge 0: read 0 forward, its mate let in; edge 2 (self-inverse): read 1 both ways, twice in locs
    CHECK((r.ce == std::vector<uint64_t>{0, 2}) && (r.loc_first == std::vector<uint64_t>{0, 1, 3}));
    CHECK((r.reads == std::vector<uint64_t>{0 << 1 | 1, 1 << 1 | 0, 0 << 1 | 0, 1 << 1 | 0, 1 << 1 | 1}));
    CHECK(r.locs[1].fw == 1 && r.locs[2].fw == 0 && r.locs[1].id == 1 && r.locs[2].id == 1);
    // one edge of 2^32 records: refused by the range
    const uint64_t big[3] = {0, 5, 5 + (1ull << 32)};
    CHECK(next_range(big, 2, 0, 10).ok && !next_range(big, 2, 1, 10).ok);
    // MAX_DIST is inclusive, and the sum does not wrap
    CHECK(mate_within(700, 48, -53) && !mate_within(700, 48, -54) && !mate_within(2147483647, 48, -2147483647 - 1) && mate_within(1, 1, 2147483647));
    // the packed words
    CHECK(loc_key(3, 0) == 6 && loc_key(3, 1) == 7 && loc_key_bits(1) == 1 && loc_key_bits(3) == 3 && bits_for(1) == 1 && bits_for(257) == 9);
    CHECK(loc_word1(-1, true) == 0x1FFFFFFFFull && loc_word1(7, false) == 7 && read_word(0x7FFFFFFF, true) == 0xFFFFFFFFu && read_word(5, false) == 10);
    uint32_t marks[2] = {0, 0};
    marks[1] |= 1u << 3;
    CHECK(marked(marks, 35) && !marked(marks, 3) && !marked(marks, 34));
    // the files' fixed parts
    const BinHead h = head_of(MAGIC_LOCS, 7);
    CHECK(memcmp(&h, "DFKCLOC1\7\0\0\0\0\0\0\0", 16) == 0 && edges_file_size(7) == 72 && table_records_at(0) == 24 && table_file_size(0, 0, 16) == 24);
    CHECK(strlen(MAGIC_EDGES) == 8 && strlen(MAGIC_ANCHORS) == 8 && strlen(MAGIC_READS) == 8);
    CHECK(range_cap(1ull << 40, 77) == 77 && range_cap(0, 0) == (1ull << 18) && range_cap(192ull << 30, 0) * BYTES_PER_WEIGHT <= (192ull << 30) / 2);
}

static void range_plan_on_random_sizes()
{
    srand(4321);
    for (int t = 0; t < 200; ++t) {
        const uint64_t n = (uint64_t)(rand() % 40);
        std::vector<uint64_t> first(n + 1, 0);
        for (uint64_t k = 0; k < n; ++k) first[k + 1] = first[k] + (uint64_t)(rand() % 5 == 0 ? 0 : rand() % 1000);
        const uint64_t cap = 1 + (uint64_t)(rand() % 2000);
        uint64_t k0 = 0, ranges = 0, total = 0;
        while (k0 < n) {
            const dfk::PidxRange g = dfk_closer::next_range(first.data(), n, k0, cap);
            CHECK(g.e0 == k0 && g.e1 > k0 && g.e1 <= n && g.ok && (g.n <= cap || g.e1 == k0 + 1));
            if (g.e1 < n) CHECK(first[g.e1 + 1] - first[k0] > cap);                 // greedy: the next rank would not have fitted
            total += g.n; k0 = g.e1; ++ranges;
        }
        CHECK(total == first[n] && ranges == dfk_closer::count_ranges(first.data(), n, cap));
    }
}

int main(int argc, char** argv)
{
    if (argc != 2) { printf("usage: test_closer <cases file>\n"); return 2; }
    refusals_and_words();
    range_plan_on_random_sizes();
    std::ifstream in(argv[1]);
    if (!in) { printf("cannot read %s\n", argv[1]); return 2; }
    std::string line;
    int n_cases = 0;
    while (std::getline(in, line)) {
        if (line.rfind("case ", 0) != 0) { printf("unexpected line: %s\n", line.c_str()); return 2; }
        Case c;
        long long E = 0, N = 0, np = 0, K = 0;
        { std::istringstream h(line.substr(5)); h >> c.name >> E >> N >> np >> K; }
        c.K = (int32_t)K;
        std::string l[15];
        for (auto& s : l) if (!std::getline(in, s)) { printf("case %s is cut short\n", c.name.c_str()); return 2; }
        c.inv = row<int32_t>(l[0]); c.kmers = row<int32_t>(l[1]); c.first = row<uint64_t>(l[2]); c.edges = row<int32_t>(l[3]); c.offsets = row<int32_t>(l[4]);
        c.pairs = row<int32_t>(l[5]); c.dup = row<uint8_t>(l[6]); c.ce = row<uint64_t>(l[7]); c.loc_first = row<uint64_t>(l[8]); c.anchor_first = row<uint64_t>(l[9]);
        c.read_first = row<uint64_t>(l[10]); c.locs = row<int64_t>(l[11]); c.anchors = row<int64_t>(l[12]); c.reads = row<uint64_t>(l[13]);
        const std::vector<uint64_t> k = row<uint64_t>(l[14]);
        if (k.size() != 4 || c.first.size() != (size_t)N + 1 || c.inv.size() != (size_t)E || c.kmers.size() != (size_t)E || c.pairs.size() != 2 * (size_t)np || c.dup.size() != (size_t)N / 2 ||
            c.offsets.size() != (size_t)N) { printf("case %s is malformed\n", c.name.c_str()); return 2; }
        c.prec = k[0]; c.mates_in = k[1]; c.mates_out = k[2]; c.dup_skipped = k[3];
        run_case(c);
        ++n_cases;
    }
    if (g_failed) { printf("%d check(s) failed\n", g_failed); return 1; }
    printf("%d recorded cases agree\n", n_cases);
    return 0;
}
