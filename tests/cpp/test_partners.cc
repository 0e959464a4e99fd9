// tests/cpp/test_partners.cc -- superplus_amd/csrc/dfk_partners.h on the host: the literal per-pair transcription against the cases
// recorded from tests/partners_oracle.py (tests/cpp/partners_cases.txt, and fixtures written out in the same form), the device
// version's order of work (partners_plan: sides, forward parts, flagged items, ranges of the table, batches of queries, lanes and
// their folds) against the literal one under query batches of 1, 37 and 2^30 and several table and item caps, the 32-mer cut at
// every residue, the plan on random sizes, the file's fixed parts.  Its own main; built plain and under
// -fsanitize=address,undefined by tests/test_partners_cpu.py.
//   test_partners <cases file>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include "dfk_partners.h"

static int g_failed = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++g_failed; } } while (0)

struct Case {
    std::string name;
    std::vector<int32_t> inv, anchors, pairs;
    std::vector<uint32_t> edge_len, read_len;
    std::vector<uint8_t> edge_packed, read_packed;
    std::vector<uint64_t> edge_off, read_off, ce, loc_first, locs, anchor_first, starts;
    std::vector<int64_t> recs;                                                 // flat: (id, pos)
    uint64_t queries = 0, positions = 0, entries = 0, any_hit = 0, kept = 0, multi = 0, searched = 0;
};

template <class T> static std::vector<T> row(const std::string& line)
{
    std::istringstream in(line);
    std::vector<T> v;
    long long x;
    while (in >> x) v.push_back((T)x);
    return v;
}
static std::vector<uint8_t> hexrow(const std::string& line)
{
    std::vector<uint8_t> v;
    if (line == "-") return v;
    auto nib = [](char c) { return (uint8_t)(c <= '9' ? c - '0' : c - 'a' + 10); };
    for (size_t i = 0; i + 1 < line.size(); i += 2) v.push_back((uint8_t)(nib(line[i]) << 4 | nib(line[i + 1])));
    return v;
}
// dense offsets: a sequence a whole number of bytes
static std::vector<uint64_t> dense(const std::vector<uint32_t>& len)
{
    std::vector<uint64_t> off(len.size() + 1, 0);
    for (size_t i = 0; i < len.size(); ++i) off[i + 1] = off[i] + (len[i] + 3) / 4;
    return off;
}

static bool same(const dfk_partners::HostResult& a, const dfk_partners::HostResult& b)
{
    if (a.starts != b.starts || a.recs.size() != b.recs.size()) return false;
    for (size_t i = 0; i < a.recs.size(); ++i) if (a.recs[i].id != b.recs[i].id || a.recs[i].pos != b.recs[i].pos || a.recs[i].fw != 1u || b.recs[i].fw != 1u) return false;
    return a.queries == b.queries && a.positions == b.positions && a.entries == b.entries && a.any_hit == b.any_hit && a.kept == b.kept && a.multi == b.multi && a.searched == b.searched;
}

static void run_case(const Case& c)
{
    using namespace dfk_partners;
    // (exactly sized copies: the last read and the last edge end at the allocation's end)
    std::vector<uint8_t> ep(c.edge_packed), rp(c.read_packed);
    ep.shrink_to_fit(); rp.shrink_to_fit();
    std::vector<uint64_t> locs(c.locs); if (locs.empty()) locs.push_back(0);
    std::vector<int32_t> anchors(c.anchors); if (anchors.empty()) anchors.push_back(0);
    std::vector<uint32_t> read_len(c.read_len); if (read_len.empty()) read_len.push_back(0);
    std::vector<uint64_t> ce(c.ce); if (ce.empty()) ce.push_back(0);
    const Input I{c.inv.size(), c.inv.data(), ep.data(), c.edge_off.data(), c.edge_len.data(), c.ce.size(), ce.data(), c.loc_first.data(), locs.data(), c.anchor_first.data(), anchors.data(),
                  c.read_len.size(), rp.data(), c.read_off.data(), read_len.data()};
    const uint64_t n_pairs = c.pairs.size() / 2;
    std::vector<int32_t> pairs(c.pairs); if (pairs.empty()) pairs.push_back(0);
    HostResult r;
    const int rc = partners_literal(I, pairs.data(), n_pairs, &r);
    CHECK(rc == 0);
    if (rc) return;
    // ---- the literal transcription against the Python restatement
    bool ok = r.starts == c.starts && r.recs.size() * 2 == c.recs.size();
    for (size_t i = 0; ok && i < r.recs.size(); ++i) ok = r.recs[i].id == c.recs[2 * i] && r.recs[i].pos == c.recs[2 * i + 1] && r.recs[i].fw == 1u;
    if (!ok) printf("case %s: the records differ from the recorded ones\n", c.name.c_str());
    CHECK(ok);
    CHECK(r.queries == c.queries && r.positions == c.positions && r.entries == c.entries && r.any_hit == c.any_hit && r.kept == c.kept && r.multi == c.multi && r.searched == c.searched);
    // ---- the device version's order of work gives the same, whatever the batches, the ranges of the table and of the sides
    for (uint64_t per : {(uint64_t)1, (uint64_t)37, (uint64_t)1 << 30})
        for (uint64_t cap : {(uint64_t)1, (uint64_t)1000, (uint64_t)1 << 30}) {
            if (per == 1 && cap == 1 && c.queries > 3000) continue;                // (a table rebuilt per rank and a batch per query: the small cases show it)
            HostResult s;
            CHECK(partners_plan(I, pairs.data(), n_pairs, per, 1ull << 20, cap, cap == 1000 ? 50 : cap, &s) == 0);
            CHECK(same(r, s));
            if (cap == (1ull << 30)) CHECK(s.ranges == (c.ce.empty() ? 0u : 1u));
            if (per == (1ull << 30) && cap == (1ull << 30)) CHECK(s.batches == (c.searched ? 1u : 0u));
            if (per == 1) CHECK(s.batches == c.searched);
        }
    // batches sized by the room: the same again
    HostResult s;
    CHECK(partners_plan(I, pairs.data(), n_pairs, 0, 1000, 1ull << 30, 1ull << 30, &s) == 0 && same(r, s));
    CHECK(file_size(2 * n_pairs, r.recs.size()) == 16 + 8 * (2 * n_pairs + 1) + 16 * r.recs.size());
}

static void cuts_words_and_plans()
{
    using namespace dfk_partners;
    // the cut at every residue of l mod 32 (and so of l mod 4) against the bases taken one by one, on a buffer that ends with the sequence
    srand(99);
    for (uint32_t len : {32u, 33u, 34u, 35u, 63u, 64u, 65u, 96u, 97u, 151u}) {
        std::vector<uint8_t> codes(len);
        for (auto& b : codes) b = (uint8_t)(rand() & 3);
        std::vector<uint8_t> packed((len + 3) / 4, 0);
        for (uint32_t i = 0; i < len; ++i) packed[i >> 2] |= (uint8_t)(codes[i] << (2 * (i & 3)));
        packed.shrink_to_fit();
        for (uint32_t l = 0; l + L <= len; ++l) {
            uint64_t want = 0;
            for (uint32_t j = 0; j < L; ++j) want |= (uint64_t)codes[l + j] << (2 * j);
            CHECK(cut32(packed.data(), l) == want);
        }
        CHECK(positions(len) == len - 31);
    }
    const std::vector<uint8_t> a(8, 0x00), t(8, 0xFF);
    CHECK(cut32(a.data(), 0) == 0 && cut32(t.data(), 0) == ~0ull);
    CHECK(positions(0) == 0 && positions(31) == 0 && positions(32) == 1);
    CHECK(find_of(-3, 5) == -8 && find_of(7, 40) == -33 && entry_pos(-3, 50) == 47 && entry_pos(2147483647, 1) == -2147483647 - 1);
    // the folds
    Fold f{0, 0, 0u};
    CHECK(status_of(f) == Q_NONE);
    fold_hit(f, 5); CHECK(status_of(f) == Q_KEPT && f.lo == 5);
    Fold g{0, 0, 0u}; fold_hit(g, 5);
    CHECK(status_of(fold_join(f, g)) == Q_KEPT && status_of(fold_join(Fold{0, 0, 0u}, g)) == Q_KEPT);
    fold_hit(g, -2); CHECK(status_of(g) == Q_MULTI && status_of(fold_join(f, g)) == Q_MULTI && fold_join(f, g).lo == -2 && fold_join(g, f).hi == 5);
    // the searches
    const uint64_t locs[] = {2, 1ull << 32, 2, 1ull << 32, 6, 1ull << 32, 3, 0, 6, 0};      // ids 2 2 6 forward, 3 6 backward
    CHECK(forward_count(locs, 0, 5) == 3 && forward_count(locs, 3, 5) == 0 && forward_count(locs, 0, 0) == 0 && forward_count(locs, 0, 2) == 2);
    CHECK(has_id(locs, 0, 3, 2) && has_id(locs, 0, 3, 6) && !has_id(locs, 0, 3, 3) && !has_id(locs, 0, 0, 2) && !has_id(locs, 0, 3, 7) && !has_id(locs, 0, 2, 6));
    const uint64_t keys[] = {1, 4, 4, 9};
    CHECK(lower_key(keys, 0, 4, 4) == 1 && lower_key(keys, 0, 4, 0) == 0 && lower_key(keys, 0, 4, 10) == 4 && lower_key(keys, 2, 4, 4) == 2);
    const uint64_t first[] = {0, 0, 3, 3, 7};
    CHECK(owner_of(first, 4, 0) == 1 && owner_of(first, 4, 2) == 1 && owner_of(first, 4, 3) == 3 && owner_of(first, 4, 6) == 3);
    // the plans
    const uint64_t cost[] = {0, 100, 200, 300, 400};
    CHECK(next_batch(cost, 4, 0, 250, 0) == 2 && next_batch(cost, 4, 0, 50, 0) == 1 && next_batch(cost, 4, 1, 1000, 0) == 4 && next_batch(cost, 4, 1, 50, 2) == 3 && next_batch(cost, 4, 3, 50, 37) == 4);
    CHECK(query_cost(0) == 64 && query_cost(151) == 64 + 38 && range_cap(1ull << 40, 77) == 77 && range_cap(0, 0) == (1ull << 18) && item_cap(0, 5) == 5);
    CHECK(range_cap(192ull << 30, 0) * BYTES_PER_ENTRY <= (192ull << 30) / 2 && batch_room(0) == (1ull << 20));
    const uint64_t big[3] = {0, 5, 5 + (1ull << 32)};
    CHECK(next_range(big, 2, 0, 10).ok && !next_range(big, 2, 1, 10).ok);
    CHECK(strlen(MAGIC) == 8 && records_at(0) == 24 && file_size(0, 0) == 24 && file_size(4, 3) == 16 + 40 + 48);
    // the refusals: an edge outside the graph, a closer edge that is not in ce
    const int32_t inv[] = {1, 0, 2};
    const uint64_t ce[] = {0, 2}, zero[3] = {0, 0, 0};
    const uint32_t el[] = {0, 0, 0};
    const Input I{3, inv, nullptr, zero, el, 2, ce, zero, zero, zero, inv, 0, nullptr, zero, el};
    HostResult r;
    const int32_t past[2] = {0, 3}, neg[2] = {-1, 0}, other[2] = {1, 2}, fine[2] = {0, 2};
    CHECK(partners_literal(I, past, 1, &r) == -1 && partners_literal(I, neg, 1, &r) == -1 && partners_literal(I, other, 1, &r) == -2);
    CHECK(partners_literal(I, fine, 1, &r) == 0 && (r.starts == std::vector<uint64_t>{0, 0, 0}) && r.recs.empty());
}

int main(int argc, char** argv)
{
    if (argc != 2) { printf("usage: test_partners <cases file>\n"); return 2; }
    cuts_words_and_plans();
    std::ifstream in(argv[1]);
    if (!in) { printf("cannot read %s\n", argv[1]); return 2; }
    std::string line;
    int n_cases = 0;
    while (std::getline(in, line)) {
        if (line.rfind("case ", 0) != 0) { printf("unexpected line: %.60s\n", line.c_str()); return 2; }
        Case c;
        long long E = 0, N = 0, np = 0, nce = 0;
        { std::istringstream h(line.substr(5)); h >> c.name >> E >> N >> np >> nce; }
        std::string l[14];
        for (auto& s : l) if (!std::getline(in, s)) { printf("case %s is cut short\n", c.name.c_str()); return 2; }
        c.inv = row<int32_t>(l[0]); c.edge_len = row<uint32_t>(l[1]); c.edge_packed = hexrow(l[2]); c.ce = row<uint64_t>(l[3]); c.loc_first = row<uint64_t>(l[4]);
        const std::vector<int64_t> lf = row<int64_t>(l[5]);
        for (size_t i = 0; i + 2 < lf.size(); i += 3) { c.locs.push_back((uint64_t)lf[i]); c.locs.push_back((uint64_t)(uint32_t)(int32_t)lf[i + 1] | ((uint64_t)(lf[i + 2] ? 1 : 0) << 32)); }
        c.anchor_first = row<uint64_t>(l[6]); c.anchors = row<int32_t>(l[7]); c.pairs = row<int32_t>(l[8]); c.read_len = row<uint32_t>(l[9]); c.read_packed = hexrow(l[10]);
        c.starts = row<uint64_t>(l[11]); c.recs = row<int64_t>(l[12]);
        const std::vector<uint64_t> k = row<uint64_t>(l[13]);
        c.edge_off = dense(c.edge_len); c.read_off = dense(c.read_len);
        if (k.size() != 7 || c.inv.size() != (size_t)E || c.edge_len.size() != (size_t)E || c.read_len.size() != (size_t)N || c.pairs.size() != 2 * (size_t)np || c.ce.size() != (size_t)nce ||
            c.loc_first.size() != (size_t)nce + 1 || c.anchor_first.size() != (size_t)nce + 1 || c.edge_packed.size() != c.edge_off.back() || c.read_packed.size() != c.read_off.back() ||
            c.locs.size() != 2 * c.loc_first.back() || c.anchors.size() != 3 * c.anchor_first.back() || c.starts.size() != 2 * (size_t)np + 1) { printf("case %s is malformed\n", c.name.c_str()); return 2; }
        c.queries = k[0]; c.positions = k[1]; c.entries = k[2]; c.any_hit = k[3]; c.kept = k[4]; c.multi = k[5]; c.searched = k[6];
        run_case(c);
        ++n_cases;
    }
    if (g_failed) { printf("%d check(s) failed\n", g_failed); return 1; }
    printf("%d recorded cases agree\n", n_cases);
    return 0;
}
