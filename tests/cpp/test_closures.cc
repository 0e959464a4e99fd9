// tests/cpp/test_closures.cc -- superplus_amd/csrc/dfk_closures.h on the host: the literal per-pair transcription (both stacks
// materialised, Merge by its resize / shift / append, Consensus1 by its sort) against the cases recorded from tests/closures_oracle.py
// (tests/cpp/closures_cases.txt, and fixtures written out in the same form), the device version's order of work (closures_plan: the
// closable pairs' stacks alone, ranges of whole pairs, batches of closures, a lane a merged column over stack 0's live rows then stack
// 1's) against the literal one under closures_per_batch 1, 37 and 2^30 and several row caps, the merged width in both of Merge's forms,
// the column maps, the (sum, id) maximum, the cross-boundary sum, the file's fixed parts.  Its own main; built plain and under
// -fsanitize=address,undefined by tests/test_closures_cpu.py.
//   test_closures <cases file>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include "dfk_closures.h"

static int g_failed = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++g_failed; } } while (0)

struct Case {
    std::string name;
    uint32_t K = 0;
    std::vector<int32_t> inv, kmers, pairs, offsets;
    std::vector<uint32_t> read_len;
    std::vector<uint8_t> read_packed, pq, bases;
    std::vector<uint64_t> read_off, pq_off, ce, loc_first, locs, part_first, parts, off_first, pair_first, starts;
    std::vector<int64_t> recs;
    uint64_t closable = 0, over = 0, columns = 0, added = 0, live = 0, empty = 0, shorter = 0, rowless = 0;
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
static std::vector<uint64_t> words(const std::vector<int64_t>& flat)        // ( id, pos, fw ) -> two words a record
{
    std::vector<uint64_t> w;
    for (size_t i = 0; i + 2 < flat.size(); i += 3) { w.push_back((uint64_t)flat[i]); w.push_back((uint64_t)(uint32_t)(int32_t)flat[i + 1] | ((uint64_t)(flat[i + 2] ? 1 : 0) << 32)); }
    return w;
}
static std::vector<uint64_t> dense(const std::vector<uint32_t>& len)
{
    std::vector<uint64_t> off(len.size() + 1, 0);
    for (size_t i = 0; i < len.size(); ++i) off[i + 1] = off[i] + (len[i] + 3) / 4;
    return off;
}

static bool same(const dfk_closures::HostResult& a, const dfk_closures::HostResult& b)
{
    if (a.pair_first != b.pair_first || a.starts != b.starts || a.bases != b.bases || a.recs.size() != b.recs.size()) return false;
    for (size_t i = 0; i < a.recs.size(); ++i) if (memcmp(&a.recs[i], &b.recs[i], sizeof(dfk_closures::Rec)) != 0) return false;
    return a.closable == b.closable && a.over == b.over && a.columns == b.columns && a.added == b.added && a.empty == b.empty && a.shorter == b.shorter && a.rowless == b.rowless;
}

static void run_case(const Case& c)
{
    using namespace dfk_closures;
    std::vector<uint8_t> rp(c.read_packed), pq(c.pq);                          // (exactly sized copies: the last read ends at the allocation's end)
    rp.shrink_to_fit(); pq.shrink_to_fit();
    auto room = [](auto v) { if (v.empty()) v.push_back(0); return v; };
    const std::vector<uint64_t> locs = room(c.locs), parts = room(c.parts), ce = room(c.ce);
    const std::vector<uint32_t> read_len = room(c.read_len);
    const std::vector<int32_t> pairs = room(c.pairs), offsets = room(c.offsets);
    const dfk_cons::Input I{c.inv.size(), c.inv.data(), c.kmers.data(), c.K, c.ce.size(), ce.data(), c.loc_first.data(), locs.data(), c.part_first.data(), parts.data(),
                            c.read_len.size(), rp.data(), c.read_off.data(), read_len.data(), pq.data(), c.pq_off.data()};
    const uint64_t n_pairs = c.pairs.size() / 2;
    HostResult r;
    const int rc = closures_literal(I, pairs.data(), n_pairs, c.off_first.data(), offsets.data(), &r);
    CHECK(rc == 0);
    if (rc) return;
    // ---- the literal transcription against the Python restatement
    bool ok = r.pair_first == c.pair_first && r.starts == c.starts && r.bases == c.bases && 4 * r.recs.size() == c.recs.size();
    for (size_t i = 0; ok && i < r.recs.size(); ++i)
        ok = r.recs[i].pair == (uint32_t)c.recs[4 * i] && r.recs[i].offset == (int32_t)c.recs[4 * i + 1] && r.recs[i].cols == (uint32_t)c.recs[4 * i + 2] && r.recs[i].rows == (uint32_t)c.recs[4 * i + 3];
    if (!ok) printf("case %s: pair table, starts, records or bases differ from the recorded ones\n", c.name.c_str());
    CHECK(ok);
    CHECK(r.closable == c.closable && r.over == c.over && r.columns == c.columns && r.added == c.added && r.empty == c.empty && r.shorter == c.shorter && r.rowless == c.rowless);
    for (size_t i = 0; i < r.recs.size(); ++i) CHECK(r.starts[i + 1] - r.starts[i] == r.recs[i].cols && r.recs[i].cols <= (uint32_t)MAX_COLS);
    // ---- the device version's order of work gives the same, whatever the batches and the ranges
    for (uint64_t per : {(uint64_t)1, (uint64_t)37, (uint64_t)1 << 30})
        for (uint64_t cap : {(uint64_t)1, (uint64_t)100, (uint64_t)1 << 30}) {
            if (per == 37 && cap == 1) continue;
            HostResult s;
            CHECK(closures_plan(I, pairs.data(), n_pairs, c.off_first.data(), offsets.data(), per, 1ull << 20, cap, &s) == 0);
            CHECK(same(r, s));
            CHECK(s.live == c.live);
            if (cap == (1ull << 30)) CHECK(s.ranges == (c.closable ? 1u : 0u));
            if (cap == 1 && c.closable > 3 && c.live > 3) CHECK(s.ranges > 1 && s.ranges <= c.closable);
            if (per == (1ull << 30)) CHECK(s.batches == s.ranges);
            if (per == 1) CHECK(s.batches == r.recs.size());
        }
    HostResult s;                                                              // batches sized by the room: the same again
    CHECK(closures_plan(I, pairs.data(), n_pairs, c.off_first.data(), offsets.data(), 0, 6000, 1ull << 30, &s) == 0 && same(r, s));
    CHECK(file_size(r.recs.size(), n_pairs, r.bases.size()) == 24 + 8 * (n_pairs + 1) + 8 * (r.recs.size() + 1) + 16 * r.recs.size() + (r.bases.size() + 7) / 8 * 8);
    // an offset past either end of its pair refuses the call in both forms
    if (!r.recs.empty()) {
        std::vector<int32_t> bad(offsets);
        const uint64_t pi = r.recs[0].pair;
        bad[c.off_first[pi]] = 401;
        HostResult x, y;
        CHECK(closures_literal(I, pairs.data(), n_pairs, c.off_first.data(), bad.data(), &x) == -4 && closures_plan(I, pairs.data(), n_pairs, c.off_first.data(), bad.data(), 0, 1ull << 20, 1ull << 30, &y) == -4);
        bad[c.off_first[pi]] = -401;
        HostResult x2, y2;
        CHECK(closures_literal(I, pairs.data(), n_pairs, c.off_first.data(), bad.data(), &x2) == -4 && closures_plan(I, pairs.data(), n_pairs, c.off_first.data(), bad.data(), 0, 1ull << 20, 1ull << 30, &y2) == -4);
    }
}

static void widths_maps_and_sums()
{
    using namespace dfk_closures;
    // Merge's width: both forms equal merged_cols wherever the offset is allowed
    for (int cols1 : {0, 1, 5, 256, 313, 400})
        for (int cols2 : {0, 1, 7, 256, 392, 400})
            for (int off = -cols2; off <= cols1; ++off) {
                int f1, f2;
                both_forms(cols1, cols2, off, &f1, &f2);
                CHECK(f1 == f2 && f1 == (int)merged_cols(cols1, cols2, off) && f1 <= (int)MAX_COLS && offset_ok(cols1, cols2, off));
            }
    CHECK(!offset_ok(5, 7, 6) && !offset_ok(5, 7, -8) && offset_ok(0, 0, 0) && !offset_ok(0, 0, 1));
    CHECK(merged_cols(256, 256, 0) == 256 && merged_cols(256, 256, 1) == 257 && merged_cols(256, 256, 256) == 512 && merged_cols(256, 256, -256) == 512 && merged_cols(400, 313, 200) == 513 &&
          merged_cols(400, 400, 392) == 792 && merged_cols(400, 400, 400) == 800 && merged_cols(400, 313, 10) == 400 && merged_cols(256, 400, -50) == 400);
    int f1, f2;
    both_forms(5, 7, 9, &f1, &f2);                                             // (past either end the forms still agree; the entry refuses such an offset for the width's sake)
    CHECK(f1 == 16 && f2 == 16 && merged_cols(5, 7, 9) == 16);
    both_forms(5, 7, -9, &f1, &f2);
    CHECK(f1 == 14 && f2 == 14 && merged_cols(5, 7, -9) == 14);
    // the column maps
    CHECK(column_of_side(0, 5, 3, 0) == 0 && column_of_side(0, 5, 3, 4) == 4 && column_of_side(0, 5, 3, 5) == -1 && column_of_side(1, 7, 3, 2) == -1 && column_of_side(1, 7, 3, 3) == 0 && column_of_side(1, 7, 3, 9) == 6 &&
          column_of_side(1, 7, 3, 10) == -1);
    CHECK(column_of_side(0, 5, -2, 1) == -1 && column_of_side(0, 5, -2, 2) == 0 && column_of_side(0, 5, -2, 6) == 4 && column_of_side(0, 5, -2, 7) == -1 && column_of_side(1, 7, -2, 0) == 0 && column_of_side(1, 7, -2, 6) == 6);
    // the maximum: the greatest (sum, id)
    const double tie[4] = {5, 5, 0, 0}, none[4] = {0, 0, 0, 0}, one[4] = {0, .1, 0, 0}, tie2[4] = {7, 0, 7, 1};
    CHECK(last_max(tie) == 1 && last_max(none) == 3 && last_max(one) == 1 && last_max(tie2) == 2 && dfk_cons::first_max(tie) == 0 && dfk_cons::first_max(none) == 0 && dfk_cons::first_max(tie2) == 0);
    // the sums cross the stack boundary
    double a[4] = {0, 0, 0, 0};
    dfk_cons::add_cell(a, 0, 20); dfk_cons::add_cell(a, 1, 2);                                                                    // stack 0
    dfk_cons::add_cell(a, 0, 0); dfk_cons::add_cell(a, 0, 0); dfk_cons::add_cell(a, 1, 10); dfk_cons::add_cell(a, 1, 10);         // stack 1
    CHECK(a[0] == 20.200000000000003 && a[1] == 20.2 && last_max(a) == 0);
    double s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};
    dfk_cons::add_cell(s0, 0, 20); dfk_cons::add_cell(s0, 1, 2);
    dfk_cons::add_cell(s1, 0, 0); dfk_cons::add_cell(s1, 0, 0); dfk_cons::add_cell(s1, 1, 10); dfk_cons::add_cell(s1, 1, 10);
    const double per_stack[4] = {s0[0] + s1[0], s0[1] + s1[1], 0, 0};
    CHECK(per_stack[0] == 20.2 && per_stack[1] == 20.2 && last_max(per_stack) == 1);
    // the plan's sizes, the file's fixed parts
    CHECK(TILES == 4 && MAX_COLS == 800 && closures_grid(0, 256) == 1 && closures_grid(5, 256) == 20 && closures_grid(1ull << 20, 256) == 8192);
    CHECK(strlen(MAGIC) == 8 && pair_first_at() == 24 && starts_at(0) == 32 && recs_at(0, 0) == 40 && bases_at(2, 3) == 24 + 32 + 24 + 32 && file_size(0, 0, 0) == 40 && file_size(1, 1, 9) == 24 + 16 + 16 + 16 + 16);
    // Merge and Consensus1 on a stack of two rows each, by hand: offset 1
    dfk_cons::Grids t, u;
    t.rows = 2; t.cols = 2; t.bases_ = {{0, 1}, {0, ' '}}; t.quals_ = {{10, 10}, {10, -1}};
    u.rows = 1; u.cols = 2; u.bases_ = {{2, 3}}; u.quals_ = {{10, 0}};
    dfk_cons::Grids m(t);
    merge_literal(&m, u, 1);
    CHECK(m.rows == 3 && m.cols == 3 && m.bases_[0].size() == 3 && m.bases_[2][0] == ' ' && m.bases_[2][1] == 2 && m.bases_[2][2] == 3 && m.quals_[0][2] == -1);
    std::vector<uint8_t> con; HostResult cnt;
    consensus1_literal(m, &con, &cnt);
    CHECK((con == std::vector<uint8_t>{0, 2, 3}) && cnt.added == 5 && cnt.empty == 0);
    dfk_cons::Grids n(t);
    merge_literal(&n, u, -2);
    CHECK(n.cols == 4 && n.bases_[0][0] == ' ' && n.bases_[0][2] == 0 && n.bases_[2][0] == 2 && n.bases_[2][3] == ' ');
    // without rows on either side: the rule's width
    dfk_cons::Grids e0, e1;
    e0.cols = 400; e1.cols = 400;
    merge_literal(&e0, e1, 100);
    CHECK(e0.rows == 0 && e0.cols == 500);
}

int main(int argc, char** argv)
{
    if (argc != 2) { printf("usage: test_closures <cases file>\n"); return 2; }
    widths_maps_and_sums();
    std::ifstream in(argv[1]);
    if (!in) { printf("cannot read %s\n", argv[1]); return 2; }
    std::string line;
    int n_cases = 0;
    while (std::getline(in, line)) {
        if (line.rfind("case ", 0) != 0) { printf("unexpected line: %.60s\n", line.c_str()); return 2; }
        Case c;
        long long E = 0, N = 0, np = 0, nce = 0, K = 0;
        { std::istringstream h(line.substr(5)); h >> c.name >> E >> N >> np >> nce >> K; }
        c.K = (uint32_t)K;
        std::string l[19];
        for (auto& s : l) if (!std::getline(in, s)) { printf("case %s is cut short\n", c.name.c_str()); return 2; }
        c.inv = row<int32_t>(l[0]); c.kmers = row<int32_t>(l[1]); c.ce = row<uint64_t>(l[2]); c.loc_first = row<uint64_t>(l[3]); c.locs = words(row<int64_t>(l[4]));
        c.part_first = row<uint64_t>(l[5]); c.parts = words(row<int64_t>(l[6])); c.pairs = row<int32_t>(l[7]); c.read_len = row<uint32_t>(l[8]); c.read_packed = hexrow(l[9]);
        c.pq_off = row<uint64_t>(l[10]); c.pq = hexrow(l[11]); c.off_first = row<uint64_t>(l[12]); c.offsets = row<int32_t>(l[13]); c.pair_first = row<uint64_t>(l[14]);
        c.starts = row<uint64_t>(l[15]); c.recs = row<int64_t>(l[16]);
        if (l[17] != "-") for (char ch : l[17]) c.bases.push_back((uint8_t)(ch - '0'));
        const std::vector<uint64_t> k = row<uint64_t>(l[18]);
        c.read_off = dense(c.read_len);
        if (k.size() != 8 || c.inv.size() != (size_t)E || c.kmers.size() != (size_t)E || c.read_len.size() != (size_t)N || c.pairs.size() != 2 * (size_t)np || c.ce.size() != (size_t)nce ||
            c.loc_first.size() != (size_t)nce + 1 || c.part_first.size() != 2 * (size_t)np + 1 || c.read_packed.size() != c.read_off.back() || c.pq_off.size() != (size_t)N + 1 || c.pq.size() != c.pq_off.back() ||
            c.locs.size() != 2 * c.loc_first.back() || c.parts.size() != 2 * c.part_first.back() || c.off_first.size() != (size_t)np + 1 || c.offsets.size() != c.off_first.back() ||
            c.pair_first.size() != (size_t)np + 1 || c.starts.size() != c.pair_first.back() + 1 || c.recs.size() != 4 * c.pair_first.back() || c.bases.size() != c.starts.back()) {
            printf("case %s is malformed\n", c.name.c_str()); return 2;
        }
        c.closable = k[0]; c.over = k[1]; c.columns = k[2]; c.added = k[3]; c.live = k[4]; c.empty = k[5]; c.shorter = k[6]; c.rowless = k[7];
        run_case(c);
        ++n_cases;
    }
    if (g_failed) { printf("%d check(s) failed\n", g_failed); return 1; }
    printf("%d recorded cases agree\n", n_cases);
    return 0;
}
