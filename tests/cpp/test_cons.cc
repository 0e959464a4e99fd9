// tests/cpp/test_cons.cc -- superplus_amd/csrc/dfk_cons.h on the host: the literal per-pair transcription (the stack materialised)
// against the cases recorded from tests/cons_oracle.py (tests/cpp/cons_cases.txt, and fixtures written out in the same form), the
// device version's order of work (cons_plan: ranges of stacks, dimensions, live rows by flag, scan and emit, batches, the reads of a
// batch each once, the decode, a lane a column over the live rows in order) against the literal one under stacks_per_batch 1, 37 and
// 2^30 and several row caps, the cell, the two double-rounding sums, the plan's sizes, the file's fixed parts.  Its own main; built
// plain and under -fsanitize=address,undefined by tests/test_cons_cpu.py.
//   test_cons <cases file>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include "dfk_cons.h"

static int g_failed = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++g_failed; } } while (0)

struct Case {
    std::string name;
    uint32_t K = 0;
    std::vector<int32_t> inv, kmers, pairs;
    std::vector<uint32_t> read_len;
    std::vector<uint8_t> read_packed, pq, bases;
    std::vector<uint64_t> read_off, pq_off, ce, loc_first, locs, part_first, parts, starts;
    std::vector<int64_t> dims;
    uint64_t rows = 0, live = 0, rows_kept = 0, trimmed = 0, reversed = 0, columns = 0, added = 0;
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

static bool same(const dfk_cons::HostResult& a, const dfk_cons::HostResult& b)
{
    if (a.starts != b.starts || a.bases != b.bases || a.dims.size() != b.dims.size()) return false;
    for (size_t i = 0; i < a.dims.size(); ++i) if (memcmp(&a.dims[i], &b.dims[i], sizeof(dfk_cons::Dim)) != 0) return false;
    return a.rows == b.rows && a.rows_kept == b.rows_kept && a.trimmed == b.trimmed && a.reversed == b.reversed && a.columns == b.columns && a.added == b.added;
}

static void run_case(const Case& c)
{
    using namespace dfk_cons;
    std::vector<uint8_t> rp(c.read_packed), pq(c.pq);                          // (exactly sized copies: the last read ends at the allocation's end)
    rp.shrink_to_fit(); pq.shrink_to_fit();
    auto room = [](auto v) { if (v.empty()) v.push_back(0); return v; };
    const std::vector<uint64_t> locs = room(c.locs), parts = room(c.parts), ce = room(c.ce);
    const std::vector<uint32_t> read_len = room(c.read_len);
    const std::vector<int32_t> pairs = room(c.pairs);
    const Input I{c.inv.size(), c.inv.data(), c.kmers.data(), c.K, c.ce.size(), ce.data(), c.loc_first.data(), locs.data(), c.part_first.data(), parts.data(),
                  c.read_len.size(), rp.data(), c.read_off.data(), read_len.data(), pq.data(), c.pq_off.data()};
    const uint64_t n_pairs = c.pairs.size() / 2;
    HostResult r;
    const int rc = cons_literal(I, pairs.data(), n_pairs, &r);
    CHECK(rc == 0);
    if (rc) return;
    // ---- the literal transcription against the Python restatement
    bool ok = r.starts == c.starts && r.bases == c.bases && 4 * r.dims.size() == c.dims.size();
    for (size_t i = 0; ok && i < r.dims.size(); ++i)
        ok = r.dims[i].rows == (uint32_t)c.dims[4 * i] && r.dims[i].rows_kept == (uint32_t)c.dims[4 * i + 1] && r.dims[i].M == (int32_t)c.dims[4 * i + 2] && r.dims[i].cols == (uint32_t)c.dims[4 * i + 3];
    if (!ok) printf("case %s: starts, dims or bases differ from the recorded ones\n", c.name.c_str());
    CHECK(ok);
    CHECK(r.rows == c.rows && r.rows_kept == c.rows_kept && r.trimmed == c.trimmed && r.reversed == c.reversed && r.columns == c.columns && r.added == c.added);
    for (size_t i = 0; i < r.dims.size(); ++i) CHECK(r.starts[i + 1] - r.starts[i] == r.dims[i].cols && r.dims[i].cols == (uint32_t)std::min<int64_t>(r.dims[i].M, MAX_WIDTH));
    // ---- the device version's order of work gives the same, whatever the batches and the ranges
    for (uint64_t per : {(uint64_t)1, (uint64_t)37, (uint64_t)1 << 30})
        for (uint64_t cap : {(uint64_t)1, (uint64_t)100, (uint64_t)1 << 30}) {
            if (per == 37 && cap == 1) continue;
            HostResult s;
            CHECK(cons_plan(I, pairs.data(), n_pairs, per, 1ull << 20, cap, &s) == 0);
            CHECK(same(r, s));
            CHECK(s.live == c.live);
            if (cap == (1ull << 30)) CHECK(s.ranges == (n_pairs ? 1u : 0u));
            if (cap == 1 && c.rows > 3) CHECK(s.ranges > 1 && s.ranges <= 2 * n_pairs);          // (stacks without rows share a range)
            if (per == (1ull << 30)) CHECK(s.batches == s.ranges);
            if (per == 1) CHECK(s.batches == 2 * n_pairs);
        }
    HostResult s;                                                              // batches sized by the room: the same again
    CHECK(cons_plan(I, pairs.data(), n_pairs, 0, 3000, 1ull << 30, &s) == 0 && same(r, s));
    CHECK(file_size(2 * n_pairs, r.bases.size()) == 16 + 8 * (2 * n_pairs + 1) + 32 * n_pairs + (r.bases.size() + 7) / 8 * 8);
    // streams that do not hold len values (every one ends at once) refuse the call in both forms
    if (c.live) {
        const std::vector<uint8_t> none(pq.size(), 0);
        Input J = I; J.pq = none.data();
        HostResult x, y;
        CHECK(cons_literal(J, pairs.data(), n_pairs, &x) == -3 && cons_plan(J, pairs.data(), n_pairs, 0, 1ull << 20, 1ull << 30, &y) == -3);
    }
}

static void cells_sums_and_plans()
{
    using namespace dfk_cons;
    // the cell: forward, and not; off either end
    CHECK(cell_index(true, 5, 3, 100, 5) == 0 && cell_index(true, 5, 3, 100, 7) == 2 && cell_index(true, 5, 3, 100, 8) == -1 && cell_index(true, 5, 3, 100, 4) == -1);
    CHECK(cell_index(true, -2, 3, 100, 0) == 2 && cell_index(true, -3, 3, 100, 0) == -1);
    CHECK(cell_index(false, 90, 3, 100, 9) == 0 && cell_index(false, 90, 3, 100, 7) == 2 && cell_index(false, 90, 3, 100, 6) == -1 && cell_index(false, 98, 5, 100, 0) == 1);
    CHECK(cell_base(1, true, false) == 1 && cell_base(1, false, false) == 2 && cell_base(1, true, true) == 2 && cell_base(1, false, true) == 1);
    CHECK(cell_defined(127) && !cell_defined(128) && !cell_defined(255) && cell_defined(0));
    CHECK(row_end(true, -200, 100, 50) == -100 && row_end(false, 3, 100, 50) == 47 && window_start(400) == 0 && window_start(401) == 1 && window_start(0) == 0);
    CHECK(!row_live(true, 0, 0, 50, 0) && row_live(true, 0, 1, 50, 0) && !row_live(true, 0, 1, 50, 1) && !row_live(true, -5, 5, 50, 0) && row_live(false, 3, 1, 50, 46) && !row_live(false, 3, 1, 50, 47));
    CHECK(stack_column(7, 400, false, 0) == 7 && stack_column(7, 400, true, 0) == 406 && stack_column(7, 400, true, 399) == 7);
    const uint8_t packed[] = {0xE4, 0x01};
    CHECK(base_at(packed, 0) == 0 && base_at(packed, 1) == 1 && base_at(packed, 2) == 2 && base_at(packed, 3) == 3 && base_at(packed, 4) == 1);
    // the sums: the order of the additions and the doubles decide
    double a[4] = {0, 0, 0, 0};
    add_cell(a, 0, 2); add_cell(a, 0, 10); add_cell(a, 0, 10); add_cell(a, 1, 20); add_cell(a, 1, 0); add_cell(a, 1, 0);
    CHECK(a[0] == 20.2 && a[1] == 20.200000000000003 && a[0] < a[1] && first_max(a) == 1);
    double b[4] = {0, 0, 0, 0};
    add_cell(b, 3, 2); add_cell(b, 3, 37); add_cell(b, 3, 10); add_cell(b, 3, 0); add_cell(b, 2, 0); add_cell(b, 2, 2); add_cell(b, 2, 10); add_cell(b, 2, 37);
    CHECK(b[3] == 47.300000000000004 && b[2] == 47.3 && first_max(b) == 3);
    const double tie[4] = {0, 5, 5, 0}, none[4] = {0, 0, 0, 0};
    CHECK(first_max(tie) == 1 && first_max(none) == 0 && quality_value(0) == .1 && quality_value(1) == .2 && quality_value(2) == .2 && quality_value(3) == 3. && quality_value(127) == 127.);
    const uint64_t first[] = {0, 0, 3, 3, 7};
    CHECK(owner_of(first, 4, 0) == 1 && owner_of(first, 4, 2) == 1 && owner_of(first, 4, 3) == 3 && owner_of(first, 4, 6) == 3);
    const uint32_t ids[] = {2, 5, 9};
    CHECK(slot_of(ids, 3, 2) == 0 && slot_of(ids, 3, 5) == 1 && slot_of(ids, 3, 9) == 2);
    // the plans
    const uint64_t cost[] = {0, 100, 200, 300, 400};
    CHECK(next_batch(cost, 4, 0, 250, 0) == 2 && next_batch(cost, 4, 0, 50, 0) == 1 && next_batch(cost, 4, 1, 1000, 0) == 4 && next_batch(cost, 4, 1, 50, 2) == 3 && next_batch(cost, 4, 3, 50, 37) == 4);
    CHECK(row_cap(1ull << 40, 77) == 77 && row_cap(0, 0) == (1ull << 18) && row_cap(192ull << 30, 0) * BYTES_PER_ROW <= (192ull << 30) / 2 && batch_room(0) == (1ull << 20));
    CHECK(live_row_cost(151) >= 48 + 38 + 151 + 151 + 3 + 1 && live_row_cost(0) == 52 && cons_grid(0, 256) == 1 && cons_grid(5, 256) == 5 && cons_grid(1ull << 20, 256) == 8192);
    CHECK(strlen(MAGIC) == 8 && dims_at(0) == 24 && bases_at(2) == 16 + 24 + 32 && padded(0) == 0 && padded(1) == 8 && padded(8) == 8 && file_size(0, 0) == 24);
    // the decoder: a constant block, a mixed block, a stream too short and too long
    const uint8_t pq[] = {3, (uint8_t)(30 << 3), 0, 0, 2, (uint8_t)(1 | (5 << 3)), 0x04, 0, 0};   // 30 30 30 | 5 6 (bits: 0, 1 from bit 9)
    uint8_t out[8] = {};
    CHECK(decode_quals(pq, 0, 4, out, 3) && out[0] == 30 && out[2] == 30 && !decode_quals(pq, 0, 4, out, 4) && !decode_quals(pq, 0, 4, out, 2));
    CHECK(decode_quals(pq, 4, 9, out, 2) && out[0] == 5 && out[1] == 6 && decode_quals(pq, 3, 4, out, 0));
    // the refusals
    const int32_t inv[] = {1, 0, 2}, km[] = {1, 1, 1};
    const uint64_t ce[] = {0, 2}, zero[4] = {0, 0, 0, 0};
    const uint32_t el[] = {0};
    const Input I{3, inv, km, 48, 2, ce, zero, zero, zero, zero, 0, nullptr, zero, el, nullptr, zero};
    HostResult r;
    const int32_t past[2] = {0, 3}, neg[2] = {-1, 0}, other[2] = {1, 2}, fine[2] = {0, 2};
    CHECK(cons_literal(I, past, 1, &r) == -1 && cons_literal(I, neg, 1, &r) == -1 && cons_literal(I, other, 1, &r) == -2);
    HostResult e;
    CHECK(cons_literal(I, fine, 1, &e) == 0 && (e.starts == std::vector<uint64_t>{0, 0, 0}) && e.bases.empty() && e.dims.size() == 2 && e.dims[0].M == 0 && e.reversed == 1);
}

int main(int argc, char** argv)
{
    if (argc != 2) { printf("usage: test_cons <cases file>\n"); return 2; }
    cells_sums_and_plans();
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
        std::string l[16];
        for (auto& s : l) if (!std::getline(in, s)) { printf("case %s is cut short\n", c.name.c_str()); return 2; }
        c.inv = row<int32_t>(l[0]); c.kmers = row<int32_t>(l[1]); c.ce = row<uint64_t>(l[2]); c.loc_first = row<uint64_t>(l[3]); c.locs = words(row<int64_t>(l[4]));
        c.part_first = row<uint64_t>(l[5]); c.parts = words(row<int64_t>(l[6])); c.pairs = row<int32_t>(l[7]); c.read_len = row<uint32_t>(l[8]); c.read_packed = hexrow(l[9]);
        c.pq_off = row<uint64_t>(l[10]); c.pq = hexrow(l[11]); c.starts = row<uint64_t>(l[12]); c.dims = row<int64_t>(l[13]);
        if (l[14] != "-") for (char ch : l[14]) c.bases.push_back((uint8_t)(ch - '0'));
        const std::vector<uint64_t> k = row<uint64_t>(l[15]);
        c.read_off = dense(c.read_len);
        if (k.size() != 7 || c.inv.size() != (size_t)E || c.kmers.size() != (size_t)E || c.read_len.size() != (size_t)N || c.pairs.size() != 2 * (size_t)np || c.ce.size() != (size_t)nce ||
            c.loc_first.size() != (size_t)nce + 1 || c.part_first.size() != 2 * (size_t)np + 1 || c.read_packed.size() != c.read_off.back() || c.pq_off.size() != (size_t)N + 1 || c.pq.size() != c.pq_off.back() ||
            c.locs.size() != 2 * c.loc_first.back() || c.parts.size() != 2 * c.part_first.back() || c.starts.size() != 2 * (size_t)np + 1 || c.dims.size() != 8 * (size_t)np || c.bases.size() != c.starts.back()) {
            printf("case %s is malformed\n", c.name.c_str()); return 2;
        }
        c.rows = k[0]; c.live = k[1]; c.rows_kept = k[2]; c.trimmed = k[3]; c.reversed = k[4]; c.columns = k[5]; c.added = k[6];
        run_case(c);
        ++n_cases;
    }
    if (g_failed) { printf("%d check(s) failed\n", g_failed); return 1; }
    printf("%d recorded cases agree\n", n_cases);
    return 0;
}
