// tests/cpp/test_sclosures.cc -- superplus_amd/csrc/dfk_sclosures.h on the host: the literal per-pair transcription (both stacks
// materialised as grids by dfk_scons.h's stack_grids, Trim, Merge and Consensus1 as written) against the cases recorded from
// tests/sclosures_oracle.py (tests/cpp/sclosures_cases.txt, and fixtures written out in the same form); the device version's order of
// work (sclosures_plan: the closable pairs' stacks alone, ranges of whole pairs, batches of closures, a lane a merged column, the rows a
// tile skips, the flags counted) against the literal one under closures_per_batch 1, 37 and 0 and three row caps; merged_cols() and
// column_of_side() held to the literal Trim + Merge for every allowed offset of several width pairs; tile_span() and row_meets() held to
// the cells one by one.  Its own main; built plain and under -fsanitize=address,undefined by tests/test_sclosures_cpu.py.
//   test_sclosures <cases file>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include "dfk_sclosures.h"

static int g_failed = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++g_failed; } } while (0)

struct Case {
    std::string name;
    uint32_t K = 48;
    std::vector<uint64_t> starts, read_off, pq_off, so_counts;
    std::vector<dfk_walks::Rec> recs;
    std::vector<dfk_walks::Loc> locs;
    std::vector<uint32_t> read_len;
    std::vector<uint8_t> read_packed, pq;
    std::vector<int64_t> dims;
    std::vector<uint32_t> words;
    std::vector<dfk_soffsets::Rec> so;
    std::vector<int64_t> want;                      // the expected records: pair offset cols rows
    std::vector<uint8_t> bases;
    std::vector<uint64_t> k;                        // pairs yields closable none over closures columns added live erased empty short rowless
};

template <class T> static std::vector<T> row(const std::string& line)
{
    std::vector<T> v;
    if (line == "-") return v;
    std::istringstream in(line);
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

static bool same(const dfk_sclosures::HostResult& a, const dfk_sclosures::HostResult& b)
{
    if (a.pair_first != b.pair_first || a.starts != b.starts || a.bases != b.bases || a.recs.size() != b.recs.size()) return false;
    if (!a.recs.empty() && memcmp(a.recs.data(), b.recs.data(), 16 * a.recs.size()) != 0) return false;
    return a.yields == b.yields && a.closable == b.closable && a.none == b.none && a.over == b.over && a.columns == b.columns && a.added == b.added && a.live == b.live && a.erased == b.erased &&
           a.empty == b.empty && a.shorter == b.shorter && a.rowless == b.rowless;
}

static void run_case(const Case& c)
{
    using namespace dfk_sclosures;
    std::vector<uint8_t> rp(c.read_packed), pq(c.pq);                          // (exactly sized copies: the last read ends at the allocation's end)
    rp.shrink_to_fit(); pq.shrink_to_fit();
    auto room = [](auto v) { if (v.empty()) v.emplace_back(); return v; };
    const std::vector<dfk_walks::Rec> recs = room(c.recs);
    const std::vector<dfk_walks::Loc> locs = room(c.locs);
    const std::vector<uint32_t> read_len = room(c.read_len);
    const std::vector<dfk_soffsets::Rec> so = room(c.so);
    const uint64_t n_pairs = c.recs.size() / 2;
    std::vector<dfk_scons::Dim> dims(2 * n_pairs + 1);
    for (uint64_t q = 0; q < 2 * n_pairs; ++q) dims[q] = dfk_scons::Dim{(uint32_t)c.dims[4 * q], (uint32_t)c.dims[4 * q + 1], (int32_t)(uint32_t)c.dims[4 * q + 2], (uint32_t)c.dims[4 * q + 3]};
    std::vector<uint64_t> so_starts(n_pairs + 1, 0);
    std::vector<dfk_soffsets::PairWords> words(n_pairs + 1);
    for (uint64_t p = 0; p < n_pairs; ++p) { so_starts[p + 1] = so_starts[p] + c.so_counts[p]; words[p] = dfk_soffsets::PairWords{c.words[4 * p], c.words[4 * p + 1], c.words[4 * p + 2], c.words[4 * p + 3]}; }
    CHECK(so_starts.back() == c.so.size());
    const Input I{dfk_scons::Input{n_pairs, c.starts.data(), recs.data(), locs.data(), c.read_len.size(), rp.data(), c.read_off.data(), read_len.data(), pq.data(), c.pq_off.data()},
                  dims.data(), so_starts.data(), words.data(), so.data()};
    HostResult r;
    const int rc = sclosures_literal(I, c.K, &r);
    CHECK(rc == 0);
    if (rc) return;
    // ---- the literal transcription against the Python restatement
    bool ok = 4 * r.recs.size() == c.want.size() && r.bases == c.bases && r.pair_first.size() == n_pairs + 1 && r.starts.size() == r.recs.size() + 1;
    for (size_t i = 0; ok && i < r.recs.size(); ++i)
        ok = r.recs[i].pair == (uint32_t)c.want[4 * i] && r.recs[i].offset == (int32_t)c.want[4 * i + 1] && r.recs[i].cols == (uint32_t)c.want[4 * i + 2] && r.recs[i].rows == (uint32_t)c.want[4 * i + 3];
    if (!ok) printf("case %s: the records or the bases differ from the recorded ones (%zu closures, %zu recorded)\n", c.name.c_str(), r.recs.size(), c.want.size() / 4);
    CHECK(ok);
    const uint64_t got[13] = {n_pairs, r.yields, r.closable, r.none, r.over, r.recs.size(), r.columns, r.added, r.live, r.erased, r.empty, r.shorter, r.rowless};
    for (int i = 0; i < 13; ++i) { if (got[i] != c.k[i]) printf("case %s: counter %d is %llu, recorded %llu\n", c.name.c_str(), i, (unsigned long long)got[i], (unsigned long long)c.k[i]); CHECK(got[i] == c.k[i]); }
    for (size_t i = 0; i < r.recs.size(); ++i) {
        const Rec& x = r.recs[i];
        CHECK(x.cols >= 8 && x.cols <= MAX_COLS && r.starts[i + 1] - r.starts[i] == x.cols && (int64_t)x.cols == merged_cols(dims[2 * x.pair + 1].cols, x.offset));
        CHECK(x.rows <= dims[2 * x.pair].rows_kept + dims[2 * x.pair + 1].rows_kept && i >= r.pair_first[x.pair] && i < r.pair_first[x.pair + 1]);
        if (i && r.recs[i - 1].pair == x.pair) CHECK(r.recs[i - 1].offset < x.offset);
    }
    for (uint64_t p = 0; p < n_pairs; ++p) CHECK(r.pair_first[p + 1] - r.pair_first[p] == (words[p].closable ? words[p].kept : 0u));
    // ---- the device version's order of work gives the same, whatever the batches and the ranges
    for (uint64_t per : {(uint64_t)1, (uint64_t)37, (uint64_t)0})
        for (uint64_t cap : {(uint64_t)1, (uint64_t)300, (uint64_t)1 << 30}) {
            HostResult s;
            CHECK(sclosures_plan(I, c.K, per, 1ull << 30, cap, &s) == 0);
            CHECK(same(r, s));
            CHECK(s.skipped <= s.visits && s.visits >= s.live);
            if (cap == (1ull << 30)) CHECK(s.ranges == (r.closable ? 1u : 0u));
            if (per == 0 && cap == (1ull << 30)) CHECK(s.batches == s.ranges);
            if (per == 1) CHECK(s.batches == r.recs.size());
        }
    {   // batches sized by a small room
        HostResult s;
        CHECK(sclosures_plan(I, c.K, 0, 30000, 1ull << 30, &s) == 0 && same(r, s));
        if (r.live > 1000) CHECK(s.batches > 1);
    }
    CHECK(file_size(r.recs.size(), n_pairs, r.bases.size()) == 24 + 8 * (n_pairs + 1) + 8 * (r.recs.size() + 1) + 16 * r.recs.size() + ((r.bases.size() + 7) & ~7ull));
    // tables that do not hold together refuse the call in both forms
    if (r.closable) {
        const uint64_t p = r.recs[0].pair, j = so_starts[p];
        auto both = [&](const Input& J, int code) { HostResult a, b; CHECK(sclosures_literal(J, c.K, &a) == code && sclosures_plan(J, c.K, 0, 1ull << 30, 1ull << 30, &b) == code); };
        Input J = I;
        std::vector<dfk_scons::Dim> wide(dims); wide[2 * p].cols += 1;
        J.dims = wide.data(); both(J, -5);
        std::vector<uint64_t> fell(so_starts); fell[0] = 1;
        J = I; J.so_starts = fell.data(); both(J, -6);
        std::vector<dfk_soffsets::Rec> bad(so); bad[j].state = 2;
        J = I; J.recs = bad.data(); both(J, -7);
        bad = so; bad[j].offset = (int32_t)dims[2 * p].cols - 7;
        J = I; J.recs = bad.data(); both(J, so_starts[p + 1] - j > 1 ? -8 : -9);
        bad = so; bad[j].offset = -(int32_t)dims[2 * p + 1].cols + 7;
        J = I; J.recs = bad.data(); both(J, -9);
        std::vector<dfk_soffsets::PairWords> w2(words); w2[p].kept += 1;
        J = I; J.words = w2.data(); both(J, -11);
        w2 = words; w2[p].closable = 0;
        J = I; J.words = w2.data(); both(J, -11);
        for (uint64_t q = 0; q < n_pairs; ++q)
            if (!dfk_scons::yields(recs.data(), q)) {
                std::vector<uint64_t> st(so_starts); for (uint64_t i = q + 1; i <= n_pairs; ++i) st[i] += 1;      // a record for a pair that does not yield
                std::vector<dfk_soffsets::Rec> more(so); more.insert(more.begin() + so_starts[q], dfk_soffsets::Rec{0, 1, 20., 0, 0});
                J = I; J.so_starts = st.data(); J.recs = more.data(); both(J, -10);
                break;
            }
        std::vector<dfk_walks::Rec> wr(recs); wr[2 * p].M += 1;
        J = I; J.W.recs = wr.data(); both(J, -4);
    }
}

// two stacks of n1 and n2 columns, one row each, every cell defined and naming its own column
static dfk_cons::Grids marked(int cols)
{
    dfk_cons::Grids g;
    g.rows = 1; g.cols = cols;
    g.bases_.assign(1, std::vector<int8_t>(cols)); g.quals_.assign(1, std::vector<int8_t>(cols));
    for (int j = 0; j < cols; ++j) { g.bases_[0][j] = (int8_t)(j / 100); g.quals_[0][j] = (int8_t)(j % 100); }
    return g;
}

static uint32_t rnd(uint64_t* s) { *s = *s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(*s >> 33); }

static void pieces()
{
    using namespace dfk_sclosures;
    // MERGED_COLS and COLUMN_OF_SIDE against the literal Trim + Merge (resize, shift, append; cols_ = bases_[0].size( )), every allowed offset
    const int widths[][2] = {{8, 8}, {8, 30}, {30, 8}, {27, 60}, {60, 27}, {255, 257}, {400, 9}, {9, 400}, {400, 400}};
    for (const auto& w : widths) {
        const int n1 = w[0], n2 = w[1];
        const dfk_cons::Grids stacks[2] = {marked(n1), marked(n2)};
        CHECK(!offset_ok(n1, n2, -(n2 - 8) - 1) && !offset_ok(n1, n2, n1 - 7));
        for (int off = -(n2 - 8); off <= n1 - 8; ++off) {
            CHECK(offset_ok(n1, n2, off));
            const dfk_cons::Grids s = merged_literal(stacks, off);
            const int64_t C = merged_cols(n2, off);
            bool ok = s.rows == 2 && s.cols == (int)C && C >= 8 && C <= MAX_COLS && (int)s.bases_[0].size() == s.cols && (int)s.bases_[1].size() == s.cols;
            for (int64_t c = 0; ok && c < C; ++c)
                for (int side = 0; side < 2; ++side) {
                    const int64_t x = column_of_side(side, n1, n2, off, c);
                    if (x < 0) ok = s.bases_[side][c] == ' ' && s.quals_[side][c] == -1;
                    else ok = s.bases_[side][c] == (int8_t)(x / 100) && s.quals_[side][c] == (int8_t)(x % 100) && x < (side ? n2 : n1);
                }
            // the stacks share 8 columns at least
            int shared = 0;
            for (int64_t c = 0; c < C; ++c) shared += column_of_side(0, n1, n2, off, c) >= 0 && column_of_side(1, n1, n2, off, c) >= 0;
            if (!ok || shared < 8) printf("widths %d %d offset %d: the merged stack is not what the column maps say\n", n1, n2, off);
            CHECK(ok && shared >= 8);
            CHECK(edge_trimmed(0, n1, n2, off) == (n1 > off + n2) && edge_trimmed(1, n1, n2, off) == (off < 0));
        }
    }
    CHECK(TILES == 4 && MAX_COLS == 792 && merged_cols(400, 392) == 792 && merged_cols(8, 0) == 8);
    // Trim erases the rows without a defined cell in the kept columns and keeps the order of the others
    {
        dfk_cons::Grids g;
        g.rows = 3; g.cols = 6;
        g.bases_ = {{0, 1, ' ', ' ', ' ', ' '}, {' ', ' ', ' ', 2, 3, ' '}, {' ', ' ', 1, 1, ' ', ' '}};
        g.quals_ = {{5, 5, -1, -1, -1, -1}, {-1, -1, -1, -128, 7, -1}, {-1, -1, 9, -66, -1, -1}};
        dfk_cons::Grids t(g);
        trim_literal(&t, 3, 6);
        CHECK(t.rows == 1 && t.cols == 3 && t.bases_[0] == (std::vector<int8_t>{2, 3, ' '}) && t.quals_[0] == (std::vector<int8_t>{-128, 7, -1}));
        t = g; trim_literal(&t, 2, 4);
        CHECK(t.rows == 1 && t.bases_[0] == (std::vector<int8_t>{1, 1}));     // the middle row's only cell there is undefined
        t = g; trim_literal(&t, 0, 6);
        CHECK(t.rows == 3);
    }
    // TILE_SPAN and ROW_MEETS against the cells one by one
    uint64_t seed = 71;
    for (int i = 0; i < 4000; ++i) {
        const int64_t M0 = 8 + rnd(&seed) % 500, M1 = 8 + rnd(&seed) % 500, w00 = dfk_scons::window_start(M0), w01 = dfk_scons::window_start(M1), n1 = M0 - w00, n2 = M1 - w01;
        const int64_t off = -(n2 - 8) + (int64_t)(rnd(&seed) % (uint32_t)(n1 + n2 - 15)), C = merged_cols(n2, off);
        CHECK(offset_ok(n1, n2, off));
        const int side = (int)(rnd(&seed) & 1);
        const int64_t w0 = side ? w01 : w00, cols = side ? n2 : n1;
        const int32_t start = (int32_t)(rnd(&seed) % 600) - 80; const uint32_t len = 1 + rnd(&seed) % 160;
        for (int64_t c0 = 0; c0 < C; c0 += GROUP) {
            const int64_t c1 = std::min<int64_t>(C, c0 + GROUP);
            int64_t lo = 0, hi = 0;
            const bool spans = tile_span(side, n1, n2, off, w0, side == 1, c0, c1, &lo, &hi);
            bool shows = false, cell = false;
            for (int64_t c = c0; c < c1; ++c) {
                const int64_t x = column_of_side(side, n1, n2, off, c);
                if (x < 0) continue;
                shows = true;
                const int64_t sc = dfk_scons::stack_column(w0, cols, side == 1, x);
                CHECK(!spans || (sc >= lo && sc <= hi));
                cell = cell || dfk_scons::cell_index(start, len, sc) >= 0;
            }
            CHECK(spans == shows && cell == (spans && row_meets(start, len, lo, hi)));
        }
    }
    // the sums cross the stack boundary in row order
    {
        double a = 0., b = 0.;
        a += 20.; a += dfk_cons::quality_value(0); a += dfk_cons::quality_value(0);
        b += dfk_cons::quality_value(1); b += 10.; b += 10.;
        const double sums[4] = {a, b, 0., 0.}, tie[4] = {20. + (.1 + .1), .2 + (10. + 10.), 0., 0.}, none[4] = {0., 0., 0., 0.};
        CHECK(a == 20.200000000000003 && b == 20.2 && dfk_closures::last_max(sums) == 0 && dfk_closures::last_max(tie) == 1 && dfk_closures::last_max(none) == 3);
    }
    CHECK(strlen(MAGIC) == 8 && pair_first_at() == 24 && closures_grid(0, 256) == 1 && closures_grid(3, 256) == 12 && rows_grid(0, 4) == 1);
}

int main(int argc, char** argv)
{
    if (argc != 2) { printf("usage: test_sclosures <cases file>\n"); return 2; }
    pieces();
    std::ifstream in(argv[1]);
    if (!in) { printf("cannot read %s\n", argv[1]); return 2; }
    std::string line;
    int n_cases = 0;
    while (std::getline(in, line)) {
        if (line.rfind("case ", 0) != 0) { printf("unexpected line: %.60s\n", line.c_str()); return 2; }
        Case c;
        long long N = 0, np = 0;
        { std::istringstream h(line.substr(5)); h >> c.name >> N >> np >> c.K; }
        std::string l[18];
        for (auto& s : l) if (!std::getline(in, s)) { printf("case %s is cut short\n", c.name.c_str()); return 2; }
        c.starts = row<uint64_t>(l[0]);
        const std::vector<int64_t> rw = row<int64_t>(l[1]), lw = row<int64_t>(l[2]);
        for (size_t i = 0; i + 7 < rw.size(); i += 8)
            c.recs.push_back(dfk_walks::Rec{(uint32_t)rw[i], (uint32_t)rw[i + 1], (uint32_t)rw[i + 2], (uint32_t)rw[i + 3], (int32_t)(uint32_t)rw[i + 4], (uint32_t)rw[i + 5], (int32_t)(uint32_t)rw[i + 6], (int32_t)(uint32_t)rw[i + 7]});
        for (size_t i = 0; i + 2 < lw.size(); i += 3) c.locs.push_back(dfk_walks::Loc{lw[i], (int32_t)lw[i + 1], (uint32_t)lw[i + 2]});
        c.read_len = row<uint32_t>(l[3]); c.read_packed = hexrow(l[4]); c.pq_off = row<uint64_t>(l[5]); c.pq = hexrow(l[6]); c.dims = row<int64_t>(l[7]);
        // (l[8] .. l[11]: the stack consensus and its counters)
        c.so_counts = row<uint64_t>(l[12]); c.words = row<uint32_t>(l[13]);
        if (l[14] != "-") {
            std::istringstream rs(l[14]);
            long long o, n, st; std::string hex;
            while (rs >> o >> n >> hex >> st) {
                const std::vector<uint8_t> b = hexrow(hex);
                dfk_soffsets::Rec r{(int32_t)o, (uint32_t)n, 0., (uint32_t)st, 0};
                if (b.size() != 8) { printf("case %s: a record's bits are not 8 bytes\n", c.name.c_str()); return 2; }
                memcpy(&r.best_bits, b.data(), 8);
                c.so.push_back(r);
            }
        }
        c.want = row<int64_t>(l[15]);
        if (l[16] != "-") for (char ch : l[16]) c.bases.push_back((uint8_t)(ch - '0'));
        c.k = row<uint64_t>(l[17]);
        c.read_off.assign(c.read_len.size() + 1, 0);
        for (size_t i = 0; i < c.read_len.size(); ++i) c.read_off[i + 1] = c.read_off[i] + ((uint64_t)c.read_len[i] + 3) / 4;
        if (c.k.size() != 13 || c.read_len.size() != (size_t)N || c.recs.size() != 2 * (size_t)np || rw.size() != 16 * (size_t)np || c.starts.size() != 2 * (size_t)np + 1 || lw.size() != 3 * c.starts.back() ||
            c.read_packed.size() != c.read_off.back() || c.pq_off.size() != (size_t)N + 1 || c.pq.size() != c.pq_off.back() || c.dims.size() != 8 * (size_t)np || c.words.size() != 4 * (size_t)np ||
            c.so_counts.size() != (size_t)np || c.want.size() % 4 != 0) {
            printf("case %s is malformed\n", c.name.c_str()); return 2;
        }
        run_case(c);
        ++n_cases;
    }
    if (g_failed) { printf("%d check(s) failed\n", g_failed); return 1; }
    printf("%d recorded cases agree\n", n_cases);
    return 0;
}
