// tests/cpp/test_scons.cc -- superplus_amd/csrc/dfk_scons.h on the host: the literal per-pair transcription (both stacks materialised,
// Trim, Reverse, Consensus1 with std::sort and std::round, MIN_FLAT, the conflicts) against the cases recorded from
// tests/scons_oracle.py (tests/cpp/scons_cases.txt, and fixtures written out in the same form), the device version's order of work
// (scons_plan: ranges of pairs, batches of stacks, the reads of a batch each once, a lane a column over the live rows, the flat pass,
// the conflicts) against the literal one under stacks_per_batch 1, 37 and 0 and several row caps; the shared pieces: the rounding
// against std::round, top_two against a sort, the flat test, the conflict count; rows_kept against the rows whose span meets the
// window.  Its own main; built plain and under -fsanitize=address,undefined by tests/test_scons_cpu.py.
//   test_scons <cases file>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include "dfk_scons.h"

static int g_failed = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++g_failed; } } while (0)

struct Case {
    std::string name;
    std::vector<uint64_t> starts, read_off, pq_off;
    std::vector<dfk_walks::Rec> recs;
    std::vector<dfk_walks::Loc> locs;
    std::vector<uint32_t> read_len;
    std::vector<uint8_t> read_packed, pq, con, conq;
    std::vector<int64_t> dims;
    std::vector<uint16_t> counts;
    uint64_t k[6] = {};
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

static bool same(const dfk_scons::HostResult& a, const dfk_scons::HostResult& b)
{
    if (a.starts != b.starts || a.cfirst != b.cfirst || a.con != b.con || a.conq != b.conq || a.counts != b.counts || a.dims.size() != b.dims.size()) return false;
    if (!a.dims.empty() && memcmp(a.dims.data(), b.dims.data(), a.dims.size() * sizeof(dfk_scons::Dim)) != 0) return false;
    return a.yielding == b.yielding && a.rows == b.rows && a.rows_kept == b.rows_kept && a.trimmed == b.trimmed && a.cells == b.cells && a.capped == b.capped && a.recount == b.recount && a.flat == b.flat &&
           a.allowed == b.allowed && a.disallowed == b.disallowed;
}

static void run_case(const Case& c)
{
    using namespace dfk_scons;
    std::vector<uint8_t> rp(c.read_packed), pq(c.pq);                          // (exactly sized copies: the last read ends at the allocation's end)
    rp.shrink_to_fit(); pq.shrink_to_fit();
    auto room = [](auto v) { if (v.empty()) v.emplace_back(); return v; };
    const std::vector<dfk_walks::Rec> recs = room(c.recs);
    const std::vector<dfk_walks::Loc> locs = room(c.locs);
    const std::vector<uint32_t> read_len = room(c.read_len);
    const uint64_t n_pairs = c.recs.size() / 2;
    const Input I{n_pairs, c.starts.data(), recs.data(), locs.data(), c.read_len.size(), rp.data(), c.read_off.data(), read_len.data(), pq.data(), c.pq_off.data()};
    HostResult r;
    const int rc = scons_literal(I, &r);
    CHECK(rc == 0);
    if (rc) return;
    // ---- the literal transcription against the Python restatement
    bool ok = 4 * r.dims.size() == c.dims.size() && r.con == c.con && r.conq == c.conq && r.counts == c.counts;
    for (size_t i = 0; ok && i < r.dims.size(); ++i) {
        const Dim& d = r.dims[i]; const int64_t* w = &c.dims[4 * i];
        ok = d.rows == (uint32_t)w[0] && d.rows_kept == (uint32_t)w[1] && d.M == (int32_t)(uint32_t)w[2] && d.cols == (uint32_t)w[3];
    }
    if (!ok) printf("case %s: dims, con, conq or the conflict counts differ from the recorded ones\n", c.name.c_str());
    CHECK(ok);
    CHECK(r.cells == c.k[0] && r.capped == c.k[1] && r.recount == c.k[2] && r.flat == c.k[3] && r.allowed == c.k[4] && r.disallowed == c.k[5]);
    bool high = false;                                                         // a quality of 128 or more somewhere: an undefined cell inside a span
    {
        std::vector<uint8_t> q;
        for (size_t id = 0; id < c.read_len.size(); ++id) {
            q.assign((size_t)c.read_len[id] + 1, 0);
            CHECK(dfk_cons::decode_quals(pq.data(), c.pq_off[id], c.pq_off[id + 1], q.data(), c.read_len[id]));
            for (uint32_t j = 0; j < c.read_len[id]; ++j) high = high || q[j] >= 128;
        }
    }
    for (uint64_t pi = 0; pi < n_pairs; ++pi) {
        const uint64_t n1 = r.dims[2 * pi].cols, n2 = r.dims[2 * pi + 1].cols;
        CHECK(r.cfirst[pi + 1] - r.cfirst[pi] == (yields(recs.data(), pi) ? n1 + n2 : 0));
        for (uint64_t q = 2 * pi; q < 2 * pi + 2; ++q) {
            const Dim& d = r.dims[q];
            CHECK(r.starts[q + 1] - r.starts[q] == d.cols && d.cols == (uint32_t)(d.M - window_start(d.M)) && d.rows_kept <= d.rows);
            if (!yields(recs.data(), pi)) { CHECK(d.rows == 0 && d.cols == 0 && d.M == 0); continue; }
            CHECK(d.M == recs[q].M && d.M - (int32_t)d.cols == recs[q].trim && d.rows == recs[q].placed);
            // rows_kept == the rows whose span meets the window, where every cell inside a span is defined
            uint64_t meet = 0;
            for (uint64_t j = c.starts[q]; j < c.starts[q + 1]; ++j) meet += span_meets(locs[j].start, c.read_len[locs[j].id], window_start(d.M));
            if (!high) CHECK(d.rows_kept == (d.M > MAX_WIDTH ? meet : d.rows));
            if (yields(recs.data(), pi) && n1 + n2) CHECK(r.counts[r.cfirst[pi]] == 0);      // offset = -n2: no overlap
        }
    }
    // ---- the device version's order of work gives the same, whatever the batches and the ranges
    for (uint64_t per : {(uint64_t)1, (uint64_t)37, (uint64_t)0})
        for (uint64_t cap : {(uint64_t)1, (uint64_t)300, (uint64_t)1 << 30}) {
            HostResult s;
            CHECK(scons_plan(I, per, 1ull << 30, cap, &s) == 0);
            CHECK(same(r, s));
            if (cap == (1ull << 30)) CHECK(s.ranges == (n_pairs ? 1u : 0u));
            if (cap == 1) CHECK(s.ranges <= n_pairs && s.ranges >= r.yielding);             // (a pair without rows joins its neighbour's range)
            if (per == 0 && cap == (1ull << 30)) CHECK(s.batches == s.ranges);
            if (per == 1) CHECK(s.batches == 2 * n_pairs);
        }
    {   // batches sized by a small room
        HostResult s;
        CHECK(scons_plan(I, 0, 30000, 1ull << 30, &s) == 0 && same(r, s));
        if (r.rows > 400) CHECK(s.batches > 1);
    }
    CHECK(file_size(2 * n_pairs, r.con.size(), r.counts.size()) == (16 + 8 * (2 * n_pairs + 1) + 8 * (n_pairs + 1) + 32 * n_pairs + 2 * r.con.size() + 2 * r.counts.size() + 7) / 8 * 8);
    // streams that do not hold len values (every one ends at once) refuse the call in both forms; tables that do not hold together too
    if (r.rows) {
        const std::vector<uint8_t> none(pq.size(), 0);
        Input J = I; J.pq = none.data();
        HostResult x, y;
        CHECK(scons_literal(J, &x) == -3 && scons_plan(J, 0, 1ull << 30, 1ull << 30, &y) == -3);
        std::vector<dfk_walks::Rec> bad(recs);
        uint64_t q = 0;
        while (!(yields(recs.data(), q / 2))) ++q;
        bad[q].M += 1;
        J = I; J.recs = bad.data();
        CHECK(scons_literal(J, &x) == -4 && scons_plan(J, 0, 1ull << 30, 1ull << 30, &y) == -4);
        bad = recs; bad[q].placed += 1;
        J.recs = bad.data();
        CHECK(scons_literal(J, &x) == -1);
        std::vector<dfk_walks::Loc> far(locs);
        far[c.starts[q]].id = (int64_t)c.read_len.size();
        J = I; J.locs = far.data();
        CHECK(scons_literal(J, &x) == -2 && scons_plan(J, 0, 1ull << 30, 1ull << 30, &y) == -2);
    }
}

static uint32_t rnd(uint64_t* s) { *s = *s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(*s >> 33); }

static void pieces()
{
    using namespace dfk_scons;
    // THE ROUNDING: the shared form is std::round
    const double fixed[] = {0.49999999999999994, 0.5, 99.5, 100.5, 0.0, 1.5, 2.5, 9.499999999999998, 99.4, 99.49999999999999, 299.8, 2147483000.5, -0.5, -0.49999999999999994, -2.5};
    for (double x : fixed) CHECK(round_half_away(x) == std::round(x));
    CHECK(round_half_away(0.49999999999999994) == 0.0 && round_half_away(0.5) == 1.0 && round_half_away(99.5) == 100.0 && round_half_away(100.5) == 101.0 && std::floor(0.49999999999999994 + 0.5) == 1.0);
    uint64_t seed = 11;
    for (int i = 0; i < 200000; ++i) {
        const double whole = (double)(rnd(&seed) % (i % 3 ? 300u : 2000000000u)), part = i % 4 == 0 ? 0.5 : (double)rnd(&seed) / 2147483648.0;
        double x = whole + part;
        if (i % 7 == 0) x = std::nextafter(whole + 0.5, i % 2 ? 0.0 : 1e18);
        CHECK(round_half_away(x) == std::round(x));
    }
    // top_two against the reference's sort of ( sum, id ) pairs; con is dfk_closures::last_max
    for (int i = 0; i < 50000; ++i) {
        double s[4];
        for (auto& x : s) x = (double)(rnd(&seed) % (i % 2 ? 3u : 1000u)) * (i % 5 == 0 ? 0.1 : 1.0);
        std::pair<double, int> m[4];
        for (int b = 0; b < 4; ++b) m[b] = {s[b], b};
        std::sort(m, m + 4, std::greater<std::pair<double, int>>());
        const TopTwo t = top_two(s);
        CHECK((int)t.id0 == m[0].second && t.val0 == m[0].first && (int)t.id1 == m[1].second && t.val1 == m[1].first && t.id0 == dfk_closures::last_max(s));
    }
    const double none[4] = {0., 0., 0., 0.}, order_a[4] = {20. + .1 + .1, .2 + 10. + 10., 0., 0.};
    CHECK(top_two(none).id0 == 3 && top_two(none).id1 == 2 && top_two(order_a).id0 == 0 && order_a[0] > order_a[1]);
    // the cap and the recount
    const uint32_t two[4] = {0, 2, 1, 0}, one[4] = {0, 1, 2, 0};
    auto conq = [&](double a, double b, const uint32_t* bad) { const double s[4] = {a, b, 0., 0.}; return conq_of(top_two(s), bad); };
    CHECK(conq(100., .6000000000000001, two).conq == 99 && !conq(100., .6000000000000001, two).capped && conq(100., .5, two).conq == 100 && conq(100., .5, two).capped && conq(300., .1, two).conq == 100);
    CHECK(conq(240., 100., two).conq == 100 && !conq(240., 100., two).recount && conq(180., 100.1, two).conq == 0 && conq(180., 100.1, two).recount && conq(180., 103., one).conq == 77 && !conq(180., 103., one).recount);
    // the flat test against the run loop of :473-489
    for (int i = 0; i < 2000; ++i) {
        std::vector<uint8_t> con(1 + rnd(&seed) % 60), q(con.size(), 7);
        for (size_t j = 0; j < con.size(); ++j) con[j] = j && rnd(&seed) % 4 ? con[j - 1] : (uint8_t)(rnd(&seed) & 3);
        HostResult h;
        min_flat_literal(con, &q, &h);
        uint64_t n = 0;
        for (size_t j = 0; j < con.size(); ++j) { const bool f = flat_at(con.data(), (int64_t)con.size(), (int64_t)j); CHECK(f == (q[j] == 0)); n += f; }
        CHECK(n == h.flat);
    }
    // the conflict count against :550-557
    for (int i = 0; i < 300; ++i) {
        std::vector<uint8_t> c1(rnd(&seed) % 50), c2(1 + rnd(&seed) % 50), q1(c1.size()), q2(c2.size());
        for (auto& x : c1) x = (uint8_t)(rnd(&seed) & 3);
        for (auto& x : c2) x = (uint8_t)(rnd(&seed) & 3);
        for (auto& x : q1) x = rnd(&seed) % 3 ? 100 : 99;
        for (auto& x : q2) x = rnd(&seed) % 3 ? 100 : 0;
        for (int off = -(int)c2.size(); off < (int)c1.size(); ++off)
            CHECK((int)conflicts_at(c1.data(), q1.data(), (int64_t)c1.size(), c2.data(), q2.data(), (int64_t)c2.size(), off) == conflicts_literal(c1, q1, c2, q2, off));
    }
    CHECK(conflict(0, 100, 1, 100) && !conflict(0, 100, 0, 100) && !conflict(0, 99, 1, 100) && !conflict(0, 100, 1, 0));
    // the cell and the window
    CHECK(window_start(400) == 0 && window_start(401) == 1 && cell_index(-7, 100, 0) == 7 && cell_index(-7, 100, 92) == 99 && cell_index(-7, 100, 93) == -1 && cell_index(5, 10, 4) == -1);
    CHECK(span_meets(0, 60, 59) && !span_meets(0, 60, 60) && !span_meets(0, 0, 0) && stack_column(60, 400, false, 0) == 60 && stack_column(60, 400, true, 0) == 459 && row_rc(false) && !row_rc(true));
    CHECK(strlen(MAGIC) == 8 && cfirst_at(0) == 24 && dims_at(0) == 32 && file_size(0, 0, 0) == 32 && file_size(2, 3, 1) == (16 + 24 + 16 + 32 + 6 + 2 + 7) / 8 * 8 && TILES == 2);
    CHECK(row_cap(1ull << 40, 77) == 77 && row_cap(0, 0) == (1ull << 18) && cons_grid(0, 256) == 1 && cons_grid(3, 256) == 6 && pair_grid(1ull << 20, 256) == 8192);
}

int main(int argc, char** argv)
{
    if (argc != 2) { printf("usage: test_scons <cases file>\n"); return 2; }
    pieces();
    std::ifstream in(argv[1]);
    if (!in) { printf("cannot read %s\n", argv[1]); return 2; }
    std::string line;
    int n_cases = 0;
    while (std::getline(in, line)) {
        if (line.rfind("case ", 0) != 0) { printf("unexpected line: %.60s\n", line.c_str()); return 2; }
        Case c;
        long long N = 0, np = 0;
        { std::istringstream h(line.substr(5)); h >> c.name >> N >> np; }
        std::string l[12];
        for (auto& s : l) if (!std::getline(in, s)) { printf("case %s is cut short\n", c.name.c_str()); return 2; }
        c.starts = row<uint64_t>(l[0]);
        const std::vector<int64_t> rw = row<int64_t>(l[1]), lw = row<int64_t>(l[2]);
        for (size_t i = 0; i + 7 < rw.size(); i += 8)
            c.recs.push_back(dfk_walks::Rec{(uint32_t)rw[i], (uint32_t)rw[i + 1], (uint32_t)rw[i + 2], (uint32_t)rw[i + 3], (int32_t)(uint32_t)rw[i + 4], (uint32_t)rw[i + 5], (int32_t)(uint32_t)rw[i + 6], (int32_t)(uint32_t)rw[i + 7]});
        for (size_t i = 0; i + 2 < lw.size(); i += 3) c.locs.push_back(dfk_walks::Loc{lw[i], (int32_t)lw[i + 1], (uint32_t)lw[i + 2]});
        c.read_len = row<uint32_t>(l[3]); c.read_packed = hexrow(l[4]); c.pq_off = row<uint64_t>(l[5]); c.pq = hexrow(l[6]); c.dims = row<int64_t>(l[7]);
        if (l[8] != "-") for (char ch : l[8]) c.con.push_back((uint8_t)(ch - '0'));
        c.conq = row<uint8_t>(l[9]); c.counts = row<uint16_t>(l[10]);
        const std::vector<uint64_t> k = row<uint64_t>(l[11]);
        c.read_off.assign(c.read_len.size() + 1, 0);
        for (size_t i = 0; i < c.read_len.size(); ++i) c.read_off[i + 1] = c.read_off[i] + ((uint64_t)c.read_len[i] + 3) / 4;
        if (k.size() != 6 || c.read_len.size() != (size_t)N || c.recs.size() != 2 * (size_t)np || rw.size() != 16 * (size_t)np || c.starts.size() != 2 * (size_t)np + 1 || lw.size() != 3 * c.starts.back() ||
            c.read_packed.size() != c.read_off.back() || c.pq_off.size() != (size_t)N + 1 || c.pq.size() != c.pq_off.back() || c.dims.size() != 8 * (size_t)np || c.con.size() != c.conq.size()) {
            printf("case %s is malformed\n", c.name.c_str()); return 2;
        }
        for (int i = 0; i < 6; ++i) c.k[i] = k[i];
        run_case(c);
        ++n_cases;
    }
    if (g_failed) { printf("%d check(s) failed\n", g_failed); return 1; }
    printf("%d recorded cases agree\n", n_cases);
    return 0;
}
