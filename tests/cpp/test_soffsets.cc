// tests/cpp/test_soffsets.cc -- superplus_amd/csrc/dfk_soffsets.h on the host: the literal per-pair transcription (both stacks
// materialised as grids, a std::set for sees, a vector of results, ReverseSort and the filter loop as written) against the cases
// recorded from tests/soffsets_oracle.py (tests/cpp/soffsets_cases.txt, and fixtures written out in the same form); the device version's
// order of work (soffsets_plan: ranges and batches of whole pairs, a row's cells and defined bits as masks, the bitmap of offsets seen,
// prefix sums, the maximum per offset on u64 and kept( best, score )) against the literal one under rows_per_batch 1, 37 and 0 and
// several row caps; the shared pieces held to the loops as written on random inputs: acceptable, minp over masked windows, kept against
// the sort-and-scan filter.  Its own main; built plain and under -fsanitize=address,undefined by tests/test_soffsets_cpu.py.
//   test_soffsets <cases file>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include "dfk_soffsets.h"

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
    std::vector<uint32_t> words;                    // the expected result: 4 a pair,
    std::vector<dfk_soffsets::Rec> want;            // the records,
    std::vector<uint64_t> k;                        // the counters: rows kmers acceptable hits seen disallowed lookups results
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

static bool same(const dfk_soffsets::HostResult& a, const dfk_soffsets::HostResult& b)
{
    if (a.starts != b.starts || a.words.size() != b.words.size() || a.recs.size() != b.recs.size()) return false;
    if (!a.words.empty() && memcmp(a.words.data(), b.words.data(), a.words.size() * sizeof(dfk_soffsets::PairWords)) != 0) return false;
    if (!a.recs.empty() && memcmp(a.recs.data(), b.recs.data(), a.recs.size() * sizeof(dfk_soffsets::Rec)) != 0) return false;      // (best_bits as its bytes)
    return a.yielding == b.yielding && a.rows == b.rows && memcmp(a.n, b.n, sizeof a.n) == 0;
}

static void run_case(const Case& c)
{
    using namespace dfk_soffsets;
    std::vector<uint8_t> rp(c.read_packed), pq(c.pq);                          // (exactly sized copies: the last read ends at the allocation's end)
    rp.shrink_to_fit(); pq.shrink_to_fit();
    auto room = [](auto v) { if (v.empty()) v.emplace_back(); return v; };
    const std::vector<dfk_walks::Rec> recs = room(c.recs);
    const std::vector<dfk_walks::Loc> locs = room(c.locs);
    const std::vector<uint32_t> read_len = room(c.read_len);
    const uint64_t n_pairs = c.recs.size() / 2;
    std::vector<dfk_scons::Dim> dims(2 * n_pairs + 1);
    std::vector<uint64_t> cons_starts(2 * n_pairs + 1, 0), cfirst(n_pairs + 1, 0);
    for (uint64_t q = 0; q < 2 * n_pairs; ++q) { dims[q] = dfk_scons::Dim{(uint32_t)c.dims[4 * q], (uint32_t)c.dims[4 * q + 1], (int32_t)(uint32_t)c.dims[4 * q + 2], (uint32_t)c.dims[4 * q + 3]}; cons_starts[q + 1] = cons_starts[q] + dims[q].cols; }
    for (uint64_t p = 0; p < n_pairs; ++p) cfirst[p + 1] = cfirst[p] + (dfk_scons::yields(recs.data(), p) ? dims[2 * p].cols + dims[2 * p + 1].cols : 0);
    CHECK(cons_starts.back() == c.con.size() && cfirst.back() == c.counts.size());
    std::vector<uint8_t> con(c.con), conq(c.conq); std::vector<uint16_t> counts(c.counts);
    con.shrink_to_fit(); counts.shrink_to_fit();
    con.reserve(con.size() + 1); conq.reserve(conq.size() + 1); counts.reserve(counts.size() + 1);      // (data() of an empty vector may be null)
    const Input I{dfk_scons::Input{n_pairs, c.starts.data(), recs.data(), locs.data(), c.read_len.size(), rp.data(), c.read_off.data(), read_len.data(), pq.data(), c.pq_off.data()},
                  cons_starts.data(), dims.data(), con.data(), conq.data(), cfirst.data(), counts.data()};
    HostResult r;
    const int rc = soffsets_literal(I, &r);
    CHECK(rc == 0);
    if (rc) return;
    // ---- the literal transcription against the Python restatement
    bool ok = 4 * r.words.size() == c.words.size() && r.recs.size() == c.want.size() && r.starts.size() == n_pairs + 1;
    if (ok && !r.words.empty()) ok = memcmp(r.words.data(), c.words.data(), 16 * r.words.size()) == 0;
    if (ok && !r.recs.empty()) ok = memcmp(r.recs.data(), c.want.data(), sizeof(Rec) * r.recs.size()) == 0;
    if (!ok) printf("case %s: the words or the records differ from the recorded ones (%zu records, %zu recorded)\n", c.name.c_str(), r.recs.size(), c.want.size());
    CHECK(ok);
    const uint64_t got[8] = {r.rows, r.n[C_KMERS], r.n[C_ACCEPTABLE], r.n[C_HITS], r.n[C_SEEN], r.n[C_DISALLOWED], r.n[C_LOOKUPS], r.n[C_RESULTS]};
    for (int i = 0; i < 8; ++i) { if (got[i] != c.k[i]) printf("case %s: counter %d is %llu, recorded %llu\n", c.name.c_str(), i, (unsigned long long)got[i], (unsigned long long)c.k[i]); CHECK(got[i] == c.k[i]); }
    for (uint64_t p = 0; p < n_pairs; ++p) {
        const PairWords& w = r.words[p];
        CHECK(r.starts[p + 1] >= r.starts[p] && w.results <= w.seen && w.kept <= r.starts[p + 1] - r.starts[p] && w.closable == (closable(w.kept) ? 1u : 0u));
        if (!dfk_scons::yields(recs.data(), p)) CHECK(r.starts[p + 1] == r.starts[p] && w.seen == 0);
        for (uint64_t i = r.starts[p]; i < r.starts[p + 1]; ++i) CHECK(r.recs[i].best_bits >= MIN_BITS && r.recs[i].results > 0 && (i == r.starts[p] || r.recs[i].offset > r.recs[i - 1].offset));
        if (r.starts[p + 1] > r.starts[p]) CHECK(w.kept >= 1);                                   // the best offset is kept
    }
    // ---- the device version's order of work gives the same, whatever the batches and the ranges
    for (uint64_t per : {(uint64_t)1, (uint64_t)37, (uint64_t)0})
        for (uint64_t cap : {(uint64_t)1, (uint64_t)300, (uint64_t)1 << 30}) {
            HostResult s;
            CHECK(soffsets_plan(I, per, 1ull << 30, cap, &s) == 0);
            CHECK(same(r, s));
            if (cap == (1ull << 30)) CHECK(s.ranges == (n_pairs ? 1u : 0u));
            if (per == 0 && cap == (1ull << 30)) CHECK(s.batches == s.ranges);
            if (per == 1) CHECK(s.batches >= r.yielding && s.batches <= n_pairs);
        }
    {   // batches sized by a small room
        HostResult s;
        CHECK(soffsets_plan(I, 0, 30000, 1ull << 30, &s) == 0 && same(r, s));
        if (r.rows > 400) CHECK(s.batches > 1);
    }
    CHECK(file_size(n_pairs, r.recs.size()) == 16 + 8 * (n_pairs + 1) + 16 * n_pairs + 24 * r.recs.size() && file_size(n_pairs, r.recs.size()) % 8 == 0);
    // tables that do not hold together refuse the call in both forms
    if (r.yielding) {
        HostResult x, y;
        uint64_t q = 0;
        while (!dfk_scons::yields(recs.data(), q / 2)) ++q;
        Input J = I;
        std::vector<uint64_t> fell(cons_starts); fell[0] = 1;
        J.cons_starts = fell.data();
        CHECK(soffsets_literal(J, &x) == -5 && soffsets_plan(J, 0, 1ull << 30, 1ull << 30, &y) == -5);
        std::vector<dfk_scons::Dim> wide(dims); wide[q].cols += 1;
        J = I; J.dims = wide.data();
        CHECK(soffsets_literal(J, &x) == -6 && soffsets_plan(J, 0, 1ull << 30, 1ull << 30, &y) == -6);
        std::vector<uint8_t> base4(con); base4[cons_starts[q]] = 4;
        J = I; J.con = base4.data();
        CHECK(soffsets_literal(J, &x) == -7 && soffsets_plan(J, 0, 1ull << 30, 1ull << 30, &y) == -7);
        std::vector<uint64_t> shortc(cfirst); for (uint64_t p = q / 2 + 1; p <= n_pairs; ++p) shortc[p] -= 1;
        J = I; J.cfirst = shortc.data();
        CHECK(soffsets_literal(J, &x) == -8 && soffsets_plan(J, 0, 1ull << 30, 1ull << 30, &y) == -8);
        std::vector<dfk_walks::Rec> bad(recs); bad[q].M += 1;
        J = I; J.W.recs = bad.data();
        CHECK(soffsets_literal(J, &x) == -4 && soffsets_plan(J, 0, 1ull << 30, 1ull << 30, &y) == -4);
    }
}

static uint32_t rnd(uint64_t* s) { *s = *s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(*s >> 33); }

static void pieces()
{
    using namespace dfk_soffsets;
    uint64_t seed = 29;
    const double* T = dfk_offsets::table().data();
    // ACCEPTABLE against :503-515 as written, on every 8-mer
    for (uint32_t km = 0; km < 65536; ++km) {
        uint8_t bb[MM];
        for (int m = 0; m < MM; ++m) bb[m] = (uint8_t)((km >> (2 * m)) & 3u);
        CHECK(dfk_offsets::pack8(bb) == km);
        bool diff = false, want = true;
        for (int m = 1; m < MM / 2; m++) if (bb[m] != bb[m - 1]) diff = true;
        if (!diff) want = false;
        diff = false;
        for (int m = 1; m < MM / 2; m++) if (bb[MM / 2 + m] != bb[MM / 2 + m - 1]) diff = true;
        if (!diff) want = false;
        bool present[4] = {false, false, false, false};
        for (int m = 0; m < MM; m++) present[bb[m]] = true;
        if (present[0] + present[1] + present[2] + present[3] < 3) want = false;
        CHECK(acceptable(km) == want);
    }
    CHECK(!acceptable(NO_KMER));
    {
        const uint8_t acc3[8] = {0, 1, 2, 0, 1, 2, 0, 1}, flat1[8] = {0, 0, 0, 0, 1, 2, 3, 1}, flat2[8] = {1, 2, 3, 1, 0, 0, 0, 0}, two[8] = {0, 1, 0, 1, 0, 1, 0, 1};
        CHECK(acceptable(dfk_offsets::pack8(acc3)) && !acceptable(dfk_offsets::pack8(flat1)) && !acceptable(dfk_offsets::pack8(flat2)) && !acceptable(dfk_offsets::pack8(two)));
        CHECK(con_kmer(acc3, 8, 0) == dfk_offsets::pack8(acc3) && con_kmer(acc3, 8, 1) == NO_KMER && con_kmer(flat1, 8, 0) == NO_KMER);
    }
    // the row 8-mer and bits8 against the cells one by one
    for (int i = 0; i < 300; ++i) {
        unsigned long long def[MASK_WORDS] = {};
        std::vector<uint8_t> cells((size_t)MAX_WIDTH + MM, BLANK);
        const int cols = 8 + (int)(rnd(&seed) % 393);
        for (int c = 0; c < cols; ++c) { cells[c] = (uint8_t)(rnd(&seed) & 3); if (rnd(&seed) % 16) def[c >> 6] |= 1ull << (c & 63); }
        for (int l = 0; l + MM <= cols; ++l) {
            bool all = true;
            for (int m = 0; m < MM; ++m) all = all && bit_at(def, l + m);
            uint16_t km = 0;
            CHECK(row_kmer(cells.data(), def, l, &km) == all);
            if (all) CHECK(km == dfk_offsets::pack8(cells.data() + l));
        }
    }
    // offset_of, overlap_of against IntervalOverlap
    CHECK(offset_of(0, 5, 3) == 2 && offset_of(1, 5, 3) == -2 && offx_of(0, 7) == 7 && offx_of(1, 7) == -7 && pos1_of(-4) == 0 && pos2_of(-4) == 4 && pos1_of(4) == 4 && pos2_of(4) == 0);
    for (int i = 0; i < 20000; ++i) {
        const int c1 = 1 + (int)(rnd(&seed) % 400), c2 = 1 + (int)(rnd(&seed) % 400), offx = (int)(rnd(&seed) % 900) - 450;
        int n = 0;
        for (int x = 0; x < c1; ++x) if (x >= offx && x < offx + c2) ++n;
        CHECK(overlap_of(offx, c1, c2) == n);
    }
    CHECK(mismatch(3, BLANK) && mismatch(0, 1) && !mismatch(2, 2));
    // MINP over masked windows against the loops of :589-595
    for (int i = 0; i < 400; ++i) {
        const int overlap = (int)(rnd(&seed) % 401);
        std::vector<int> err_sum(overlap + 1, 0);
        std::vector<char> def(overlap + 1, 0);
        unsigned long long mask[MASK_WORDS] = {};
        const uint32_t pm = 1 + rnd(&seed) % 8, pd = 2 + rnd(&seed) % 30;
        const int lo = (int)(rnd(&seed) % (overlap + 1)), hi = lo + (int)(rnd(&seed) % 160);      // a row's span inside the overlap, some cells undefined
        for (int v = 0; v < overlap; ++v) {
            err_sum[v + 1] = err_sum[v] + ((i % 5 == 0) ? 1 : (rnd(&seed) % pm == 0));
            def[v] = v >= lo && v < hi && rnd(&seed) % pd != 0;
            if (def[v]) mask[v >> 6] |= 1ull << (v & 63);
        }
        double minp = 0;
        uint64_t looked = 0;
        for (int start = 0; start < overlap; start++)
            for (int n = WID; n <= overlap - start; n++) {
                if (!def[start] || !def[start + n - 1]) continue;
                const int k = err_sum[start + n] - err_sum[start];
                minp = std::min(minp, T[n * dfk_offsets::T_DIM + k]);
                ++looked;
            }
        double got = 0.;
        uint32_t n_looked = 0;
        for (int start = overlap - 1; start >= 0; --start) got = minp_of_start(err_sum, mask, overlap, start, T, got, &n_looked);
        CHECK(got == minp && n_looked == looked);
        CHECK(bits_of(got) == -minp * 10.0 / 6.0);
    }
    CHECK(T[20 * dfk_offsets::T_DIM + 20] == 0.0 && T[400 * dfk_offsets::T_DIM + 400] == 0.0 && passes(bits_of(T[20 * dfk_offsets::T_DIM])) && !passes(bits_of(T[20 * dfk_offsets::T_DIM + 1])) && !passes(bits_of(0.)));
    // KEPT and the maximum per offset against ReverseSort and the filter loop of :634-645
    for (int i = 0; i < 3000; ++i) {
        std::vector<std::pair<double, int>> results(rnd(&seed) % 40);
        for (auto& x : results) { x.first = 20.0 + (double)(rnd(&seed) % 4000) / 100.0; x.second = (int)(rnd(&seed) % 9) - 4; if (rnd(&seed) % 4 == 0) x.first = 60.0 - 20.0 * (rnd(&seed) & 1) + (rnd(&seed) % 3 ? 0. : std::nextafter(0.07, 1.) - 0.07); }
        std::vector<std::pair<double, int>> sorted(results);
        std::sort(sorted.begin(), sorted.end(), std::greater<std::pair<double, int>>());
        std::vector<int> offsets;
        for (size_t j = 0; j < sorted.size(); j++) {
            const double score = sorted[j].first;
            const int offset = sorted[j].second;
            if (offsets.empty()) offsets.push_back(offset);
            else if (std::find(offsets.begin(), offsets.end(), offset) != offsets.end()) continue;
            else if (sorted[0].first - score <= MAX_DIFF) offsets.push_back(offset);
        }
        std::sort(offsets.begin(), offsets.end());
        uint64_t best = 0, mx[9] = {};
        for (const auto& x : results) { uint64_t u; memcpy(&u, &x.first, 8); mx[x.second + 4] = std::max(mx[x.second + 4], u); best = std::max(best, u); }
        double bestd; memcpy(&bestd, &best, 8);
        std::vector<int> got;
        for (int o = 0; o < 9; ++o) { double sc; memcpy(&sc, &mx[o], 8); if (mx[o] && kept(bestd, sc)) got.push_back(o - 4); }
        CHECK(got == offsets);
    }
    CHECK(kept(60., 40.) && !kept(60., std::nextafter(40., 0.)) && closable(1) && closable(3) && !closable(0) && !closable(4));
    // the plan's batches: whole pairs, one at least
    {
        const uint64_t live[5] = {0, 5, 5, 9, 40}, cost[5] = {0, 100, 110, 300, 1000};
        CHECK(next_batch(live, cost, 4, 0, 0, 1) == 1 && next_batch(live, cost, 4, 0, 0, 9) == 3 && next_batch(live, cost, 4, 3, 0, 1) == 4 && next_batch(live, cost, 4, 0, 300, 0) == 3 && next_batch(live, cost, 4, 0, 1, 0) == 1 &&
              next_batch(live, cost, 4, 0, 1ull << 30, 0) == 4);
    }
    CHECK(strlen(MAGIC) == 8 && words_at(0) == 24 && recs_at(2) == 16 + 24 + 32 && file_size(2, 3) == 16 + 24 + 32 + 72 && sizeof(Rec) == 24);
}

int main(int argc, char** argv)
{
    if (argc != 2) { printf("usage: test_soffsets <cases file>\n"); return 2; }
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
        std::string l[15];
        for (auto& s : l) if (!std::getline(in, s)) { printf("case %s is cut short\n", c.name.c_str()); return 2; }
        c.starts = row<uint64_t>(l[0]);
        const std::vector<int64_t> rw = row<int64_t>(l[1]), lw = row<int64_t>(l[2]);
        for (size_t i = 0; i + 7 < rw.size(); i += 8)
            c.recs.push_back(dfk_walks::Rec{(uint32_t)rw[i], (uint32_t)rw[i + 1], (uint32_t)rw[i + 2], (uint32_t)rw[i + 3], (int32_t)(uint32_t)rw[i + 4], (uint32_t)rw[i + 5], (int32_t)(uint32_t)rw[i + 6], (int32_t)(uint32_t)rw[i + 7]});
        for (size_t i = 0; i + 2 < lw.size(); i += 3) c.locs.push_back(dfk_walks::Loc{lw[i], (int32_t)lw[i + 1], (uint32_t)lw[i + 2]});
        c.read_len = row<uint32_t>(l[3]); c.read_packed = hexrow(l[4]); c.pq_off = row<uint64_t>(l[5]); c.pq = hexrow(l[6]); c.dims = row<int64_t>(l[7]);
        if (l[8] != "-") for (char ch : l[8]) c.con.push_back((uint8_t)(ch - '0'));
        c.conq = row<uint8_t>(l[9]); c.counts = row<uint16_t>(l[10]);
        // (l[11]: the consensus' own counters)
        c.words = row<uint32_t>(l[12]);
        if (l[13] != "-") {
            std::istringstream rs(l[13]);
            long long o, n, st; std::string hex;
            while (rs >> o >> n >> hex >> st) {
                const std::vector<uint8_t> b = hexrow(hex);
                dfk_soffsets::Rec r{(int32_t)o, (uint32_t)n, 0., (uint32_t)st, 0};
                if (b.size() != 8) { printf("case %s: a record's bits are not 8 bytes\n", c.name.c_str()); return 2; }
                memcpy(&r.best_bits, b.data(), 8);
                c.want.push_back(r);
            }
        }
        c.k = row<uint64_t>(l[14]);
        c.read_off.assign(c.read_len.size() + 1, 0);
        for (size_t i = 0; i < c.read_len.size(); ++i) c.read_off[i + 1] = c.read_off[i] + ((uint64_t)c.read_len[i] + 3) / 4;
        if (c.k.size() != 8 || c.read_len.size() != (size_t)N || c.recs.size() != 2 * (size_t)np || rw.size() != 16 * (size_t)np || c.starts.size() != 2 * (size_t)np + 1 || lw.size() != 3 * c.starts.back() ||
            c.read_packed.size() != c.read_off.back() || c.pq_off.size() != (size_t)N + 1 || c.pq.size() != c.pq_off.back() || c.dims.size() != 8 * (size_t)np || c.con.size() != c.conq.size() || c.words.size() != 4 * (size_t)np) {
            printf("case %s is malformed\n", c.name.c_str()); return 2;
        }
        run_case(c);
        ++n_cases;
    }
    if (g_failed) { printf("%d check(s) failed\n", g_failed); return 1; }
    printf("%d recorded cases agree\n", n_cases);
    return 0;
}
