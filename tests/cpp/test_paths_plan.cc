// tests/cpp/test_paths_plan.cc -- the plans of pathing, the paths index and the duplicate marks
// (superplus_amd/csrc/dfk_paths_plan.h) on a CPU: tables of what the host code of dfk_paths.inc and dfk_paths_shard.inc
// computed for fixed inputs before its arithmetic moved into the header (paths_plan_expected.h), the properties every plan
// must have over seeded random cases, and the batch planner replayed over a small case.  One "name: ok" line per group, exit
// status 1 if any failed.
//   g++ -O1 -std=c++17 -Wall -o test_paths_plan tests/cpp/test_paths_plan.cc && ./test_paths_plan
#include "../../superplus_amd/csrc/dfk_paths_plan.h"
#include "paths_plan_expected.h"
#include <cstdio>
#include <cstring>
#include <random>

using namespace dfk;

static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { if (++g_bad <= 5) printf("  line %d: %s\n", __LINE__, #x); } } while (0)
static int done(const char* name) { printf("%s: %s\n", name, g_bad ? "FAILED" : "ok"); const int b = g_bad; g_bad = 0; return b != 0; }
template <class T, size_t N> constexpr size_t len(const T (&)[N]) { return N; }
constexpr uint64_t FNV0 = 1469598103934665603ull, FNVP = 1099511628211ull;

static PathSwitches switches(uint32_t slots, uint64_t batch_reads) { PathSwitches sw; sw.slots = slots; sw.batch_reads = batch_reads; return sw; }

// ------------------------------------------------------------------ tables
static int test_bound_table()
{
    bool below_k = false, above_k = false, mult4 = false, not4 = false;
    for (size_t i = 0; i < len(X_BOUND); i += X_BOUND_COLS) {
        const uint64_t* r = X_BOUND + i;
        CHECK(path_batch_bound((uint32_t)r[1], (uint32_t)r[0]) == r[2]);
        below_k |= r[1] < r[0]; above_k |= r[1] > r[0]; mult4 |= r[1] % 4 == 0; not4 |= r[1] % 4 != 0;
    }
    CHECK(below_k && above_k && mult4 && not4 && len(X_BOUND) / X_BOUND_COLS > 100);
    for (size_t i = 0; i < len(X_BOUND_ALL); i += 2) {                    // every max_len the pathing accepts
        uint64_t h = FNV0;
        for (uint32_t l = 0; l <= 65535; ++l) { const uint64_t b = path_batch_bound(l, (uint32_t)X_BOUND_ALL[i]); CHECK(b >= 1 && b < (1ull << 32)); h ^= b; h *= FNVP; }
        CHECK(h == X_BOUND_ALL[i + 1]);
    }
    CHECK(len(X_BOUND_ALL) == 6);
    return done("the batch bound against the recorded table (max_len 0 .. 65535; K = 40, 48, 60)");
}

static int test_filter_table()
{
    size_t seen[3] = {0, 0, 0};
    for (size_t i = 0; i < len(X_FILTER); i += X_FILTER_COLS) {
        const uint64_t* r = X_FILTER + i;
        const PathFilterPlan p = plan_path_filter(r[0], r[1], r[2], r[3], r[4] != 0);
        CHECK((uint64_t)p.use == r[5] && p.words == r[6]);
        ++seen[r[5]];
    }
    CHECK(seen[0] > 50 && seen[1] > 50 && seen[2] > 50);
    CHECK((int)PathFilter::None == 0 && (int)PathFilter::Reuse == 1 && (int)PathFilter::Build == 2);
    return done("the k-mer filter's decision against the recorded table (both sides of its threshold)");
}

static int test_batch_table()
{
    bool squeezed = false, roomy = false, by_bound = false, by_switch = false, by_reads = false, all = false;
    for (size_t i = 0; i < len(X_BATCH); i += X_BATCH_COLS) {
        const uint64_t* r = X_BATCH + i;
        PathBatcher b(r[0], r[3], switches(r[2] == 0xFFFFFFFFull ? 12 : (uint32_t)r[2], r[4]));
        b.all_slots = r[2] == 0xFFFFFFFFull;
        b.begin(r[1]);
        CHECK(b.room == r[5] && b.nb == r[6] && b.r0 == 0 && b.file_base == 24 && b.cap == (uint32_t)r[2]);
        squeezed |= r[5] == r[1] / 8 && r[1] > 0; roomy |= r[5] == r[1] - 18 * r[0] && r[1] > 0;
        by_bound |= r[6] == r[3] && r[3] < r[0]; by_switch |= r[4] && r[6] == r[4] && r[4] < r[3]; by_reads |= r[6] == r[0] && r[0] > 1; all |= b.all_slots;
    }
    CHECK(squeezed && roomy && by_bound && by_switch && by_reads && all && len(X_BATCH) / X_BATCH_COLS > 1000);
    for (size_t i = 0; i < len(X_NEED); i += X_NEED_COLS) {
        const uint64_t* r = X_NEED + i;
        CHECK(PathBatcher::need(r[0], r[1], r[2]) == r[3]);
        PathBatcher b(r[2], r[2], switches(12, 0));
        b.nb = r[2];
        const PathScratch s = b.scratch(r[0], r[1]);
        CHECK(s.parts == r[4] && s.path == r[5] && s.quals == r[6] && s.o_off == r[7] && s.o_len == r[8] && s.o_first == r[9] && s.sizes == r[10] && s.size_off == r[11]);
    }
    return done("a batch's room, reads, need and scratch sizes against the recorded tables (both sides of to_come + 256 MB; 12, 2, 64, 65 and all slots)");
}

static int test_index_tables()
{
    size_t on = 0, off = 0;
    for (size_t i = 0; i < len(X_TAIL); i += X_TAIL_COLS) {
        const uint64_t* r = X_TAIL + i;
        CHECK(pidx_tail_applies(r[0] != 0, r[1], r[2]) == (r[3] != 0));
        (r[3] ? on : off)++;
    }
    CHECK(on >= 8 && off >= 8);
    bool floor = false, ceil = false, between = false;
    for (size_t i = 0; i < len(X_CAP); i += X_CAP_COLS) {
        const uint64_t* r = X_CAP + i;
        CHECK(pidx_range_cap(r[0], r[1]) == r[2]);
        if (!r[1]) { floor |= r[2] == 1ull << 20; ceil |= r[2] == (1ull << 31) - 1; between |= r[2] > (1ull << 20) && r[2] < (1ull << 31) - 1; }
    }
    CHECK(floor && ceil && between);
    for (size_t i = 0; i < len(X_BITS); i += X_BITS_COLS) CHECK(pidx_key_bits(X_BITS[i]) == X_BITS[i + 1] && X_BITS[i + 1] == X_BITS[i + 2]);
    for (size_t i = 0; i < len(X_MAP); i += X_MAP_COLS) {
        const uint64_t* r = X_MAP + i;
        const PidxMap m = pidx_map(r[0], feudal_layout(1816, 16, 8, 8 * r[1]).var_tab, r[2], r[3]);
        CHECK(m.mapped == (r[4] != 0) && m.lo == r[5] && m.hi == r[6]);
    }
    return done("the index's tail thread, range cap, key bits and mapping against the recorded tables (both sides of 2^20, 2^31 - 1, free / 4)");
}

static int test_ranges_table()
{
    size_t at = 0, lists = 0, refused = 0, heavy_alone = 0, empty_ends = 0;
    while (at < len(X_RANGES)) {
        const uint64_t n_he = X_RANGES[at], cap = X_RANGES[at + 1];
        const uint64_t* counts = X_RANGES + at + 2;
        const uint64_t n_r = X_RANGES[at + 2 + n_he];
        const uint64_t* want = X_RANGES + at + 3 + n_he;
        const bool want_refused = X_RANGES[at + 3 + n_he + 3 * n_r] != 0;
        const std::vector<uint64_t> first = prefix_sums(counts, n_he);
        uint64_t e0 = 0, k = 0; bool stop = false;
        while (e0 < n_he && !stop) {
            const PidxRange r = pidx_next_range(first.data(), n_he, e0, cap);
            CHECK(k < n_r && r.e0 == want[3 * k] && r.e1 == want[3 * k + 1] && r.n == want[3 * k + 2]);
            if (r.e1 == r.e0 + 1 && r.n > cap) ++heavy_alone;
            stop = !r.ok; e0 = r.e1; ++k;
        }
        CHECK(k == n_r && stop == want_refused);
        refused += want_refused; empty_ends += n_he > 2 && !counts[0] && !counts[n_he - 1];
        at += 3 + n_he + 3 * n_r + 1; ++lists;
    }
    CHECK(at == len(X_RANGES) && lists == X_RANGES_LISTS && refused >= 3 && heavy_alone >= 10 && empty_ends >= 6);
    return done("the ranges of edges against the recorded walks (heavy edges alone, empty edges at both ends, the 2^32 refusal)");
}

static int test_dups_table()
{
    bool stop = false, one = false, many = false, forced = false;
    for (size_t i = 0; i < len(X_DUPS); i += X_DUPS_COLS) {
        const uint64_t* r = X_DUPS + i;
        const DupPlan p = plan_dups(r[0], r[1], (uint32_t)r[2]);
        CHECK(p.n_pass == r[3] && p.slots == r[4]);
        stop |= r[3] == 1024 && 16 * r[4] > r[1] / 2; one |= r[3] == 1; many |= !r[2] && r[3] > 1 && r[3] < 1024; forced |= r[2] > 1 && r[3] == r[2];
    }
    CHECK(stop && one && many && forced && len(X_DUPS) / X_DUPS_COLS > 300);
    return done("the duplicate table's passes and slots against the recorded table (0 .. 2x10^9 placed reads, 64 KB .. 288 GB, the stop at 1024 passes)");
}

static int test_feudal_table()
{
    for (size_t i = 0; i < len(X_FEUDAL); i += X_FEUDAL_COLS) {
        const uint64_t* r = X_FEUDAL + i;
        const FeudalLayout l = feudal_layout(r[0], (uint8_t)r[1], (uint8_t)r[2], r[3]);
        uint64_t w[3]; memcpy(w, &l.head, 24);
        CHECK(w[0] == r[4] && w[1] == r[5] && w[2] == r[6] && l.var_tab == r[7] && l.file_size == r[8]);
        CHECK(l.head.varTab == l.var_tab && l.head.fixedOff == l.file_size && l.head.flags == 1 && l.head.szFixed == 0);
    }
    CHECK(len(X_FEUDAL) / X_FEUDAL_COLS == 60);
    return done("the feudal control block and layout against the recorded bytes (ReadPath, ULongVec, a one-byte element)");
}

static int test_shard_table()
{
    for (size_t i = 0; i < len(X_SHARD); i += X_SHARD_COLS) {
        const uint64_t* r = X_SHARD + i;
        uint64_t h = FNV0;
        for (uint32_t k = 0; k <= r[1]; ++k) { h ^= edge_range_start(r[0], (uint32_t)r[1], k); h *= FNVP; }
        CHECK(h == r[2]);
    }
    return done("the ranks' edge ranges against the recorded table");
}

// The default benchmark (configs[1]): 1.8x10^9 reads of 100 bases at K = 48, 1.76x10^9 index entries.  DESIGN.md gives no
// free-byte figure for these steps; the rows below take 200 GB free (a 288-GB device after the dictionary and the graph) and
// 69 and 138 GB for the duplicate table (on either side of the 128 GB a single pass wants).
static int test_benchmark_figures()
{
    const uint64_t n = 1800000000ull, entries = 1760000000ull, free_now = 200ull << 30;
    const uint64_t bound = path_batch_bound(100, 48);
    CHECK(bound == 0xFFFFFFFFull / 100 - 1);
    PathBatcher b(n, bound, PathSwitches{});
    b.begin(free_now);
    CHECK(b.room == free_now - 18 * n && b.nb == std::min<uint64_t>(bound, b.room / 2 / 464) && b.nb == bound);   // the bound cuts the first batches
    bool in_table = false;
    for (size_t i = 0; i < len(X_BATCH); i += X_BATCH_COLS) in_table |= X_BATCH[i] == n && X_BATCH[i + 2] == 12 && X_BATCH[i + 1] == 250ull << 30;
    CHECK(in_table);
    CHECK(pidx_tail_applies(true, entries, free_now) && pidx_range_cap(free_now, 0) == (1ull << 31) - 1);
    const uint64_t first[2] = {0, entries};
    const PidxRange r = pidx_next_range(first, 1, 0, (1ull << 31) - 1);
    CHECK(r.ok && r.e1 == 1 && r.n == entries);
    const FeudalLayout inv = feudal_layout(400000000, 16, 8, 8 * entries);
    CHECK(inv.var_tab == 24 + 14080000000ull && inv.file_size == inv.var_tab + 8 * 400000001ull);                   // the 14 GB of lists
    // 1.7x10^9 placed reads: one pass over a table of 2^32 slots (69 GB) where half the room holds it, two over 2^31 (34 GB) where not
    const DupPlan two = plan_dups(1700000000ull, 69ull << 30, 0), one = plan_dups(1700000000ull, 138ull << 30, 0);
    CHECK(two.n_pass == 2 && two.slots == 1ull << 31 && one.n_pass == 1 && one.slots == 1ull << 32);
    int rows = 0;
    for (size_t i = 0; i < len(X_DUPS); i += X_DUPS_COLS)
        rows += X_DUPS[i] == 1700000000ull && !X_DUPS[i + 2] && ((X_DUPS[i + 1] == 69ull << 30 && X_DUPS[i + 3] == 2) || (X_DUPS[i + 1] == 138ull << 30 && X_DUPS[i + 3] == 1));
    CHECK(rows == 2);
    return done("the default benchmark's figures (1.8x10^9 reads, 1.76x10^9 index entries)");
}

// ------------------------------------------------------------------ properties over seeded random cases
static int test_batch_properties()
{
    std::mt19937_64 rng(20261019);
    auto pick = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
    for (int it = 0; it < 10000; ++it) {
        const uint64_t n = it % 7 == 0 ? pick(0, 3) : pick(1, 1ull << pick(1, 24));
        const uint64_t bound = std::max<uint64_t>(1, it % 3 ? path_batch_bound((uint32_t)pick(0, 65535), 48) : pick(1, n + 1));
        PathSwitches sw; sw.slots = (uint32_t)pick(1, 80); sw.batch_reads = it % 2 ? pick(1, n + 5) : 0;
        const uint64_t per_slot = pick(1, 120), q_per_read = pick(0, 300), free0 = pick(0, 1ull << pick(10, 38));
        PathBatcher b(n, bound, sw);
        uint64_t at = 0, file_at = 24; int batches = 0; bool retried = false;
        while (b.more()) {
            const uint64_t free_now = it % 5 ? free0 : pick(0, free0);
            b.begin(free_now);
            CHECK(b.r0 == at && b.file_base == file_at);                                 // in order, no gap; 24 plus the earlier var_bytes
            CHECK(b.cap == (retried ? 0xFFFFFFFFu : sw.slots));                          // after a retried batch: back to the slot cap
            CHECK(b.nb >= 1 && b.nb <= bound && b.nb <= n - at && (!sw.batch_reads || b.nb <= sw.batch_reads));
            const uint64_t nb0 = b.nb;
            uint64_t total, qtotal, halvings = 0;
            for (;;) {
                total = b.nb * std::min<uint64_t>(per_slot, b.cap); qtotal = b.nb * q_per_read;
                const uint64_t before = b.nb;
                if (b.fits(total, qtotal)) {
                    CHECK(b.nb == before && (PathBatcher::need(total, qtotal, b.nb) <= b.room || b.nb == 1));   // a single read is taken whatever it needs
                    break;
                }
                CHECK(before > 1 && b.nb == before / 2 && b.nb >= 1 && ++halvings <= 64);
            }
            CHECK(b.nb <= nb0 && b.r0 == at);
            const PathScratch s = b.scratch(total, qtotal);
            CHECK(s.parts + s.path + s.quals + s.o_off + s.o_len + s.o_first + s.sizes + s.size_off <= PathBatcher::need(total, qtotal, b.nb));
            const bool again = !retried && per_slot > sw.slots && pick(0, 3) == 0;     // the pather asks for all slots
            const uint64_t var_bytes = pick(0, 40 * b.nb), r0 = b.r0, nb = b.nb;
            b.end(again, var_bytes);
            if (again) {
                CHECK(b.r0 == r0 && b.file_base == file_at && b.more());
                b.begin(free_now);                                                       // the same reads again: as many where the room does not say otherwise
                CHECK(b.r0 == r0 && b.cap == 0xFFFFFFFFu && b.nb <= std::max(nb0, nb));
                PathBatcher same = b; same.begin(~0ull >> 8);                            // ... and exactly as many with room to spare
                CHECK(same.nb == std::min<uint64_t>(std::min<uint64_t>(n - r0, bound), sw.batch_reads ? sw.batch_reads : ~0ull) && same.nb >= nb0);
            } else { at += nb; file_at += var_bytes; ++batches; }
            retried = again;
        }
        CHECK(at == n && !retried && (n == 0) == (batches == 0));
    }
    return done("batches over 10^4 random cases (they tile the reads in order, file_base, the bound and the switch hold, halving ends at one read, the retry keeps its reads)");
}

static int test_range_properties()
{
    std::mt19937_64 rng(7);
    auto pick = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
    for (int it = 0; it < 10000; ++it) {
        const uint64_t n_he = pick(1, 60), big = it % 50 == 0 ? 1ull << 32 : 0;
        std::vector<uint64_t> counts(n_he);
        for (uint64_t& x : counts) x = pick(0, 3) ? pick(0, 1ull << pick(0, 12)) : 0;
        if (big) counts[pick(0, n_he - 1)] = big - pick(0, 1);
        const std::vector<uint64_t> first = prefix_sums(counts.data(), n_he);
        CHECK(first.size() == n_he + 1 && first[0] == 0);
        const uint64_t cap = it % 4 ? pick(1, 1ull << pick(0, 14)) : pidx_range_cap(pick(0, 1ull << 40), 0);
        uint64_t e0 = 0, sum = 0;
        while (e0 < n_he) {
            const PidxRange r = pidx_next_range(first.data(), n_he, e0, cap);
            CHECK(r.e0 == e0 && r.e1 > e0 && r.e1 <= n_he && r.n == first[r.e1] - first[e0]);
            CHECK(r.n <= cap || r.e1 == e0 + 1);                                      // over the cap: a single edge
            CHECK(r.e1 == n_he || first[r.e1 + 1] - first[e0] > cap);                 // and no range stops early
            CHECK(r.ok == (r.n < (1ull << 32)));
            CHECK(pidx_key_bits(r.e1 - e0) >= 1 && (1ull << pidx_key_bits(r.e1 - e0)) >= r.e1 - e0);
            if (!r.ok) break;
            sum += r.n; e0 = r.e1;
        }
        CHECK(e0 == n_he ? sum == first[n_he] : big != 0);
    }
    return done("ranges over 10^4 random prefix sums (they tile the edges, hold at most cap entries unless a single edge, 2^32 refused)");
}

static int test_dup_properties()
{
    std::mt19937_64 rng(11);
    auto pick = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
    for (int it = 0; it < 10000; ++it) {
        const uint64_t n_placed = pick(0, 1ull << pick(0, 31)), free_now = pick(0, 1ull << pick(12, 39));
        const uint32_t min_passes = it % 3 ? 0 : (uint32_t)pick(1, 40);
        const DupPlan p = plan_dups(n_placed, free_now, min_passes);
        CHECK((p.n_pass & (p.n_pass - 1)) == 0 && p.n_pass >= 1 && p.n_pass <= 1024 && p.n_pass >= min_passes);
        CHECK((p.slots & (p.slots - 1)) == 0 && p.slots >= 1ull << 10);
        CHECK(2 * p.slots * p.n_pass >= 5 * n_placed);                               // load <= 0.5 with a quarter to spare: slots >= 2.5 n_placed / n_pass
        CHECK(16 * p.slots <= free_now / 2 || p.n_pass == 1024);
        const uint32_t start = std::max<uint32_t>(1, min_passes);
        if (p.n_pass / 2 >= start) CHECK(16 * plan_dups(n_placed, ~0ull, p.n_pass / 2).slots > free_now / 2);   // no pass more than the room asks for
    }
    return done("duplicate passes over 10^4 random cases (powers of two, load at most 0.5, half the room, the fewest passes that fit)");
}

static int test_piece_properties()
{
    std::mt19937_64 rng(13);
    auto pick = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
    static const char base[1] = {0};
    for (int it = 0; it < 10000; ++it) {
        const uint64_t chunk = 32 * pick(2, 1ull << pick(1, 12)), bytes = it % 9 ? pick(0, chunk * pick(1, 9)) : chunk * pick(0, 5), off = pick(0, 1ull << 40);
        std::vector<FilePiece> v(1, FilePiece{base, 1, 2});
        append_pieces(v, base, bytes, off, chunk);
        CHECK(v.size() == 1 + (bytes + chunk - 1) / chunk && v[0].bytes == 1);
        uint64_t at = 0;
        for (size_t i = 1; i < v.size(); ++i) {
            CHECK(v[i].src == base + at && v[i].file_off == off + at && !v[i].widen && v[i].add == 0 && v[i].bytes > 0);
            CHECK(i + 1 == v.size() ? v[i].bytes <= chunk : v[i].bytes == chunk);
            at += v[i].bytes;
        }
        CHECK(at == bytes);
        const uint64_t wbytes = 4 * (bytes / 4), add = pick(0, 1ull << 36);
        std::vector<FilePiece> w;
        append_wide_pieces(w, base, wbytes, off, add, chunk);
        CHECK(w.size() == (wbytes + chunk / 2 - 1) / (chunk / 2));
        at = 0;
        for (size_t i = 0; i < w.size(); ++i) {
            CHECK(w[i].src == base + at && w[i].file_off == off + 2 * at && w[i].widen && w[i].add == add && w[i].bytes % 4 == 0);   // twice its bytes in the file
            CHECK(i + 1 == w.size() ? w[i].bytes <= chunk / 2 && w[i].bytes > 0 : w[i].bytes == chunk / 2);
            at += w[i].bytes;
        }
        CHECK(at == wbytes);
    }
    return done("file pieces over 10^4 random ranges (no gap or overlap, every piece but the last a whole chunk, the widened ones advance by twice their bytes)");
}

static int test_shard_properties()
{
    std::mt19937_64 rng(17);
    auto pick = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
    for (int it = 0; it < 10000; ++it) {
        const uint32_t world = it < 640 ? 1 + it % 64 : (uint32_t)pick(1, 64);           // every world from 1 to 64, then at random
        const uint64_t n_he = it % 11 ? pick(1, 300) : pick(1, 1ull << 32);
        CHECK(edge_range_start(n_he, world, 0) == 0 && edge_range_start(n_he, world, world) == n_he);
        for (uint32_t r = 0; r < world; ++r) CHECK(edge_range_start(n_he, world, r) <= edge_range_start(n_he, world, r + 1));
        if (n_he > 300) continue;
        std::vector<uint32_t> counts(n_he); std::vector<uint64_t> c64(n_he);
        uint64_t total = 0;
        for (uint64_t e = 0; e < n_he; ++e) { counts[e] = (uint32_t)pick(0, 1ull << pick(0, 31)); c64[e] = counts[e]; total += counts[e]; }
        uint64_t send[64], sum = 0;
        shard_send_counts(counts.data(), n_he, world, send);
        const std::vector<uint64_t> first = prefix_sums(c64.data(), n_he);
        uint64_t last_writers = 0, entries = 0;
        for (uint32_t r = 0; r < world; ++r) {
            const uint64_t e0 = edge_range_start(n_he, world, r), e1 = edge_range_start(n_he, world, r + 1);
            CHECK(send[r] == first[e1] - first[e0]);
            sum += send[r];
            const uint64_t n_eo = shard_table_entries(e1 - e0, world, r);
            const std::vector<uint64_t> eo = shard_table_slice(first, e0, e1);
            CHECK(eo.size() == e1 - e0 + 1 && n_eo <= eo.size());
            for (uint64_t e = 0; e < eo.size(); ++e) CHECK(eo[e] == 24 + 8 * first[e0 + e]);
            last_writers += e0 + n_eo == n_he + 1; entries += n_eo;
        }
        CHECK(sum == total && first[n_he] == total && last_writers == 1 && entries == n_he + 1);
    }
    return done("the sharded index over 10^4 random cases (the ranks' edges tile for every world from 1 to 64, the send counts add up, one rank writes the table's last entry)");
}

// ------------------------------------------------------------------ a replay and the grid
// 6000 reads in batches of at most 257 (what tests/test_gpu_paths.py runs on the `frag` fixture): 24 batches, the 10th of
// which asks for all slots
static int test_replay()
{
    PathSwitches sw; sw.slots = 2; sw.batch_reads = 257;
    PathBatcher b(6000, path_batch_bound(152, 48), sw);
    uint64_t file_at = 24; int batches = 0, attempts = 0;
    while (b.more()) {
        b.begin(100ull << 30);
        ++attempts;
        CHECK(b.r0 == 257ull * batches && b.nb == (batches == 23 ? 6000 - 23 * 257 : 257) && b.file_base == file_at && b.room == (100ull << 30) - 18 * (6000 - b.r0));
        const bool retry = attempts == 11;
        CHECK(b.cap == (retry ? 0xFFFFFFFFu : 2u));
        CHECK(b.fits(b.nb * (retry ? 105 : 2), b.nb * 152));
        const bool again = attempts == 10;
        const uint64_t var = 8 * b.nb + 4 * (b.r0 % 97);
        b.end(again, var);
        if (!again) { ++batches; file_at += var; }
    }
    CHECK(batches == 24 && attempts == 25 && b.r0 == 6000 && b.file_base == file_at);
    return done("the batch planner replayed: 6000 reads, at most 257 a batch, 24 batches, one done again with all slots");
}

static int test_grid()
{
    for (unsigned cus : {1u, 8u, 256u}) for (uint32_t per : {16u, 32u, 64u})
        for (uint64_t n : {0ull, 1ull, 255ull, 256ull, 257ull, 511ull, 512ull, 6000ull, 1800000000ull, (1ull << 32) + 5}) {
            CHECK(grid_256(n, cus, per) == (unsigned)std::min<uint64_t>((n + 255) / 256, (uint64_t)per * cus));
            CHECK(grid_256(n + 1, cus, per) == (unsigned)std::min<uint64_t>((n + 256) / 256, (uint64_t)per * cus));   // the sites that always had one block more
            CHECK(grid_256(n, cus) == grid_256(n, cus, 32));
        }
    return done("the grid of a 256-thread launch");
}

int main()
{
    int bad = 0;
    bad += test_bound_table(); bad += test_filter_table(); bad += test_batch_table(); bad += test_index_tables(); bad += test_ranges_table();
    bad += test_dups_table(); bad += test_feudal_table(); bad += test_shard_table(); bad += test_benchmark_figures();
    bad += test_batch_properties(); bad += test_range_properties(); bad += test_dup_properties(); bad += test_piece_properties(); bad += test_shard_properties();
    bad += test_replay(); bad += test_grid();
    return bad ? 1 : 0;
}
